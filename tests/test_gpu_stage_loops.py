"""The grid-stride loops of the stats-by and top-histogram stages, run several times over, and the shapes of fmx_value_hist.hip that
the fixture never reaches.  Every kernel of fmx_hit_first.hip, fmx_value_hist.hip, the "by" kernels of fmx_hit_numbers.hip and the
group-of-hit twin of fmx_hit_values.hip loops over a grid that fmx_hit_lines_geometry caps at 2 workgroups per CU x 1,024 hits (the
key kernels: KEY slots a pass) or 8 per CU x 256 (the element-wise kernels: FLAT items a pass), whatever `block` and `groups_per_cu`
say.  The fixture's few thousand hits fit one pass of every one of them.

Here the inputs are as large as a second and a third pass need.  Every size comes from fmx_hit_lines_geometry, and every test first
asserts the pass counts it was built for (the arithmetic of passes() in tests/test_gpu_launch_shapes.py), so that a size that no
longer loops fails instead of passing quietly.

Two stages take their groups and hits as plain arrays, so their inputs are made up: fmx_values_top_histogram_dev +
fmx_values_gather_rows_dev and fmx_first_hits_of_lines_dev, judged by the numpy judges of tests/stage_judges.py (held to the oracle's
judges in tests/test_stage_judges_cpu.py).  The two stages that read the text run over the fixture's real hits, the batch repeated;
the judge is the one-repetition judge of the older files, tiled.  Every output is prefilled with a sentinel and padded by 64
entries that must keep it, whole arrays are compared, and the packed blocks carry 3 slots in front and 70 behind."""
import ctypes as C

import numpy as np
import pytest

import index4j_amd as ia
import orc
from common import hdfs_text
from stage_judges import buckets_of, lines_of, np_first_hits, np_top_hist, slot_patterns
from test_field_values_cpu import judge_values
from test_field_values_histogram_cpu import Hits, hit_groups
from test_field_values_where_cpu import Where
from test_gpu_field_values import last_error
from test_gpu_locate_rows import _torch
from test_gpu_number_stats_by import dev_by
from test_line_histogram_cpu import EDGES_250, EDGES_UNEVEN
from test_locate_all_cpu import SENT
from test_match_lines_cpu import judge_n_lines, judge_table
from test_number_stats_by_cpu import judge_by

pytestmark = pytest.mark.gpu

HD = hdfs_text()
PAD = 64            # entries behind the answer that must keep the sentinel
LEAD, EXTRA = 3, 70  # slots in front of hit_off[0] and behind hit_off[n] that hold no hit
TILE, LANES = 1024, 256  # slots of a key kernel's workgroup a pass, items of an element-wise one's
CHAR_SENT = 0x7B7B
WS_LIMIT = 2 << 30  # no test needs more device memory than this for a workspace
DEEP_LINES = 8300


def stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def filled(count, dtype):
    torch = _torch()
    return torch.full((count + PAD,), SENT, dtype=dtype, device="cuda")


def cut(t, count, what):
    a = t.cpu().numpy()
    assert len(a) == count + PAD and (a[count:] == SENT).all(), "stored beyond the answer: " + what
    return a[:count]


def up(a, dtype):
    return _torch().from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def workspace(need, what):
    assert 0 < need < WS_LIMIT, "%s: a workspace of %d bytes" % (what, need)
    torch = _torch()
    return torch.empty(need, dtype=torch.uint8, device="cuda")


# ---- the grids (fmx_hit_lines_geometry) and the passes of a loop over them ----
def geometry(fm, items):
    key_grid, flat_grid = C.c_int32(0), C.c_int32(0)
    assert ia.lib.fmx_hit_lines_geometry(fm.handle, int(items), C.byref(key_grid), C.byref(flat_grid)) == 0
    return key_grid.value, flat_grid.value


def caps(fm):
    """KEY, FLAT: what the largest grids cover in one pass"""
    key_grid, flat_grid = geometry(fm, 10 ** 9)
    return key_grid * TILE, flat_grid * LANES


def key_passes(fm, slots):
    """passes of a key kernel's loop over `slots` slots (its grid is the geometry's for these slots)"""
    return -(-slots // (geometry(fm, slots)[0] * TILE))


def flat_passes(fm, items, grid_of=None):
    """passes of an element-wise loop over `items` items on the flat grid the launcher asks for `grid_of` items (default: items)"""
    return -(-items // (geometry(fm, items if grid_of is None else grid_of)[1] * LANES))


def assert_loops(what, **passes):
    """every named loop runs at least three passes on this card; the figures are printed for the record"""
    print("%s: passes %s" % (what, ", ".join("%s %d" % kv for kv in passes.items())))
    assert min(passes.values()) >= 3, (what, passes)


# ---- packed blocks of made-up hits ----
class Block:
    """per[i] hits of pattern i at the positions `locs`, packed with `lead` slots in front (hit_off[0] = lead) and `extra` behind"""

    def __init__(self, per, locs, lead=LEAD, extra=EXTRA):
        self.per = np.asarray(per, np.int64)
        self.n, self.hits, self.lead, self.extra = len(self.per), int(self.per.sum()), lead, extra
        assert len(locs) == self.hits
        self.hit_off = (lead + np.concatenate([[0], np.cumsum(self.per)])).astype(np.int64)
        self.locs = self.around(locs, -5)
        self.slots = lead + self.hits + extra
        self.pattern = np.repeat(np.arange(self.n), self.per)  # of every hit

    def around(self, per_hit, fill):
        """a per-hit array as a per-slot one"""
        return np.concatenate([np.full(self.lead, fill, np.int32), np.asarray(per_hit, np.int32), np.full(self.extra, fill, np.int32)])


def widest_tile(hit_off, n_slots):
    """the most patterns a tile of 1,024 slots sees: fm_hit_tile's [p_lo, p_hi] over the tiles that hold a hit"""
    n = len(hit_off) - 1
    first, total, _ = slot_patterns(hit_off, n_slots)
    tiles = np.arange(0, n_slots, TILE)
    tiles = tiles[(tiles < total) & (tiles + TILE > first)]
    last = np.minimum(tiles + TILE, total) - 1
    p_lo = np.maximum(np.searchsorted(hit_off[:n], tiles, "right") - 1, 0)
    p_hi = np.searchsorted(hit_off[:n], last, "right") - 1
    return int((p_hi - p_lo + 1).max())


def made_up_groups(rng, blk, groups, skew):
    """groups[i] groups for pattern i (0 where it has no hit; at most its hits): every group gets a hit, the other hits fall on
    group floor(G_i * u ** skew[i]) — a few large groups and a long tail of equal small counts.  Returns val_off, count (what the
    hits add up to) and the group of every hit"""
    groups = np.asarray(groups, np.int64)
    assert (groups <= blk.per).all() and ((groups > 0) == (blk.per > 0)).all()
    val_off = np.concatenate([[0], np.cumsum(groups)]).astype(np.int64)
    group = np.zeros(blk.hits, np.int64)
    at = 0
    for i in range(blk.n):
        h, g = int(blk.per[i]), int(groups[i])
        if h:
            mine = np.concatenate([np.arange(g), (g * rng.random(h - g) ** skew[i]).astype(np.int64)])
            group[at:at + h] = rng.permutation(mine)
        at += h
    count = np.bincount(val_off[blk.pattern] + group, minlength=int(val_off[-1])).astype(np.int32)
    return val_off, count, group.astype(np.int32)


def made_up_text(rng, G, lo, hi):
    """text_off and chars of G groups of lo .. hi code units each"""
    text_off = np.concatenate([[0], np.cumsum(rng.integers(lo, hi + 1, G))]).astype(np.int64)
    return text_off, rng.integers(0, 65536, int(text_off[-1]), dtype=np.uint16)


# ---- the stages ----
def run_top_hist(fm, blk, val_off, count, group, edges, top, text_off=None, chars=None):
    """fmx_values_top_histogram_dev and, with text, fmx_values_gather_rows_dev over a Block; group: per SLOT; a dict under the
    judge's names"""
    torch = _torch()
    lib, n, st = ia.lib, blk.n, stream()
    voff = np.array(val_off, np.int64)
    G = int(voff[n])
    edges_a = np.zeros(0, np.int32) if edges is None else np.array(edges, np.int32)
    B = max(len(edges_a) - 1, 1)
    R = int(np.minimum(np.diff(voff), top).sum())
    assert len(group) == blk.slots and len(count) == G
    hit_off, locs = up(blk.hit_off, np.int64), up(np.concatenate([blk.locs, np.zeros(1, np.int32)]), np.int32)
    d_count, d_group = up(count, np.int32), up(group, np.int32)
    row_off, row_group, row_count = filled(n + 1, torch.int64), filled(R, torch.int32), filled(R, torch.int32)
    hist, other = filled(R * B, torch.int32), filled(n * B, torch.int32)
    ws = workspace(lib.fmx_values_top_histogram_scratch_bytes(n, G, blk.slots, len(edges_a)), "fmx_values_top_histogram_scratch_bytes")
    rc = lib.fmx_values_top_histogram_dev(fm.handle, n, voff.ctypes.data, top, edges_a.ctypes.data if len(edges_a) else None, len(edges_a),
                                          hit_off.data_ptr(), locs.data_ptr(), blk.slots, d_count.data_ptr(), d_group.data_ptr(), row_off.data_ptr(),
                                          row_group.data_ptr(), row_count.data_ptr(), hist.data_ptr(), other.data_ptr(), ws.data_ptr(), ws.numel(), st)
    keep = voff.copy()
    voff[:] = -9  # (the call has copied what it needs before it returns)
    edges_a[:] = -9
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    got = dict(row_off=cut(row_off, n + 1, "row_off"), row_group=cut(row_group, R, "row_group"), row_count=cut(row_count, R, "row_count"),
               hist=cut(hist, R * B, "hist").reshape(R, B), other=cut(other, n * B, "other").reshape(n, B))
    if text_off is None:
        return got
    units = int(text_off[G])
    d_text_off, d_chars = up(text_off, np.int64), up(np.concatenate([chars, np.zeros(1, np.uint16)]).view(np.int16), np.int16)
    row_text_off = filled(R + 1, torch.int64)
    row_chars = torch.full((units + PAD,), CHAR_SENT, dtype=torch.int16, device="cuda")
    ws = workspace(lib.fmx_values_gather_rows_scratch_bytes(n, R), "fmx_values_gather_rows_scratch_bytes")
    rc = lib.fmx_values_gather_rows_dev(fm.handle, n, keep.ctypes.data, top, units, row_group.data_ptr(), d_text_off.data_ptr(), d_chars.data_ptr(),
                                        row_text_off.data_ptr(), row_chars.data_ptr(), ws.data_ptr(), ws.numel(), st)
    keep[:] = -9
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    got["row_text_off"] = cut(row_text_off, R + 1, "row_text_off")
    c = row_chars.cpu().numpy()
    row_units = int(got["row_text_off"][R])
    assert 0 <= row_units <= units and (c[row_units:] == CHAR_SENT).all(), "stored beyond the answer: row_chars"
    got["row_chars"] = c[:row_units].view(np.uint16)
    return got


def check_whole(got, want, names, what):
    for name in names:
        a, b = np.asarray(got[name]), np.asarray(getattr(want, name))
        assert a.shape == b.shape, "%s: %s has the shape %r, expected %r" % (what, name, a.shape, b.shape)
        bad = np.flatnonzero(a.ravel() != b.ravel())
        assert len(bad) == 0, "%s: %s differs at %d places, first %r: %r, expected %r" % (what, name, len(bad), bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])


TOP_HIST = ("row_off", "row_group", "row_count", "hist", "other")
GATHER = ("row_text_off", "row_chars")


def check_bucket_sums(got, blk, T, edges, what):
    """independent of the ranking: per pattern the rows' counters and `other` add up to a direct bincount of its hits' buckets"""
    n, B = blk.n, len(edges) - 1
    b, _ = buckets_of(edges, lines_of(T, blk.locs[blk.lead:blk.lead + blk.hits]))
    direct = np.bincount((blk.pattern * B + b)[b >= 0], minlength=n * B).reshape(n, B)
    total = got["other"].astype(np.int64).copy()
    np.add.at(total, np.repeat(np.arange(n), np.diff(got["row_off"])), got["hist"])
    assert (total == direct).all(), what + ": hist.sum(axis=0) + other per pattern against the hits' buckets"
    return direct


def top_hist_case(fm, T, blk, val_off, count, group, edges, top, what, text=None):
    """the stage (and the gather) against np_top_hist, whole arrays; the cross-check where there are edges"""
    slots_group = blk.around(group, -1)
    text_off, chars = text if text else (None, None)
    want = np_top_hist(blk.hit_off, blk.locs, blk.slots, val_off, count, slots_group, edges, top, T, text_off, chars)
    got = run_top_hist(fm, blk, val_off, count, slots_group, edges, top, text_off, chars)
    check_whole(got, want, TOP_HIST + (GATHER if text else ()), what)
    if edges is not None:
        check_bucket_sums(got, blk, T, edges, what)
    return want, got


def run_first_hits(fm, blk):
    torch = _torch()
    lib, m = ia.lib, blk.n
    hit_off, locs = up(blk.hit_off, np.int64), up(np.concatenate([blk.locs, np.zeros(1, np.int32)]), np.int32)
    K = max(blk.hits, 1)
    first_off, first_lines, first_locs = filled(m + 1, torch.int64), filled(K, torch.int32), filled(K, torch.int32)
    ws = workspace(lib.fmx_first_hits_of_lines_scratch_bytes(m, blk.slots), "fmx_first_hits_of_lines_scratch_bytes")
    rc = lib.fmx_first_hits_of_lines_dev(fm.handle, m, hit_off.data_ptr(), locs.data_ptr(), blk.slots, first_off.data_ptr(), first_lines.data_ptr(),
                                         first_locs.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    got = dict(first_off=cut(first_off, m + 1, "first_off"))
    F = int(got["first_off"][m])
    assert 0 <= F <= K
    got.update(first_lines=cut(first_lines[:F + PAD], F, "first_lines"), first_locs=cut(first_locs[:F + PAD], F, "first_locs"))
    assert (first_lines[F:].cpu().numpy() == SENT).all() and (first_locs[F:].cpu().numpy() == SENT).all(), "stored beyond the first hits"
    return got


# ---- the indexes ----
@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    fm = ia.FmIndex(HD, 16, True, device=0)
    T = judge_table(o, "\n")
    assert fm.build_line_table("\n") == judge_n_lines(T, len(HD)) == 2000
    yield o, fm, T
    fm.close()


@pytest.fixture(scope="module")
def deep():
    """8,300 lines (the text of test_deep_line_table_and_wide_batches): more entries than the 4,096 fences of a workgroup, so
    fm_line_fence_shift is above 0 and the last levels of fm_line_of run over the table itself.  T is read off the text"""
    text = "\n".join("id=%d k=v%d n=%d" % (i, i % 13, (i * 7919) % 1009) if i % 50 else "n=%d nokey%d" % (i, i) for i in range(DEEP_LINES))
    fm = ia.FmIndex(text, 8, True, device=0)
    T = np.flatnonzero(ia.as_chars(text) == ord("\n")).astype(np.int32)
    assert fm.build_line_table("\n") == DEEP_LINES and len(T) == DEEP_LINES - 1 > 4096
    yield fm, T, len(text)
    fm.close()


# ---- a. the top-histogram stage, every loop three times ----
def test_top_histogram_loops(hd):
    """n = 5 (the third pattern has no hit), G = 3 FLAT + 1 groups and at least 3 KEY + 1 hits at positions all over the text; the
    groups of a pattern drawn with a skew of its own (u ** 1: every count small, the seven rows are the tie rule alone); about 1 %
    of the hits carry the group -1 and 1 % the group G_i + 5, both "other".  EDGES_UNEVEN, top = 7; 0 .. 5 code units a group.
    Passes asserted: k_vh_keys, k_vh_rank_keys, k_vh_ranks >= 3"""
    o, fm, T = hd
    KEY, FLAT = caps(fm)
    rng = np.random.default_rng(20240501)
    G = 3 * FLAT + 1
    groups = np.array([G * 2 // 5, G // 10, 0, G * 3 // 10, 0], np.int64)
    groups[4] = G - groups.sum()
    n_hits = max(3 * KEY + 1, G + 400_000)
    per = groups + np.array([1, 1, 0, 1, 1]) * ((n_hits - G) // 4)
    per[4] += n_hits - per.sum()
    blk = Block(per, rng.integers(0, len(HD), n_hits))
    assert_loops("top histogram", k_vh_keys=key_passes(fm, blk.slots), k_vh_rank_keys=flat_passes(fm, G), k_vh_ranks=flat_passes(fm, G))
    val_off, count, group = made_up_groups(rng, blk, groups, [4, 1, 1, 2, 8])
    draw = rng.random(n_hits)
    group[draw < 0.01] = -1
    beyond = (draw >= 0.01) & (draw < 0.02)
    group[beyond] = (groups[blk.pattern] + 5)[beyond]
    text = made_up_text(rng, G, 0, 5)
    assert (np.diff(text[0]) == 0).any()
    want, got = top_hist_case(fm, T, blk, val_off, count, group, EDGES_UNEVEN, 7, "three passes of every loop", text)
    assert want.row_off.tolist() == [0, 7, 14, 14, 21, 28] and (want.buckets < 0).any() and want.other.sum() > n_hits // 100
    assert len(np.unique(want.row_count[7:14])) < 7  # equal counts among the rows of the pattern drawn evenly


# ---- b. more rows, counters and code units than one grid covers ----
def test_rows_counters_and_units_beyond_one_grid(hd):
    """one pattern of 70,000 groups, top = 65,536: the rank cap min(rank, top) and the code "other" at code_bits = 17, 4,464 groups
    in "other", the cut in the middle of a long run of equal counts.  (R + n) * B counters with B = 25 (more where the card's FLAT
    asks for it) and 20 .. 40 code units a row.  Passes asserted: k_vh_counts and k_vh_gather >= 3.  k_vh_row_sources and
    k_vh_row_lengths run over R = 65,536 rows: one pass on a card of 256 CUs, they loop only on smaller cards"""
    o, fm, T = hd
    KEY, FLAT = caps(fm)
    rng = np.random.default_rng(20240502)
    G, top, n_hits = 70_000, 65_536, 300_000
    R = top
    B = max(25, -(-(2 * FLAT + 1) // (R + 1)))
    assert_loops("counters", k_vh_counts=flat_passes(fm, (R + 1) * B))
    assert (top + 1) * B <= 1 << 27, B
    edges = np.linspace(10, 1990, B + 1).astype(np.int32)
    assert (np.diff(edges) > 0).all()
    blk = Block([n_hits], rng.integers(0, len(HD), n_hits))
    val_off, count, group = made_up_groups(rng, blk, [G], [3])
    text_off, chars = made_up_text(rng, G, 20, 40)
    want, got = top_hist_case(fm, T, blk, val_off, count, group, edges, top, "70,000 groups, top 65,536", (text_off, chars))
    row_units = int(got["row_text_off"][R])
    assert_loops("gather", k_vh_gather=flat_passes(fm, row_units, grid_of=int(text_off[G])))
    assert row_units >= 3 * FLAT, row_units
    print("rows: passes k_vh_row_sources %d, k_vh_row_lengths %d (not asserted)" % (flat_passes(fm, R), flat_passes(fm, R + 1, grid_of=R)))
    # the rank cap and the ties at scale
    assert G - R == 4464 and len(got["row_group"]) == R and len(np.unique(got["row_group"])) == R
    assert (np.diff(got["row_count"]) <= 0).all()
    tie = np.diff(got["row_count"]) == 0
    assert tie.sum() > R // 2 and (np.diff(got["row_group"])[tie] > 0).all()  # equal counts: the smaller group first
    rest = np.setdiff1d(np.arange(G), got["row_group"])
    assert len(rest) == 4464 and count[rest].max() <= got["row_count"][-1]
    assert (rest[count[rest] == got["row_count"][-1]] > got["row_group"][got["row_count"] == got["row_count"][-1]].max()).all()
    b, _ = buckets_of(edges, lines_of(T, blk.locs[LEAD:LEAD + n_hits]))
    assert got["other"].sum() == (np.isin(group, rest) & (b >= 0)).sum() > 0
    outside = np.bincount(group[b < 0], minlength=G)  # the hits of a group that lie in no bucket
    assert (outside > 0).any() and (outside[got["row_group"]] == 0).any()
    assert (got["hist"].sum(axis=1) == got["row_count"] - outside[got["row_group"]]).all()  # (== row_count where every hit has a bucket)


# ---- c. a tile of more than 2,048 patterns; the pattern field's extra bit ----
def wide_batch(rng, lead, extra):
    n = 4096
    per = np.zeros(n, np.int64)
    per[0], per[2201] = 1500, 3000
    per[2202:] = rng.integers(1, 5, n - 2202)
    blk = Block(per, rng.integers(0, len(HD), int(per.sum())), lead, extra)
    groups = np.minimum(per, rng.integers(1, 6, n))
    return (blk,) + made_up_groups(rng, blk, groups, np.full(n, 2.0)) + (made_up_text(rng, int(groups.sum()), 0, 5),)


def test_wide_slice_and_the_pattern_fields_extra_bit(hd):
    """n = 4,096 exactly: the key of a slot that is no hit, pattern = n, needs the thirteenth bit of fm_bits(n), with such slots in
    front of and behind the hits.  2,200 patterns without a hit between two that have hits: the tile that holds the boundary sees
    more than kLocateAllSlice = 2,048 patterns, searches hit_off where it lies and skips the barrier.  top = 3; EDGES_250 and no
    edges; once more with 1,023 slots in front and 1,025 behind"""
    o, fm, T = hd
    for lead, extra, edge_sets in ((LEAD, EXTRA, (EDGES_250, None)), (1023, 1025, (EDGES_250,))):
        blk, val_off, count, group, text = wide_batch(np.random.default_rng(20240503), lead, extra)
        assert blk.n == 4096 == 1 << 12 and blk.hit_off[0] == lead and blk.slots - blk.hit_off[-1] == extra
        assert (blk.per[1:2201] == 0).all() and widest_tile(blk.hit_off, blk.slots) > 2048
        for edges in edge_sets:
            want, got = top_hist_case(fm, T, blk, val_off, count, group, edges, 3, "4,096 patterns, %d in front, %d behind" % (lead, extra), text)
            assert (want.row_off[1:2202] == want.row_off[1]).all() and want.other.sum() > 0
            if edges is None:
                assert (got["hist"].sum(axis=1) == got["row_count"]).all()


# ---- d. a line table deeper than the fences; edges in HBM with several patterns ----
def test_deep_line_table_and_edges_in_hbm(deep):
    """8,300 lines (shift > 0 in k_vh_keys), n = 3, top = 2, 200,000 hits; 4,200 strictly rising edges (more than kHistEdgesLds =
    4,096: searched in HBM) that begin above line 0 and end below the line count, so hits fall out on both sides; then 26 edges
    over the same table (staged in LDS)"""
    fm, T, text_len = deep
    rng = np.random.default_rng(20240504)
    blk = Block([120_000, 30_000, 50_000], rng.integers(0, text_len, 200_000))
    val_off, count, group = made_up_groups(rng, blk, [50, 1, 3000], [2, 1, 3])
    many = np.sort(rng.choice(np.arange(40, 8200), 4200, replace=False)).astype(np.int32)
    few = np.linspace(40, 8200, 26).astype(np.int32)
    for edges in (many, few):
        assert (np.diff(edges) > 0).all() and 0 < edges[0] and edges[-1] < DEEP_LINES and (len(edges) > 4096) == (edges is many)
        want, got = top_hist_case(fm, T, blk, val_off, count, group, edges, 2, "%d edges over 8,300 lines" % len(edges))
        lines = lines_of(T, blk.locs[LEAD:LEAD + blk.hits])
        assert (lines < edges[0]).any() and (lines >= edges[-1]).any() and (got["hist"].sum(axis=1) < got["row_count"]).all()
        assert want.row_off.tolist() == [0, 2, 3, 5]


# ---- e. the first hits of lines ----
def test_first_hits_loops(deep):
    """m = 2,300 key patterns, 2,100 of them without a hit between two that have hits (a tile of more than 2,048 patterns), and at
    least 3 KEY + 1 hits at random positions of a text of 8,300 lines: many hits per (pattern, line).  Passes asserted: k_first_keys
    and k_first_lines (key grid), k_first_heads and the hit loop of k_first_store (flat grid) >= 3.  Then m = 3 FLAT + 2 patterns
    of at most one hit each: the loop over p <= m of k_first_store >= 3, hit_off large and the hits few"""
    fm, T, text_len = deep
    KEY, FLAT = caps(fm)
    rng = np.random.default_rng(20240505)
    m, n_hits = 2300, 3 * KEY + 1
    per = np.zeros(m, np.int64)
    per[0] = n_hits // 2
    per[2101:] = rng.multinomial(n_hits - per[0], np.full(m - 2101, 1.0 / (m - 2101)))
    blk = Block(per, rng.integers(0, text_len, n_hits))
    assert (per[1:2101] == 0).all() and per[2101] > 0 and widest_tile(blk.hit_off, blk.slots) > 2048
    assert_loops("first hits", k_first_keys=key_passes(fm, blk.slots), k_first_lines=key_passes(fm, blk.slots),
                 k_first_heads=flat_passes(fm, blk.slots + 1, grid_of=blk.slots), k_first_store_hits=flat_passes(fm, blk.slots))
    want = np_first_hits(blk.hit_off, blk.locs, blk.slots, T)
    assert len(want.first_lines) * 2 < n_hits and want.first_off[1] * 50 < per[0]  # duplicates: many hits per (pattern, line)
    check_whole(run_first_hits(fm, blk), want, ("first_off", "first_lines", "first_locs"), "2,300 patterns, %d hits" % n_hits)
    # more patterns than three grids of lanes
    m = 3 * FLAT + 2
    per = (rng.random(m) < 0.02).astype(np.int64)
    per[0], per[-1] = 0, 1
    blk = Block(per, rng.integers(0, text_len, int(per.sum())))
    assert_loops("first hits, many patterns", k_first_store_patterns=flat_passes(fm, m + 1, grid_of=blk.slots))
    assert blk.hits < FLAT
    want = np_first_hits(blk.hit_off, blk.locs, blk.slots, T)
    assert (np.diff(want.first_off) == per).all()
    check_whole(run_first_hits(fm, blk), want, ("first_off", "first_lines", "first_locs"), "%d patterns of at most one hit" % m)


# ---- f. the group of every hit, over the text ----
def test_group_of_hit_twin_loops(hd):
    """(" ", "1", "0") under two queries, the batch repeated until its slots are more than three passes of the larger grid, through
    fmx_values_of_hits_groups_dev: val_off, count and text_off are the one-repetition judge's, tiled, and every repetition's
    group_of_hit is the judge's of the base batch; the slots behind the hits hold -1.  Passes asserted: every element-wise kernel of
    the stage (k_val_run_groups and k_val_hit_groups among them) and its key kernels >= 3"""
    o, fm, T = hd
    torch = _torch()
    KEY, FLAT = caps(fm)
    stop, max_len = " \n", 16
    w = Where("hd16 heavy", o, T, [" ", "1", "0"], [dict(all=["terminating"]), dict(any=["WARN", "/10.250.1"])], [0, -1, 1], (2, 1999))
    hits = Hits(w.kept_off, w.kept_locs, w.lens)
    values = judge_values(o, hits.kept_locs, hits.kept_off, hits.lens, stop, max_len)
    base_group = hit_groups(values, hits, stop)
    per = int(w.kept_off[-1])
    reps = 3 * max(KEY, FLAT) // per + 1
    n, total = 3 * reps, reps * per
    K = total + EXTRA
    assert w.kept.min() > 0 and total > 3 * max(KEY, FLAT)
    assert_loops("group of hit", key_kernels=key_passes(fm, K), k_val_run_groups=flat_passes(fm, K), k_val_hit_groups=flat_passes(fm, K))
    hit_off = up(np.concatenate([[0], np.cumsum(np.tile(w.kept, reps))]), np.int64)
    locs = up(np.concatenate([np.tile(w.kept_locs, reps), np.full(EXTRA + 1, -5, np.int32)]), np.int32)
    val_off, count, text_off, group = filled(n + 1, torch.int64), filled(K, torch.int32), filled(K + 1, torch.int64), filled(K, torch.int32)
    status = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    tl, sp = np.tile(np.asarray(w.lens, np.int32), reps), ia.as_chars(stop).astype(np.uint16)
    ws = workspace(ia.lib.fmx_values_of_hits_groups_scratch_bytes(n, K, max_len), "fmx_values_of_hits_groups_scratch_bytes")
    rc = ia.lib.fmx_values_of_hits_groups_dev(fm.handle, n, tl.ctypes.data, sp.ctypes.data, len(sp), max_len, hit_off.data_ptr(), locs.data_ptr(), K,
                                              val_off.data_ptr(), count.data_ptr(), text_off.data_ptr(), group.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                              ws.numel(), stream())
    tl[:] = -9  # (the call has copied what it needs before it returns)
    sp[:] = 9
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    G1 = int(values.val_off[-1])
    G = reps * G1

    class Tiled:
        val_off = np.concatenate([[0], np.cumsum(np.tile(np.diff(values.val_off), reps))]).astype(np.int64)
        count = np.tile(values.counts, reps).astype(np.int32)
        text_off = np.concatenate([[0], np.cumsum(np.tile(np.diff(values.text_off), reps))]).astype(np.int64)

    got = dict(val_off=cut(val_off, n + 1, "val_off"), count=cut(count[:G + PAD], G, "count"), text_off=cut(text_off[:G + 1 + PAD], G + 1, "text_off"))
    check_whole(got, Tiled, ("val_off", "count", "text_off"), "%d repetitions of %d hits" % (reps, per))
    assert (count[G:].cpu().numpy() == SENT).all() and (text_off[G + 1:].cpu().numpy() == SENT).all(), "stored beyond the groups"
    g = cut(group, K, "group_of_hit")
    assert (g[total:] == -1).all(), "the slots behind the hits"
    bad = np.flatnonzero((g[:total].reshape(reps, per) != base_group).any(axis=1))
    assert len(bad) == 0, "group_of_hit differs in the repetitions %r" % bad[:8]
    assert (status.cpu().numpy() == 0).all()


# ---- g. stats-by, over the text ----
def test_stats_by_loops(hd):
    """the number patterns ("size ", "blk_", "size ") by the key patterns ("INFO ", "updated: 10."), the number patterns repeated
    with by_of alongside until their hits are more than three passes of the key grid, through the three stages (dev_by of
    tests/test_gpu_number_stats_by.py over a prebuilt block): every repetition's rows and counters are judge_by's for the base
    case, row_off the base offsets tiled and accumulated.  Passes asserted: k_by_ranges >= 3, and with it the element-wise loops
    over the slots.  The rows of a repetition are a few hundred, so three passes of k_by_rows' loop over the rows (and of
    k_by_tails' over the patterns) would cost several times the hits this test already has: only the hit loops are asserted"""
    o, fm, T = hd
    KEY, FLAT = caps(fm)
    keys, numbers, by_of, stop, max_len, permille = ["INFO ", "updated: 10."], ["size ", "blk_", "size "], [0, 0, 1], " :.", 16, (0, 500, 1000)
    m, nb, P = len(keys), len(numbers), len(permille)
    w = Where("hd16 by", o, T, keys + numbers, [], [-1] * (m + nb))
    want = judge_by(o, w, T, m, by_of, stop, max_len, permille, 0)
    key_hits = int(w.kept_off[m])
    per = int(w.kept_off[-1]) - key_hits
    reps = 3 * KEY // per + 2

    class Tiled:
        n = m + nb * reps
        kept_off = np.concatenate([w.kept_off[:m + 1], key_hits + np.cumsum(np.tile(w.kept[m:], reps))]).astype(np.int64)
        kept_locs = np.concatenate([w.kept_locs[:key_hits], np.tile(w.kept_locs[key_hits:], reps)]).astype(np.int32)
        lens = np.concatenate([w.lens[:m], np.tile(w.lens[m:], reps)]).astype(np.int32)

    slots = LEAD + key_hits + reps * per + EXTRA
    assert_loops("stats by", k_by_ranges=key_passes(fm, slots), element_wise_over_slots=flat_passes(fm, slots))
    print("rows: passes k_by_rows %d, k_by_tails %d (not asserted)" % (flat_passes(fm, reps * int(want.row_off[-1])), flat_passes(fm, nb * reps)))
    assert 0 < ia.lib.fmx_numbers_by_key_scratch_bytes(nb * reps, slots, P) < WS_LIMIT
    rc, got = dev_by(fm, Tiled, m, by_of * reps, stop, max_len, permille, 0, LEAD, EXTRA)
    assert rc == 0, (got, last_error())
    check_whole(got, want, ("first_off", "first_lines", "first_locs", "group_of_first", "val_off", "lines", "text_off", "chars"), "the key patterns' stages")
    Rb = int(want.row_off[-1])

    class Rows:
        row_off = np.concatenate([[0], np.cumsum(np.tile(np.diff(want.row_off), reps))]).astype(np.int64)
        count, min, max = np.tile(want.count, reps), np.tile(want.min, reps), np.tile(want.max, reps)
        pct = np.tile(want.pct.reshape(Rb * P), reps)
        sum_lo = np.tile(np.array([s & (2 ** 64 - 1) for s in want.sums], np.uint64), reps)
        sum_hi = np.tile(np.array([s >> 64 for s in want.sums], np.uint64), reps)
        no_key, not_number, overflow = np.tile(want.no_key, reps), np.tile(want.not_number, reps), np.tile(want.overflow, reps)

    assert Rb > 0 and want.count.sum() > 0 and max(want.sums) > 2 ** 64
    check_whole(got, Rows, ("row_off", "count", "min", "max", "pct", "sum_lo", "sum_hi", "no_key", "not_number", "overflow"),
                "%d repetitions of %d number hits" % (reps, per))
