"""Plain numpy judges for the two device stages whose inputs can be synthesised: the top values of a field per bucket of lines
(fmx_values_top_histogram_dev + fmx_values_gather_rows_dev) and the first hit of every line (fmx_first_hits_of_lines_dev).  They
take what the stages take — a packed block of slots, the groups as plain arrays, the line table — and nothing of the library under
test, so that a test may hand the stages millions of made-up hits.

tests/test_stage_judges_cpu.py holds them to the oracle-based judges (judge_top_hist, judge_by) on the fixture;
tests/test_gpu_stage_loops.py holds the kernels to them."""
import numpy as np


class Answer:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def slot_patterns(hit_off, n_slots):
    """(first, total, the pattern of every hit slot in [first, total)): the slots in front of hit_off[0], behind hit_off[n] and
    beyond n_slots are no hits"""
    off = np.clip(np.asarray(hit_off, np.int64), 0, n_slots)
    return int(off[0]), int(off[-1]), np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))


def lines_of(T, locs):
    """a hit belongs to the line of its first character: the number of boundaries in front of it (tests/test_match_lines_cpu.py)"""
    return np.searchsorted(np.asarray(T), locs, side="left").astype(np.int64)


def buckets_of(edges, lines):
    """fm_hist_bucket's rule, as judge_bins has it: the last edge at or below the line; -1 where the line lies below edges[0] or at
    or beyond the last edge.  edges None: one bucket that holds every line"""
    if edges is None:
        return np.zeros(len(lines), np.int64), 1
    edges = np.asarray(edges, np.int64)
    B = len(edges) - 1
    b = np.searchsorted(edges, lines, side="right") - 1
    return np.where((b >= 0) & (b < B), b, -1), B


def np_top_hist(hit_off, locs, n_slots, val_off, count, group_of_hit, edges, top, T, text_off=None, chars=None):
    """hit_off: n + 1 slots of a block of n_slots; locs, group_of_hit: per slot; val_off: n + 1; count: per group; text_off / chars:
    the text of ALL groups (None: no gather).  Returns row_off, row_group, row_count, hist (R, B), other (n, B), codes (per hit
    slot), buckets (per hit slot, -1: none) and, with text, row_text_off and row_chars"""
    val_off, count = np.asarray(val_off, np.int64), np.asarray(count, np.int64)
    n = len(val_off) - 1
    first, total, pat = slot_patterns(hit_off, n_slots)
    groups = np.diff(val_off)
    row_off = np.concatenate([[0], np.cumsum(np.minimum(groups, top))]).astype(np.int64)
    R = int(row_off[n])
    rank = np.zeros(int(val_off[n]), np.int64)
    row_group, row_count = np.zeros(R, np.int32), np.zeros(R, np.int32)
    for i in np.flatnonzero(groups):
        a, b = int(val_off[i]), int(val_off[i + 1])
        order = np.argsort(-count[a:b], kind="stable")  # descending by count, ties by ascending group index
        rank[a + order] = np.arange(b - a)
        rows = order[:top]
        row_group[row_off[i]:row_off[i + 1]] = rows
        row_count[row_off[i]:row_off[i + 1]] = count[a:b][rows]
    g = np.asarray(group_of_hit)[first:total].astype(np.int64)
    inside = (g >= 0) & (g < groups[pat])
    codes = np.full(len(g), top, np.int64)  # the rank of the hit's group; top: "other"
    codes[inside] = np.minimum(rank[(val_off[pat] + g)[inside]], top)
    lines = lines_of(T, np.asarray(locs)[first:total]) if edges is not None else np.zeros(total - first, np.int64)
    buckets, B = buckets_of(edges, lines)
    binned = buckets >= 0
    row_hit = binned & (codes < top)
    hist = np.bincount(((row_off[pat] + codes) * B + buckets)[row_hit], minlength=R * B).astype(np.int32).reshape(R, B)
    other_hit = binned & (codes == top)
    other = np.bincount((pat * B + buckets)[other_hit], minlength=n * B).astype(np.int32).reshape(n, B)
    out = Answer(n=n, B=B, top=top, row_off=row_off, row_group=row_group, row_count=row_count, hist=hist, other=other, codes=codes, buckets=buckets,
                 patterns=pat, n_values=groups.astype(np.int32))
    if text_off is not None:
        text_off, chars = np.asarray(text_off, np.int64), np.asarray(chars)
        src = val_off[np.repeat(np.arange(n), np.diff(row_off))] + row_group
        out.row_text_off = np.concatenate([[0], np.cumsum((text_off[1:] - text_off[:-1])[src])]).astype(np.int64)
        out.row_chars = np.concatenate([chars[text_off[s]:text_off[s + 1]] for s in src] + [chars[:0]])
    return out


def np_first_hits(hit_off, locs, n_slots, T):
    """per pattern its distinct lines ascending and the smallest position of a hit on each: first_off (m + 1), first_lines,
    first_locs"""
    m = len(hit_off) - 1
    first, total, pat = slot_patterns(hit_off, n_slots)
    loc = np.asarray(locs)[first:total].astype(np.int64)
    line = lines_of(T, loc)
    order = np.lexsort((loc, line, pat))
    pair = (pat * (len(T) + 1) + line)[order]  # (pattern, line), ascending; within a pair the positions ascend
    _, head = np.unique(pair, return_index=True)
    per = np.bincount(pat[order][head], minlength=m)
    return Answer(first_off=np.concatenate([[0], np.cumsum(per)]).astype(np.int64), first_lines=line[order][head].astype(np.int32),
                  first_locs=loc[order][head].astype(np.int32))
