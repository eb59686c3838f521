"""The numpy judges of tests/stage_judges.py against the oracle-based judges, on the CPU: np_top_hist must give exactly what
judge_top_hist gives (tests/test_field_values_histogram_cpu.py) on the fixture cases that file judges, fed judge_top_hist's own
groups (val_off, counts, group_of_hit, the groups' text); np_first_hits must give what judge_by derives for the key patterns
(tests/test_number_stats_by_cpu.py).  The oracle judges the judge: nothing here touches the library under test beyond as_chars and
pack_patterns inside the older judges."""
import numpy as np
import pytest

import orc
from common import hdfs_text
from stage_judges import np_first_hits, np_top_hist
from test_field_values_histogram_cpu import Hits, check_top_hist, judge_top_hist, judged
from test_field_values_where_cpu import EVERY_LINE, Where
from test_line_histogram_cpu import EDGES_250, EDGES_BEYOND, EDGES_UNEVEN
from test_match_lines_cpu import judge_table
from test_number_stats_by_cpu import EDGE_KEYS, EDGE_NUMBERS, edge_text, judge_by

HD = hdfs_text()
ALL_EDGES = (None, EDGES_250, EDGES_UNEVEN, EDGES_BEYOND)
TERMINATING = [dict(all=["terminating"])]
BLK_NOT_RESPONDER = [dict(all=["blk_"], none=["PacketResponder"])]
# (patterns, queries, where_of, stop, max_len): the batches test_field_values_histogram_cpu.py judges
BATCHES = [
    (["INFO "], [], [-1], " :", 64),
    (["INFO "], BLK_NOT_RESPONDER, [0], " :", 64),
    ([" from /10."], [], [-1], ".", 64),
    (["WARN "], [], [-1], " :", 64),                                          # ties across the cut
    (["WARN ", "INFO "], [], [-1, -1], " :", 64),
    ([" from /10.25", "zzzq#", "INFO dfs.FSNamesystem"], [], [-1, -1, -1], "01:", 64),  # every hit one value, a hitless pattern
    (["blk_"], TERMINATING, [0], " \t\r\n", 32),                              # every hit its own value
]
EMPTY_AND_HITLESS = ([" ", "blk_", "zzzq#", "", "1"], TERMINATING, [-1, 0, -1, -1, 0], " \n", 16)


@pytest.fixture(scope="module")
def hd():
    o = orc.OracleFmIndex(HD, 16, True)
    return o, judge_table(o, "\n")


def agree(hits, want, T, edges, top, what, lead=0, extra=0):
    """np_top_hist over the hits as a packed block with `lead` slots in front and `extra` behind, against the judge's answer"""
    total = int(hits.kept_off[-1])
    locs = np.concatenate([np.full(lead, -5, np.int32), hits.kept_locs, np.full(extra, -5, np.int32)])
    group = np.concatenate([np.full(lead, -7, np.int32), want.group_of_hit, np.full(extra, -7, np.int32)])
    got = np_top_hist(hits.kept_off + lead, locs, lead + total + extra, want.val_off, want.counts, group, edges, top, T, want.values.text_off,
                      want.values.chars)
    check_top_hist(dict(row_off=got.row_off, row_group=got.row_group, row_count=got.row_count, hist=got.hist, other=got.other, text_off=got.row_text_off,
                        chars=got.row_chars), want, what)
    assert got.hist.shape == want.hist.shape and got.other.shape == want.other.shape and (got.n_values == want.n_values).all(), what
    return got


def test_top_hist_judge_on_the_fixture(hd):
    """every batch at every edge shape (None, EDGES_250, EDGES_UNEVEN, EDGES_BEYOND) and top 1, 3 and 65,536, the window of the
    Where being the span of the edges as in the host form; with slots in front of and behind the hits"""
    o, T = hd
    cases = 0
    for patterns, queries, where_of, stop, max_len in BATCHES:
        for edges in ALL_EDGES:
            for top in (1, 3, 65536):
                w, want = judged("hd16 top", o, T, patterns, queries, where_of, edges, top, stop, max_len)
                what = "%r, %s edges, top %d" % (patterns, None if edges is None else len(edges), top)
                hits = Hits(w.kept_off, w.kept_locs, w.lens)
                agree(hits, want, T, edges, top, what)
                agree(hits, want, T, edges, top, what + ", slots around", lead=3, extra=70)
                cases += 1
    assert cases == len(BATCHES) * 4 * 3


def test_top_hist_judge_on_the_empty_and_the_hitless_pattern(hd):
    """the batch with an empty pattern (status 9, no hits) and a hitless one between patterns with hits: every edge shape at the
    top = 6 of test_field_values_histogram_cpu.py (one judgement per case for both files), top 1, 3 and 65,536 at the uneven edges"""
    o, T = hd
    patterns, queries, where_of, stop, max_len = EMPTY_AND_HITLESS
    for edges, top in [(e, 6) for e in ALL_EDGES] + [(EDGES_UNEVEN, t) for t in (1, 3, 65536)]:
        w, want = judged("hd16 top", o, T, patterns, queries, where_of, edges, top, stop, max_len)
        assert want.n_values[2] == 0 and want.n_values[3] == 0 and want.n_values[1] > 0 and want.n_values[4] > 0
        agree(Hits(w.kept_off, w.kept_locs, w.lens), want, T, edges, top, "empty and hitless, top %d" % top, lead=7, extra=9)


def test_top_hist_judge_on_hits_in_no_bucket(hd):
    """hits that were NOT cut to the span of the edges: counted in their row's count and in no counter; and fewer slots than hits"""
    o, T = hd
    w = Where("hd16 top", o, T, ["INFO ", "WARN "], [], [-1, -1], EVERY_LINE)
    for edges in ALL_EDGES:
        for top in (1, 3, 65536):
            hits = Hits(w.kept_off, w.kept_locs, w.lens)
            want = judge_top_hist(o, T, hits, edges, top, " :", 64)
            got = agree(hits, want, T, edges, top, "hits outside the span, top %d" % top, lead=2, extra=3)
            if edges is EDGES_UNEVEN:
                assert (got.hist.sum(axis=1) < got.row_count).any() and (got.buckets < 0).any()
    for n_hits in (0, 1, 1023, 1024, 1025, 2049):
        cut = Hits(w.kept_off, w.kept_locs, w.lens, n_hits)
        agree(cut, judge_top_hist(o, T, cut, EDGES_250, 2, " :", 64), T, EDGES_250, 2, "%d slots" % n_hits, lead=1 if n_hits else 0, extra=2)


def first_hits_agree(w, want, T, m, what):
    total = len(w.kept_locs)
    key_end = int(w.kept_off[m])
    for lead, n_slots in ((0, total), (0, key_end), (3, 3 + key_end + 70)):  # the number hits behind hit_off[m] are no hits of this stage
        locs = np.concatenate([np.full(lead, -5, np.int32), w.kept_locs, np.full(73, -5, np.int32)])
        got = np_first_hits(w.kept_off[:m + 1] + lead, locs, n_slots, T)
        for name in ("first_off", "first_lines", "first_locs"):
            a, b = getattr(got, name), getattr(want, name)
            assert a.shape == b.shape and (a == b).all(), "%s: %s" % (what, name)


def test_first_hits_judge(hd):
    """the fixture's key patterns and the edge text's (two key hits on one line, a key pattern without a hit, as many groups as
    lines) against judge_by's first_off / first_lines / first_locs"""
    o, T = hd
    for keys, numbers, by_of, stop, max_len in ((["INFO ", "updated: 10."], ["size ", "blk_", "size "], [0, 0, 1], " :.", 16),
                                                (["updated: 10."], ["size "], [0], ".:", 32), ([" from /10."], ["size "], [0], ".", 32)):
        w = Where("hd16 by", o, T, keys + numbers, [], [-1] * (len(keys) + len(numbers)))
        first_hits_agree(w, judge_by(o, w, T, len(keys), by_of, stop, max_len), T, len(keys), repr(keys))
    text = edge_text()
    eo = orc.OracleFmIndex(text, 8, True)
    eT = judge_table(eo, "\n")
    w = Where("edge", eo, eT, EDGE_KEYS + EDGE_NUMBERS, [], [-1] * (len(EDGE_KEYS) + len(EDGE_NUMBERS)))
    want = judge_by(eo, w, eT, len(EDGE_KEYS), [0, 0, 0], " \n", 32)
    assert want.first_off[4] == want.first_off[3] and len(want.first_lines) < w.kept_off[len(EDGE_KEYS)]  # a hitless pattern; a line with two key hits
    first_hits_agree(w, want, eT, len(EDGE_KEYS), "the edge text")
