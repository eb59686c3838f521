"""tests/plan_model.py — the reference the GPU plan-order test compares the device with — checked without a GPU, so that it cannot
drift unnoticed: its code key against a sort of character tuples, its SA ranges against the oracle's count(), its cumulativeCounts
against a direct count, its shapes against values worked out by hand from sort_shape()."""
import os
import random

import numpy as np
import pytest

import orc
import plan_model as pm
from common import GOLDEN, hdfs_text


def _texts():
    synth = np.frombuffer(open(os.path.join(GOLDEN, "synth_64k.txt"), "rb").read(), dtype=np.uint8).astype(np.uint16)
    hdfs = orc.u16(hdfs_text())
    return {"synth_64k": synth, "hdfs_multichar": hdfs}


def _codes_by_first_appearance(text):
    """FM:396-435, restated with a dict: the sentinel is 0, a character's code the next free one at its first appearance"""
    code = {}
    for c in text.tolist():
        if c != 0:
            code.setdefault(c, len(code) + 1)
    return code


def _substrings(text, rnd, n, lo, hi):
    return [text[s:s + rnd.randrange(lo, hi + 1)] for s in (rnd.randrange(len(text) - hi - 1) for _ in range(n))]


def _pack(pats):
    off = np.zeros(len(pats) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(p) for p in pats])
    ch = np.concatenate([np.asarray(p, dtype=np.uint16) for p in pats]) if off[-1] else np.zeros(0, np.uint16)
    return ch, off


@pytest.mark.parametrize("name", ["synth_64k", "hdfs_multichar"])
@pytest.mark.parametrize("code_bits_12", [1, 0])
def test_code_key_orders_patterns_by_their_reversed_trailing_characters(name, code_bits_12):
    text = _texts()[name]
    rnd = random.Random(5)
    al = pm.Alphabet(text)
    pats = _substrings(text, rnd, 3000, 0, 12)
    for k in range(0, len(pats), 50):  # an absent character at a random place, the last among them
        if len(pats[k]):
            pats[k] = pats[k].copy()
            pats[k][rnd.choice([len(pats[k]) - 1, rnd.randrange(len(pats[k]))])] = 0x7A7B
    ch, off = _pack(pats)
    sh = pm.Shape(al.sigma, sort_bits=32, code_bits_12=code_bits_12)  # 32: as many whole characters as a key holds
    assert (1 << sh.bits) >= al.sigma and sh.chars == min(32 // sh.bits, 64 // sh.code_bits) and sh.chars >= 2
    words = pm.code_words(al, ch, off, sh.code_bits)
    keys = pm.code_keys(words, sh)
    code = _codes_by_first_appearance(text)
    # the word itself: code of the j-th character from the end at bits j * code_bits
    for i in (0, 1, 7, 50, 100, 2999):
        p = pats[i]
        want = 0
        for j in range(min(len(p), 64 // sh.code_bits)):
            want |= code.get(int(p[len(p) - 1 - j]), 0) << (j * sh.code_bits)
        assert int(words[i]) == want, (i, hex(int(words[i])), hex(want))
    tuples = [tuple(code.get(int(c), 0) for c in p[::-1][:sh.chars]) + (0,) * max(0, sh.chars - len(p)) for p in pats]
    by_tuple = sorted(range(len(pats)), key=lambda i: tuples[i])  # (stable, like the argsort)
    by_key = np.argsort(keys, kind="stable").tolist()
    assert by_key == by_tuple
    assert (pm.length_field(pm.lengths(off)) == [len(p) for p in pats]).all()
    assert pm.length_field([0, 5, 0x3FFFFE, 0x3FFFFF, 0x400000, 1 << 30]).tolist() == [0, 5, 0x3FFFFE, 0x3FFFFF, 0x3FFFFF, 0x3FFFFF]


def test_bins_are_cuts_of_the_key():
    sh = pm.Shape(70, sort_bits=28, coarse_bits=12)
    keys = np.array([0, 1, 0xFFFF, 0x10000, 0x0ABCDEF0, (1 << 28) - 1, 0xFFFFFFFF], dtype=np.uint32)
    assert (sh.below, sh.fine_shift, sh.bins) == (16, 8, 4096)
    assert pm.coarse_bin(keys, sh).tolist() == [0, 0, 0, 1, 0xABC, 4095, 4095]  # (the last: above 2^total_bits, clamped)
    assert pm.fine_bin(keys, sh).tolist() == [0, 0, 0xFF, 0x100, 0xBCDEF0 >> 8 & 1023, 1023, 1023]


def test_sa_ranges_against_the_oracle_count():
    text = _texts()["synth_64k"]
    rnd = random.Random(9)
    al = pm.Alphabet(text)
    assert al.sigma <= 256
    rows = pm.SaRows(al, text, 8)
    o = orc.OracleFmIndex(text, 32, True)
    assert o.getInputLength() == al.text_length and o.getAlphabetLength() == al.sigma
    pats = {p.tobytes(): p for p in _substrings(text, rnd, 4000, 1, 8)}
    for _ in range(300):  # strings that do not occur, and strings with an absent character
        p = np.array([rnd.choice(al.symbols.tolist()) for _ in range(rnd.randrange(2, 9))], dtype=np.uint16)
        pats.setdefault(p.tobytes(), p)
        q = p.copy()
        q[rnd.randrange(len(q))] = 0x7A7B
        pats.setdefault(q.tobytes(), q)
    pats = list(pats.values())
    ch, off = _pack(pats)
    counts, status = o.count_batch(ch, off)
    assert (status == 0).all()
    words = pm.code_words(al, ch, off, 8)
    start, end = rows.ranges_of_words(words, pm.lengths(off))
    bad = np.flatnonzero(end - start != counts)
    assert len(bad) == 0, "SA range and oracle count differ at %r" % bad[:5]
    assert (counts == 0).sum() >= 300 and (counts > 0).sum() >= 1000
    assert ((0 <= start) & (start <= end) & (end <= al.text_length)).all()
    # start is the number of suffixes of text + sentinel that sort before the string BY CODE: a direct count over a few strings
    code = _codes_by_first_appearance(text)
    t = bytes(code[c] for c in text.tolist()) + b"\0"
    for i in rnd.sample(range(len(pats)), 25):
        p = bytes(code.get(c, 0) for c in pats[i].tolist())
        before = sum(1 for k in range(len(t)) if t[k:k + len(p)] < p)
        assert before == start[i], (p, before, int(start[i]))
        assert rows.range_of(al.codes(pats[i])) == (int(start[i]), int(end[i]))


def test_start_of_a_single_character_is_its_cumulative_count():
    for text in _texts().values():
        al = pm.Alphabet(text)
        rows = pm.SaRows(al, text, pm.code_bits_for(al.sigma))
        code = _codes_by_first_appearance(text)
        assert al.sigma == len(code) + 1
        for sym in al.symbols[:: max(1, len(al.symbols) // 97)].tolist() + [int(al.symbols[-1])]:
            c = int(al.codes([sym])[0])
            assert c == code[sym]
            smaller = 1 + sum(int((text == other).sum()) for other, k in code.items() if k < c)  # (+ the sentinel)
            s, e = rows.range_of([c])
            assert s == smaller == al.C[c] and e == al.C[c + 1] and e - s == int((text == sym).sum())
        assert rows.range_of([0]) == (0, 0)  # an absent character: nothing, in front


# (bits, chars, total_bits, coarse_bits, below, fine_shift, code_bits) by hand from sort_shape():
# bits = ceil(log2 sigma); chars = max(1, sort_bits / bits) capped at 64 / code_bits; coarse = min(total, coarse_bits)
SHAPES = {
    # sigma 70: 7 bits, 8-bit codes
    (70, 1, 4): (7, 1, 7, 4, 3, 0, 8), (70, 1, 12): (7, 1, 7, 7, 0, 0, 8), (70, 1, 13): (7, 1, 7, 7, 0, 0, 8),
    (70, 9, 4): (7, 1, 7, 4, 3, 0, 8), (70, 9, 12): (7, 1, 7, 7, 0, 0, 8), (70, 9, 13): (7, 1, 7, 7, 0, 0, 8),
    (70, 28, 4): (7, 4, 28, 4, 24, 16, 8), (70, 28, 12): (7, 4, 28, 12, 16, 8, 8), (70, 28, 13): (7, 4, 28, 13, 15, 7, 8),
    (70, 32, 4): (7, 4, 28, 4, 24, 16, 8), (70, 32, 12): (7, 4, 28, 12, 16, 8, 8), (70, 32, 13): (7, 4, 28, 13, 15, 7, 8),
    # sigma 200: 8 bits, 8-bit codes
    (200, 1, 4): (8, 1, 8, 4, 4, 0, 8), (200, 1, 12): (8, 1, 8, 8, 0, 0, 8), (200, 1, 13): (8, 1, 8, 8, 0, 0, 8),
    (200, 9, 4): (8, 1, 8, 4, 4, 0, 8), (200, 9, 12): (8, 1, 8, 8, 0, 0, 8), (200, 9, 13): (8, 1, 8, 8, 0, 0, 8),
    (200, 28, 4): (8, 3, 24, 4, 20, 12, 8), (200, 28, 12): (8, 3, 24, 12, 12, 4, 8), (200, 28, 13): (8, 3, 24, 13, 11, 3, 8),
    (200, 32, 4): (8, 4, 32, 4, 28, 20, 8), (200, 32, 12): (8, 4, 32, 12, 20, 12, 8), (200, 32, 13): (8, 4, 32, 13, 19, 11, 8),
    # sigma 1,100 (1,099 symbols + the sentinel): 11 bits, 12-bit codes
    (1100, 1, 4): (11, 1, 11, 4, 7, 0, 12), (1100, 1, 12): (11, 1, 11, 11, 0, 0, 12), (1100, 1, 13): (11, 1, 11, 11, 0, 0, 12),
    (1100, 9, 4): (11, 1, 11, 4, 7, 0, 12), (1100, 9, 12): (11, 1, 11, 11, 0, 0, 12), (1100, 9, 13): (11, 1, 11, 11, 0, 0, 12),
    (1100, 28, 4): (11, 2, 22, 4, 18, 10, 12), (1100, 28, 12): (11, 2, 22, 12, 10, 2, 12), (1100, 28, 13): (11, 2, 22, 13, 9, 1, 12),
    (1100, 32, 4): (11, 2, 22, 4, 18, 10, 12), (1100, 32, 12): (11, 2, 22, 12, 10, 2, 12), (1100, 32, 13): (11, 2, 22, 13, 9, 1, 12),
}


def test_shapes_worked_out_by_hand():
    for (sigma, sort_bits, coarse_bits), want in SHAPES.items():
        got = pm.Shape(sigma, sort_bits, coarse_bits).as_tuple()
        assert got == want, ((sigma, sort_bits, coarse_bits), got, want)
    # 16-bit codes where 12 are switched off: nothing else moves while chars <= 4
    assert pm.Shape(1100, 28, 12, code_bits_12=0).as_tuple() == (11, 2, 22, 12, 10, 2, 16)
    assert pm.Shape(5000, 32, 12).as_tuple() == (13, 2, 26, 12, 14, 6, 16)
    # the SA-row key: total_bits = bits of a row number of a text of 2^20 characters + the sentinel; only with a table
    sa = pm.Shape(70, 28, 12, plan_sa_key=2, has_table=True, text_length=(1 << 20) + 1)
    assert (sa.sa_key, sa.total_bits, sa.coarse_bits, sa.below, sa.fine_shift) == (2, 21, 12, 9, 1)
    sa = pm.Shape(70, 28, 13, plan_sa_key=1, has_table=True, text_length=1 << 20)
    assert (sa.sa_key, sa.total_bits, sa.coarse_bits, sa.below, sa.fine_shift) == (1, 21, 13, 8, 0)
    sa = pm.Shape(70, 28, 4, plan_sa_key=1, has_table=True, text_length=(1 << 20) - 1)
    assert (sa.sa_key, sa.total_bits, sa.coarse_bits, sa.below, sa.fine_shift) == (1, 20, 4, 16, 8)
    no = pm.Shape(70, 28, 12, plan_sa_key=2, has_table=False, text_length=(1 << 20) + 1)
    assert (no.sa_key,) + no.as_tuple() == (0, 7, 4, 28, 12, 16, 8, 8)


def test_ulp32():
    assert pm.ulp32(1) == 1.0 and pm.ulp32((1 << 24) - 1) == 1.0 and pm.ulp32(1 << 24) == 2.0 and pm.ulp32(1 << 21) == 1.0
    assert pm.ulp32((1 << 26) + 5) == 8.0
