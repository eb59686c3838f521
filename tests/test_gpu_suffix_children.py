"""The suffix table's deepest level as child lists (fmx_device.hpp: DevIndex.suffix_child_rows; fmx_api.cpp: grow_child_lists).

Where the next hashed level would pass the table's size limit and the same level fits as child lists — per string a code byte
and a first row, sorted under the slot of the string without its last character — the table is one character deeper, COMPLETE,
inside the same limit.  Counts, statuses, per-pattern LF-steps and located hits must be what they are without a table and what
the oracle says; the steps the kernel reports as executed must be exactly what a table of that depth leaves.  Options are set inside
the tests and put back in `finally`."""
import contextlib
import random

import numpy as np
import pytest

import index4j_amd as ia
import orc

pytestmark = pytest.mark.gpu

DEFAULTS = {"suffix_table": 1, "suffix_table_mb": 256, "suffix_table_chars": 8, "suffix_table_image_fraction": 8, "image_compact": 0,
            "plan_sa_min": 786432, "plan_sa_key": 2, "lf_steps_executed_only": 0}
SLOT = 16


@contextlib.contextmanager
def options(**kw):
    try:
        for k, v in kw.items():
            assert ia.lib.fmx_set_option(k.encode(), int(v)) == 0, (k, v)
        yield
    finally:
        for k in kw:
            ia.lib.fmx_set_option(k.encode(), ia._lib.ENV_OPTIONS.get(k, DEFAULTS[k]))


def strings_by_length(text, upto):
    """distinct strings of 1 .. upto characters of the text"""
    symbols, t = np.unique(np.asarray(text), return_inverse=True)
    t = t.astype(np.uint64)
    assert len(symbols) ** upto < 2 ** 63
    out, key = [], t.copy()
    for k in range(1, upto + 1):
        if k > 1:
            key = key[:-1] * np.uint64(len(symbols)) + t[k - 1:]
        out.append(len(np.unique(key)))
    return out


def hashed_bytes(strings, limit):
    """build_suffix_table's sizing: a power of two of 16-byte slots, half full at most — or 0.7 where only that fits the limit"""
    slots = 1024
    while slots < 2 * strings:
        slots *= 2
    if slots * SLOT > limit and slots // 2 >= 1024 and 10 * strings <= 7 * (slots // 2):
        slots //= 2
    return slots * SLOT


def make_patterns(text, rnd, n):
    """as test_suffix_table_changes_nothing_but_the_time makes them: 1 .. 11 characters, early ends, absent characters"""
    pats, plain = [], []
    for i in range(n):
        s0 = rnd.randrange(len(text) - 16)
        p = np.array(text[s0:s0 + rnd.randrange(1, 12)], dtype=np.uint16)
        if i % 7 == 0:
            p[rnd.randrange(len(p))] = text[rnd.randrange(len(text))]  # ends early somewhere
        if i % 17 == 0:
            p[rnd.randrange(len(p))] = 7  # absent character
        plain.append(i % 7 != 0 and i % 17 != 0)
        pats.append(p)
    return pats, np.array(plain)


def oracle_steps(o, ch, off):
    orc.counters_reset()
    cnt, st = o.count_batch(ch, off, threads=8)
    return cnt, st, orc.counters()["lf_steps"]


def check_case(text, seed, depth, limit_options, expect_statuses):
    rnd = random.Random(seed)
    o = orc.OracleFmIndex(text, 32, True)
    ser = o.write(False)
    N = 24_000
    pats, plain = make_patterns(text, rnd, N)
    ch, off = ia.pack_patterns(pats)
    oc, ost, o_steps = oracle_steps(o, ch, off)
    assert bool((ost != 0).any()) == expect_statuses
    # the same patterns cut to their last `depth` characters: what a complete table of that depth answers
    cuts = [p[-depth:] for p in pats]
    cch, coff = ia.pack_patterns(cuts)
    cut_cnt, cut_st, cut_steps = oracle_steps(o, cch, coff)
    pch, poff = ia.pack_patterns([p for p, keep in zip(pats, plain) if keep])
    pcch, pcoff = ia.pack_patterns([c for c, keep in zip(cuts, plain) if keep])
    plain_steps, plain_cut_steps = oracle_steps(o, pch, poff)[2], oracle_steps(o, pcch, pcoff)[2]

    counts = strings_by_length(text, depth)
    seen_bytes = {}
    for compact in (0, 1):
        with options(image_compact=compact, **limit_options):
            fm = ia.FmIndex.read(ser, device=0)
            k, nbytes = fm.suffix_table_info()
            image = fm.device_blob()[1]
            with options(suffix_table_chars=depth - 1):
                shallow = ia.FmIndex.read(ser, device=0)
            k_shallow, nbytes_shallow = shallow.suffix_table_info()
            shallow.close()
        # the limit these options give, and what fits it: not the hashed form of this depth, but the hashed levels below plus
        # five bytes per entry (a string of the deepest level, or the terminator of a string of the level below)
        frac, mb = limit_options.get("suffix_table_image_fraction", 8), limit_options.get("suffix_table_mb", 256)
        limit = min(mb << 20, max(image // frac, 64 << 10)) if frac else mb << 20
        below = hashed_bytes(sum(counts[1:depth - 1]), limit)
        assert hashed_bytes(sum(counts[1:depth]), limit) > limit, (limit, counts)
        if not expect_statuses:
            assert below + 5 * (counts[depth - 1] + counts[depth - 2]) + 48 <= limit, (limit, counts)
        assert k == depth and k_shallow == depth - 1, (k, k_shallow, nbytes, limit, compact)
        assert nbytes_shallow == below and nbytes_shallow < nbytes <= limit, (nbytes_shallow, nbytes, limit)
        if not expect_statuses:
            # every string occurs with its whole interval: no gaps, and a terminator per string of the level below (but the one
            # at the text's end, which nothing follows); behind the lists 32 bytes a lookup may read into, rounded up to 16
            lists = 5 * (counts[depth - 1] + counts[depth - 2])
            assert below + lists - 10 <= nbytes <= below + lists + 48, (nbytes, below, lists)
        seen_bytes[compact] = nbytes
        try:
            ref_lf = None
            # the caller's order, then the plan stage under the order-1 estimate and under the table's own answer
            for use, sa_min, sa_key in ((0, 1 << 30, 2), (1, 1 << 30, 2), (1, 0, 2), (1, 0, 1)):
                with options(suffix_table=use, plan_sa_min=sa_min, plan_sa_key=sa_key):
                    assert ia.lib.fmx_count_batch_is_planned(fm.handle, N) == (1 if (sa_min == 0 or not use) else 0)
                    cnt, st, lf = fm.count_batch(ch, off, want_steps=True)
                    assert (cnt == oc).all() and (st == ost).all(), (compact, use, sa_min, sa_key)
                    assert int(lf.astype(np.int64).sum()) == o_steps, (compact, use, sa_min, sa_key)
                    if ref_lf is None:
                        ref_lf = lf.copy()  # per pattern: the run that ignores the table
                    assert (lf == ref_lf).all(), (compact, use, sa_min, sa_key)
                    locs, found, st2 = fm.locate_batch(ch, off, 3)
                    for i in range(0, N, 97):
                        try:
                            kk, ll = o.locate(pats[i], max_matches=3, cap=3)
                            assert st2[i] == 0 and found[i] == kk and (locs[i, :kk] == ll).all(), (compact, use, sa_min, sa_key, i)
                        except IndexError:  # Q3
                            assert st2[i] == 9
                    if use and not expect_statuses:
                        with options(lf_steps_executed_only=1):
                            ex = fm.count_batch(ch, off, want_steps=True)[2].astype(np.int64)
                            pex = fm.count_batch(pch, poff, want_steps=True)[2].astype(np.int64)
                        # patterns as the text has them: the oracle's total minus its total for the patterns cut to `depth` characters
                        assert int(pex.sum()) == plain_steps - plain_cut_steps, (compact, sa_min, sa_key)
                        # every pattern: a cut that occurs is answered whole (2 ranks per character after its first), any other
                        # cut is not in the table and the loop runs from the last character
                        answered = np.where(cut_cnt > 0, 2 * (np.minimum(np.diff(off), depth) - 1), 0)
                        assert (ex == ref_lf.astype(np.int64) - answered).all(), (compact, sa_min, sa_key)
        finally:
            fm.close()
    return seen_bytes


def test_one_more_complete_level_inside_the_same_limit_on_a_log():
    """synth_log(2^22): 533 / 3,224 / 25,710 strings of 2 / 3 / 4 characters.  Under a limit of about 600 KB the hashed table
    stops at 3 characters (131 KB; 4 characters hashed take 1 MB) and the child lists give 4 (about 145 KB more); with
    suffix_table_chars = 3 the table is the hashed one alone.  24,000 patterns of 1 .. 11 characters in the caller's order and
    planned (both SA-row orders), expanded and compact image: counts, statuses, per-pattern LF-steps, located hits of a sample;
    executed steps = the oracle's total minus its total for the patterns cut to their last 4 characters."""
    text = ia.synth_log(1 << 22)
    fm = ia.FmIndex(text, 32, True, device=0)
    image = fm.device_blob()[1]
    fm.close()
    frac = max(1, image // (600 << 10))  # limit = image / frac: between 600 KB and 1 MB - 1 while the image has 1.2 MB or more
    assert (600 << 10) <= image // frac < (1 << 20), (image, frac)
    seen = check_case(text, 4242, 4, {"suffix_table_mb": 256, "suffix_table_image_fraction": frac}, expect_statuses=False)
    assert set(seen) == {0, 1}


def test_child_lists_beside_strings_that_were_dropped_for_a_status():
    """12 random symbols over 2^20 - 1 characters: the index is 2^20 long, rank(size) raises in the JVM (Q3) and the strings whose
    search meets it are not tabulated — among them parents of strings that are: their lists hang on slots without an interval.
    A 4 MB budget holds 4 characters hashed (1 MB; 5 take 8 MB) and the 245,065 strings of 5 as child lists."""
    rnd = random.Random(77)
    text = np.array([rnd.randrange(33, 33 + 12) for _ in range((1 << 20) - 1)], dtype=np.uint16)
    check_case(text, 4243, 5, {"suffix_table_mb": 4, "suffix_table_image_fraction": 0}, expect_statuses=True)
