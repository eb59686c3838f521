"""Texts at the edges of the line table's and the sort keys' geometry, and a judge that works from the text alone.

The line-stack kernels (fmx_hit_lines.hip, fmx_query_lines.hip, fmx_sequence_lines.hip, fmx_hit_values.hip, the packed extract) are
steered by the text's GEOMETRY: `count` (the entries of the line table T: the fence shift, the fences staged, fm_bits(count) and so
the end bit of the device-wide sorts), where the boundaries stand (position 0, none, nothing else, none at the end), hits that
overlap and run into textLength (texts of period 1 and 2), and code units at and above 0x8000.  CASES names one small text per
edge, each with a batch of patterns cut from the text itself and padded with absent patterns to a size that moves fm_bits(n) and
puts more than kLocateAllSlice = 2048 hitless patterns between two patterns with hits.  Everything is generated from fixed seeds.

The judge never looks at the code under test, nor at the oracle: occurrences by str.find, lines by bisect over the boundary
positions, queries by the set formula of fmx.h, sequences by Python's re (non-greedy, line by line), values by slicing into a
collections.Counter.  A text is a Python str whose characters are UTF-16 code units one to one (lone surrogates included, so a str
cannot be encoded: units() gives the array).  tests/test_text_geometry_cpu.py proves the judge against the oracle and the host
mirrors; tests/test_gpu_text_geometry.py runs the kernels against it."""
import bisect
import collections
import random
import re

import numpy as np

import index4j_amd as ia

NL = "\n"
ABSENT = 0x7A7B  # a character no text of the suite holds
HIGH = (0x0001, 0x007F, 0x7FFF, 0x8000, 0xD800, 0xDFFF, 0xFFFF)  # (never 0xFFFE: the suites' SENT16)
PARTNER = {0x7FFF: 0x8000, 0x8000: 0x7FFF, 0xD800: 0xDFFF, 0xDFFF: 0xD800, 0x0001: 0x007F, 0x007F: 0x0001}
COUNT_KS = (1, 2, 3, 4095, 4096, 4097, 8191, 8192, 8193, 16385, 32767, 32768, 32769)
ALPHA6 = "abcABC"
BATCH_SIZES = (2047, 2048, 2049, 4097)
SLICE, TILE = 2048, 1024  # kLocateAllSlice, kLocateAllTile of index4j_amd/csrc/fmx_device.hpp
KINDS = ((0,), (1, 1), (0, 1, 2), (), (0, 2))  # PackedBatch.KINDS of tests/test_gpu_concurrency.py
HIGH_PREFIX = "\x7f\x01\x7f"
HIGH_BASE = "".join(chr(HIGH[(3 * j + 1) % 7]) for j in range(10))
CHUNK_EDGES = (3, 4, 7, 8)  # the offsets test_synthetic_texts of tests/test_field_values_cpu.py names
RESIDENT = ("count_4097", "count_8193", "count_32768", "period1", "high_units")  # the texts that run on every residency


def units(s):
    """str -> uint16 code units, one per character"""
    return np.fromiter(map(ord, s), np.uint16, len(s))


def count_text(K, closed):
    rnd = random.Random(1000 + K)
    lines = ["".join(rnd.choices(ALPHA6, k=rnd.randint(1, 3))) for _ in range(K + 1)]
    return NL.join(lines[:K]) + NL if closed else NL.join(lines)


def high_variants():
    return [HIGH_BASE] + [HIGH_BASE[:k] + chr(u) + HIGH_BASE[k + 1:] for k in CHUNK_EDGES for u in HIGH if chr(u) != HIGH_BASE[k]]


def high_text():
    rnd = random.Random(77)
    word = lambda: "".join(chr(u) for u in rnd.choices(HIGH[:1] + HIGH[2:], k=rnd.randint(3, 12)))  # (no 0x007F: the prefix stands only where it is put)
    variants = high_variants()
    order = list(range(len(variants))) * 12
    rnd.shuffle(order)
    return "".join("%s\x01%s\x01%s%s\n" % (word(), word(), HIGH_PREFIX, variants[v]) for v in order)


def period_text(unit, total, every):
    s = unit * (total // len(unit))
    return NL.join(s[a:a + every] for a in range(0, len(s), every))


def _texts():
    rnd = random.Random(5)
    out = collections.OrderedDict()
    out["no_boundary"] = "".join(rnd.choices("abcde", k=5000))
    out["only_boundary"] = NL
    out["only_boundary_no_hits"] = NL
    out["single_a"] = "a"
    out["a_boundary"] = "a\n"
    out["boundary_a"] = "\na"
    out["empty_lines"] = NL * 5000
    body = "".join(rnd.choices("abcd\n", k=3000)).replace("\n\n\n", "\nx\n")
    out["leading_and_double"] = "\n\n" + body + "ab\n\ncd" + body[::-1] + "dc"
    for K in COUNT_KS:
        out["count_%d" % K] = count_text(K, True)
        out["count_%d_open" % K] = count_text(K, False)
    g = rnd.choices("ab", k=65536)
    g[32768] = NL
    out["giant_line"] = "".join(g)
    out["period1"] = period_text("a", 4000, 997)
    out["period2"] = period_text("ab", 8000, 1001)
    out["high_units"] = high_text()
    return out


def boundaries(text):
    return [i for i, c in enumerate(text) if c == NL]


def n_lines_of(text):
    """one line behind the last boundary unless the text ends in one (or is empty)"""
    return text.count(NL) + (1 if text and not text.endswith(NL) else 0)


def occurrences(text, pattern):
    """every position of `pattern` in `text`, overlapping ones included; the empty pattern has none (the reference throws)"""
    out = []
    if pattern:
        at = text.find(pattern)
        while at >= 0:
            out.append(at)
            at = text.find(pattern, at + 1)
    return np.array(out, np.int32)


def classes_of(pattern):
    """the class form of a literal: per code unit its spellings in any case (ia.ignore_case), its PARTNER among the high units,
    and, where that leaves the unit alone, a character the text does not hold"""
    out = []
    for ch, spelt in zip(pattern, ia.ignore_case(units(pattern))):
        alts = spelt + (chr(PARTNER[ord(ch)]) if ord(ch) in PARTNER else "")
        out.append([ord(c) for c in (alts if len(alts) > 1 else alts + chr(ABSENT))])
    return out


def class_occurrences(text, classes, u=None):
    """positions where every unit lies in its position's class, by numpy over the code units (u = units(text))"""
    if not classes or len(classes) > len(text) or not all(any(chr(a) in text for a in alts) for alts in classes):
        return np.zeros(0, np.int32)
    u = units(text) if u is None else u
    m = len(u) - len(classes) + 1
    ok = np.ones(m, bool)
    for j, alts in enumerate(classes):
        ok &= np.isin(u[j:j + m], np.array(alts, np.uint16))
    return np.flatnonzero(ok).astype(np.int32)


def class_regex(classes):
    return "".join("[" + "".join(re.escape(chr(a)) for a in alts) + "]" for alts in classes)


def lines_of_hits(T, hits):
    """the distinct lines of a pattern's hits, ascending: a hit belongs to the line of its first character"""
    return sorted({bisect.bisect_left(T, int(h)) for h in hits})


def packed(lists, dtype=np.int32):
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return np.array([v for x in lists for v in x], dtype), off


def cut(lists, max_lines):
    """(lines, line_off, line_count) under a limit"""
    kept = [x[:max_lines] if max_lines > 0 else x for x in lists]
    lines, off = packed(kept)
    return lines, off, np.array([len(x) for x in lists], np.int32)


def query_cut(n):
    """n terms cut into queries of ALL / ANY / NONE terms as tests/test_gpu_concurrency.py cuts them: (query_off, kinds)"""
    kinds, query_off = [], [0]
    while len(kinds) < n:
        kinds += KINDS[(len(query_off) - 1) % len(KINDS)]
        query_off.append(min(len(kinds), n))
    return np.array(query_off, np.int32), np.array(kinds[:n], np.uint8)


def query_lines(per_term, query_off, kinds):
    """the set formula of fmx.h: all the ALL terms, one of the ANY terms if there are any, no NONE term; nothing without ALL and ANY"""
    out = []
    for Q in range(len(query_off) - 1):
        terms = range(query_off[Q], query_off[Q + 1])
        alls, anys, nones = ([set(per_term[t]) for t in terms if kinds[t] == k] for k in (0, 1, 2))
        res = set()
        if alls or anys:
            res = set.intersection(*alls) if alls else set.union(*anys)
            if alls and anys:
                res &= set.union(*anys)
            res = res.difference(*nones)
        out.append(sorted(res))
    return out


def sequence_lines(text, regexes):
    """(lines, spans) of one sequence by re, line by line: t_0.*?t_1.*? ... at its leftmost start, from there the earliest end; a
    sequence without terms, or with an empty term, has no lines.  (A line that lacks one of the terms is passed over before the
    whole expression runs: that search fails anyway, only slowly.)"""
    if not regexes or not all(regexes):
        return [], []
    each = [re.compile(r, re.S) for r in set(regexes)]
    if not all(r.search(text) for r in each):
        return [], []
    rx = re.compile(".*?".join(regexes), re.S)
    lines, spans, at = [], [], 0
    for k, ln in enumerate(text.split(NL)[:n_lines_of(text)]):
        m = rx.search(ln) if all(r.search(ln) for r in each) else None
        if m:
            lines.append(k)
            spans.append((at + m.start(), at + m.end()))
        at += len(ln) + 1
    return lines, spans


def values_of(text, hits, length, stop, max_len):
    """[(value, count)] of one pattern: the text behind each hit up to the first stop unit, max_len units and textLength; ordered by
    code unit, a value in front of its extensions (Python's order of str is that: every character here is one code unit)"""
    n = len(text)
    starts = [min(max(h + length, 0), n) for h in hits.tolist()]
    if not stop:
        found = collections.Counter(text[s:s + max_len] for s in starts)
    elif len(stop) == 1:
        ends = ((s, text.find(stop, s, s + max_len)) for s in starts)
        found = collections.Counter(text[s:e if e >= 0 else s + max_len] for s, e in ends)
    else:
        cut_at = re.compile("[" + "".join(re.escape(c) for c in stop) + "]")
        found = collections.Counter(cut_at.split(text[s:s + max_len], 1)[0] for s in starts)
    return sorted(found.items())


class Values:
    """the packed answer of a batch, as fmx_field_values_batch lays it out (the fields check_values of test_field_values_cpu reads)"""

    def __init__(self, per):
        self.per = per
        flat = [vc for p in per for vc in p]
        self.val_off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
        self.counts = np.array([c for _, c in flat], np.int32)
        self.text_off = np.concatenate([[0], np.cumsum([len(v) for v, _ in flat])]).astype(np.int64)
        self.chars = units("".join(v for v, _ in flat))


class Case:
    """one text, its batch of patterns and its sequences; the judge's answers, each computed once"""

    def __init__(self, name, text, index):
        self.name, self.text, self.index = name, text, index
        self.T = boundaries(text)
        self.count, self.n_lines, self.text_len = len(self.T), n_lines_of(text), len(text)
        self._cache = {}
        rnd = random.Random(index)
        grams = sorted(set(text))
        if len(text) > 8:
            for m in (2, 3):
                grams += sorted({text[s:s + m] for s in (rnd.randrange(len(text) - m) for _ in range(10))})
        if name.startswith("period"):
            grams += [g for g in ("a", "aa", "aaa", "ab", "ba", "aba") if g not in grams]
        if name == "high_units":
            grams = [HIGH_PREFIX] + grams
        absent = lambda k: chr(ABSENT) + "q%d" % k
        if name == "only_boundary_no_hits":
            self.real, self.patterns = [], [absent(0), chr(ABSENT), absent(2)]
        elif len(text) <= 8:
            self.real = grams
            self.patterns = (grams + ["", absent(0)])[:1 if name == "only_boundary" else 3]
        else:
            # hitless patterns at both ends, and all of the padding BETWEEN two patterns with hits: a tile of packed hits that
            # holds both has every one of them in its slice of hit_off
            n = BATCH_SIZES[index % len(BATCH_SIZES)]
            half = len(grams) // 2
            pad = n - len(grams) - 3
            assert pad > 0
            self.real = grams
            self.patterns = [absent(0)] + grams[:half] + [absent(3 + k) for k in range(pad)] + grams[half:] + ["", absent(1)]
        self.n = len(self.patterns)
        self.lens = np.array([len(p) for p in self.patterns], np.int32)
        self.status = np.array([0 if p else 9 for p in self.patterns], np.int32)  # (the empty pattern: ArrayIndexOutOfBounds)
        self.ch, off = ia.pack_patterns([units(p) for p in self.patterns])
        self.off = off.astype(np.int32)
        self.query_off, self.kinds = query_cut(self.n)
        self.classes = [classes_of(p) for p in self.patterns]
        self.class_arrays = ia.pack_class_patterns(self.classes)
        # sequences: none, single terms, a term twice and three times, seeded pairs and triples of the batch's own patterns, a
        # term without hits, the empty term
        r = self.real or [absent(0)]
        pick = lambda k: [r[rnd.randrange(len(r))] for _ in range(k)]
        seqs = [[]] + [[g] for g in r[:6]] + [[r[0], r[0]], [r[-1], r[-1], r[-1]]] + [pick(2) for _ in range(24)] + [pick(3) for _ in range(10)]
        seqs += [[r[0], absent(0)], [absent(0), r[0]]] + ([[r[0], ""]] if self.real else [])  # (the batch without hits: no status either)
        if name.startswith("period"):
            seqs += [["aa", "aa"], ["ab", "ba"], ["a", "a", "a"], ["aaa", "aa", "a"], ["aba", "ba"], ["ba", "ab", "ba"]]
        self.sequences = seqs + [[]]
        self.seq_terms = [t for sq in self.sequences for t in sq]
        self.seq_off = np.concatenate([[0], np.cumsum([len(sq) for sq in self.sequences])]).astype(np.int32)
        self.seq_ch, soff = ia.pack_patterns([units(t) for t in self.seq_terms])
        self.seq_pat_off = soff.astype(np.int32)
        self.seq_classes = ia.pack_class_patterns([classes_of(t) for t in self.seq_terms])
        self.stops = [NL, ""] + ([chr(0x8000)] if name == "high_units" else [])

    def units(self):
        return self.once("units", lambda: units(self.text))

    def once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def hits(self, any_case=False):
        """per pattern of the batch its positions, ascending"""
        if any_case:
            return self.once("class hits", lambda: [class_occurrences(self.text, c, self.units()) for c in self.classes])
        return self.once("hits", lambda: [occurrences(self.text, p) for p in self.patterns])

    def term_lines(self, any_case=False):
        return self.once(("lines", any_case), lambda: [lines_of_hits(self.T, h) for h in self.hits(any_case)])

    def lines(self, max_lines, any_case=False):
        return cut(self.term_lines(any_case), max_lines)

    def queries(self, max_lines, any_case=False):
        per = self.once(("queries", any_case), lambda: query_lines(self.term_lines(any_case), self.query_off, self.kinds))
        return cut(per, max_lines)

    def sequence_answers(self, any_case=False):
        """per sequence (lines, spans)"""
        rx = (lambda t: class_regex(classes_of(t))) if any_case else re.escape
        return self.once(("sequences", any_case), lambda: [sequence_lines(self.text, [rx(t) for t in sq]) for sq in self.sequences])

    def sequence_packed(self, max_lines, any_case=False):
        """((lines, line_off, line_count), spans) as check_sequence of tests/test_match_sequence_cpu.py takes them"""
        per = self.sequence_answers(any_case)
        res = cut([ln for ln, _ in per], max_lines)
        spans = [sp[:max_lines] if max_lines > 0 else sp for _, sp in per]
        flat = np.array([ab for sp in spans for ab in sp], np.int32).reshape(-1, 2)
        return res, flat

    def seq_hits(self, any_case=False):
        if any_case:
            return self.once("class seq hits", lambda: [class_occurrences(self.text, classes_of(t), self.units()) for t in self.seq_terms])
        return self.once("seq hits", lambda: [occurrences(self.text, t) for t in self.seq_terms])

    def values(self, stop, max_len, any_case=False):
        hits = self.hits(any_case)
        return self.once(("values", stop, max_len, any_case),
                         lambda: Values([values_of(self.text, hits[i], int(self.lens[i]), stop, max_len) for i in range(self.n)]))

    def line_ids(self):
        """all lines, or the first and the last 200; two ids that are no lines in front"""
        ids = list(range(self.n_lines)) if self.n_lines <= 400 else list(range(200)) + list(range(self.n_lines - 200, self.n_lines))
        return np.array(ids, np.int32)

    def line_texts(self, ids):
        parts = self.text.split(NL)
        return [parts[k] for k in ids.tolist()]

    def bounds(self, ids):
        """(start, stop) of line ids, -1 for an id that is no line"""
        start, stop = np.full(len(ids), -1, np.int32), np.full(len(ids), -1, np.int32)
        for j, k in enumerate(ids):
            if 0 <= k < self.n_lines:
                start[j] = 0 if k == 0 else self.T[k - 1] + 1
                stop[j] = self.T[k] if k < self.count else self.text_len
        return start, stop

    def widest_slice(self, hit_off):
        """the most entries of hit_off one tile of TILE packed hits needs (fm_hit_tile: the patterns from the last one that begins at
        or before the tile's first hit to the last one that begins at or before its last hit)"""
        total, widest = int(hit_off[-1]), 0
        for tile in range(0, total, TILE):
            last = min(tile + TILE, total) - 1
            p_lo = bisect.bisect_right(hit_off, tile) - 1
            p_hi = min(bisect.bisect_right(hit_off, last) - 1, self.n - 1)
            widest = max(widest, p_hi - p_lo + 1)
        return widest


_CASES = {}


def names():
    return list(_texts_once())


def _texts_once():
    if "texts" not in _CASES:
        _CASES["texts"] = _texts()
    return _CASES["texts"]


def case(name):
    if name not in _CASES:
        texts = _texts_once()
        _CASES[name] = Case(name, texts[name], list(texts).index(name))
    return _CASES[name]
