"""A plain numpy reference of what the plan stage of a count batch must produce (fmx_kernels.hip: sort_shape,
pattern_code_word, suffix_key, plan_record, k_plan_scatter, k_plan_fine) — test infrastructure only.

All arithmetic is in Python ints or uint64.  Nothing here is shared with the library: the alphabet is read off the text
(FM:396-435: the sentinel is code 0, every other character gets the next code at its first appearance — the suffixes sort by
these codes, not by character value), the SA rows come
from the text's sorted suffixes.

  Shape            sort_shape(): bits, chars, total_bits, coarse_bits, below, fine_shift, code_bits, sa_key
  Alphabet         character -> code (0: absent), cumulativeCounts
  code_words       codes of the trailing 64 / code_bits characters, the LAST character in the low bits
  code_keys        suffix_key: the first `chars` codes of the word, packed `bits` wide, the last character most significant
  coarse_bin       min(key >> below, bins - 1)
  fine_bin         (key >> fine_shift) & 1023
  length_field     min(m, 0x3fffff)
  SaRows           first SA row and row count of any string of up to 64 / width codes, in the start / end convention of the
                   reference's backward search (FM:455-474: start = suffixes of text + sentinel that sort before the string,
                   end - start = count(string)); suffixes sorted by their first 64 / width codes, which is a full sort for every
                   string that short
"""
import numpy as np

LONG_PATTERN = 0x3FFFFF  # kPlanLongPattern
FINE_BITS = 10           # kFineBits
FINE_WINDOW = 1024       # kFineWindow
TILE = 4096              # patterns per workgroup of the plan kernels


def code_bits_for(sigma, code_bits_12=True):
    """fmx_code_bits_for: width of one code in a code word"""
    if sigma <= 256:
        return 8
    return 12 if (code_bits_12 and sigma <= 4096) else 16


class Shape:
    """sort_shape() + what plan_tables_stage derives from it.
    sigma: alphabet size WITH the sentinel's code 0; text_length: characters + 1 (the sentinel), as FM:162"""

    def __init__(self, sigma, sort_bits=28, coarse_bits=12, code_bits_12=1, plan_sa_key=0, has_table=False, text_length=0):
        bits = 1
        while (1 << bits) < sigma and bits < 15:
            bits += 1
        self.bits = bits
        self.code_bits = code_bits_for(sigma, bool(code_bits_12))
        chars = max(1, sort_bits // bits)
        self.chars = min(chars, 64 // self.code_bits)
        self.total_bits = self.chars * bits
        self.sa_key = 0
        if plan_sa_key and has_table:
            self.sa_key = plan_sa_key
            self.total_bits = 1
            while self.total_bits < 32 and (1 << self.total_bits) <= text_length:
                self.total_bits += 1
        self.coarse_bits = min(self.total_bits, coarse_bits)
        self.bins = 1 << self.coarse_bits
        self.below = self.total_bits - self.coarse_bits
        self.fine_shift = self.below - 8 if self.below > 8 else 0

    def as_tuple(self):
        return (self.bits, self.chars, self.total_bits, self.coarse_bits, self.below, self.fine_shift, self.code_bits)


class Alphabet:
    def __init__(self, text):
        t = np.ascontiguousarray(text, dtype=np.uint16)
        values, where, counts = np.unique(t, return_index=True, return_counts=True)
        zeros = 0
        if len(values) and values[0] == 0:  # an embedded '\0' shares the sentinel's code (FM:401-414)
            values, where, zeros, counts = values[1:], where[1:], int(counts[0]), counts[1:]
        by_appearance = np.argsort(where)  # FM:417-421: a character's code is 1 + how many others appear before its first use
        self.symbols = values[by_appearance]  # code - 1 -> character
        counts = counts[by_appearance]
        self.sigma = len(values) + 1
        self.text_length = len(t) + 1
        self.map = np.zeros(1 << 16, dtype=np.int64)
        self.map[self.symbols] = np.arange(1, len(values) + 1)
        # cumulativeCounts (FM:307-327): C[c] = characters with a smaller code, the sentinel among them
        self.C = np.zeros(self.sigma + 1, dtype=np.int64)
        self.C[1] = 1 + zeros
        self.C[2:] = self.C[1] + np.cumsum(counts)
        assert self.C[-1] == self.text_length

    def codes(self, chars):
        return self.map[np.ascontiguousarray(chars, dtype=np.uint16)]


def lengths(pat_off):
    off = np.asarray(pat_off, dtype=np.int64)
    return off[1:] - off[:-1]


def length_field(m):
    return np.minimum(np.asarray(m, dtype=np.int64), LONG_PATTERN).astype(np.uint32)


def code_words(alphabet, pat, pat_off, code_bits):
    """uint64[n]: code j (j characters before the pattern's end) at bits [j * code_bits, (j + 1) * code_bits)"""
    pat = np.ascontiguousarray(pat, dtype=np.uint16)
    off = np.asarray(pat_off, dtype=np.int64)
    m = off[1:] - off[:-1]
    words = np.zeros(len(m), dtype=np.uint64)
    for j in range(64 // code_bits):
        has = m > j
        at = np.where(has, off[1:] - 1 - j, 0)
        c = np.where(has, alphabet.codes(pat[at]) if len(pat) else 0, 0).astype(np.uint64)
        words |= c << np.uint64(j * code_bits)
    return words


def word_code(words, j, code_bits):
    return (np.asarray(words, dtype=np.uint64) >> np.uint64(j * code_bits)) & np.uint64((1 << code_bits) - 1)


def code_keys(words, shape):
    """suffix_key: uint32 arithmetic, as the kernel's (the key has at most 32 bits)"""
    key = np.zeros(len(words), dtype=np.uint64)
    for j in range(shape.chars):
        key = ((key << np.uint64(shape.bits)) | word_code(words, j, shape.code_bits)) & np.uint64(0xFFFFFFFF)
    return key.astype(np.uint32)


def coarse_bin(keys, shape):
    return np.minimum(np.asarray(keys, dtype=np.uint64) >> np.uint64(shape.below), shape.bins - 1).astype(np.int64)


def fine_bin(keys, shape):
    return ((np.asarray(keys, dtype=np.uint64) >> np.uint64(shape.fine_shift)) & np.uint64((1 << FINE_BITS) - 1)).astype(np.int64)


def ulp32(v):
    """spacing of float32 at v (>= 1)"""
    return max(1.0, 2.0 ** (int(v).bit_length() - 1 - 23)) if v >= 1 else 1.0


class SaRows:
    """SA ranges of strings of up to `depth` = 64 / width codes over text + sentinel: the suffixes sorted by their first `depth`
    codes (each `width` bits wide, the FIRST character most significant, 0 past the end of the text)."""

    def __init__(self, alphabet, text, width):
        self.width = width
        self.depth = 64 // width
        codes = alphabet.codes(text).astype(np.uint64)
        n = len(codes)
        padded = np.concatenate([codes, np.zeros(self.depth, dtype=np.uint64)])
        keys = np.zeros(n + 1, dtype=np.uint64)  # (+ the sentinel's own suffix: all zero)
        for j in range(self.depth):
            keys |= padded[j:j + n + 1] << np.uint64(width * (self.depth - 1 - j))
        keys.sort()
        self.keys = keys

    def ranges_of_words(self, words, lens):
        """(start, end) int64[n] of the strings spelt by the low `lens` codes of code words (the LAST character in the low bits,
        so the string's first character is code lens - 1).  lens in 1 .. depth.  A string that holds code 0 (an absent character)
        occurs nowhere: end == start == where it would be inserted."""
        words = np.asarray(words, dtype=np.uint64)
        lens = np.asarray(lens, dtype=np.int64)
        assert len(lens) == 0 or (lens.min() >= 1 and lens.max() <= self.depth)
        w = self.width
        lo = np.zeros(len(words), dtype=np.uint64)
        hi = np.zeros(len(words), dtype=np.uint64)
        zero = np.zeros(len(words), dtype=bool)
        for L in np.unique(lens):
            sel = lens == L
            bits = int(L) * w
            s = words[sel] if bits >= 64 else words[sel] & np.uint64((1 << bits) - 1)
            free = w * (self.depth - int(L))  # low bits of the key that the string leaves open
            lo[sel] = s << np.uint64(free)
            hi[sel] = lo[sel] | np.uint64((1 << free) - 1)
            z = np.zeros(int(sel.sum()), dtype=bool)
            for j in range(int(L)):
                z |= ((s >> np.uint64(j * w)) & np.uint64((1 << w) - 1)) == 0
            zero[sel] = z
        start = np.searchsorted(self.keys, lo, side="left").astype(np.int64)
        end = np.searchsorted(self.keys, hi, side="right").astype(np.int64)
        end[zero] = start[zero]
        return start, end

    def range_of(self, codes):
        """(start, end) of one string given as its codes, first character first"""
        L = len(codes)
        word = 0
        for j, c in enumerate(reversed(list(codes))):
            word |= int(c) << (j * self.width)
        s, e = self.ranges_of_words(np.array([word], dtype=np.uint64), np.array([L]))
        return int(s[0]), int(e[0])


def sa_key_len(m, table_chars, code_bits):
    """characters of a pattern's suffix the SA-row key is made from: min(m, the table's depth, 64 / code_bits)"""
    return np.minimum(np.minimum(np.asarray(m, dtype=np.int64), table_chars), 64 // code_bits)


def sa_row_keys(alphabet, rows, words, m, table_chars, code_bits):
    """plan_sa_key 1: the first SA row of the pattern's tabulated suffix; 0 for a pattern that ends at once (empty, or its last
    character absent); C[last character] where the table has no answer (the suffix does not occur, or holds an absent character)"""
    words = np.asarray(words, dtype=np.uint64)
    m = np.asarray(m, dtype=np.int64)
    c_last = word_code(words, 0, code_bits).astype(np.int64)
    live = (m > 0) & (c_last != 0)
    lens = sa_key_len(m, table_chars, code_bits)
    key = np.where(live, alphabet.C[np.where(live, c_last, 0)], 0).astype(np.int64)
    deep = live & (lens >= 2)
    if deep.any():
        s, e = rows.ranges_of_words(words[deep], lens[deep])
        k = key[deep]
        k[e > s] = s[e > s]
        key[deep] = k
    return key.astype(np.uint32)
