// fmx_hit_top.hpp — THE LINES RANKED BY THE NUMBER BEHIND A PATTERN (fmx_top_lines_of_hits_dev, fmx_top_lines_where_batch;
// ... | sort -k latency -nr | head -10): the per-item functions of fmx_hit_top.hip, host and device alike, so that the CPU suite
// compiles them as plain C++ (tests/top_lines_hostsim.cpp).
//
// For number pattern i of a batch of n, over its packed (kept) hits:
//   THE VALUE OF A HIT is fmx_hit_numbers.hpp's, bit for bit: the window fm_val_window(loc, len, kNumWindow, textLength), parsed by
//     fm_num_parse(win, e - s, F, value) with ONE F = frac_digits in [0, 9] per call.  Only kNumOk hits take part; the others are
//     counted per pattern as not_number and overflow.
//   THE ORDER: descending[i] (one byte per pattern) — 1 is largest first, 0 smallest first.  The ORDERED VALUE of a hit is
//     u = descending ? INT64_MAX - value : value, so that "ranks better" is "smaller u" in both orders.
//   THE CANDIDATE OF A LINE (a hit belongs to the line of its first character) is the parsing hit on it with the smallest
//     (u, position): the best value, and among hits of equal value the smallest text position.  A line without a parsing hit has none.
//   THE RANKING of pattern i orders its candidates by (u, line id): a total order, a line has one candidate.  lines[i] = the
//     candidates, numbers[i] = the parsing hits, so numbers + not_number + overflow = the hits of the pattern.
//   THE ROWS: first >= 0 and top >= 1 hold for the whole call; the rows of pattern i are the ranks first .. first + top - 1,
//     rows[i] = min(top, max(0, lines[i] - first)); row (i, j) lives at i * top + j and carries row_line, row_value and row_loc (the
//     candidate's position); the entries at j >= rows[i] are stored as 0.  n * top <= 2^27.
//
// THE KEYS.  A slot's first key is fmx_hit_by.hpp's (pattern << pos_bits) | position, the pattern n for a slot that is no hit or
// whose window does not parse: ONE sort by it leaves every pattern's parsing hits side by side, ascending by position, so their
// lines never decrease.  The key of a run is fm_top_line_key(pattern, line); the reduction over runs of equal key keeps the minimum
// of TopCand {u, position} — associative and commutative, so the answer does not depend on how the runs are cut.  The candidates
// then lie in (pattern, line) order: a stable sort by u and a stable sort by pattern rank them, stability being the tie rule.
#pragma once

#include "fmx_hit_by.hpp"
#include "fmx_hit_range.hpp"

namespace fmx {

// u of a value in [0, INT64_MAX], and back
FMX_HD uint64_t fm_top_ordered(int64_t value, bool descending) { return descending ? (uint64_t)(kNumValueMax - value) : (uint64_t)value; }
FMX_HD int64_t fm_top_value(uint64_t u, bool descending) { return descending ? kNumValueMax - (int64_t)u : (int64_t)u; }

// what the reduction over the hits of one (pattern, line) carries
struct TopCand {
    uint64_t u;
    int64_t loc;
};
FMX_HD TopCand fm_top_better(const TopCand &a, const TopCand &b) { return (b.u < a.u || (b.u == a.u && b.loc < a.loc)) ? b : a; }
struct TopBetter {
    FMX_HHD TopCand operator()(const TopCand &a, const TopCand &b) const { return (b.u < a.u || (b.u == a.u && b.loc < a.loc)) ? b : a; }
};

// the key of a run: the pattern in [0, n] (n: no candidate) above the line in [0, count]
FMX_HHD uint64_t fm_top_line_key(int32_t pattern, int32_t line) { return ((uint64_t)(uint32_t)pattern << 32) | (uint32_t)line; }
FMX_HD int32_t fm_top_line_key_pattern(uint64_t key) { return (int32_t)(key >> 32); }
FMX_HD int32_t fm_top_line_key_line(uint64_t key) { return (int32_t)(key & 0xffffffffu); }

// the code of a slot for fm_range_tail's word of the two reasons, from the parser's kind
FMX_HD int32_t fm_top_tail_code(int32_t kind) { return kind == kNumOk ? kRangeKeep : kind == kNumNotNumber ? kRangeNotNumber : kRangeOverflow; }

// the first of the `count` ranked slots whose pattern is not below p (pat: ascending, the pattern n behind the candidates)
FMX_HD int64_t fm_top_segment(const uint32_t *pat, int64_t count, int32_t p) {
    int64_t lo = 0, hi = count;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (pat[mid] < (uint32_t)p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// rows of a pattern with `lines` candidates
FMX_HD int32_t fm_top_rows(int64_t lines, int32_t first, int32_t top) {
    const int64_t left = lines - first;
    return left <= 0 ? 0 : left < top ? (int32_t)left : top;
}

// the HOST checks of the call's small arguments: 0, or which rule is broken
//   1  frac_digits outside [0, 9]   2  a negative term_len   3  first < 0   4  top < 1   5  n * top > 2^27   6  a missing array
FMX_HHD int32_t fm_top_args_bad(int32_t n, const int32_t *term_len, const uint8_t *descending, int32_t frac_digits, int32_t first, int32_t top) {
    if (frac_digits < 0 || frac_digits > kNumFracMax) return 1;
    if (n > 0 && (!term_len || !descending)) return 6;
    for (int32_t i = 0; i < n; ++i)
        if (term_len[i] < 0) return 2;
    if (first < 0) return 3;
    if (top < 1) return 4;
    if ((int64_t)n * top > kHistCellsMax) return 5;
    return 0;
}

}  // namespace fmx
