// fmx_hit_by.hpp — STATISTICS OF THE NUMBER BEHIND A PATTERN, GROUPED BY THE VALUE BEHIND ANOTHER PATTERN OF THE SAME LINE
// (fmx_first_hits_of_lines_dev, fmx_values_of_hits_groups_dev, fmx_numbers_by_key_dev, fmx_number_stats_by_batch; stats count,
// sum(bytes=), p95(latency_ms=) by status=): the per-item functions of fmx_hit_first.hip and of the "by" kernels of
// fmx_hit_numbers.hip, host and device alike, so that the CPU suite compiles them as plain C++ (tests/by_key_hostsim.cpp).
//
// THE KEY OF A LINE for key pattern k: among the hits of k on line L (a hit belongs to the line of its first character) the one
// with the smallest text position; the key is that hit's VALUE by fmx_hit_values.hpp's rule.  A line without a hit of k has no key.
//   stage a  (fmx_hit_first.hip)   packed hits of m key patterns -> per pattern its distinct lines ascending, each with the smallest
//            position of a hit on it: ONE device-wide sort of the keys (pattern << pos_bits) | position — by position lines ascend,
//            so the first hit of a line is the sorted hit whose predecessor has another pattern or another line;
//   stage b  (fmx_hit_values.hip)  the values stage over those first hits, which also stores the GROUP of every hit: the index of
//            its value among its pattern's distinct values.  The groups of key k are the distinct keys of its lines, count = lines;
//   stage c  (fmx_hit_numbers.hip) a lane per number hit finds its line and, by ONE lower bound in the first lines of its key
//            pattern by_of[i], the group of that line: the CODE of the hit, in fmx_hit_numbers.hpp's key (pattern << code_bits) |
//            code with B = the largest number of groups of one key pattern: a group in [0, B), B = NO KEY (decided before the
//            parse: fm_num_code keeps B whatever the window holds), B + 1 = not a number, B + 2 = overflow.  The parse, the two
//            sorts and the two running sums are the numbers stage's own; the rows are PACKED: pattern i has row_off[i + 1] -
//            row_off[i] = the groups of key by_of[i] rows, row (i, g) at row_off[i] + g.
#pragma once

#include "fmx_hit_numbers.hpp"

namespace fmx {

// the sort key of one packed hit of stage a: position in [0, text_len] takes pos_bits = fm_bits(text_len), the pattern in [0, m]
// (m: a slot that is no hit, it sorts behind every hit) fm_bits(m): at most 31 + 31 bits
FMX_HD uint64_t fm_first_key(int32_t pattern, int32_t loc, int32_t pos_bits) { return ((uint64_t)(uint32_t)pattern << pos_bits) | (uint32_t)loc; }
FMX_HD int32_t fm_first_key_pattern(uint64_t key, int32_t pos_bits) { return (int32_t)(key >> pos_bits); }
FMX_HD int32_t fm_first_key_loc(uint64_t key, int32_t pos_bits) { return (int32_t)(key & (((uint64_t)1 << pos_bits) - 1)); }

// sorted slot i is the first hit of its (pattern, line): a hit (pattern < m) whose predecessor has another pattern or another line.
// line_of[i] = the line of sorted slot i.
FMX_HD bool fm_first_head(const uint64_t *keys, const int32_t *line_of, int64_t i, int32_t m, int32_t pos_bits) {
    const int32_t p = fm_first_key_pattern(keys[i], pos_bits);
    if (p >= m) return false;
    return i == 0 || fm_first_key_pattern(keys[i - 1], pos_bits) != p || line_of[i - 1] != line_of[i];
}

// where line L stands in lines[lo, hi) (ascending, distinct), or -1: the line has no key
FMX_HD int64_t fm_by_find(const int32_t *lines, int64_t lo, int64_t hi, int32_t L) {
    const int64_t f = fm_hist_rank(lines, lo, hi, L);
    return f < hi && lines[f] == L ? f : -1;
}

// the code of a number hit whose line's first key hit is `found` (fm_by_find's answer over the first hits of its key pattern):
// that hit's group, B where there is none (or where the group is no group of the call: nothing is read through a code)
FMX_HD int32_t fm_by_code(const int32_t *group_of_first, int64_t found, int32_t B) {
    if (found < 0) return B;
    const int32_t g = group_of_first[found];
    return g >= 0 && g < B ? g : B;
}

// the pattern of packed row r in [0, row_off[n]): the LAST i with row_off[i] <= r (a pattern without rows has row_off[i] ==
// row_off[i + 1]: a run of equal entries ends in the pattern that holds the row)
FMX_HD int32_t fm_by_row_pattern(const int64_t *row_off, int32_t n, int64_t r) {
    int32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (row_off[mid] <= r)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// the HOST checks of a call's small arrays and the rows they make: 0, or which rule is broken.  val_off: m + 1 offsets of the key
// patterns' groups (stage b's answer, read by the caller); row_off (n + 1, out; nullable) and *max_groups (out; nullable, at least 1)
//   1  m <= 0 with n > 0, or a missing array      2  by_of[i] outside [0, m)      3  val_off starts below 0 or decreases
//   4  more than 2^27 rows                         5  more than 2^27 percentiles (rows * max(n_permille, 1))
FMX_HHD int32_t fm_by_rows_bad(int32_t n, const int32_t *by_of, int32_t m, const int64_t *val_off, int32_t n_permille, int64_t *row_off,
                               int32_t *max_groups) {
    if (n <= 0) return 0;
    if (m <= 0 || !by_of) return 1;
    for (int32_t i = 0; i < n; ++i)
        if (by_of[i] < 0 || by_of[i] >= m) return 2;
    if (!val_off) return 0;  // (the by_of check alone: the host form judges it before anything is searched)
    if (val_off[0] < 0) return 3;
    for (int32_t k = 0; k < m; ++k)
        if (val_off[k + 1] < val_off[k]) return 3;
    int64_t rows = 0, widest = 1;  // (the widest key pattern some number pattern asks for: at most 2^27 groups)
    for (int32_t i = 0; i < n; ++i) {
        const int64_t groups = val_off[by_of[i] + 1] - val_off[by_of[i]];
        if (row_off) row_off[i] = rows;
        rows += groups;
        if (rows > kHistCellsMax) return 4;
        if (groups > widest) widest = groups;
    }
    if (row_off) row_off[n] = rows;
    if (rows * (n_permille > 0 ? n_permille : 1) > kHistCellsMax) return 5;
    if (max_groups) *max_groups = (int32_t)widest;
    return 0;
}

}  // namespace fmx
