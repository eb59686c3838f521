// fmx_value_hist.hpp — THE TOP VALUES OF A FIELD PER BUCKET OF LINES, the stacked timeline of a log search ("count by status over
// time": fmx_values_top_histogram_dev, fmx_values_gather_rows_dev, fmx_field_values_histogram_where_batch): the per-item functions
// of fmx_value_hist.hip, host and device alike, so that the CPU suite compiles them as plain C++ (tests/value_hist_hostsim.cpp).
//
// IN: the packed kept hits of n patterns, the groups of the values stage over them (val_off, count) and the group of every hit
// (fmx_values_of_hits_groups_dev).  OUT, per pattern i with G_i groups and R_i = min(top, G_i):
//   rows     the R_i groups with the largest counts, descending; equal counts in value order (the smaller group index first);
//            row r: row_group (the group's index within the pattern), row_count, hist[r * B + b] = its hits in bucket b
//   other    other[i * B + b] = the hits of pattern i in bucket b whose value is no row
// RANK: the key of group g of pattern p is (p << 31) | (INT32_MAX - count): 31 + fm_bits(n) bits, at most 62.  ONE stable sort
// puts each pattern's groups in descending order of count; within a pattern the groups arrive in value order, so stability is the
// tie rule.  Sorted index j of pattern p has the rank j - val_off[p]; rank_of_group = min(rank, top), `top` being the code "other".
// KEYS: the sort key of one slot is pattern | code | bucket with the code in [0, top] (code_bits = fm_bits(top), at most 17), the
// bucket in [0, B] (B: no bucket; bucket_bits = fm_bits(B), at most 28) and the pattern in [0, n] (n: a slot that is no hit; it sorts
// last): fm_vh_key_width = fm_bits(n) + fm_bits(top) + fm_bits(B), up to 31 + 17 + 28 = 76 bits — a call whose key is wider than 64
// is refused (the limit on n * (top + 1) * B keeps every call that passes it far below).
// COUNTERS: counter (pattern, code, bucket) = two lower bounds in the sorted keys inside the pattern's slot range, as fm_hist_count.
#pragma once

#include "fmx_line_hist.hpp"

namespace fmx {

constexpr int32_t kValueHistTopMax = 65536;  // `top` lies in [1, 65536]

// ---- rank --------------------------------------------------------------------------------------------------------------------
// count in [0, INT32_MAX]: the larger count gets the smaller key
FMX_HD uint64_t fm_vh_rank_key(int32_t pattern, int32_t count) {
    return ((uint64_t)(uint32_t)pattern << 31) | (uint32_t)(INT32_MAX - count);
}
FMX_HD int32_t fm_vh_rank_key_pattern(uint64_t key) { return (int32_t)(key >> 31); }
FMX_HD int32_t fm_vh_rank_key_count(uint64_t key) { return INT32_MAX - (int32_t)(key & 0x7fffffffu); }
FMX_HHD int32_t fm_vh_rank_key_width(int32_t n) { return 31 + fm_bits((uint32_t)n); }
// the rank of sorted index j inside the pattern whose groups begin at first_group, capped at top (= "other")
FMX_HD int32_t fm_vh_rank(int64_t sorted_index, int64_t first_group, int32_t top) {
    const int64_t r = sorted_index - first_group;
    return r < top ? (int32_t)r : top;
}
// the rows of a pattern of `groups` groups
FMX_HHD int64_t fm_vh_rows(int64_t groups, int32_t top) { return groups < top ? groups : top; }

// the HOST check of a call's shape and its row offsets (row_off: n + 1, nullable): 0, or which rule it breaks —
// 1 top outside [1, 65536]; 2 val_off does not start at 0 or decreases, or holds more than 2^31 - 1 groups; 3 n * (top + 1) * B
// above 2^27; 4 a key wider than 64 bits
FMX_HHD int32_t fm_vh_shape_bad(int32_t n, const int64_t *val_off, int32_t top, int32_t B, int64_t *row_off) {
    if (top < 1 || top > kValueHistTopMax) return 1;
    if (n > 0 && val_off[0] != 0) return 2;
    int64_t rows = 0;
    if (row_off) row_off[0] = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (val_off[i + 1] < val_off[i] || val_off[i + 1] > 0x7fffffff) return 2;
        rows += fm_vh_rows(val_off[i + 1] - val_off[i], top);
        if (row_off) row_off[i + 1] = rows;
    }
    if ((int64_t)n * ((int64_t)top + 1) * B > kHistCellsMax) return 3;
    if (fm_bits((uint32_t)n) + fm_bits((uint32_t)top) + fm_bits((uint32_t)B) > 64) return 4;
    return 0;
}

// ---- keys --------------------------------------------------------------------------------------------------------------------
FMX_HHD int32_t fm_vh_key_width(int32_t n, int32_t top, int32_t B) {
    return fm_bits((uint32_t)n) + fm_bits((uint32_t)top) + fm_bits((uint32_t)B);
}
FMX_HD uint64_t fm_vh_key(int32_t pattern, int32_t code, int32_t bucket, int32_t code_bits, int32_t bucket_bits) {
    return ((((uint64_t)(uint32_t)pattern << code_bits) | (uint32_t)code) << bucket_bits) | (uint32_t)bucket;
}
FMX_HD int32_t fm_vh_key_pattern(uint64_t key, int32_t code_bits, int32_t bucket_bits) { return (int32_t)(key >> (code_bits + bucket_bits)); }
FMX_HD int32_t fm_vh_key_code(uint64_t key, int32_t code_bits, int32_t bucket_bits) {
    return (int32_t)((key >> bucket_bits) & (((uint64_t)1 << code_bits) - 1));
}
FMX_HD int32_t fm_vh_key_bucket(uint64_t key, int32_t bucket_bits) { return (int32_t)(key & (((uint64_t)1 << bucket_bits) - 1)); }

// the code of a hit of a pattern whose groups are [first_group, first_group + groups): the rank of its group, or top ("other") for
// a group index outside the pattern's groups (-1: the values stage gave the slot no group)
FMX_HD int32_t fm_vh_code(const int32_t *rank_of_group, int64_t first_group, int64_t groups, int32_t group_of_hit, int32_t top) {
    return group_of_hit >= 0 && group_of_hit < groups ? rank_of_group[first_group + group_of_hit] : top;
}

// ---- counters ----------------------------------------------------------------------------------------------------------------
// counter (pattern, code, bucket) off the sorted keys; the slots of the call and the pattern's range as in fm_hist_count
FMX_HD int32_t fm_vh_count(const uint64_t *keys, const int64_t *hit_off, int64_t n_hits, int64_t first, int32_t pattern, int32_t code,
                           int32_t bucket, int32_t code_bits, int32_t bucket_bits) {
    int64_t a = hit_off[pattern], b = hit_off[pattern + 1];
    a = (a < first ? first : a < n_hits ? a : n_hits) - first;
    b = (b < first ? first : b < n_hits ? b : n_hits) - first;
    if (b <= a) return 0;
    const uint64_t key = fm_vh_key(pattern, code, bucket, code_bits, bucket_bits);
    const int64_t lo = fm_hist_key_rank(keys, a, b, key);
    return (int32_t)(fm_hist_key_rank(keys, lo, b, key + 1) - lo);  // (bucket + 1 <= B fits the bucket's bits)
}
// counter i of the (R + n) * B of a call: the first R * B are the rows' (row i / B: its pattern is the last p with row_off[p] <=
// row, its code the row's rank), the n * B behind them the patterns' "other" (code = top)
FMX_HD void fm_vh_counter(const int64_t *row_off, int32_t n, int64_t R, int32_t B, int32_t top, int64_t i, int32_t &pattern, int32_t &code,
                          int32_t &bucket) {
    const int64_t row = i / B;
    bucket = (int32_t)(i - row * B);
    if (row < R) {
        pattern = fm_hit_pattern(row_off, n, row);
        code = (int32_t)(row - row_off[pattern]);
    } else {
        pattern = (int32_t)(row - R);
        code = top;
    }
}

// ---- the gather of the rows' text --------------------------------------------------------------------------------------------
// the row of packed code unit u: the last r in [0, R) with row_text_off[r] <= u (u < row_text_off[R]; empty rows are skipped)
FMX_HD int64_t fm_vh_unit_row(const int64_t *row_text_off, int64_t R, int64_t u) {
    int64_t lo = 0, hi = R;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (row_text_off[mid] <= u)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

}  // namespace fmx
