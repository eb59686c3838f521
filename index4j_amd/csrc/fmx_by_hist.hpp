// fmx_by_hist.hpp — STATISTICS OF THE NUMBER BEHIND A PATTERN, BY THE VALUE OF A FIELD OF THE SAME LINE, PER BUCKET OF LINES
// (fmx_numbers_by_key_buckets_dev, fmx_number_stats_by_histogram_batch; timechart p95(latency_ms=) by status=): the per-item
// functions of fmx_by_hist.hip, host and device alike, so that the CPU suite compiles them as plain C++ (tests/by_hist_hostsim.cpp).
//
// IN: stages a and b of "stats ... by" (fmx_hit_by.hpp) over the key patterns' kept hits — the first lines of every key pattern,
// the group of every first hit, the groups' offsets val_off and their lines — and the packed kept hits of n number patterns.
// OUT, with B buckets (fmx_line_hist.hpp's edges; none at all: B = 1, every line), G_k the groups of key pattern k and
// R_k = min(top, G_k):
//   key rows  the R_k groups of k with the most lines, descending; equal lines in value order (the smaller group index first):
//             key_row_off (m + 1), key_row_group (the group's index within the pattern), key_row_lines
//   cells     number pattern i with k = by_of[i] has (R_k + 1) * B cells at cell_off[i]; cell (i, r, b) = cell_off[i] + r * B + b holds
//             the hits of i that parse, lie in bucket b and whose line's key is key row r; row R_k is "other": a key that is no row
// RANK: fmx_value_hist.hpp's, over the lines of the groups: ONE stable sort of (k << 31) | (INT32_MAX - lines) puts each pattern's
// groups in descending order; rank_of_group = min(sorted index - val_off[k], top).
// CODE of a number slot: min(rank_of_group, R_k) * B + bucket — R_k folds the pattern's own "other", not the call's — in
// fmx_hit_numbers.hpp's key (pattern << code_bits) | code with C = (min(top, max_k G_k) + 1) * B in the place of its B: a cell in
// [0, C), C = NO KEY (decided before the parse: fm_num_code keeps C whatever the window holds; a hit whose line lies in no bucket
// has no place among the cells and is counted here too — the host form's filter leaves none), C + 1 = not a number, C + 2 =
// overflow.  The parse, the two sorts and the two running sums are the numbers stage's own.
#pragma once

#include "fmx_hit_by.hpp"
#include "fmx_value_hist.hpp"

namespace fmx {

// the code of a number slot of bucket `bucket` in [0, B] (B: no bucket) whose line's first key hit is `found` (fm_by_find's answer
// over the first hits of key pattern k, whose groups are [g0, g0 + groups)): its cell within its pattern, or C
FMX_HD int32_t fm_bh_code(const int32_t *rank_of_group, const int32_t *group_of_first, int64_t found, int64_t g0, int64_t groups, int32_t top,
                          int32_t bucket, int32_t B, int32_t C) {
    if (found < 0 || bucket >= B) return C;
    const int32_t g = group_of_first[found];
    if (g < 0 || g >= groups) return C;
    const int32_t rows = (int32_t)fm_vh_rows(groups, top), rank = rank_of_group[g0 + g];
    return (rank < rows ? rank : rows) * B + bucket;
}

// the HOST checks of a call's shape from its arguments alone (before anything is searched): 0, or which rule is broken
//   1  top outside [1, 65536]      2  n * (top + 1) * B above 2^27      3  that times max(n_permille, 1) above 2^27
FMX_HHD int32_t fm_bh_args_bad(int32_t n, int32_t top, int32_t B, int32_t n_permille) {
    if (top < 1 || top > kValueHistTopMax) return 1;
    const int64_t per = ((int64_t)top + 1) * (B > 0 ? B : 0);  // (at most 2^48: the product with n is judged by a division)
    if (n > 0 && per > kHistCellsMax / n) return 2;
    const int64_t cells = (n > 0 ? n : 0) * per;
    if (cells * (n_permille > 0 ? n_permille : 1) > kHistCellsMax) return 3;
    return 0;
}

// ... and of its small arrays, with the offsets they make: fm_by_rows_bad's rules 1 .. 3 (val_off must start AT 0 here), then
//   6  a key pattern with more than 2^31 - 1 groups      7  fm_bh_args_bad's rules
// key_row_off (m + 1), cell_off (n + 1) and *code_space (C, at least B) are outputs, each nullable
FMX_HHD int32_t fm_bh_shape_bad(int32_t n, const int32_t *by_of, int32_t m, const int64_t *val_off, int32_t top, int32_t B, int32_t n_permille,
                                int64_t *key_row_off, int64_t *cell_off, int32_t *code_space) {
    if (fm_bh_args_bad(n, top, B, n_permille) || B < 1) return 7;
    if (n > 0 && (m <= 0 || !by_of)) return 1;
    for (int32_t i = 0; i < n; ++i)
        if (by_of[i] < 0 || by_of[i] >= m) return 2;
    if (m > 0 && (!val_off || val_off[0] != 0)) return 3;
    int64_t rows = 0, widest = 0;
    if (key_row_off) key_row_off[0] = 0;
    for (int32_t k = 0; k < m; ++k) {
        const int64_t groups = val_off[k + 1] - val_off[k];
        if (groups < 0) return 3;
        if (val_off[k + 1] > 0x7fffffff) return 6;
        const int64_t r = fm_vh_rows(groups, top);
        rows += r;
        if (key_row_off) key_row_off[k + 1] = rows;
        if (r > widest) widest = r;
    }
    int64_t cells = 0;
    if (cell_off) cell_off[0] = 0;
    for (int32_t i = 0; i < n; ++i) {
        cells += (fm_vh_rows(val_off[by_of[i] + 1] - val_off[by_of[i]], top) + 1) * B;
        if (cell_off) cell_off[i + 1] = cells;
    }
    if (code_space) *code_space = (int32_t)((widest + 1) * B);  // (at most (top + 1) * B <= 2^27)
    return 0;
}

}  // namespace fmx
