// fmx_by_api.cpp — STATISTICS OF THE NUMBER BEHIND A PATTERN, GROUPED BY THE VALUE OF A FIELD OF THE SAME LINE (include/fmx.h
// "STATISTICS BY KEY"; fmx_hit_by.hpp has the definition): the three device stages fmx_first_hits_of_lines_dev,
// fmx_values_of_hits_groups_dev and fmx_numbers_by_key_dev over the launchers of fmx_hit_first.hip, fmx_hit_values.hip and
// fmx_hit_numbers.hip with the packed extract between them, and the host forms fmx_number_stats_by_batch /
// fmx_number_stats_by_class_batch.  Of a handle this file sees what fmx::line_view and fmx::text_view hand out; a host form runs
// the packed sequence of fmx_api.cpp up to the stage of this file (fmx::hits_stage_call) over ONE merged batch terms | key patterns
// | number patterns (fmx::merge_keyed_*_batch), then the keyed front half of the host-stage layer (fmx::keyed_front_stage: the
// filter, stage a, stage b, ONE read of the group offsets and the units of the groups' text), which sizes the rows, and stage c
// over the numbers' part and the groups' text.  The checks, the statistics arrays, the packed result and the call plumbing are that
// layer's too (fmx_host_stage.hpp); this file keeps the rows of a call and stage c.
#include "fmx_hit_by.hpp"
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

#include <cstring>

namespace {

using fmx::api_fail;
using fmx::guarded;
using fmx::hip_fail;
using fmx::no_line_table;
using fmx::zero;

// the rows of a call from the key patterns' group offsets (fm_by_rows_bad's rules as messages)
int check_rows(int32_t n, const int32_t *by_of, int32_t m, const int64_t *val_off, int32_t n_permille, int64_t *row_off) {
    switch (fmx::fm_by_rows_bad(n, by_of, m, val_off, n_permille, row_off, nullptr)) {
        case 0: return FMX_OK;
        case 1: return api_fail(FMX_E_ARG, "number patterns without a key pattern (m == 0 with n > 0)");
        case 2: return api_fail(FMX_E_ARG, "a by_of entry is outside 0 .. m - 1");
        case 3: return api_fail(FMX_E_ARG, "val_off starts below 0 or decreases");
        case 4: return api_fail(FMX_E_ARG, "more than 2^27 rows in one call (the groups of by_of[i], over the number patterns)");
        default: return api_fail(FMX_E_ARG, "more than 2^27 percentiles in one call (rows * n_permille)");
    }
}

// ---- the stages behind the arguments' checks ----------------------------------------------------------------------------------------
using Rows = fmx::StatRows;
struct FirstHits {
    const int64_t *off;
    const int32_t *lines, *group;
};

// stage c: the windows and codes, the windows' text, the rows (n > 0, n_hits > 0, an index with extraction)
int rows_impl(const fmx_index *idx, const fmx::LineView &view, const fmx::TextView &text, int32_t n, const int32_t *term_len,
              const int32_t *by_of, int32_t m, const int64_t *val_off, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits,
              const FirstHits &f, int32_t frac_digits, const int32_t *permille, int32_t P, int64_t *d_row_off, const Rows &r, int32_t *d_status,
              void *ws, size_t ws_bytes, hipStream_t st) {
    fmx::ValuesWindows w;
    if (!fmx::numbers_by_key_windows(ws, ws_bytes, n, n_hits, P, &w))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_numbers_by_key_scratch_bytes");
    int e = fmx::launch_numbers_by_key_ranges(view.table, view.count, text.text_len, view.n_cu, n, term_len, by_of, m, val_off, d_hit_off, d_locs,
                                              n_hits, f.off, f.lines, f.group, permille, P, d_row_off, ws, ws_bytes, st);
    if (e) return hip_fail("windows of hits", e);
    if (const int rc = fmx::extract_windows(idx, w, (int32_t)n_hits, st)) return rc;
    e = fmx::launch_numbers_by_key_rows(view.n_cu, n, by_of, m, val_off, d_hit_off, n_hits, frac_digits, P, r.count, r.sum_lo, r.sum_hi, r.min,
                                        r.max, r.pct, r.no_key, r.not_number, r.overflow, d_status, ws, ws_bytes, st);
    if (e) return hip_fail("numbers by key", e);
    return FMX_OK;
}

// ---- the host form --------------------------------------------------------------------------------------------------------------------
// the regions of the ONE allocation of the answer
enum { kLines, kTextOff, kChars, kCount, kSumLo, kSumHi, kMin, kMax, kPct };

struct ByArgs : fmx::KeyedArgs {
    std::vector<int64_t> row_off;  // n + 1
};

// the keyed front half, the groups' lines and text, stage c over the numbers' part
int by_stage(const fmx::HitsBetween &h, void *arg) {
    ByArgs &a = *static_cast<ByArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const int32_t m = a.m, n = a.n;
    fmx::KeyedFront f{};
    bool done = false;
    int rc;
    if ((rc = fmx::keyed_front_stage(h, a, "numbers by key", &f, &done)) || done) return rc;
    if ((rc = check_rows(n, a.by_of, m, a.val_off.data(), a.P, a.row_off.data()))) return rc;  // (the group offsets size the rows)
    const size_t G = (size_t)a.val_off[(size_t)m], units = (size_t)a.val_off[(size_t)m + 1], R = (size_t)a.row_off[(size_t)n], P = (size_t)a.P;
    if (!a.result.alloc({G * 4, (G + 1) * 8, units * 2 + 2, R * 4, R * 8, R * 8, R * 8, R * 8, R * P * 8}))
        return api_fail(FMX_E_NOMEM, "out of host memory for " + std::to_string(G) + " groups");
    if (units > 0) {
        uint16_t *d_chars = nullptr;
        if ((rc = h.block(h.call, units * 2 + 8, reinterpret_cast<void **>(&d_chars)))) return rc;
        const int e = fmx::launch_values_fill(h.view->n_cu, (int64_t)G, f.text_off, d_chars, f.ws_b, st);
        if (e) return hip_fail("k_val_fill launch", e);
        FMX_HIP_TRY(hipMemcpyAsync(a.result.region<uint16_t>(kChars), d_chars, units * 2, hipMemcpyDeviceToHost, st));
    }
    FMX_HIP_TRY(hipMemcpyAsync(a.result.region<int32_t>(kLines), f.lines, G * 4, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipMemcpyAsync(a.result.region<int64_t>(kTextOff), f.text_off, (G + 1) * 8, hipMemcpyDeviceToHost, st));
    if (f.N == 0) return FMX_OK;  // (no number hit is kept: the groups with zero rows — the allocation is zeroed)
    Rows d;
    void *ws_c = nullptr;
    const size_t c_bytes = fmx::numbers_by_key_scratch_bytes(n, f.N, a.P);
    if ((rc = fmx::stat_rows_blocks(h, nullptr, R, P, n, &d)) || (rc = h.block(h.call, c_bytes + 8, &ws_c)) ||
        (rc = rows_impl(h.idx, *h.view, a.text, n, a.term_len.data() + m, a.by_of, m, a.val_off.data(), f.num_off, f.num_locs, f.N,
                        FirstHits{f.first_off, f.first_lines, f.group}, a.frac_digits, a.permille, a.P, nullptr, d, h.status ? h.status + m : nullptr,
                        ws_c, c_bytes, st)))
        return rc;
    return fmx::stat_rows_down(fmx::keyed_host_rows(a, kCount), d, R, P, n, st);
}

// what the two host forms take besides their patterns, and what they hand back
struct ByCall : fmx::KeyedCall {
    int32_t line_lo, line_hi;
    int64_t *val_off;
    int32_t **lines;
    int64_t *row_off;
};

void null_results(const ByCall &c) {
    if (c.lines) *c.lines = nullptr;
    fmx::keyed_null_results(c);
}
bool results_missing(const ByCall &c) { return !c.val_off || !c.row_off || !c.lines || fmx::keyed_results_missing(c); }

// the checks of the HOST arrays both forms share (behind their own batches'), the handle's views and the empty call; *done: answered
int by_call_args(const fmx_index *idx, const ByCall &c, ByArgs *a, bool *done) {
    int rc;
    if ((rc = fmx::keyed_call_checks(c))) return rc;
    if (c.line_lo < 0 || c.line_hi < c.line_lo) return api_fail(FMX_E_ARG, "the window of lines is not 0 <= line_lo <= line_hi");
    if ((rc = fmx::keyed_call_views(idx, &a->text))) return rc;
    zero(c.val_off, (size_t)c.m + 1);
    zero(c.row_off, (size_t)c.n + 1);
    *done = !fmx::keyed_call_fill(c, c.line_lo, c.line_hi, a);
    a->row_off.assign((size_t)c.n + 1, 0);
    return FMX_OK;
}

// the call over the merged batch terms | key patterns | number patterns, and the answer into the caller's arrays
int by_call_run(const fmx_index *idx, const ByCall &c, const fmx::ValuesBatch &batch, ByArgs &a) {
    if (const int rc = fmx::keyed_call_run(idx, c, batch, by_stage, &a, a)) return rc;
    memcpy(c.val_off, a.val_off.data(), ((size_t)c.m + 1) * 8);
    memcpy(c.row_off, a.row_off.data(), ((size_t)c.n + 1) * 8);
    if (a.result.p) {  // the ONE allocation: freed with fmx_free_buffer((uint8_t *)*lines)
        *c.lines = a.result.region<int32_t>(kLines);
        fmx::keyed_hand_over(c, a, kTextOff);
    }
    return FMX_OK;
}

}  // namespace

extern "C" {

size_t fmx_first_hits_of_lines_scratch_bytes(int32_t m, int64_t n_hits) { return fmx::first_hits_scratch_bytes(m, n_hits); }

int fmx_first_hits_of_lines_dev(const fmx_index *idx, int32_t m, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits,
                                int64_t *d_first_off, int32_t *d_first_lines, int32_t *d_first_locs, void *d_ws, size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || m < 0 || n_hits < 0 || (m > 0 && (!d_hit_off || !d_first_off)) || (m > 0 && n_hits > 0 && (!d_locs || !d_first_lines || !d_first_locs)))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    fmx::LineView view;
    fmx::TextView text;
    int rc;
    if ((rc = fmx::line_view(idx, &view)) || (rc = fmx::text_view(idx, &text))) return rc;
    if (!view.table) return no_line_table();
    if (m == 0) return FMX_OK;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_hits == 0) {
        FMX_HIP_TRY(hipMemsetAsync(d_first_off, 0, ((size_t)m + 1) * 8, st));
        return FMX_OK;
    }
    if (!d_ws || ws_bytes < fmx::first_hits_scratch_bytes(m, n_hits))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_first_hits_of_lines_scratch_bytes");
    const int e = fmx::launch_first_hits(view.table, view.count, text.text_len, view.n_cu, m, d_hit_off, d_locs, n_hits, d_first_off, d_first_lines,
                                         d_first_locs, d_ws, ws_bytes, st);
    return e ? hip_fail("first hits of lines", e) : FMX_OK;
    });
}

size_t fmx_values_of_hits_groups_scratch_bytes(int32_t n, int64_t n_hits, int32_t max_len) {
    return fmx::values_groups_of_hits_scratch_bytes(n, n_hits, max_len);
}

int fmx_values_of_hits_groups_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const uint16_t *stop, int32_t n_stop, int32_t max_len,
                                  const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, int64_t *d_val_off, int32_t *d_count,
                                  int64_t *d_text_off, int32_t *d_group_of_hit, int32_t *d_status, void *d_ws, size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_hits < 0 || !d_val_off || !d_text_off || (n > 0 && (!d_hit_off || !term_len)) ||
        (n > 0 && n_hits > 0 && (!d_locs || !d_count || !d_group_of_hit)))
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_values_shape(stop, n_stop, max_len)) || (rc = fmx::check_values_hits(n_hits, max_len)) || (rc = fmx::check_term_len(n, term_len))) return rc;
    fmx::LineView view;
    fmx::TextView text;
    if ((rc = fmx::line_view(idx, &view)) || (rc = fmx::text_view(idx, &text))) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0 || n_hits == 0 || !text.extract) {
        FMX_HIP_TRY(hipMemsetAsync(d_val_off, 0, ((size_t)n + 1) * 8, st));
        FMX_HIP_TRY(hipMemsetAsync(d_text_off, 0, 8, st));
        if (n > 0 && n_hits > 0) {  // (an index without extraction: no groups, no hit has one)
            FMX_HIP_TRY(hipMemsetAsync(d_group_of_hit, 0xff, (size_t)n_hits * 4, st));
            const int e = fmx::launch_values_status_all(view.n_cu, d_status, n, FMX_ST_NOT_ENABLED, st);
            if (e) return hip_fail("groups of hits", e);
        }
        return FMX_OK;
    }
    if (!d_ws || ws_bytes < fmx::values_groups_of_hits_scratch_bytes(n, n_hits, max_len))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_values_of_hits_groups_scratch_bytes");
    return fmx::values_groups_run(idx, view, text, n, term_len, stop, n_stop, max_len, d_hit_off, d_locs, n_hits, d_val_off, d_count, d_text_off,
                                  d_group_of_hit, d_status, d_ws, ws_bytes, st);
    });
}

size_t fmx_numbers_by_key_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_permille) {
    return fmx::numbers_by_key_scratch_bytes(n, n_hits, n_permille);
}

int fmx_numbers_by_key_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const int32_t *by_of, int32_t m, const int64_t *val_off,
                           const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, const int64_t *d_first_off,
                           const int32_t *d_first_lines, const int32_t *d_group_of_first, int32_t frac_digits, const int32_t *permille,
                           int32_t n_permille, int64_t *d_row_off, int32_t *d_count, uint64_t *d_sum_lo, uint64_t *d_sum_hi, int64_t *d_min,
                           int64_t *d_max, int64_t *d_pct, int32_t *d_no_key, int32_t *d_not_number, int32_t *d_overflow, int32_t *d_status,
                           void *d_ws, size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || m < 0 || n_hits < 0 || (n > 0 && (!d_hit_off || !term_len || !by_of || !val_off || !d_row_off || !d_first_off)) ||
        (n > 0 && n_hits > 0 && !d_locs))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    int rc;
    if ((rc = fmx::check_numbers_shape(frac_digits, permille, n_permille)) || (rc = fmx::check_term_len(n, term_len))) return rc;
    std::vector<int64_t> row_off((size_t)n + 1, 0);
    if ((rc = check_rows(n, by_of, m, val_off, n_permille, row_off.data()))) return rc;
    fmx::LineView view;
    fmx::TextView text;
    if ((rc = fmx::line_view(idx, &view)) || (rc = fmx::text_view(idx, &text))) return rc;
    if (!view.table) return no_line_table();
    if (n == 0) return FMX_OK;
    const size_t R = (size_t)row_off[(size_t)n], P = (size_t)n_permille;
    if (R > 0 && (!d_count || !d_first_lines || !d_group_of_first)) return api_fail(FMX_E_ARG, "bad arguments");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Rows r{d_count, d_sum_lo, d_sum_hi, d_min, d_max, n_permille > 0 ? d_pct : nullptr, d_no_key, d_not_number, d_overflow};
    if (n_hits == 0 || !text.extract) {  // the rows and the per-pattern counters zeroed (an index without extraction: the statuses too)
        FMX_HIP_TRY(hipMemcpyAsync(d_row_off, row_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
        if ((rc = fmx::stat_rows_zero(r, R, P, n, st))) return rc;
        if (n_hits > 0) {
            const int e = fmx::launch_values_status_all(view.n_cu, d_status, n, FMX_ST_NOT_ENABLED, st);
            if (e) return hip_fail("numbers by key", e);
        }
        return FMX_OK;
    }
    if (!d_first_lines || !d_group_of_first) return api_fail(FMX_E_ARG, "bad arguments");
    if (!d_ws || ws_bytes < fmx::numbers_by_key_scratch_bytes(n, n_hits, n_permille))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_numbers_by_key_scratch_bytes");
    return rows_impl(idx, view, text, n, term_len, by_of, m, val_off, d_hit_off, d_locs, n_hits, FirstHits{d_first_off, d_first_lines, d_group_of_first},
                     frac_digits, permille, n_permille, d_row_off, r, d_status, d_ws, ws_bytes, st);
    });
}

int fmx_number_stats_by_batch(const fmx_index *idx, const uint16_t *key_pat, const int32_t *key_off, int32_t m, const uint16_t *pat,
                              const int32_t *pat_off, int32_t n, const int32_t *by_of, const uint16_t *term_pat, const int32_t *term_off,
                              int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q, const int32_t *key_where_of,
                              const int32_t *where_of, int32_t line_lo, int32_t line_hi, const uint16_t *stop, int32_t n_stop, int32_t max_len,
                              int32_t frac_digits, const int32_t *permille, int32_t n_permille, int64_t *val_off, int32_t **lines,
                              int64_t **text_off, uint16_t **chars, int64_t *row_off, int32_t **count, uint64_t **sum_lo, uint64_t **sum_hi,
                              int64_t **min, int64_t **max, int64_t **pct, int32_t *no_key, int32_t *not_number, int32_t *overflow,
                              int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *key_occurrences, int32_t *key_kept,
                              int32_t *key_status, int32_t *term_status) {
    return guarded([&]() -> int {
    const ByCall c{{m, n, by_of, n_terms, query_off, term_kind, q, key_where_of, where_of, stop, n_stop, max_len, frac_digits, permille, n_permille,
                    text_off, chars, count, sum_lo, sum_hi, min, max, pct, no_key, not_number, overflow, occurrences, kept, status, key_occurrences,
                    key_kept, key_status, term_status},
                   line_lo, line_hi, val_off, lines, row_off};
    null_results(c);
    if (!idx || m < 0 || n < 0 || n_terms < 0 || q < 0 || results_missing(c) || (m > 0 && (!key_off || !key_where_of)) ||
        (n > 0 && (!pat_off || !where_of || !by_of)) || (n_terms > 0 && !term_off))
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_literal_batches(pat_off, n, term_off, n_terms)) || (m > 0 && (rc = fmx::check_offsets(key_off, m, "key pattern")))) return rc;
    ByArgs a;
    bool done = false;
    if ((rc = by_call_args(idx, c, &a, &done)) || done) return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_keyed_literal_batch(key_pat, key_off, m, pat, pat_off, n, term_pat, term_off, n_terms, &merged, &batch, &a.term_len))) return rc;
    return by_call_run(idx, c, batch, a);
    });
}

int fmx_number_stats_by_class_batch(const fmx_index *idx, const uint16_t *key_alt, const int32_t *key_pos_off, int32_t key_n_pos,
                                    const int32_t *key_off, int32_t m, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                    const int32_t *pat_off, int32_t n, const int32_t *by_of, const uint16_t *term_alt, const int32_t *term_pos_off,
                                    int32_t term_n_pos, const int32_t *term_off, int32_t n_terms, int32_t max_ranges, const int32_t *query_off,
                                    const uint8_t *term_kind, int32_t q, const int32_t *key_where_of, const int32_t *where_of, int32_t line_lo,
                                    int32_t line_hi, const uint16_t *stop, int32_t n_stop, int32_t max_len, int32_t frac_digits,
                                    const int32_t *permille, int32_t n_permille, int64_t *val_off, int32_t **lines, int64_t **text_off,
                                    uint16_t **chars, int64_t *row_off, int32_t **count, uint64_t **sum_lo, uint64_t **sum_hi, int64_t **min,
                                    int64_t **max, int64_t **pct, int32_t *no_key, int32_t *not_number, int32_t *overflow, int32_t *occurrences,
                                    int32_t *kept, int32_t *status, int32_t *key_occurrences, int32_t *key_kept, int32_t *key_status,
                                    int32_t *term_status) {
    return guarded([&]() -> int {
    const ByCall c{{m, n, by_of, n_terms, query_off, term_kind, q, key_where_of, where_of, stop, n_stop, max_len, frac_digits, permille, n_permille,
                    text_off, chars, count, sum_lo, sum_hi, min, max, pct, no_key, not_number, overflow, occurrences, kept, status, key_occurrences,
                    key_kept, key_status, term_status},
                   line_lo, line_hi, val_off, lines, row_off};
    null_results(c);
    if (!idx || m < 0 || n < 0 || n_pos < 0 || key_n_pos < 0 || n_terms < 0 || term_n_pos < 0 || q < 0 || results_missing(c) || !pos_off || !pat_off ||
        !key_pos_off || !key_off || (m > 0 && !key_where_of) || (n > 0 && (!where_of || !by_of)) || (n_terms > 0 && (!term_pos_off || !term_off)) ||
        max_ranges < 1 || max_ranges > FMX_CLASS_RANGES_MAX)
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    // the key patterns are judged as the number patterns are: the terms' slot of the check takes them
    if ((rc = fmx::check_class_batches(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms)) ||
        (rc = fmx::check_class_batches(key_alt, key_pos_off, key_n_pos, key_off, m, nullptr, nullptr, 0, nullptr, 0)))
        return rc;
    ByArgs a;
    bool done = false;
    if ((rc = by_call_args(idx, c, &a, &done)) || done) return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_keyed_class_batch(key_alt, key_pos_off, key_n_pos, key_off, m, alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off,
                                           term_n_pos, term_off, n_terms, max_ranges, &merged, &batch, &a.term_len)))
        return rc;
    return by_call_run(idx, c, batch, a);
    });
}

}  // extern "C"
