// fmx_where_api.cpp — FIELD VALUES AND HITS ONLY WITHIN THE LINES OF A QUERY (include/fmx.h "THE HITS THAT LIE IN GIVEN LINES", "THE
// VALUES THAT FOLLOW A PATTERN, WHERE THE LINE MATCHES A QUERY"): the device stage fmx_hits_in_lines_dev over fmx_hit_filter.hip's
// launcher, and the host forms fmx_field_values_where_batch / fmx_field_values_where_class_batch.  Of a handle this file sees what
// fmx::line_view hands out.  The host forms check and merge the filter terms and the value patterns into ONE batch
// (fmx_host_batch.cpp) and run the packed sequence of fmx_api.cpp (fmx::values_between_call) with the filter stage of
// fmx_host_stage.cpp between the fill and the values stages: the lines of the queries, then the filter over the value patterns' hits.
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

namespace {

using fmx::api_fail;
using fmx::guarded;

// the value patterns' hits that lie in the lines of their queries and in the window.  A call that does not filter needs no line
// table: every hit is kept.
int where_between(const fmx::HitsBetween &h, void *arg) {
    if (h.n == 0 || h.total - h.term_hits == 0) {
        FMX_HIP_TRY(hipMemsetAsync(h.kept_off, 0, ((size_t)h.n + 1) * sizeof(int64_t), static_cast<hipStream_t>(h.stream)));
        return FMX_OK;
    }
    return fmx::hits_in_lines_stage(h, *static_cast<const fmx::HitsFilter *>(arg), h.kept_off, h.kept_locs);
}

// what the two host forms share behind their own batches' checks; *done: an empty call that has been answered
int where_call_args(const fmx_index *idx, int32_t n, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                    const int32_t *where_of, int32_t line_lo, int32_t line_hi, int64_t *val_off, int32_t *term_status, fmx::HitsFilter *filter,
                    bool *done) {
    fmx::LineView view;
    int rc;
    if ((rc = fmx::check_query_arrays(n_terms, q, query_off, term_kind)) || (rc = fmx::check_where(n, where_of, q, line_lo, line_hi)) ||
        (rc = fmx::line_view(idx, &view)))
        return rc;
    *filter = fmx::HitsFilter{query_off, term_kind, q, where_of, line_lo, line_hi, fmx::hits_filter_asked(n, where_of, line_lo, line_hi)};
    if (filter->filters && !view.table) return fmx::no_line_table();
    *done = n == 0;
    if (n == 0) {  // (nothing is searched: the terms are not judged)
        val_off[0] = 0;
        fmx::zero(term_status, (size_t)n_terms);
    }
    return FMX_OK;
}

void null_outputs(int32_t **counts, int64_t **text_off, uint16_t **chars) {
    if (counts) *counts = nullptr;
    if (text_off) *text_off = nullptr;
    if (chars) *chars = nullptr;
}

}  // namespace

extern "C" {

size_t fmx_hits_in_lines_scratch_bytes(int32_t n, int64_t n_hits) { return fmx::hits_in_lines_scratch_bytes(n, n_hits); }

int fmx_hits_in_lines_dev(const fmx_index *idx, int32_t n, const int32_t *where_of, int32_t q, const int64_t *d_line_off, const int32_t *d_lines,
                          int32_t line_lo, int32_t line_hi, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits,
                          int64_t *d_kept_off, int32_t *d_kept_locs, void *d_ws, size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || q < 0 || n_hits < 0 || !d_kept_off || (n > 0 && (!where_of || !d_hit_off)) ||
        (n > 0 && n_hits > 0 && (!d_locs || !d_kept_locs)))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    int rc = fmx::check_where(n, where_of, q, line_lo, line_hi);
    if (rc) return rc;
    for (int32_t i = 0; i < n; ++i)
        if (where_of[i] >= 0 && !d_line_off) return api_fail(FMX_E_ARG, "bad arguments");
    fmx::LineView view;
    if ((rc = fmx::line_view(idx, &view))) return rc;
    if (!view.table) return fmx::no_line_table();
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0 || n_hits == 0) {
        FMX_HIP_TRY(hipMemsetAsync(d_kept_off, 0, ((size_t)n + 1) * sizeof(int64_t), st));
        return FMX_OK;
    }
    if (!d_ws || ws_bytes < fmx::hits_in_lines_scratch_bytes(n, n_hits))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_hits_in_lines_scratch_bytes");
    const int e = fmx::launch_hits_in_lines(view.table, view.count, view.n_cu, n, where_of, d_line_off, d_lines, line_lo, line_hi, d_hit_off,
                                            d_locs, n_hits, d_kept_off, d_kept_locs, d_ws, ws_bytes, stream);
    return e ? fmx::hip_fail("hits in lines", e) : FMX_OK;
    });
}

int fmx_field_values_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                                 const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                 const int32_t *where_of, int32_t line_lo, int32_t line_hi, const uint16_t *stop, int32_t n_stop,
                                 int32_t max_len, int64_t *val_off, int32_t **counts, int64_t **text_off, uint16_t **chars,
                                 int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *term_status) {
    return guarded([&]() -> int {
    null_outputs(counts, text_off, chars);
    if (!idx || n < 0 || n_terms < 0 || !val_off || !counts || !text_off || !chars || (n > 0 && !pat_off) || (n_terms > 0 && !term_off))
        return api_fail(FMX_E_ARG, "bad arguments");
    fmx::HitsFilter filter;
    bool done = false;
    int rc;
    if ((rc = fmx::check_values_shape(stop, n_stop, max_len)) || (rc = fmx::check_literal_batches(pat_off, n, term_off, n_terms)) ||
        (rc = where_call_args(idx, n, n_terms, query_off, term_kind, q, where_of, line_lo, line_hi, val_off, term_status, &filter, &done)) || done)
        return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_literal_batch(pat, pat_off, n, term_pat, term_off, n_terms, &merged, &batch))) return rc;
    return fmx::values_between_call(idx, batch, stop, n_stop, max_len, where_between, &filter, val_off, counts, text_off, chars, occurrences,
                                    status, kept, term_status);
    });
}

int fmx_field_values_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                       int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off, int32_t term_n_pos,
                                       const int32_t *term_off, int32_t n_terms, int32_t max_ranges, const int32_t *query_off,
                                       const uint8_t *term_kind, int32_t q, const int32_t *where_of, int32_t line_lo, int32_t line_hi,
                                       const uint16_t *stop, int32_t n_stop, int32_t max_len, int64_t *val_off, int32_t **counts,
                                       int64_t **text_off, uint16_t **chars, int32_t *occurrences, int32_t *kept, int32_t *status,
                                       int32_t *term_status) {
    return guarded([&]() -> int {
    null_outputs(counts, text_off, chars);
    if (!idx || n < 0 || n_pos < 0 || n_terms < 0 || term_n_pos < 0 || !val_off || !counts || !text_off || !chars || !pos_off || !pat_off ||
        (n_terms > 0 && (!term_pos_off || !term_off)) || max_ranges < 1 || max_ranges > FMX_CLASS_RANGES_MAX)
        return api_fail(FMX_E_ARG, "bad arguments");
    fmx::HitsFilter filter;
    bool done = false;
    int rc;
    if ((rc = fmx::check_values_shape(stop, n_stop, max_len)) ||
        (rc = fmx::check_class_batches(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms)) ||
        (rc = where_call_args(idx, n, n_terms, query_off, term_kind, q, where_of, line_lo, line_hi, val_off, term_status, &filter, &done)) || done)
        return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_class_batch(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms, max_ranges, &merged,
                                     &batch)))
        return rc;
    return fmx::values_between_call(idx, batch, stop, n_stop, max_len, where_between, &filter, val_off, counts, text_off, chars, occurrences,
                                    status, kept, term_status);
    });
}

}  // extern "C"
