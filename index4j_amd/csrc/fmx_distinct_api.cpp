// fmx_distinct_api.cpp — THE DISTINCT VALUES OF A FIELD PER BUCKET OF LINES, "dc(field) over time" (include/fmx.h "DISTINCT VALUES
// PER BUCKET"; fmx_distinct.hpp has the definition): the device stage fmx_values_distinct_histogram_dev over fmx_distinct.hip's
// launcher, and the host forms fmx_distinct_values_histogram_where_batch / fmx_distinct_values_histogram_where_class_batch.  Of a
// handle this file sees what fmx::line_view and fmx::text_view hand out; a host form runs the packed sequence of fmx_api.cpp up to
// the stage of this file (fmx::hits_stage_call) over ONE merged batch terms | value patterns, then the filter with the edges' span
// as its window, fmx_values_of_hits_groups_dev over the kept hits and ONE read of the group offsets (fmx::groups_front_stage, the
// front half it shares with the top values per bucket), the new stage and the two copies down.  No text is filled: the groups'
// text is never needed.
#include "fmx_distinct.hpp"
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

namespace {

using fmx::api_fail;
using fmx::guarded;
using fmx::hip_fail;
using fmx::no_line_table;
using fmx::zero;

// the shape of the answer and the HOST array that cuts it: the edges (none at all: one bucket, every line)
struct Shape {
    const int32_t *edges;
    int32_t n_edges, B;
};
int check_shape(int32_t n, const int32_t *edges, int32_t n_edges, Shape *s) {
    if (edges || n_edges != 0)
        if (const int rc = fmx::check_edges_array(edges, n_edges)) return rc;
    *s = Shape{edges, n_edges, edges ? n_edges - 1 : 1};
    if ((int64_t)n * s->B > fmx::kHistCellsMax) return api_fail(FMX_E_ARG, "more than 2^27 counters in one call (patterns * buckets)");
    return FMX_OK;
}
// the group offsets of a call (fm_dv_shape_bad's rules as messages; the shape has been judged by check_shape)
int check_groups(int32_t n, const int64_t *val_off, const Shape &s) {
    switch (fmx::fm_dv_shape_bad(n, val_off, s.B, nullptr)) {
        case 0: return FMX_OK;
        case 2: return api_fail(FMX_E_ARG, "val_off does not start at 0, decreases or holds more than 2^31 - 1 groups");
        default: return api_fail(FMX_E_ARG, "more than 2^27 counters in one call (patterns * buckets)");
    }
}

// ---- the host form --------------------------------------------------------------------------------------------------------------------
struct DistinctArgs : fmx::GroupsArgs {
    Shape shape{};
    int32_t *distinct = nullptr, *first_seen = nullptr;  // the caller's n * B ints each, zeroed before the stage runs
};

// n > 0 value patterns behind n_terms filter terms
int distinct_stage(const fmx::HitsBetween &h, void *arg) {
    DistinctArgs &a = *static_cast<DistinctArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const Shape &s = a.shape;
    const int32_t n = h.n;
    int rc;
    fmx::GroupsFront f{};
    bool done = false;
    if ((rc = fmx::groups_front_stage(h, a, false, "distinct values per bucket", &f, &done)) || done) return rc;  // (no hit is kept: the counters stay zero)
    auto block = [&](size_t bytes, auto **out) -> int { return h.block(h.call, bytes + 8, reinterpret_cast<void **>(out)); };
    if ((rc = check_groups(n, a.val_off.data(), s))) return rc;
    const size_t cells = (size_t)n * (size_t)s.B;
    int32_t *d_distinct = nullptr, *d_first = nullptr;
    void *ws_d = nullptr;
    const size_t d_bytes = fmx::values_distinct_histogram_scratch_bytes(n, a.val_off[(size_t)n], f.K, s.n_edges);
    if ((rc = block(cells * 4, &d_distinct)) || (rc = block(cells * 4, &d_first)) || (rc = block(d_bytes, &ws_d))) return rc;
    const int e = fmx::launch_values_distinct_histogram(s.edges ? h.view->table : nullptr, h.view->count, h.view->n_cu, n, a.val_off.data(), s.edges,
                                                        s.n_edges, f.part_off, f.locs, f.K, f.group, d_distinct, d_first, ws_d, d_bytes, st);
    if (e) return hip_fail("distinct values per bucket", e);
    FMX_HIP_TRY(hipMemcpyAsync(a.distinct, d_distinct, cells * 4, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipMemcpyAsync(a.first_seen, d_first, cells * 4, hipMemcpyDeviceToHost, st));
    return FMX_OK;
}

// what the two host forms take besides their batches, and what they hand back
struct DistinctCall {
    int32_t n, n_terms;
    const int32_t *query_off;
    const uint8_t *term_kind;
    int32_t q;
    const int32_t *where_of, *edges;
    int32_t n_edges;
    const uint16_t *stop;
    int32_t n_stop, max_len;
    int32_t *distinct, *first_seen, *n_values, *occurrences, *kept, *status, *term_status;
};

// the checks of the HOST arrays both forms share (behind their own batches'), the handle's views and the empty call; *done: answered
int distinct_call_args(const fmx_index *idx, const DistinctCall &c, DistinctArgs *a, bool *done) {
    int rc;
    fmx::LineView view;
    if ((rc = fmx::check_values_shape(c.stop, c.n_stop, c.max_len)) || (rc = fmx::check_query_arrays(c.n_terms, c.q, c.query_off, c.term_kind)) ||
        (rc = fmx::check_where_of(c.n, c.where_of, c.q)) || (rc = check_shape(c.n, c.edges, c.n_edges, &a->shape)) ||
        (rc = fmx::line_view(idx, &view)) || (rc = fmx::text_view(idx, &a->text)))
        return rc;
    // the window of the filter is the span of the edges: every kept hit has a bucket
    const int32_t lo = c.edges ? c.edges[0] : 0, hi = c.edges ? c.edges[c.n_edges - 1] : INT32_MAX;
    a->filter = fmx::HitsFilter{c.query_off, c.term_kind, c.q, c.where_of, lo, hi, fmx::hits_filter_asked(c.n, c.where_of, lo, hi)};
    if ((c.edges || a->filter.filters) && !view.table) return no_line_table();  // (the buckets and the filter are lines)
    const size_t cells = (size_t)c.n * (size_t)a->shape.B;
    zero(c.n_values, (size_t)c.n);
    zero(c.distinct, cells);
    zero(c.first_seen, cells);
    *done = c.n == 0;
    if (c.n == 0) {  // nothing is searched, the terms are not judged
        zero(c.term_status, (size_t)c.n_terms);
        return FMX_OK;
    }
    a->stop = c.stop;
    a->n_stop = c.n_stop;
    a->max_len = c.max_len;
    a->distinct = c.distinct;
    a->first_seen = c.first_seen;
    a->sized(c.n);
    return FMX_OK;
}

// the call over the merged batch terms | value patterns, and the answer into the caller's arrays
int distinct_call_run(const fmx_index *idx, const DistinctCall &c, const fmx::ValuesBatch &batch, DistinctArgs &a) {
    if (const int rc = fmx::hits_stage_call(idx, batch, distinct_stage, &a, c.occurrences, c.status, nullptr, c.term_status)) {
        const size_t cells = (size_t)c.n * (size_t)a.shape.B;  // (a copy of the stage may have arrived)
        zero(c.distinct, cells);
        zero(c.first_seen, cells);
        return rc;
    }
    fmx::kept_of(a.kept_off.data(), c.n, c.kept);
    for (int32_t i = 0; i < c.n && c.n_values; ++i) c.n_values[i] = (int32_t)(a.val_off[(size_t)i + 1] - a.val_off[(size_t)i]);
    return FMX_OK;
}

}  // namespace

extern "C" {

size_t fmx_values_distinct_histogram_scratch_bytes(int32_t n, int64_t n_groups, int64_t n_hits, int32_t n_edges) {
    return fmx::values_distinct_histogram_scratch_bytes(n, n_groups, n_hits, n_edges);
}

int fmx_values_distinct_histogram_dev(const fmx_index *idx, int32_t n, const int64_t *val_off, const int32_t *edges, int32_t n_edges,
                                      const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, const int32_t *d_group_of_hit,
                                      int32_t *d_distinct, int32_t *d_first_seen, void *d_ws, size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_hits < 0 || n_edges < 0 || (n > 0 && (!val_off || !d_hit_off || !d_distinct || !d_first_seen)) ||
        (n > 0 && n_hits > 0 && (!d_locs || !d_group_of_hit)))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    Shape s;
    int rc;
    if ((rc = check_shape(n, edges, n_edges, &s)) || (rc = check_groups(n, val_off, s))) return rc;
    fmx::LineView view;
    if ((rc = fmx::line_view(idx, &view))) return rc;
    if (edges && !view.table) return no_line_table();
    if (n == 0) return FMX_OK;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_hits == 0) {  // (no hit: every counter is zero)
        FMX_HIP_TRY(hipMemsetAsync(d_distinct, 0, (size_t)n * (size_t)s.B * 4, st));
        FMX_HIP_TRY(hipMemsetAsync(d_first_seen, 0, (size_t)n * (size_t)s.B * 4, st));
        return FMX_OK;
    }
    if (!d_ws || ws_bytes < fmx::values_distinct_histogram_scratch_bytes(n, val_off[n], n_hits, n_edges))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_values_distinct_histogram_scratch_bytes");
    const int e = fmx::launch_values_distinct_histogram(edges ? view.table : nullptr, view.count, view.n_cu, n, val_off, edges, n_edges, d_hit_off,
                                                        d_locs, n_hits, d_group_of_hit, d_distinct, d_first_seen, d_ws, ws_bytes, st);
    return e ? hip_fail("distinct values per bucket", e) : FMX_OK;
    });
}

int fmx_distinct_values_histogram_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                                              const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind,
                                              int32_t q, const int32_t *where_of, const int32_t *edges, int32_t n_edges, const uint16_t *stop,
                                              int32_t n_stop, int32_t max_len, int32_t *distinct, int32_t *first_seen, int32_t *n_values,
                                              int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *term_status) {
    return guarded([&]() -> int {
    const DistinctCall c{n, n_terms, query_off, term_kind, q, where_of, edges, n_edges, stop, n_stop, max_len, distinct, first_seen, n_values,
                         occurrences, kept, status, term_status};
    if (!idx || n < 0 || n_terms < 0 || q < 0 || n_edges < 0 || (n > 0 && (!pat_off || !where_of || !distinct || !first_seen)) ||
        (n_terms > 0 && !term_off))
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_literal_batches(pat_off, n, term_off, n_terms))) return rc;
    DistinctArgs a;
    bool done = false;
    if ((rc = distinct_call_args(idx, c, &a, &done)) || done) return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_literal_batch(pat, pat_off, n, term_pat, term_off, n_terms, &merged, &batch))) return rc;
    for (int32_t i = 0; i < n; ++i) a.term_len.push_back(pat_off[i + 1] - pat_off[i]);
    return distinct_call_run(idx, c, batch, a);
    });
}

int fmx_distinct_values_histogram_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                                    const int32_t *pat_off, int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off,
                                                    int32_t term_n_pos, const int32_t *term_off, int32_t n_terms, int32_t max_ranges,
                                                    const int32_t *query_off, const uint8_t *term_kind, int32_t q, const int32_t *where_of,
                                                    const int32_t *edges, int32_t n_edges, const uint16_t *stop, int32_t n_stop, int32_t max_len,
                                                    int32_t *distinct, int32_t *first_seen, int32_t *n_values, int32_t *occurrences, int32_t *kept,
                                                    int32_t *status, int32_t *term_status) {
    return guarded([&]() -> int {
    const DistinctCall c{n, n_terms, query_off, term_kind, q, where_of, edges, n_edges, stop, n_stop, max_len, distinct, first_seen, n_values,
                         occurrences, kept, status, term_status};
    if (!idx || n < 0 || n_pos < 0 || n_terms < 0 || term_n_pos < 0 || q < 0 || n_edges < 0 || !pos_off || !pat_off ||
        (n > 0 && (!where_of || !distinct || !first_seen)) || (n_terms > 0 && (!term_pos_off || !term_off)) || max_ranges < 1 ||
        max_ranges > FMX_CLASS_RANGES_MAX)
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_class_batches(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms))) return rc;
    DistinctArgs a;
    bool done = false;
    if ((rc = distinct_call_args(idx, c, &a, &done)) || done) return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_class_batch(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms, max_ranges, &merged,
                                     &batch)))
        return rc;
    for (int32_t i = 0; i < n; ++i) a.term_len.push_back(pat_off[i + 1] - pat_off[i]);  // (a position is a character)
    return distinct_call_run(idx, c, batch, a);
    });
}

}  // extern "C"
