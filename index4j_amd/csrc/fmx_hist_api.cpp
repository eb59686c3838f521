// fmx_hist_api.cpp — MATCHING LINES AND HITS PER BUCKET OF LINES, the timeline (include/fmx.h "LINES AND HITS PER BUCKET OF LINES"): the
// device stages fmx_lines_histogram_dev / fmx_hits_histogram_dev over fmx_line_hist.hip's launchers, and the host forms
// fmx_line_histogram_batch / fmx_hit_histogram_where_batch with their class twins.  Of a handle this file sees what fmx::line_view
// hands out; the host forms run the packed sequence of fmx_api.cpp up to a stage of this file (fmx::hits_stage_call):
//   lines form   the lines of the queries (fmx::query_lines_stage over the terms' hits, no limit), launch_lines_histogram over them;
//   hits form    fmx_field_values_where_batch's call without the values stage: the lines of the queries and the filter over the value
//                patterns' hits (fmx::kept_hits_stage, skipped when no pattern asks for a query), launch_hits_histogram over what is
//                kept.
// The checks of the batches, their merge and those two stages are the host-stage layer's (fmx_host_stage.hpp).  Only the counters
// and the small per-query, per-pattern and per-term arrays come down.
#include "fmx_host_stage.hpp"
#include "fmx_line_hist.hpp"

#include <hip/hip_runtime.h>

namespace {

using fmx::api_fail;
using fmx::guarded;
using fmx::no_line_table;
using fmx::zero;

// the HOST array of edges and the size of the answer: rows * B counters
int check_edges(const int32_t *edges, int32_t n_edges, int32_t rows) {
    if (const int rc = fmx::check_edges_array(edges, n_edges)) return rc;
    if ((int64_t)rows * (n_edges - 1) > fmx::kHistCellsMax)
        return api_fail(FMX_E_ARG, "more than 2^27 counters in one call (rows * buckets)");
    return FMX_OK;
}

// what the stages need of the call's arguments: the queries and the filter (fmx_host_stage.hpp), then the edges and the outputs
struct HistArgs : fmx::HitsFilter {
    const int32_t *edges;
    int32_t n_edges;
    int32_t *hist, *line_count;
    std::vector<int64_t> kept_off;  // hits form: n + 1, filled when the call has synchronised
};

// lines form: q > 0 queries over the n_terms terms of the batch (no value patterns)
int lines_stage(const fmx::HitsBetween &h, void *arg) {
    HistArgs &a = *static_cast<HistArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const size_t cells = (size_t)a.q * (size_t)(a.n_edges - 1), ws_bytes = fmx::lines_histogram_scratch_bytes(a.q, a.n_edges);
    int64_t *d_line_off = nullptr;
    int32_t *d_lines = nullptr, *d_hist = nullptr, *d_lcnt = nullptr;
    void *ws = nullptr;
    int rc;
    if ((rc = h.block(h.call, cells * 4 + 8, reinterpret_cast<void **>(&d_hist))) ||
        (rc = h.block(h.call, (size_t)a.q * 4 + 8, reinterpret_cast<void **>(&d_lcnt))) || (rc = h.block(h.call, ws_bytes, &ws)) ||
        (rc = fmx::query_lines_stage(h, a, &d_line_off, &d_lines, d_lcnt)))
        return rc;
    const int e = fmx::launch_lines_histogram(h.view->n_cu, a.q, d_line_off, d_lines, a.edges, a.n_edges, d_hist, ws, ws_bytes, st);
    if (e) return api_fail(FMX_E_HIP, std::string("lines per bucket: ") + hipGetErrorString((hipError_t)e));
    if (cells > 0) FMX_HIP_TRY(hipMemcpyAsync(a.hist, d_hist, cells * 4, hipMemcpyDeviceToHost, st));
    if (a.line_count) FMX_HIP_TRY(hipMemcpyAsync(a.line_count, d_lcnt, (size_t)a.q * 4, hipMemcpyDeviceToHost, st));
    return FMX_OK;
}

// hits form: n > 0 value patterns behind n_terms filter terms
int hits_stage(const fmx::HitsBetween &h, void *arg) {
    HistArgs &a = *static_cast<HistArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const int64_t value_hits = h.total - h.term_hits;
    const size_t cells = (size_t)h.n * (size_t)(a.n_edges - 1);
    int32_t *d_hist = nullptr;
    int rc;
    if ((rc = h.block(h.call, cells * 4 + 8, reinterpret_cast<void **>(&d_hist)))) return rc;
    const int64_t *d_off = nullptr;
    const int32_t *d_locs = nullptr;
    int64_t n_hits = 0;
    if (value_hits == 0) {
        if (cells > 0) FMX_HIP_TRY(hipMemsetAsync(d_hist, 0, cells * 4, st));
        a.kept_off.assign((size_t)h.n + 1, 0);
    } else {
        if ((rc = fmx::kept_hits_stage(h, a, &d_off, &d_locs, &n_hits))) return rc;
        const size_t ws_bytes = fmx::hits_histogram_scratch_bytes(h.n, n_hits, a.n_edges);
        void *ws = nullptr;
        if ((rc = h.block(h.call, ws_bytes, &ws))) return rc;
        const int e = fmx::launch_hits_histogram(h.view->table, h.view->count, h.view->n_cu, h.n, d_off, d_locs, n_hits, a.edges, a.n_edges, d_hist,
                                                 ws, ws_bytes, st);
        if (e) return api_fail(FMX_E_HIP, std::string("hits per bucket: ") + hipGetErrorString((hipError_t)e));
        FMX_HIP_TRY(hipMemcpyAsync(a.kept_off.data(), d_off, ((size_t)h.n + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    if (cells > 0) FMX_HIP_TRY(hipMemcpyAsync(a.hist, d_hist, cells * 4, hipMemcpyDeviceToHost, st));
    return FMX_OK;
}

// the checks the two lines forms share, behind their own batches'; *done: an empty call that has been answered
int lines_call_args(const fmx_index *idx, int32_t n, const int32_t *query_off, const uint8_t *term_kind, int32_t q, const int32_t *edges,
                    int32_t n_edges, int32_t *hist, int32_t *line_count, HistArgs *args, bool *done) {
    fmx::LineView view;
    int rc;
    if ((rc = fmx::check_query_arrays(n, q, query_off, term_kind)) || (rc = check_edges(edges, n_edges, q)) || (rc = fmx::line_view(idx, &view)))
        return rc;
    if (!view.table) return no_line_table();
    if ((rc = fmx::check_query_key_width(q, view.count, query_off))) return rc;
    *args = HistArgs{{query_off, term_kind, q, nullptr, 0, INT32_MAX, false}, edges, n_edges, hist, line_count, {}};
    *done = n == 0 || q == 0;
    if (*done) {  // (no terms: no query has a line; nothing is searched)
        zero(hist, (size_t)q * (size_t)(n_edges - 1));
        zero(line_count, (size_t)q);
    }
    return FMX_OK;
}

int hits_call_args(const fmx_index *idx, int32_t n, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                   const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t *hist, int32_t *term_status, HistArgs *args, bool *done) {
    fmx::LineView view;
    int rc;
    if ((rc = fmx::check_query_arrays(n_terms, q, query_off, term_kind)) || (rc = fmx::check_where_of(n, where_of, q)) ||
        (rc = check_edges(edges, n_edges, n)) || (rc = fmx::line_view(idx, &view)))
        return rc;
    if (!view.table) return no_line_table();  // (the buckets are lines: with or without a filter)
    *args = HistArgs{{query_off, term_kind, q, where_of, 0, INT32_MAX, fmx::hits_filter_asked(n, where_of)}, edges, n_edges, hist, nullptr,
                     std::vector<int64_t>((size_t)n + 1)};
    *done = n == 0;
    if (n == 0) zero(term_status, (size_t)n_terms);  // (nothing is searched: the terms are not judged)
    return FMX_OK;
}

}  // namespace

extern "C" {

size_t fmx_lines_histogram_scratch_bytes(int32_t q, int32_t n_edges) { return fmx::lines_histogram_scratch_bytes(q, n_edges); }
size_t fmx_hits_histogram_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_edges) { return fmx::hits_histogram_scratch_bytes(n, n_hits, n_edges); }

int fmx_lines_histogram_dev(const fmx_index *idx, int32_t q, const int64_t *d_line_off, const int32_t *d_lines, const int32_t *edges,
                            int32_t n_edges, int32_t *d_hist, void *d_ws, size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || q < 0 || n_edges < 0 || !edges || (q > 0 && (!d_line_off || !d_hist))) return api_fail(FMX_E_ARG, "bad arguments");
    int rc = check_edges(edges, n_edges, q);
    if (rc) return rc;
    fmx::LineView view;
    if ((rc = fmx::line_view(idx, &view))) return rc;
    if (q == 0) return FMX_OK;
    if (!d_ws || ws_bytes < fmx::lines_histogram_scratch_bytes(q, n_edges))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_lines_histogram_scratch_bytes");
    const int e = fmx::launch_lines_histogram(view.n_cu, q, d_line_off, d_lines, edges, n_edges, d_hist, d_ws, ws_bytes, stream);
    if (e) return api_fail(FMX_E_HIP, std::string("lines per bucket: ") + hipGetErrorString((hipError_t)e));
    return FMX_OK;
    });
}

int fmx_hits_histogram_dev(const fmx_index *idx, int32_t n, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, const int32_t *edges,
                           int32_t n_edges, int32_t *d_hist, void *d_ws, size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_hits < 0 || n_edges < 0 || !edges || (n > 0 && (!d_hit_off || !d_hist)) || (n > 0 && n_hits > 0 && !d_locs))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    int rc = check_edges(edges, n_edges, n);
    if (rc) return rc;
    fmx::LineView view;
    if ((rc = fmx::line_view(idx, &view))) return rc;
    if (!view.table) return no_line_table();
    if (n == 0) return FMX_OK;
    const size_t cells = (size_t)n * (size_t)(n_edges - 1);
    if (n_hits == 0) {
        FMX_HIP_TRY(hipMemsetAsync(d_hist, 0, cells * 4, static_cast<hipStream_t>(stream)));
        return FMX_OK;
    }
    if (!d_ws || ws_bytes < fmx::hits_histogram_scratch_bytes(n, n_hits, n_edges))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_hits_histogram_scratch_bytes");
    const int e = fmx::launch_hits_histogram(view.table, view.count, view.n_cu, n, d_hit_off, d_locs, n_hits, edges, n_edges, d_hist, d_ws,
                                             ws_bytes, stream);
    if (e) return api_fail(FMX_E_HIP, std::string("hits per bucket: ") + hipGetErrorString((hipError_t)e));
    return FMX_OK;
    });
}

int fmx_line_histogram_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const int32_t *query_off,
                             const uint8_t *term_kind, int32_t q, const int32_t *edges, int32_t n_edges, int32_t *hist, int32_t *line_count,
                             int32_t *occurrences, int32_t *status) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || q < 0 || n_edges < 0 || !edges || !query_off || (q > 0 && !hist) || (n > 0 && (!pat_off || !term_kind)))
        return api_fail(FMX_E_ARG, "bad arguments");
    HistArgs args;
    bool done = false;
    int rc;
    if ((rc = fmx::check_literal_batches(pat_off, n, nullptr, 0)) ||
        (rc = lines_call_args(idx, n, query_off, term_kind, q, edges, n_edges, hist, line_count, &args, &done)) || done)
        return rc;
    const fmx::ValuesBatch batch{pat, nullptr, 0, pat_off, n, 0, 0};
    return fmx::hits_stage_call(idx, batch, lines_stage, &args, nullptr, nullptr, occurrences, status);
    });
}

int fmx_line_histogram_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                   int32_t n, int32_t max_ranges, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                   const int32_t *edges, int32_t n_edges, int32_t *hist, int32_t *line_count, int32_t *occurrences,
                                   int32_t *status) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_pos < 0 || q < 0 || n_edges < 0 || !edges || !query_off || !pos_off || !pat_off || (q > 0 && !hist) ||
        (n > 0 && !term_kind) || max_ranges < 1 || max_ranges > FMX_CLASS_RANGES_MAX)
        return api_fail(FMX_E_ARG, "bad arguments");
    HistArgs args;
    bool done = false;
    int rc;
    if ((rc = fmx::check_class_batches(alt, pos_off, n_pos, pat_off, n, nullptr, nullptr, 0, nullptr, 0))) return rc;
    if ((rc = lines_call_args(idx, n, query_off, term_kind, q, edges, n_edges, hist, line_count, &args, &done)) || done) return rc;
    const fmx::ValuesBatch batch{alt, pos_off, n_pos, pat_off, n, 0, max_ranges};
    return fmx::hits_stage_call(idx, batch, lines_stage, &args, nullptr, nullptr, occurrences, status);
    });
}

int fmx_hit_histogram_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                                  const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                  const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t *hist, int32_t *occurrences,
                                  int32_t *kept, int32_t *status, int32_t *term_status) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_terms < 0 || q < 0 || n_edges < 0 || !edges || (n > 0 && (!pat_off || !where_of || !hist)) || (n_terms > 0 && !term_off))
        return api_fail(FMX_E_ARG, "bad arguments");
    HistArgs args;
    bool done = false;
    int rc;
    if ((rc = fmx::check_literal_batches(pat_off, n, term_off, n_terms))) return rc;
    if ((rc = hits_call_args(idx, n, n_terms, query_off, term_kind, q, where_of, edges, n_edges, hist, term_status, &args, &done)) || done) return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_literal_batch(pat, pat_off, n, term_pat, term_off, n_terms, &merged, &batch))) return rc;
    if ((rc = fmx::hits_stage_call(idx, batch, hits_stage, &args, occurrences, status, nullptr, term_status))) return rc;
    fmx::kept_of(args.kept_off.data(), n, kept);
    return FMX_OK;
    });
}

int fmx_hit_histogram_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                        int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off, int32_t term_n_pos,
                                        const int32_t *term_off, int32_t n_terms, int32_t max_ranges, const int32_t *query_off,
                                        const uint8_t *term_kind, int32_t q, const int32_t *where_of, const int32_t *edges, int32_t n_edges,
                                        int32_t *hist, int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *term_status) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_pos < 0 || n_terms < 0 || term_n_pos < 0 || q < 0 || n_edges < 0 || !edges || !pos_off || !pat_off ||
        (n > 0 && (!where_of || !hist)) || (n_terms > 0 && (!term_pos_off || !term_off)) || max_ranges < 1 || max_ranges > FMX_CLASS_RANGES_MAX)
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_class_batches(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms))) return rc;
    HistArgs args;
    bool done = false;
    if ((rc = hits_call_args(idx, n, n_terms, query_off, term_kind, q, where_of, edges, n_edges, hist, term_status, &args, &done)) || done) return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_class_batch(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms, max_ranges, &merged,
                                     &batch)))
        return rc;
    if ((rc = fmx::hits_stage_call(idx, batch, hits_stage, &args, occurrences, status, nullptr, term_status))) return rc;
    fmx::kept_of(args.kept_off.data(), n, kept);
    return FMX_OK;
    });
}

}  // extern "C"
