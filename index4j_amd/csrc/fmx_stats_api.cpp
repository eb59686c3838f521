// fmx_stats_api.cpp — STATISTICS OF THE NUMBER BEHIND A PATTERN, PER BUCKET OF LINES (include/fmx.h "THE NUMBER BEHIND A PATTERN"):
// the device stage fmx_numbers_of_hits_dev over fmx_hit_numbers.hip's launchers with the packed extract between them, and the host
// forms fmx_number_stats_where_batch / fmx_number_stats_where_class_batch.  Of a handle this file sees what fmx::line_view and
// fmx::text_view hand out; the host forms run the packed sequence of fmx_api.cpp up to the stage of this file
// (fmx::hits_stage_call), as fmx_hit_histogram_where_batch does: the lines of the queries and the filter over the value patterns'
// hits (fmx::kept_hits_stage, skipped when no pattern asks for a query), then the numbers stage over what is kept.  The checks of
// the batches, their merge and that stage are the host-stage layer's (fmx_host_stage.hpp).  Only the rows and the small per-pattern
// and per-term arrays come down.
#include "fmx_hit_numbers.hpp"
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

namespace {

using fmx::api_fail;
using fmx::guarded;
using fmx::hip_fail;
using fmx::no_line_table;
using fmx::zero;

// the shape of the answer and the HOST arrays that cut it: the edges (none at all: one bucket, every line), the permilles
struct Shape {
    const int32_t *edges;
    int32_t n_edges, B, frac_digits;
    const int32_t *permille;
    int32_t P;
    size_t cells(int32_t n) const { return (size_t)n * (size_t)B; }
};
int check_shape(int32_t n, const int32_t *edges, int32_t n_edges, int32_t frac_digits, const int32_t *permille, int32_t n_permille, Shape *s) {
    int rc;
    if ((rc = fmx::check_numbers_shape(frac_digits, permille, n_permille)) || ((edges || n_edges != 0) && (rc = fmx::check_edges_array(edges, n_edges))))
        return rc;
    *s = Shape{edges, n_edges, edges ? n_edges - 1 : 1, frac_digits, permille, n_permille};
    const int64_t cells = (int64_t)n * s->B;
    if (cells > fmx::kHistCellsMax) return api_fail(FMX_E_ARG, "more than 2^27 rows in one call (patterns * buckets)");
    if (cells * (n_permille > 0 ? n_permille : 1) > fmx::kHistCellsMax)
        return api_fail(FMX_E_ARG, "more than 2^27 percentiles in one call (patterns * buckets * n_permille)");
    return FMX_OK;
}

// the outputs of the stage, on the device or on the host: count is required, every other one nullable, no_key is never there
using Rows = fmx::StatRows;

// the three steps behind the arguments' checks (n > 0, n_hits > 0, the workspace large enough): the windows and keys, the windows'
// text, the rows.  An index without extraction: zero rows, FMX_ST_NOT_ENABLED for every pattern.
int numbers_impl(const fmx_index *idx, const fmx::LineView &view, const fmx::TextView &text, int32_t n, const int32_t *term_len,
                 const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, const Shape &s, const Rows &r, int32_t *d_status, void *ws,
                 size_t ws_bytes, hipStream_t st) {
    if (!text.extract) {
        if (const int rc = fmx::stat_rows_zero(r, s.cells(n), (size_t)s.P, n, st)) return rc;
        const int e = fmx::launch_values_status_all(view.n_cu, d_status, n, FMX_ST_NOT_ENABLED, st);
        return e ? hip_fail("numbers of hits", e) : FMX_OK;
    }
    fmx::ValuesWindows w;
    if (!fmx::numbers_windows(ws, ws_bytes, n, n_hits, s.n_edges, s.P, &w))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_numbers_of_hits_scratch_bytes");
    int e = fmx::launch_numbers_ranges(view.table, view.count, text.text_len, view.n_cu, n, term_len, d_hit_off, d_locs, n_hits, s.edges, s.n_edges,
                                       s.permille, s.P, ws, ws_bytes, st);
    if (e) return hip_fail("windows of hits", e);
    if (const int rc = fmx::extract_windows(idx, w, (int32_t)n_hits, st)) return rc;
    e = fmx::launch_numbers_rows(view.n_cu, n, d_hit_off, n_hits, s.n_edges, s.frac_digits, s.P, r.count, r.sum_lo, r.sum_hi, r.min, r.max, r.pct,
                                 r.not_number, r.overflow, d_status, ws, ws_bytes, st);
    return e ? hip_fail("numbers of hits", e) : FMX_OK;
}

// what the host forms' stage needs of the call's arguments
struct StatsArgs {
    fmx::HitsFilter filter;
    Shape shape;
    fmx::TextView text;
    std::vector<int32_t> term_len;  // the value patterns'
    Rows host;
    std::vector<int64_t> kept_off;  // n + 1, filled when the call has synchronised
};

void zero_host_rows(const Rows &r, int32_t n, const Shape &s) {
    const size_t cells = s.cells(n);
    zero(r.count, cells);
    zero(r.sum_lo, cells);
    zero(r.sum_hi, cells);
    zero(r.min, cells);
    zero(r.max, cells);
    zero(r.pct, cells * (size_t)s.P);
    zero(r.not_number, (size_t)n);
    zero(r.overflow, (size_t)n);
}

// n > 0 value patterns behind n_terms filter terms
int stats_stage(const fmx::HitsBetween &h, void *arg) {
    StatsArgs &a = *static_cast<StatsArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const Shape &s = a.shape;
    const size_t cells = s.cells(h.n), P = (size_t)s.P;
    if (h.total - h.term_hits == 0) {  // (no value pattern has a hit: nothing runs on the device)
        zero_host_rows(a.host, h.n, s);
        a.kept_off.assign((size_t)h.n + 1, 0);
        return a.text.extract ? FMX_OK : fmx::status_all(h, FMX_ST_NOT_ENABLED, "numbers of hits");
    }
    Rows d;
    int rc;
    if ((rc = fmx::stat_rows_blocks(h, &a.host, cells, P, h.n, &d))) return rc;
    const int64_t *d_off = nullptr;
    const int32_t *d_locs = nullptr;
    int64_t n_hits = 0;
    if ((rc = fmx::kept_hits_stage(h, a.filter, &d_off, &d_locs, &n_hits))) return rc;
    const size_t ws_bytes = a.text.extract ? fmx::numbers_of_hits_scratch_bytes(h.n, n_hits, s.n_edges, s.P) : 0;
    void *ws = nullptr;
    if (ws_bytes > 0 && (rc = h.block(h.call, ws_bytes, &ws))) return rc;
    if ((rc = numbers_impl(h.idx, *h.view, a.text, h.n, a.term_len.data(), d_off, d_locs, n_hits, s, d, h.status, ws, ws_bytes, st))) return rc;
    FMX_HIP_TRY(hipMemcpyAsync(a.kept_off.data(), d_off, ((size_t)h.n + 1) * 8, hipMemcpyDeviceToHost, st));
    return fmx::stat_rows_down(a.host, d, cells, P, h.n, st);
}

// the checks the two host forms share, behind their own batches'; *done: an empty call that has been answered
int stats_call_args(const fmx_index *idx, int32_t n, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                    const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t frac_digits, const int32_t *permille,
                    int32_t n_permille, const Rows &host, int32_t *term_status, StatsArgs *args, bool *done) {
    fmx::LineView view;
    int rc;
    if ((rc = fmx::check_query_arrays(n_terms, q, query_off, term_kind)) || (rc = fmx::check_where_of(n, where_of, q)) ||
        (rc = check_shape(n, edges, n_edges, frac_digits, permille, n_permille, &args->shape)) || (rc = fmx::line_view(idx, &view)) ||
        (rc = fmx::text_view(idx, &args->text)))
        return rc;
    args->filter = fmx::HitsFilter{query_off, term_kind, q, where_of, 0, INT32_MAX, fmx::hits_filter_asked(n, where_of)};
    if ((edges || args->filter.filters) && !view.table) return no_line_table();  // (the buckets and the filter are lines)
    args->host = host;
    args->kept_off.assign((size_t)n + 1, 0);
    *done = n == 0;
    if (n == 0) zero(term_status, (size_t)n_terms);  // (nothing is searched: the terms are not judged)
    return FMX_OK;
}

}  // namespace

extern "C" {

size_t fmx_numbers_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_edges, int32_t n_permille) {
    return fmx::numbers_of_hits_scratch_bytes(n, n_hits, n_edges, n_permille);
}

int fmx_numbers_of_hits_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const int64_t *d_hit_off, const int32_t *d_locs,
                            int64_t n_hits, const int32_t *edges, int32_t n_edges, int32_t frac_digits, const int32_t *permille,
                            int32_t n_permille, int32_t *d_count, uint64_t *d_sum_lo, uint64_t *d_sum_hi, int64_t *d_min, int64_t *d_max,
                            int64_t *d_pct, int32_t *d_not_number, int32_t *d_overflow, int32_t *d_status, void *d_ws, size_t ws_bytes,
                            void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_hits < 0 || n_edges < 0 || (n > 0 && (!d_hit_off || !term_len || !d_count)) || (n > 0 && n_hits > 0 && !d_locs))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    Shape s;
    int rc = check_shape(n, edges, n_edges, frac_digits, permille, n_permille, &s);
    if (rc) return rc;
    if ((rc = fmx::check_term_len(n, term_len))) return rc;
    fmx::LineView view;
    fmx::TextView text;
    if ((rc = fmx::line_view(idx, &view)) || (rc = fmx::text_view(idx, &text))) return rc;
    if (edges && !view.table) return no_line_table();
    if (n == 0) return FMX_OK;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Rows rows{d_count, d_sum_lo, d_sum_hi, d_min, d_max, n_permille > 0 ? d_pct : nullptr, nullptr, d_not_number, d_overflow};
    if (n_hits == 0) return fmx::stat_rows_zero(rows, s.cells(n), (size_t)s.P, n, st);
    if (!d_ws || ws_bytes < fmx::numbers_of_hits_scratch_bytes(n, n_hits, n_edges, n_permille))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_numbers_of_hits_scratch_bytes");
    return numbers_impl(idx, view, text, n, term_len, d_hit_off, d_locs, n_hits, s, rows, d_status, d_ws, ws_bytes, st);
    });
}

int fmx_number_stats_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                                 const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                 const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t frac_digits, const int32_t *permille,
                                 int32_t n_permille, int32_t *count, uint64_t *sum_lo, uint64_t *sum_hi, int64_t *min, int64_t *max,
                                 int64_t *pct, int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept, int32_t *status,
                                 int32_t *term_status) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_terms < 0 || q < 0 || n_edges < 0 || (n > 0 && (!pat_off || !where_of || !count)) || (n_terms > 0 && !term_off))
        return api_fail(FMX_E_ARG, "bad arguments");
    StatsArgs args;
    bool done = false;
    int rc;
    if ((rc = fmx::check_literal_batches(pat_off, n, term_off, n_terms))) return rc;
    if ((rc = stats_call_args(idx, n, n_terms, query_off, term_kind, q, where_of, edges, n_edges, frac_digits, permille, n_permille,
                              Rows{count, sum_lo, sum_hi, min, max, pct, nullptr, not_number, overflow}, term_status, &args, &done)) ||
        done)
        return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_literal_batch(pat, pat_off, n, term_pat, term_off, n_terms, &merged, &batch))) return rc;
    for (int32_t i = 0; i < n; ++i) args.term_len.push_back(pat_off[i + 1] - pat_off[i]);
    if ((rc = fmx::hits_stage_call(idx, batch, stats_stage, &args, occurrences, status, nullptr, term_status))) return rc;
    fmx::kept_of(args.kept_off.data(), n, kept);
    return FMX_OK;
    });
}

int fmx_number_stats_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                       int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off, int32_t term_n_pos,
                                       const int32_t *term_off, int32_t n_terms, int32_t max_ranges, const int32_t *query_off,
                                       const uint8_t *term_kind, int32_t q, const int32_t *where_of, const int32_t *edges, int32_t n_edges,
                                       int32_t frac_digits, const int32_t *permille, int32_t n_permille, int32_t *count, uint64_t *sum_lo,
                                       uint64_t *sum_hi, int64_t *min, int64_t *max, int64_t *pct, int32_t *not_number, int32_t *overflow,
                                       int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *term_status) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_pos < 0 || n_terms < 0 || term_n_pos < 0 || q < 0 || n_edges < 0 || !pos_off || !pat_off ||
        (n > 0 && (!where_of || !count)) || (n_terms > 0 && (!term_pos_off || !term_off)) || max_ranges < 1 || max_ranges > FMX_CLASS_RANGES_MAX)
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_class_batches(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms))) return rc;
    StatsArgs args;
    bool done = false;
    if ((rc = stats_call_args(idx, n, n_terms, query_off, term_kind, q, where_of, edges, n_edges, frac_digits, permille, n_permille,
                              Rows{count, sum_lo, sum_hi, min, max, pct, nullptr, not_number, overflow}, term_status, &args, &done)) ||
        done)
        return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_class_batch(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms, max_ranges, &merged,
                                     &batch)))
        return rc;
    for (int32_t i = 0; i < n; ++i) args.term_len.push_back(pat_off[i + 1] - pat_off[i]);  // (a position is a character)
    if ((rc = fmx::hits_stage_call(idx, batch, stats_stage, &args, occurrences, status, nullptr, term_status))) return rc;
    fmx::kept_of(args.kept_off.data(), n, kept);
    return FMX_OK;
    });
}

}  // extern "C"
