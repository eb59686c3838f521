// fmx_top_api.cpp — THE LINES RANKED BY THE NUMBER BEHIND A PATTERN (include/fmx.h "THE LINES RANKED BY THE NUMBER BEHIND A PATTERN"):
// the device stage fmx_top_lines_of_hits_dev over fmx_hit_top.hip's launchers with the packed extract between them, and the host
// forms fmx_top_lines_where_batch / fmx_top_lines_where_class_batch.  Of a handle this file sees what fmx::line_view and
// fmx::text_view hand out; the host forms run the packed sequence of fmx_api.cpp up to the stage of this file
// (fmx::hits_stage_call), as fmx_number_stats_where_batch does: the lines of the queries and the filter over the value patterns'
// hits (fmx::kept_hits_stage, skipped when the call does not filter), then the ranking stage over what is kept.  Only the n x top
// rows and the small per-pattern and per-term arrays come down, never the hits.
#include "fmx_hit_top.hpp"
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

namespace {

using fmx::api_fail;
using fmx::guarded;
using fmx::hip_fail;
using fmx::no_line_table;
using fmx::zero;

// the shape of the answer: which ranks, of which parse
struct Shape {
    int32_t frac_digits, first, top;
    size_t cells(int32_t n) const { return (size_t)n * (size_t)top; }
};
int check_shape(int32_t n, const int32_t *term_len, const uint8_t *descending, int32_t frac_digits, int32_t first, int32_t top, Shape *s) {
    switch (fmx::fm_top_args_bad(n, term_len, descending, frac_digits, first, top)) {
        case 0: break;
        case 1: return api_fail(FMX_E_ARG, "frac_digits is outside [0, 9]");
        case 2: return api_fail(FMX_E_ARG, "a term_len is negative");
        case 3: return api_fail(FMX_E_ARG, "first is negative");
        case 4: return api_fail(FMX_E_ARG, "top is below 1");
        case 5: return api_fail(FMX_E_ARG, "more than 2^27 rows in one call (patterns * top)");
        default: return api_fail(FMX_E_ARG, "bad arguments");
    }
    *s = Shape{frac_digits, first, top};
    return FMX_OK;
}

// the outputs of the stage, on the device or on the host: rows is required, every other one nullable
struct Rows {
    int32_t *rows, *row_line;
    int64_t *row_value;
    int32_t *row_loc, *lines, *numbers, *not_number, *overflow;
};

// rows and per-pattern counters of the device, all zero
int zero_rows(const Rows &r, int32_t n, const Shape &s, hipStream_t st) {
    const size_t cells = s.cells(n);
    for (int32_t *p : {r.row_line, r.row_loc})
        if (p && cells > 0) FMX_HIP_TRY(hipMemsetAsync(p, 0, cells * 4, st));
    if (r.row_value && cells > 0) FMX_HIP_TRY(hipMemsetAsync(r.row_value, 0, cells * 8, st));
    for (int32_t *p : {r.rows, r.lines, r.numbers, r.not_number, r.overflow})
        if (p && n > 0) FMX_HIP_TRY(hipMemsetAsync(p, 0, (size_t)n * 4, st));
    return FMX_OK;
}

// the three steps behind the arguments' checks (n > 0, n_hits > 0, the workspace large enough, a line table): the windows and keys,
// the windows' text, the ranking.  An index without extraction: zero rows, FMX_ST_NOT_ENABLED for every pattern.
int top_impl(const fmx_index *idx, const fmx::LineView &view, const fmx::TextView &text, int32_t n, const int32_t *term_len,
             const uint8_t *descending, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, const Shape &s, const Rows &r,
             int32_t *d_status, void *ws, size_t ws_bytes, hipStream_t st) {
    if (!text.extract) {
        if (const int rc = zero_rows(r, n, s, st)) return rc;
        const int e = fmx::launch_values_status_all(view.n_cu, d_status, n, FMX_ST_NOT_ENABLED, st);
        return e ? hip_fail("top lines of hits", e) : FMX_OK;
    }
    fmx::ValuesWindows w;
    if (!fmx::top_lines_windows(ws, ws_bytes, n, n_hits, s.top, &w))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_top_lines_of_hits_scratch_bytes");
    int e = fmx::launch_top_lines_windows(text.text_len, view.n_cu, n, term_len, descending, d_hit_off, d_locs, n_hits, s.top, ws, ws_bytes, st);
    if (e) return hip_fail("windows of hits", e);
    if (const int rc = fmx::extract_windows(idx, w, (int32_t)n_hits, st)) return rc;
    e = fmx::launch_top_lines_rows(view.table, view.count, text.text_len, view.n_cu, n, d_hit_off, n_hits, s.frac_digits, s.first, s.top, r.rows,
                                   r.row_line, r.row_value, r.row_loc, r.lines, r.numbers, r.not_number, r.overflow, d_status, ws, ws_bytes, st);
    return e ? hip_fail("top lines of hits", e) : FMX_OK;
}

// what the host forms' stage needs of the call's arguments
struct TopArgs {
    fmx::HitsFilter filter;
    Shape shape;
    fmx::TextView text;
    std::vector<int32_t> term_len;  // the value patterns'
    const uint8_t *descending;
    Rows host;
    std::vector<int64_t> kept_off;  // n + 1, filled when the call has synchronised
};

void zero_host_rows(const Rows &r, int32_t n, const Shape &s) {
    const size_t cells = s.cells(n);
    zero(r.row_line, cells);
    zero(r.row_value, cells);
    zero(r.row_loc, cells);
    zero(r.rows, (size_t)n);
    zero(r.lines, (size_t)n);
    zero(r.numbers, (size_t)n);
    zero(r.not_number, (size_t)n);
    zero(r.overflow, (size_t)n);
}

// n > 0 value patterns behind n_terms filter terms
int top_stage(const fmx::HitsBetween &h, void *arg) {
    TopArgs &a = *static_cast<TopArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const Shape &s = a.shape;
    const size_t cells = s.cells(h.n);
    if (h.total - h.term_hits == 0) {  // (no value pattern has a hit: nothing runs on the device)
        zero_host_rows(a.host, h.n, s);
        a.kept_off.assign((size_t)h.n + 1, 0);
        return a.text.extract ? FMX_OK : fmx::status_all(h, FMX_ST_NOT_ENABLED, "top lines of hits");
    }
    Rows d{};
    int rc;
    auto room = [&](const void *wanted, size_t bytes, auto **out) -> int {
        return wanted ? h.block(h.call, bytes + 8, reinterpret_cast<void **>(out)) : FMX_OK;
    };
    if ((rc = room(a.host.rows, (size_t)h.n * 4, &d.rows)) || (rc = room(a.host.row_line, cells * 4, &d.row_line)) ||
        (rc = room(a.host.row_value, cells * 8, &d.row_value)) || (rc = room(a.host.row_loc, cells * 4, &d.row_loc)) ||
        (rc = room(a.host.lines, (size_t)h.n * 4, &d.lines)) || (rc = room(a.host.numbers, (size_t)h.n * 4, &d.numbers)) ||
        (rc = room(a.host.not_number, (size_t)h.n * 4, &d.not_number)) || (rc = room(a.host.overflow, (size_t)h.n * 4, &d.overflow)))
        return rc;
    const int64_t *d_off = nullptr;
    const int32_t *d_locs = nullptr;
    int64_t n_hits = 0;
    if ((rc = fmx::kept_hits_stage(h, a.filter, &d_off, &d_locs, &n_hits))) return rc;
    const size_t ws_bytes = a.text.extract ? fmx::top_lines_of_hits_scratch_bytes(h.n, n_hits, s.top) : 0;
    void *ws = nullptr;
    if (ws_bytes > 0 && (rc = h.block(h.call, ws_bytes, &ws))) return rc;
    if ((rc = top_impl(h.idx, *h.view, a.text, h.n, a.term_len.data(), a.descending, d_off, d_locs, n_hits, s, d, h.status, ws, ws_bytes, st)))
        return rc;
    FMX_HIP_TRY(hipMemcpyAsync(a.kept_off.data(), d_off, ((size_t)h.n + 1) * 8, hipMemcpyDeviceToHost, st));
    auto down = [&](void *host, const void *dev, size_t bytes) -> hipError_t {
        return host && bytes > 0 ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    FMX_HIP_TRY(down(a.host.rows, d.rows, (size_t)h.n * 4));
    FMX_HIP_TRY(down(a.host.row_line, d.row_line, cells * 4));
    FMX_HIP_TRY(down(a.host.row_value, d.row_value, cells * 8));
    FMX_HIP_TRY(down(a.host.row_loc, d.row_loc, cells * 4));
    FMX_HIP_TRY(down(a.host.lines, d.lines, (size_t)h.n * 4));
    FMX_HIP_TRY(down(a.host.numbers, d.numbers, (size_t)h.n * 4));
    FMX_HIP_TRY(down(a.host.not_number, d.not_number, (size_t)h.n * 4));
    FMX_HIP_TRY(down(a.host.overflow, d.overflow, (size_t)h.n * 4));
    return FMX_OK;
}

// the checks the two host forms share, behind their own batches'; *done: an empty call that has been answered.  The pattern
// lengths are made by the caller from its own offsets (judged by then).
int top_call_args(const fmx_index *idx, int32_t n, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                  const int32_t *where_of, int32_t line_lo, int32_t line_hi, const uint8_t *descending, int32_t frac_digits, int32_t first,
                  int32_t top, const Rows &host, int32_t *term_status, TopArgs *args, bool *done) {
    fmx::LineView view;
    int rc;
    if ((rc = fmx::check_query_arrays(n_terms, q, query_off, term_kind)) || (rc = fmx::check_where(n, where_of, q, line_lo, line_hi)) ||
        (rc = check_shape(n, args->term_len.data(), descending, frac_digits, first, top, &args->shape)) || (rc = fmx::line_view(idx, &view)) ||
        (rc = fmx::text_view(idx, &args->text)))
        return rc;
    if (!view.table) return no_line_table();  // (the answer is lines)
    args->filter = fmx::HitsFilter{query_off, term_kind, q, where_of, line_lo, line_hi, fmx::hits_filter_asked(n, where_of, line_lo, line_hi)};
    args->descending = descending;
    args->host = host;
    args->kept_off.assign((size_t)n + 1, 0);
    *done = n == 0;
    if (n == 0) zero(term_status, (size_t)n_terms);  // (nothing is searched: the terms are not judged)
    return FMX_OK;
}

}  // namespace

extern "C" {

size_t fmx_top_lines_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t top) { return fmx::top_lines_of_hits_scratch_bytes(n, n_hits, top); }

int fmx_top_lines_of_hits_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const uint8_t *descending, const int64_t *d_hit_off,
                              const int32_t *d_locs, int64_t n_hits, int32_t frac_digits, int32_t first, int32_t top, int32_t *d_rows,
                              int32_t *d_row_line, int64_t *d_row_value, int32_t *d_row_loc, int32_t *d_lines, int32_t *d_numbers,
                              int32_t *d_not_number, int32_t *d_overflow, int32_t *d_status, void *d_ws, size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_hits < 0 || (n > 0 && (!d_hit_off || !term_len || !descending || !d_rows)) || (n > 0 && n_hits > 0 && !d_locs))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    Shape s;
    int rc = check_shape(n, term_len, descending, frac_digits, first, top, &s);
    if (rc) return rc;
    fmx::LineView view;
    fmx::TextView text;
    if ((rc = fmx::line_view(idx, &view)) || (rc = fmx::text_view(idx, &text))) return rc;
    if (!view.table) return no_line_table();
    if (n == 0) return FMX_OK;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Rows rows{d_rows, d_row_line, d_row_value, d_row_loc, d_lines, d_numbers, d_not_number, d_overflow};
    if (n_hits == 0) return zero_rows(rows, n, s, st);
    const size_t need = fmx::top_lines_of_hits_scratch_bytes(n, n_hits, top);
    if (text.extract && (!d_ws || need == 0 || ws_bytes < need))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_top_lines_of_hits_scratch_bytes");
    return top_impl(idx, view, text, n, term_len, descending, d_hit_off, d_locs, n_hits, s, rows, d_status, d_ws, ws_bytes, st);
    });
}

int fmx_top_lines_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                              const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                              const int32_t *where_of, int32_t line_lo, int32_t line_hi, const uint8_t *descending, int32_t frac_digits,
                              int32_t first, int32_t top, int32_t *rows, int32_t *row_line, int64_t *row_value, int32_t *row_loc, int32_t *lines,
                              int32_t *numbers, int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept, int32_t *status,
                              int32_t *term_status) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_terms < 0 || q < 0 || (n > 0 && (!pat_off || !where_of || !descending || !rows)) || (n_terms > 0 && !term_off))
        return api_fail(FMX_E_ARG, "bad arguments");
    TopArgs args;
    bool done = false;
    int rc;
    if ((rc = fmx::check_literal_batches(pat_off, n, term_off, n_terms))) return rc;
    for (int32_t i = 0; i < n; ++i) args.term_len.push_back(pat_off[i + 1] - pat_off[i]);
    if ((rc = top_call_args(idx, n, n_terms, query_off, term_kind, q, where_of, line_lo, line_hi, descending, frac_digits, first, top,
                            Rows{rows, row_line, row_value, row_loc, lines, numbers, not_number, overflow}, term_status, &args, &done)) ||
        done)
        return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_literal_batch(pat, pat_off, n, term_pat, term_off, n_terms, &merged, &batch))) return rc;
    if ((rc = fmx::hits_stage_call(idx, batch, top_stage, &args, occurrences, status, nullptr, term_status))) return rc;
    fmx::kept_of(args.kept_off.data(), n, kept);
    return FMX_OK;
    });
}

int fmx_top_lines_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                    int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off,
                                    int32_t n_terms, int32_t max_ranges, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                    const int32_t *where_of, int32_t line_lo, int32_t line_hi, const uint8_t *descending, int32_t frac_digits,
                                    int32_t first, int32_t top, int32_t *rows, int32_t *row_line, int64_t *row_value, int32_t *row_loc,
                                    int32_t *lines, int32_t *numbers, int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept,
                                    int32_t *status, int32_t *term_status) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_pos < 0 || n_terms < 0 || term_n_pos < 0 || q < 0 || !pos_off || !pat_off ||
        (n > 0 && (!where_of || !descending || !rows)) || (n_terms > 0 && (!term_pos_off || !term_off)) || max_ranges < 1 ||
        max_ranges > FMX_CLASS_RANGES_MAX)
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_class_batches(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms))) return rc;
    TopArgs args;
    bool done = false;
    for (int32_t i = 0; i < n; ++i) args.term_len.push_back(pat_off[i + 1] - pat_off[i]);  // (a position is a character)
    if ((rc = top_call_args(idx, n, n_terms, query_off, term_kind, q, where_of, line_lo, line_hi, descending, frac_digits, first, top,
                            Rows{rows, row_line, row_value, row_loc, lines, numbers, not_number, overflow}, term_status, &args, &done)) ||
        done)
        return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_class_batch(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms, max_ranges, &merged,
                                     &batch)))
        return rc;
    if ((rc = fmx::hits_stage_call(idx, batch, top_stage, &args, occurrences, status, nullptr, term_status))) return rc;
    fmx::kept_of(args.kept_off.data(), n, kept);
    return FMX_OK;
    });
}

}  // extern "C"
