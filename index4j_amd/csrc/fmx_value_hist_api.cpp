// fmx_value_hist_api.cpp — THE TOP VALUES OF A FIELD PER BUCKET OF LINES, the stacked timeline (include/fmx.h "TOP VALUES PER
// BUCKET"; fmx_value_hist.hpp has the definition): the device stages fmx_values_top_histogram_dev and fmx_values_gather_rows_dev
// over fmx_value_hist.hip's launchers, and the host forms fmx_field_values_histogram_where_batch /
// fmx_field_values_histogram_where_class_batch.  Of a handle this file sees what fmx::line_view and fmx::text_view hand out; a host
// form runs the packed sequence of fmx_api.cpp up to the stage of this file (fmx::hits_stage_call) over ONE merged batch terms |
// value patterns, then the filter with the edges' span as its window, fmx_values_of_hits_groups_dev over the kept hits and ONE
// read of the group offsets and the size of the groups' text (fmx::groups_front_stage, the front half it shares with the distinct
// values per bucket), the ranking and binning stage, the fill of the groups' text, the gather of the rows' text and the copies down.
#include "fmx_host_stage.hpp"
#include "fmx_value_hist.hpp"

#include <hip/hip_runtime.h>

#include <cstring>

namespace {

using fmx::api_fail;
using fmx::guarded;
using fmx::hip_fail;
using fmx::no_line_table;
using fmx::zero;

// the shape of the answer and the HOST arrays that cut it: the edges (none at all: one bucket, every line) and top
struct Shape {
    const int32_t *edges;
    int32_t n_edges, B, top;
};
int check_shape(int32_t n, const int32_t *edges, int32_t n_edges, int32_t top, Shape *s) {
    if (top < 1 || top > fmx::kValueHistTopMax) return api_fail(FMX_E_ARG, "top is outside [1, 65536]");
    if (edges || n_edges != 0)
        if (const int rc = fmx::check_edges_array(edges, n_edges)) return rc;
    *s = Shape{edges, n_edges, edges ? n_edges - 1 : 1, top};
    if ((int64_t)n * ((int64_t)top + 1) * s->B > fmx::kHistCellsMax)
        return api_fail(FMX_E_ARG, "more than 2^27 counters in one call (patterns * (top + 1) * buckets)");
    if (fmx::fm_vh_key_width(n, top, s->B) > 64) return api_fail(FMX_E_ARG, "the sort key pattern | rank | bucket is wider than 64 bits");
    return FMX_OK;
}
// the group offsets of a call (fm_vh_shape_bad's rules as messages; the shape has been judged by check_shape)
int check_groups(int32_t n, const int64_t *val_off, const Shape &s, int64_t *row_off) {
    switch (fmx::fm_vh_shape_bad(n, val_off, s.top, s.B, row_off)) {
        case 0: return FMX_OK;
        case 1: return api_fail(FMX_E_ARG, "top is outside [1, 65536]");
        case 2: return api_fail(FMX_E_ARG, "val_off does not start at 0, decreases or holds more than 2^31 - 1 groups");
        case 3: return api_fail(FMX_E_ARG, "more than 2^27 counters in one call (patterns * (top + 1) * buckets)");
        default: return api_fail(FMX_E_ARG, "the sort key pattern | rank | bucket is wider than 64 bits");
    }
}

// ---- the host form --------------------------------------------------------------------------------------------------------------------
// the regions of the ONE allocation of the answer
enum { kRowCount, kRowGroup, kTextOff, kChars, kHist };

struct HistArgs : fmx::GroupsArgs {
    Shape shape{};
    int32_t *other = nullptr;  // the caller's n * B ints, zeroed before the stage runs
    // what the stage leaves beside GroupsArgs' (host; arrived when the call has synchronised)
    std::vector<int64_t> row_off;  // n + 1
    fmx::PackedResult result;
};

// n > 0 value patterns behind n_terms filter terms
int hist_stage(const fmx::HitsBetween &h, void *arg) {
    HistArgs &a = *static_cast<HistArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const Shape &s = a.shape;
    const int32_t n = h.n;
    int rc, e;
    fmx::GroupsFront f{};
    bool done = false;
    if ((rc = fmx::groups_front_stage(h, a, true, "top values per bucket", &f, &done)) || done) return rc;  // (no hit is kept: `other` stays zero)
    auto block = [&](size_t bytes, auto **out) -> int { return h.block(h.call, bytes + 8, reinterpret_cast<void **>(out)); };
    const int64_t K = f.K;
    const int64_t *d_part_off = f.part_off, *d_text_off = f.text_off;
    const int32_t *d_klocs = f.locs, *d_count = f.count, *d_group = f.group;
    void *ws_b = f.ws_b;
    const size_t b_bytes = f.b_bytes;
    if ((rc = check_groups(n, a.val_off.data(), s, a.row_off.data()))) return rc;
    const size_t G = (size_t)a.val_off[(size_t)n], R = (size_t)a.row_off[(size_t)n], B = (size_t)s.B;
    const int64_t units = a.val_off[(size_t)n + 1];
    // the ranks, the rows and the counters
    int64_t *d_row_off = nullptr, *d_row_text_off = nullptr;
    int32_t *d_row_group = nullptr, *d_row_count = nullptr, *d_hist = nullptr, *d_other = nullptr;
    uint16_t *d_chars = nullptr, *d_row_chars = nullptr;
    void *ws_h = nullptr, *ws_g = nullptr;
    const size_t h_bytes = fmx::values_top_histogram_scratch_bytes(n, (int64_t)G, K, s.n_edges), g_bytes = fmx::values_gather_rows_scratch_bytes(n, (int64_t)R);
    if ((rc = block(((size_t)n + 1) * 8, &d_row_off)) || (rc = block(R * 4, &d_row_group)) || (rc = block(R * 4, &d_row_count)) ||
        (rc = block(R * B * 4, &d_hist)) || (rc = block((size_t)n * B * 4, &d_other)) || (rc = block(h_bytes, &ws_h)))
        return rc;
    e = fmx::launch_values_top_histogram(s.edges ? h.view->table : nullptr, h.view->count, h.view->n_cu, n, a.val_off.data(), s.top, s.edges, s.n_edges,
                                         d_part_off, d_klocs, K, d_count, d_group, d_row_off, d_row_group, d_row_count, d_hist, d_other, ws_h,
                                         h_bytes, st);
    if (e) return hip_fail("top values per bucket", e);
    FMX_HIP_TRY(hipMemcpyAsync(a.other, d_other, (size_t)n * B * 4, hipMemcpyDeviceToHost, st));
    if (R == 0) return FMX_OK;
    // the text of ALL groups on the device, the text of the rows alone on the way down
    if ((rc = block((size_t)units * 2, &d_chars)) || (rc = block((size_t)units * 2, &d_row_chars)) || (rc = block((R + 1) * 8, &d_row_text_off)) ||
        (rc = block(g_bytes, &ws_g)))
        return rc;
    if (units > 0 && (rc = fmx_values_fill_dev(h.idx, (int64_t)G, d_text_off, d_chars, ws_b, b_bytes, st))) return rc;
    e = fmx::launch_values_gather_rows(h.view->n_cu, n, a.val_off.data(), s.top, units, d_row_group, d_text_off, d_chars, d_row_text_off, d_row_chars,
                                       ws_g, g_bytes, st);
    if (e) return hip_fail("text of the rows", e);
    int64_t row_units = 0;  // ONE 8-byte read: the packed length of the rows' text sizes the allocation
    FMX_HIP_TRY(hipMemcpyAsync(&row_units, d_row_text_off + R, 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipStreamSynchronize(st));
    if (!a.result.alloc({R * 4, R * 4, (R + 1) * 8, (size_t)row_units * 2 + 2, R * B * 4}))
        return api_fail(FMX_E_NOMEM, "out of host memory for " + std::to_string(R) + " rows");
    FMX_HIP_TRY(hipMemcpyAsync(a.result.region<int32_t>(kRowCount), d_row_count, R * 4, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipMemcpyAsync(a.result.region<int32_t>(kRowGroup), d_row_group, R * 4, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipMemcpyAsync(a.result.region<int64_t>(kTextOff), d_row_text_off, (R + 1) * 8, hipMemcpyDeviceToHost, st));
    if (row_units > 0) FMX_HIP_TRY(hipMemcpyAsync(a.result.region<uint16_t>(kChars), d_row_chars, (size_t)row_units * 2, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipMemcpyAsync(a.result.region<int32_t>(kHist), d_hist, R * B * 4, hipMemcpyDeviceToHost, st));
    return FMX_OK;
}

// what the two host forms take besides their batches, and what they hand back
struct HistCall {
    int32_t n, n_terms;
    const int32_t *query_off;
    const uint8_t *term_kind;
    int32_t q;
    const int32_t *where_of, *edges;
    int32_t n_edges, top;
    const uint16_t *stop;
    int32_t n_stop, max_len;
    int32_t *n_values;
    int64_t *row_off;
    int32_t **row_count, **row_group;
    int64_t **text_off;
    uint16_t **chars;
    int32_t **hist;
    int32_t *other, *occurrences, *kept, *status, *term_status;
};

void null_results(const HistCall &c) {
    for (void **p : {(void **)c.row_count, (void **)c.row_group, (void **)c.text_off, (void **)c.chars, (void **)c.hist})
        if (p) *p = nullptr;
}
bool results_missing(const HistCall &c) {
    return !c.row_off || !c.row_count || !c.row_group || !c.text_off || !c.chars || !c.hist || (c.n > 0 && !c.other);
}

// the checks of the HOST arrays both forms share (behind their own batches'), the handle's views and the empty call; *done: answered
int hist_call_args(const fmx_index *idx, const HistCall &c, HistArgs *a, bool *done) {
    int rc;
    fmx::LineView view;
    if ((rc = fmx::check_values_shape(c.stop, c.n_stop, c.max_len)) || (rc = fmx::check_query_arrays(c.n_terms, c.q, c.query_off, c.term_kind)) ||
        (rc = fmx::check_where_of(c.n, c.where_of, c.q)) || (rc = check_shape(c.n, c.edges, c.n_edges, c.top, &a->shape)) ||
        (rc = fmx::line_view(idx, &view)) || (rc = fmx::text_view(idx, &a->text)))
        return rc;
    // the window of the filter is the span of the edges: every kept hit has a bucket
    const int32_t lo = c.edges ? c.edges[0] : 0, hi = c.edges ? c.edges[c.n_edges - 1] : INT32_MAX;
    a->filter = fmx::HitsFilter{c.query_off, c.term_kind, c.q, c.where_of, lo, hi, fmx::hits_filter_asked(c.n, c.where_of, lo, hi)};
    if ((c.edges || a->filter.filters) && !view.table) return no_line_table();  // (the buckets and the filter are lines)
    zero(c.n_values, (size_t)c.n);
    zero(c.row_off, (size_t)c.n + 1);
    zero(c.other, (size_t)c.n * (size_t)a->shape.B);
    *done = c.n == 0;
    if (c.n == 0) {  // nothing is searched: no rows, the terms are not judged
        zero(c.term_status, (size_t)c.n_terms);
        return FMX_OK;
    }
    a->stop = c.stop;
    a->n_stop = c.n_stop;
    a->max_len = c.max_len;
    a->other = c.other;
    a->sized(c.n);
    a->row_off.assign((size_t)c.n + 1, 0);
    return FMX_OK;
}

// the call over the merged batch terms | value patterns, and the answer into the caller's arrays
int hist_call_run(const fmx_index *idx, const HistCall &c, const fmx::ValuesBatch &batch, HistArgs &a) {
    if (const int rc = fmx::hits_stage_call(idx, batch, hist_stage, &a, c.occurrences, c.status, nullptr, c.term_status)) {
        zero(c.other, (size_t)c.n * (size_t)a.shape.B);  // (a copy of the stage may have arrived)
        return rc;
    }
    fmx::kept_of(a.kept_off.data(), c.n, c.kept);
    for (int32_t i = 0; i < c.n && c.n_values; ++i) c.n_values[i] = (int32_t)(a.val_off[(size_t)i + 1] - a.val_off[(size_t)i]);
    memcpy(c.row_off, a.row_off.data(), ((size_t)c.n + 1) * 8);
    if (a.result.p) {  // the ONE allocation: freed with fmx_free_buffer((uint8_t *)*row_count)
        *c.row_count = a.result.region<int32_t>(kRowCount);
        *c.row_group = a.result.region<int32_t>(kRowGroup);
        *c.text_off = a.result.region<int64_t>(kTextOff);
        *c.chars = a.result.region<uint16_t>(kChars);
        *c.hist = a.result.region<int32_t>(kHist);
        a.result.release();
    }
    return FMX_OK;
}

}  // namespace

extern "C" {

size_t fmx_values_top_histogram_scratch_bytes(int32_t n, int64_t n_groups, int64_t n_hits, int32_t n_edges) {
    return fmx::values_top_histogram_scratch_bytes(n, n_groups, n_hits, n_edges);
}

int fmx_values_top_histogram_dev(const fmx_index *idx, int32_t n, const int64_t *val_off, int32_t top, const int32_t *edges, int32_t n_edges,
                                 const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, const int32_t *d_count,
                                 const int32_t *d_group_of_hit, int64_t *d_row_off, int32_t *d_row_group, int32_t *d_row_count, int32_t *d_hist,
                                 int32_t *d_other, void *d_ws, size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_hits < 0 || n_edges < 0 || (n > 0 && (!val_off || !d_hit_off || !d_row_off || !d_other)) ||
        (n > 0 && n_hits > 0 && (!d_locs || !d_group_of_hit)))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    Shape s;
    int rc;
    if ((rc = check_shape(n, edges, n_edges, top, &s))) return rc;
    std::vector<int64_t> row_off((size_t)n + 1, 0);
    if ((rc = check_groups(n, val_off, s, row_off.data()))) return rc;
    fmx::LineView view;
    if ((rc = fmx::line_view(idx, &view))) return rc;
    if (edges && !view.table) return no_line_table();
    if (n == 0) return FMX_OK;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_hits == 0) {  // (no hit, so no group: no rows, `other` is zero)
        FMX_HIP_TRY(hipMemsetAsync(d_row_off, 0, ((size_t)n + 1) * 8, st));
        FMX_HIP_TRY(hipMemsetAsync(d_other, 0, (size_t)n * (size_t)s.B * 4, st));
        return FMX_OK;
    }
    const int64_t G = val_off[n], R = row_off[(size_t)n];
    if ((G > 0 && !d_count) || (R > 0 && (!d_row_group || !d_row_count || !d_hist))) return api_fail(FMX_E_ARG, "bad arguments");
    if (!d_ws || ws_bytes < fmx::values_top_histogram_scratch_bytes(n, G, n_hits, n_edges))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_values_top_histogram_scratch_bytes");
    const int e = fmx::launch_values_top_histogram(edges ? view.table : nullptr, view.count, view.n_cu, n, val_off, top, edges, n_edges, d_hit_off,
                                                   d_locs, n_hits, d_count, d_group_of_hit, d_row_off, d_row_group, d_row_count, d_hist, d_other,
                                                   d_ws, ws_bytes, st);
    return e ? hip_fail("top values per bucket", e) : FMX_OK;
    });
}

size_t fmx_values_gather_rows_scratch_bytes(int32_t n, int64_t n_rows) { return fmx::values_gather_rows_scratch_bytes(n, n_rows); }

int fmx_values_gather_rows_dev(const fmx_index *idx, int32_t n, const int64_t *val_off, int32_t top, int64_t max_units, const int32_t *d_row_group,
                               const int64_t *d_text_off, const uint16_t *d_chars, int64_t *d_row_text_off, uint16_t *d_row_chars, void *d_ws,
                               size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || max_units < 0 || !d_row_text_off || (n > 0 && !val_off)) return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    std::vector<int64_t> row_off((size_t)n + 1, 0);
    if ((rc = check_groups(n, val_off, Shape{nullptr, 0, 1, top}, row_off.data()))) return rc;
    const int64_t R = row_off[(size_t)n];
    if (R > fmx::kHistCellsMax) return api_fail(FMX_E_ARG, "more than 2^27 rows in one call");
    fmx::LineView view;
    if ((rc = fmx::line_view(idx, &view))) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (R == 0) {
        FMX_HIP_TRY(hipMemsetAsync(d_row_text_off, 0, 8, st));
        return FMX_OK;
    }
    if (!d_row_group || !d_text_off || (max_units > 0 && (!d_chars || !d_row_chars))) return api_fail(FMX_E_ARG, "bad arguments");
    if (!d_ws || ws_bytes < fmx::values_gather_rows_scratch_bytes(n, R))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_values_gather_rows_scratch_bytes");
    const int e = fmx::launch_values_gather_rows(view.n_cu, n, val_off, top, max_units, d_row_group, d_text_off, d_chars, d_row_text_off, d_row_chars,
                                                 d_ws, ws_bytes, st);
    return e ? hip_fail("text of the rows", e) : FMX_OK;
    });
}

int fmx_field_values_histogram_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                                           const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                           const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t top, const uint16_t *stop,
                                           int32_t n_stop, int32_t max_len, int32_t *n_values, int64_t *row_off, int32_t **row_count,
                                           int32_t **row_group, int64_t **text_off, uint16_t **chars, int32_t **hist, int32_t *other,
                                           int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *term_status) {
    return guarded([&]() -> int {
    const HistCall c{n, n_terms, query_off, term_kind, q, where_of, edges, n_edges, top, stop, n_stop, max_len, n_values, row_off, row_count,
                     row_group, text_off, chars, hist, other, occurrences, kept, status, term_status};
    null_results(c);
    if (!idx || n < 0 || n_terms < 0 || q < 0 || n_edges < 0 || results_missing(c) || (n > 0 && (!pat_off || !where_of)) || (n_terms > 0 && !term_off))
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_literal_batches(pat_off, n, term_off, n_terms))) return rc;
    HistArgs a;
    bool done = false;
    if ((rc = hist_call_args(idx, c, &a, &done)) || done) return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_literal_batch(pat, pat_off, n, term_pat, term_off, n_terms, &merged, &batch))) return rc;
    for (int32_t i = 0; i < n; ++i) a.term_len.push_back(pat_off[i + 1] - pat_off[i]);
    return hist_call_run(idx, c, batch, a);
    });
}

int fmx_field_values_histogram_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                                 const int32_t *pat_off, int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off,
                                                 int32_t term_n_pos, const int32_t *term_off, int32_t n_terms, int32_t max_ranges,
                                                 const int32_t *query_off, const uint8_t *term_kind, int32_t q, const int32_t *where_of,
                                                 const int32_t *edges, int32_t n_edges, int32_t top, const uint16_t *stop, int32_t n_stop,
                                                 int32_t max_len, int32_t *n_values, int64_t *row_off, int32_t **row_count, int32_t **row_group,
                                                 int64_t **text_off, uint16_t **chars, int32_t **hist, int32_t *other, int32_t *occurrences,
                                                 int32_t *kept, int32_t *status, int32_t *term_status) {
    return guarded([&]() -> int {
    const HistCall c{n, n_terms, query_off, term_kind, q, where_of, edges, n_edges, top, stop, n_stop, max_len, n_values, row_off, row_count,
                     row_group, text_off, chars, hist, other, occurrences, kept, status, term_status};
    null_results(c);
    if (!idx || n < 0 || n_pos < 0 || n_terms < 0 || term_n_pos < 0 || q < 0 || n_edges < 0 || results_missing(c) || !pos_off || !pat_off ||
        (n > 0 && !where_of) || (n_terms > 0 && (!term_pos_off || !term_off)) || max_ranges < 1 || max_ranges > FMX_CLASS_RANGES_MAX)
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_class_batches(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms))) return rc;
    HistArgs a;
    bool done = false;
    if ((rc = hist_call_args(idx, c, &a, &done)) || done) return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_class_batch(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms, max_ranges, &merged,
                                     &batch)))
        return rc;
    for (int32_t i = 0; i < n; ++i) a.term_len.push_back(pat_off[i + 1] - pat_off[i]);  // (a position is a character)
    return hist_call_run(idx, c, batch, a);
    });
}

}  // extern "C"
