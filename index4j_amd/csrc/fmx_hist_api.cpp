// fmx_hist_api.cpp — MATCHING LINES AND HITS PER BUCKET OF LINES, the timeline (include/fmx.h "LINES AND HITS PER BUCKET OF LINES"): the
// device stages fmx_lines_histogram_dev / fmx_hits_histogram_dev over fmx_line_hist.hip's launchers, and the host forms
// fmx_line_histogram_batch / fmx_hit_histogram_where_batch with their class twins.  Of a handle this file sees what fmx::line_view
// hands out; the host forms run the packed sequence of fmx_api.cpp up to a stage of this file (fmx::hits_stage_call):
//   lines form   the lines of the queries (launch_query_lines over the terms' hits, no limit), launch_lines_histogram over them;
//   hits form    fmx_field_values_where_batch's call without the values stage: the lines of the queries, the filter over the value
//                patterns' hits (skipped when no pattern asks for a query), launch_hits_histogram over what is kept.
// Only the counters and the small per-query, per-pattern and per-term arrays come down.
#include "../../include/fmx.h"
#include "fmx_line_hist.hpp"
#include "fmx_plan.hpp"

#include <hip/hip_runtime.h>

#include <climits>
#include <exception>
#include <new>
#include <string>
#include <vector>

namespace fmx {
int api_fail(int code, const std::string &msg);  // fmx_api.cpp: the calling thread's fmx_last_error
}  // namespace fmx

namespace {

using fmx::api_fail;

template <class F>
int guarded(F &&body) {  // (the ABI never throws)
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return api_fail(FMX_E_UNSUPPORTED, "out of host memory");
    } catch (const std::exception &e) {
        return api_fail(FMX_E_UNSUPPORTED, std::string("internal error: ") + e.what());
    }
}

#define HIST_HIP_TRY(expr)                                                                   \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            (void)hipGetLastError();                                                         \
            return api_fail(FMX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
        }                                                                                    \
    } while (0)

int no_line_table() { return api_fail(FMX_E_ARG, "the index has no line table (call fmx_line_table_build)"); }

// the HOST array of edges and the size of the answer: rows * B counters
int check_edges(const int32_t *edges, int32_t n_edges, int32_t rows) {
    switch (fmx::fm_hist_edges_bad(edges, n_edges)) {
        case 0: break;
        case 1: return api_fail(FMX_E_ARG, "fewer than 2 edges");
        case 2: return api_fail(FMX_E_ARG, "the first edge is negative");
        default: return api_fail(FMX_E_ARG, "the edges decrease");
    }
    if ((int64_t)rows * (n_edges - 1) > fmx::kHistCellsMax)
        return api_fail(FMX_E_ARG, "more than 2^27 counters in one call (rows * buckets)");
    return FMX_OK;
}

int check_where_of(int32_t n, const int32_t *where_of, int32_t q) {
    for (int32_t i = 0; i < n; ++i)
        if (where_of[i] < -1 || where_of[i] >= q) return api_fail(FMX_E_ARG, "where_of[" + std::to_string(i) + "] is outside -1 .. q - 1");
    return FMX_OK;
}

// offsets that start at or above 0 and never decrease (what the range stages ask of theirs: judged here, ahead of the merge)
int check_offsets(const int32_t *off, int32_t n, const char *what) {
    if (off[0] < 0) return api_fail(FMX_E_ARG, std::string(what) + " offsets start below 0");
    for (int32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return api_fail(FMX_E_ARG, std::string(what) + " offsets decrease");
    return FMX_OK;
}

// what the stages need of the call's arguments: the queries and the filter (fmx_plan.hpp), then the edges and the outputs
struct HistArgs : fmx::HitsFilter {
    const int32_t *edges;
    int32_t n_edges;
    int32_t *hist, *line_count;
    std::vector<int64_t> kept_off;  // hits form: n + 1, filled when the call has synchronised
};

// the lines of the q queries from the terms' hits, no limit: line_off (q + 1) and lines on the device
int query_lines_stage(const fmx::HitsBetween &h, const fmx::HitsFilter &a, int64_t **d_line_off, int32_t **d_lines, int32_t *d_line_count) {
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const int32_t bits = fmx::fm_query_key_width(a.q, h.view->count, fmx::query_lines_max_terms(a.q, a.query_off));
    if (bits > 64) return api_fail(FMX_E_ARG, "the key query | line | term would take " + std::to_string(bits) + " bits (at most 64)");
    int rc;
    if ((rc = h.block(h.call, ((size_t)a.q + 1) * 8, reinterpret_cast<void **>(d_line_off)))) return rc;
    if (h.n_terms > 0 && h.term_hits > 0) {
        const size_t ws_bytes = fmx::query_lines_scratch_bytes(h.n_terms, a.q, h.term_hits);
        void *ws = nullptr;
        if ((rc = h.block(h.call, (size_t)h.term_hits * 4, reinterpret_cast<void **>(d_lines))) || (rc = h.block(h.call, ws_bytes, &ws))) return rc;
        const int e = fmx::launch_query_lines(h.view->table, h.view->count, h.view->n_cu, h.n_terms, a.q, a.query_off, a.term_kind, h.hit_off,
                                              h.locs, h.term_hits, 0, *d_line_off, *d_lines, d_line_count, ws, ws_bytes, st);
        if (e) return api_fail(FMX_E_HIP, std::string("lines of queries: ") + hipGetErrorString((hipError_t)e));
    } else {  // (terms without hits: no query has a line)
        HIST_HIP_TRY(hipMemsetAsync(*d_line_off, 0, ((size_t)a.q + 1) * sizeof(int64_t), st));
        if (d_line_count) HIST_HIP_TRY(hipMemsetAsync(d_line_count, 0, (size_t)a.q * 4, st));
    }
    return FMX_OK;
}

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
        (rc = query_lines_stage(h, a, &d_line_off, &d_lines, d_lcnt)))
        return rc;
    const int e = fmx::launch_lines_histogram(h.view->n_cu, a.q, d_line_off, d_lines, a.edges, a.n_edges, d_hist, ws, ws_bytes, st);
    if (e) return api_fail(FMX_E_HIP, std::string("lines per bucket: ") + hipGetErrorString((hipError_t)e));
    if (cells > 0) HIST_HIP_TRY(hipMemcpyAsync(a.hist, d_hist, cells * 4, hipMemcpyDeviceToHost, st));
    if (a.line_count) HIST_HIP_TRY(hipMemcpyAsync(a.line_count, d_lcnt, (size_t)a.q * 4, hipMemcpyDeviceToHost, st));
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
        if (cells > 0) HIST_HIP_TRY(hipMemsetAsync(d_hist, 0, cells * 4, st));
        a.kept_off.assign((size_t)h.n + 1, 0);
    } else {
        if ((rc = fmx::kept_hits_stage(h, a, &d_off, &d_locs, &n_hits))) return rc;
        const size_t ws_bytes = fmx::hits_histogram_scratch_bytes(h.n, n_hits, a.n_edges);
        void *ws = nullptr;
        if ((rc = h.block(h.call, ws_bytes, &ws))) return rc;
        const int e = fmx::launch_hits_histogram(h.view->table, h.view->count, h.view->n_cu, h.n, d_off, d_locs, n_hits, a.edges, a.n_edges, d_hist,
                                                 ws, ws_bytes, st);
        if (e) return api_fail(FMX_E_HIP, std::string("hits per bucket: ") + hipGetErrorString((hipError_t)e));
        HIST_HIP_TRY(hipMemcpyAsync(a.kept_off.data(), d_off, ((size_t)h.n + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    if (cells > 0) HIST_HIP_TRY(hipMemcpyAsync(a.hist, d_hist, cells * 4, hipMemcpyDeviceToHost, st));
    return FMX_OK;
}

void zero(int32_t *a, size_t count) {
    for (size_t i = 0; i < count && a; ++i) a[i] = 0;
}

// the checks the two lines forms share, behind their own batches'; *done: an empty call that has been answered
int lines_call_args(const fmx_index *idx, int32_t n, const int32_t *query_off, const uint8_t *term_kind, int32_t q, const int32_t *edges,
                    int32_t n_edges, int32_t *hist, int32_t *line_count, HistArgs *args, bool *done) {
    fmx::LineView view;
    int rc;
    if ((rc = fmx::check_query_arrays(n, q, query_off, term_kind)) || (rc = check_edges(edges, n_edges, q)) || (rc = fmx::line_view(idx, &view)))
        return rc;
    if (!view.table) return no_line_table();
    const int32_t bits = fmx::fm_query_key_width(q, view.count, fmx::query_lines_max_terms(q, query_off));
    if (bits > 64) return api_fail(FMX_E_ARG, "the key query | line | term would take " + std::to_string(bits) + " bits (at most 64)");
    *args = HistArgs{{query_off, term_kind, q, nullptr, false}, edges, n_edges, hist, line_count, {}};
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
    if ((rc = fmx::check_query_arrays(n_terms, q, query_off, term_kind)) || (rc = check_where_of(n, where_of, q)) ||
        (rc = check_edges(edges, n_edges, n)) || (rc = fmx::line_view(idx, &view)))
        return rc;
    if (!view.table) return no_line_table();  // (the buckets are lines: with or without a filter)
    *args = HistArgs{{query_off, term_kind, q, where_of, fmx::hits_filter_asked(n, where_of)}, edges, n_edges, hist, nullptr,
                     std::vector<int64_t>((size_t)n + 1)};
    *done = n == 0;
    if (n == 0) zero(term_status, (size_t)n_terms);  // (nothing is searched: the terms are not judged)
    return FMX_OK;
}

void kept_of(const HistArgs &args, int32_t n, int32_t *kept) {
    for (int32_t i = 0; i < n && kept; ++i) kept[i] = (int32_t)(args.kept_off[(size_t)i + 1] - args.kept_off[(size_t)i]);
}

}  // namespace

// what the hits forms of this file share with fmx_stats_api.cpp (fmx_plan.hpp)
namespace fmx {

bool hits_filter_asked(int32_t n, const int32_t *where_of) {
    for (int32_t i = 0; i < n; ++i)
        if (where_of[i] >= 0) return true;
    return false;
}

int check_hits_filter(int32_t n, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q, const int32_t *where_of) {
    if (const int rc = check_query_arrays(n_terms, q, query_off, term_kind)) return rc;
    return check_where_of(n, where_of, q);
}

int kept_hits_stage(const HitsBetween &h, const HitsFilter &a, const int64_t **d_off, const int32_t **d_locs, int64_t *n_hits) {
    // the value patterns' part of the packed block: hit_off + n_terms starts at term_hits, not at 0; the slots are all `total`
    *d_off = h.hit_off + h.n_terms;
    *d_locs = h.locs;
    *n_hits = h.total;
    if (!a.filters) return FMX_OK;
    const int64_t value_hits = h.total - h.term_hits;
    int64_t *d_line_off = nullptr, *d_koff = nullptr;
    int32_t *d_lines = nullptr, *d_kept = nullptr;
    const size_t ws_bytes = hits_in_lines_scratch_bytes(h.n, h.total);
    void *ws = nullptr;
    int rc;
    if ((a.q > 0 && (rc = query_lines_stage(h, a, &d_line_off, &d_lines, nullptr))) ||
        (rc = h.block(h.call, ((size_t)h.n + 1) * 8, reinterpret_cast<void **>(&d_koff))) ||
        (rc = h.block(h.call, (size_t)value_hits * 4 + 8, reinterpret_cast<void **>(&d_kept))) || (rc = h.block(h.call, ws_bytes, &ws)))
        return rc;
    const int e = launch_hits_in_lines(h.view->table, h.view->count, h.view->n_cu, h.n, a.where_of, d_line_off, d_lines, 0, INT32_MAX, *d_off,
                                       *d_locs, h.total, d_koff, d_kept, ws, ws_bytes, static_cast<hipStream_t>(h.stream));
    if (e) return api_fail(FMX_E_HIP, std::string("hits in lines: ") + hipGetErrorString((hipError_t)e));
    *d_off = d_koff;
    *d_locs = d_kept;
    *n_hits = value_hits;  // (kept_off[n] <= value_hits: the slots behind are ignored)
    return FMX_OK;
}

int check_literal_batches(const int32_t *pat_off, int32_t n, const int32_t *term_off, int32_t n_terms) {
    int rc;
    if ((n > 0 && (rc = check_offsets(pat_off, n, "pattern"))) || (n_terms > 0 && (rc = check_offsets(term_off, n_terms, "term")))) return rc;
    return FMX_OK;
}

int check_class_batches(const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n, const uint16_t *term_alt,
                        const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off, int32_t n_terms) {
    int rc;
    if ((rc = check_offsets(pos_off, n_pos, "position")) || (rc = check_offsets(pat_off, n, "pattern"))) return rc;
    if (pat_off[n] > n_pos) return api_fail(FMX_E_ARG, "pattern offsets end behind the positions");
    if (pos_off[n_pos] > 0 && !alt) return api_fail(FMX_E_ARG, "bad arguments");
    if (n_terms > 0) {
        if ((rc = check_offsets(term_pos_off, term_n_pos, "term position")) || (rc = check_offsets(term_off, n_terms, "term"))) return rc;
        if (term_off[n_terms] > term_n_pos) return api_fail(FMX_E_ARG, "term offsets end behind the positions");
        if (term_pos_off[term_n_pos] > 0 && !term_alt) return api_fail(FMX_E_ARG, "bad arguments");
    }
    return FMX_OK;
}

// ONE batch: the terms in front, the value patterns behind them
int merge_literal_batch(const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat, const int32_t *term_off,
                        int32_t n_terms, MergedBatch *m, ValuesBatch *batch) {
    const int64_t term_chars = n_terms > 0 ? (int64_t)term_off[n_terms] - term_off[0] : 0, pat_chars = (int64_t)pat_off[n] - pat_off[0];
    if (term_chars + pat_chars > INT32_MAX) return api_fail(FMX_E_ARG, "more than 2^31 - 1 characters in one batch");
    if ((term_chars > 0 && !term_pat) || (pat_chars > 0 && !pat)) return api_fail(FMX_E_ARG, "bad arguments");
    m->chars.assign((size_t)(term_chars + pat_chars) + 1, 0);
    m->off.assign((size_t)n_terms + n + 1, 0);
    for (int32_t t = 0; t < n_terms; ++t) m->off[(size_t)t] = term_off[t] - term_off[0];
    for (int32_t i = 0; i <= n; ++i) m->off[(size_t)n_terms + i] = (int32_t)(term_chars + (pat_off[i] - pat_off[0]));
    for (int64_t k = 0; k < term_chars; ++k) m->chars[(size_t)k] = term_pat[term_off[0] + k];
    for (int64_t k = 0; k < pat_chars; ++k) m->chars[(size_t)(term_chars + k)] = pat[pat_off[0] + k];
    *batch = ValuesBatch{m->chars.data(), nullptr, 0, m->off.data(), n_terms, n, 0};
    return FMX_OK;
}

// ... position by position
int merge_class_batch(const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n, const uint16_t *term_alt,
                      const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off, int32_t n_terms, int32_t max_ranges,
                      MergedBatch *m, ValuesBatch *batch) {
    m->chars.clear();
    m->pos.assign(1, 0);
    m->off.assign(1, 0);
    auto append = [&](const uint16_t *a, const int32_t *pos, const int32_t *off, int32_t count) {
        for (int32_t i = 0; i < count; ++i) {
            for (int32_t j = off[i]; j < off[i + 1]; ++j) {
                m->chars.insert(m->chars.end(), a + pos[j], a + pos[j + 1]);
                m->pos.push_back((int32_t)m->chars.size());
            }
            m->off.push_back((int32_t)m->pos.size() - 1);
        }
    };
    if ((int64_t)(n_terms > 0 ? term_pos_off[term_n_pos] : 0) + pos_off[n_pos] > INT32_MAX)
        return api_fail(FMX_E_ARG, "more than 2^31 - 1 alternatives in one batch");
    if (n_terms > 0) append(term_alt, term_pos_off, term_off, n_terms);
    append(alt, pos_off, pat_off, n);
    m->chars.push_back(0);  // (never an empty array)
    *batch = ValuesBatch{m->chars.data(), m->pos.data(), (int32_t)m->pos.size() - 1, m->off.data(), n_terms, n, max_ranges};
    return FMX_OK;
}

}  // namespace fmx

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
        HIST_HIP_TRY(hipMemsetAsync(d_hist, 0, cells * 4, static_cast<hipStream_t>(stream)));
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
    if ((n > 0 && (rc = check_offsets(pat_off, n, "pattern"))) ||
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
    if ((rc = check_offsets(pos_off, n_pos, "position")) || (rc = check_offsets(pat_off, n, "pattern"))) return rc;
    if (pat_off[n] > n_pos) return api_fail(FMX_E_ARG, "pattern offsets end behind the positions");
    if (pos_off[n_pos] > 0 && !alt) return api_fail(FMX_E_ARG, "bad arguments");
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
    kept_of(args, n, kept);
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
    kept_of(args, n, kept);
    return FMX_OK;
    });
}

}  // extern "C"
