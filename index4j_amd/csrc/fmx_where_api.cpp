// fmx_where_api.cpp — FIELD VALUES AND HITS ONLY WITHIN THE LINES OF A QUERY (include/fmx.h "THE HITS THAT LIE IN GIVEN LINES", "THE
// VALUES THAT FOLLOW A PATTERN, WHERE THE LINE MATCHES A QUERY"): the device stage fmx_hits_in_lines_dev over fmx_hit_filter.hip's
// launcher, and the host forms fmx_field_values_where_batch / fmx_field_values_where_class_batch.  Of a handle this file sees what
// fmx::line_view hands out; the host forms merge the filter terms and the value patterns into ONE batch and run the packed
// sequence of fmx_api.cpp (fmx::values_between_call) with the stage of this file between the fill and the values stages: the
// lines of the queries (launch_query_lines over the terms' hits, no limit), then the filter over the value patterns' hits.
#include "../../include/fmx.h"
#include "fmx_device.hpp"
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

#define WHERE_HIP_TRY(expr)                                                                  \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            (void)hipGetLastError();                                                         \
            return api_fail(FMX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
        }                                                                                    \
    } while (0)

int no_line_table() { return api_fail(FMX_E_ARG, "the index has no line table (call fmx_line_table_build)"); }

// the HOST arrays of a filter: where_of (n entries, -1 .. q - 1) and the window of lines
int check_where(int32_t n, const int32_t *where_of, int32_t q, int32_t line_lo, int32_t line_hi) {
    if (n < 0 || q < 0 || line_lo < 0 || line_hi < 0 || (n > 0 && !where_of)) return api_fail(FMX_E_ARG, "bad arguments");
    if (line_lo > line_hi) return api_fail(FMX_E_ARG, "the window of lines ends in front of its start");
    for (int32_t i = 0; i < n; ++i)
        if (where_of[i] < -1 || where_of[i] >= q)
            return api_fail(FMX_E_ARG, "where_of[" + std::to_string(i) + "] is outside -1 .. q - 1");
    return FMX_OK;
}
// the call filters at all: a pattern asks for a query, or the window is not 0 .. INT32_MAX
bool filters(int32_t n, const int32_t *where_of, int32_t line_lo, int32_t line_hi) {
    if (line_lo != 0 || line_hi != INT32_MAX) return true;
    for (int32_t i = 0; i < n; ++i)
        if (where_of[i] >= 0) return true;
    return false;
}

// what the stage between the fill and the values stages needs of the call's arguments
struct WhereArgs {
    const int32_t *query_off;
    const uint8_t *term_kind;
    int32_t q;
    const int32_t *where_of;
    int32_t line_lo, line_hi;
    bool filters;
};

// the lines of the q queries from the terms' hits, then the value patterns' hits that lie in them.  A call that does not filter
// needs no line table: every hit is kept.
int where_between(const fmx::HitsBetween &h, void *arg) {
    const WhereArgs &a = *static_cast<const WhereArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const int64_t value_hits = h.total - h.term_hits;
    if (h.n == 0 || value_hits == 0) {
        WHERE_HIP_TRY(hipMemsetAsync(h.kept_off, 0, ((size_t)h.n + 1) * sizeof(int64_t), st));
        return FMX_OK;
    }
    const int32_t *table = a.filters ? h.view->table : nullptr;
    int64_t *d_line_off = nullptr;
    int32_t *d_lines = nullptr;
    int rc;
    if (a.filters && a.q > 0) {
        const int32_t bits = fmx::fm_query_key_width(a.q, h.view->count, fmx::query_lines_max_terms(a.q, a.query_off));
        if (bits > 64) return api_fail(FMX_E_ARG, "the key query | line | term would take " + std::to_string(bits) + " bits (at most 64)");
        if ((rc = h.block(h.call, ((size_t)a.q + 1) * 8, reinterpret_cast<void **>(&d_line_off)))) return rc;
        if (h.n_terms > 0 && h.term_hits > 0) {
            const size_t ws_bytes = fmx::query_lines_scratch_bytes(h.n_terms, a.q, h.term_hits);
            void *ws = nullptr;
            if ((rc = h.block(h.call, (size_t)h.term_hits * 4, reinterpret_cast<void **>(&d_lines))) || (rc = h.block(h.call, ws_bytes, &ws)))
                return rc;
            const int e = fmx::launch_query_lines(table, h.view->count, h.view->n_cu, h.n_terms, a.q, a.query_off, a.term_kind, h.hit_off, h.locs,
                                                  h.term_hits, 0, d_line_off, d_lines, nullptr, ws, ws_bytes, st);
            if (e) return api_fail(FMX_E_HIP, std::string("lines of queries: ") + hipGetErrorString((hipError_t)e));
        } else {  // (terms without hits: no query has a line)
            WHERE_HIP_TRY(hipMemsetAsync(d_line_off, 0, ((size_t)a.q + 1) * sizeof(int64_t), st));
        }
    }
    // the value patterns' part of the packed block: hit_off + n_terms starts at term_hits, not at 0; the slots are all `total`
    const size_t ws_bytes = fmx::hits_in_lines_scratch_bytes(h.n, h.total);
    void *ws = nullptr;
    if ((rc = h.block(h.call, ws_bytes, &ws))) return rc;
    const int e = fmx::launch_hits_in_lines(table, h.view->count, h.view->n_cu, h.n, a.where_of, d_line_off, d_lines, a.line_lo, a.line_hi,
                                            h.hit_off + h.n_terms, h.locs, h.total, h.kept_off, h.kept_locs, ws, ws_bytes, st);
    if (e) return api_fail(FMX_E_HIP, std::string("hits in lines: ") + hipGetErrorString((hipError_t)e));
    return FMX_OK;
}

// offsets that start at or above 0 and never decrease (what the range stages ask of theirs: judged here, ahead of the merge)
int check_offsets(const int32_t *off, int32_t n, const char *what) {
    if (off[0] < 0) return api_fail(FMX_E_ARG, std::string(what) + " offsets start below 0");
    for (int32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return api_fail(FMX_E_ARG, std::string(what) + " offsets decrease");
    return FMX_OK;
}

void null_outputs(int32_t **counts, int64_t **text_off, uint16_t **chars) {
    if (counts) *counts = nullptr;
    if (text_off) *text_off = nullptr;
    if (chars) *chars = nullptr;
}

// the checks the two host forms share, behind their own batches'; *done: an empty call that has been answered
int where_call_args(const fmx_index *idx, int32_t n, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                    const int32_t *where_of, int32_t line_lo, int32_t line_hi, int64_t *val_off, int32_t *term_status, WhereArgs *args,
                    fmx::LineView *view, bool *done) {
    int rc;
    if ((rc = fmx::check_query_arrays(n_terms, q, query_off, term_kind)) || (rc = check_where(n, where_of, q, line_lo, line_hi)) ||
        (rc = fmx::line_view(idx, view)))
        return rc;
    *args = WhereArgs{query_off, term_kind, q, where_of, line_lo, line_hi, filters(n, where_of, line_lo, line_hi)};
    if (args->filters && !view->table) return no_line_table();
    *done = n == 0;
    if (n == 0) {  // (nothing is searched: the terms are not judged)
        val_off[0] = 0;
        for (int32_t t = 0; t < n_terms && term_status; ++t) term_status[t] = 0;
    }
    return FMX_OK;
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
    int rc = check_where(n, where_of, q, line_lo, line_hi);
    if (rc) return rc;
    for (int32_t i = 0; i < n; ++i)
        if (where_of[i] >= 0 && !d_line_off) return api_fail(FMX_E_ARG, "bad arguments");
    fmx::LineView view;
    if ((rc = fmx::line_view(idx, &view))) return rc;
    if (!view.table) return no_line_table();
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0 || n_hits == 0) {
        WHERE_HIP_TRY(hipMemsetAsync(d_kept_off, 0, ((size_t)n + 1) * sizeof(int64_t), st));
        return FMX_OK;
    }
    if (!d_ws || ws_bytes < fmx::hits_in_lines_scratch_bytes(n, n_hits))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_hits_in_lines_scratch_bytes");
    const int e = fmx::launch_hits_in_lines(view.table, view.count, view.n_cu, n, where_of, d_line_off, d_lines, line_lo, line_hi, d_hit_off,
                                            d_locs, n_hits, d_kept_off, d_kept_locs, d_ws, ws_bytes, stream);
    if (e) return api_fail(FMX_E_HIP, std::string("hits in lines: ") + hipGetErrorString((hipError_t)e));
    return FMX_OK;
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
    if (max_len < 1 || max_len > 64) return api_fail(FMX_E_ARG, "max_len is outside [1, 64]");
    if (n_stop < 0 || n_stop > 64 || (n_stop > 0 && !stop)) return api_fail(FMX_E_ARG, "the stop set is outside [0, 64] code units");
    WhereArgs args;
    fmx::LineView view;
    bool done = false;
    int rc;
    if ((n > 0 && (rc = check_offsets(pat_off, n, "pattern"))) || (n_terms > 0 && (rc = check_offsets(term_off, n_terms, "term")))) return rc;
    if ((rc = where_call_args(idx, n, n_terms, query_off, term_kind, q, where_of, line_lo, line_hi, val_off, term_status, &args, &view, &done)) ||
        done)
        return rc;
    const int64_t term_chars = n_terms > 0 ? (int64_t)term_off[n_terms] - term_off[0] : 0, pat_chars = (int64_t)pat_off[n] - pat_off[0];
    if (term_chars + pat_chars > INT32_MAX) return api_fail(FMX_E_ARG, "more than 2^31 - 1 characters in one batch");
    if ((term_chars > 0 && !term_pat) || (pat_chars > 0 && !pat)) return api_fail(FMX_E_ARG, "bad arguments");
    // ONE batch: the terms in front, the value patterns behind them
    std::vector<uint16_t> all_chars((size_t)(term_chars + pat_chars) + 1);
    std::vector<int32_t> all_off((size_t)n_terms + n + 1);
    for (int32_t t = 0; t < n_terms; ++t) all_off[(size_t)t] = term_off[t] - term_off[0];
    for (int32_t i = 0; i <= n; ++i) all_off[(size_t)n_terms + i] = (int32_t)(term_chars + (pat_off[i] - pat_off[0]));
    for (int64_t k = 0; k < term_chars; ++k) all_chars[(size_t)k] = term_pat[term_off[0] + k];
    for (int64_t k = 0; k < pat_chars; ++k) all_chars[(size_t)(term_chars + k)] = pat[pat_off[0] + k];
    const fmx::ValuesBatch batch{all_chars.data(), nullptr, 0, all_off.data(), n_terms, n, 0};
    return fmx::values_between_call(idx, batch, stop, n_stop, max_len, where_between, &args, val_off, counts, text_off, chars, occurrences, status,
                                    kept, term_status);
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
    if (max_len < 1 || max_len > 64) return api_fail(FMX_E_ARG, "max_len is outside [1, 64]");
    if (n_stop < 0 || n_stop > 64 || (n_stop > 0 && !stop)) return api_fail(FMX_E_ARG, "the stop set is outside [0, 64] code units");
    int rc;
    if ((rc = check_offsets(pos_off, n_pos, "position")) || (rc = check_offsets(pat_off, n, "pattern"))) return rc;
    if (pat_off[n] > n_pos) return api_fail(FMX_E_ARG, "pattern offsets end behind the positions");
    if (pos_off[n_pos] > 0 && !alt) return api_fail(FMX_E_ARG, "bad arguments");
    if (n_terms > 0) {
        if ((rc = check_offsets(term_pos_off, term_n_pos, "term position")) || (rc = check_offsets(term_off, n_terms, "term"))) return rc;
        if (term_off[n_terms] > term_n_pos) return api_fail(FMX_E_ARG, "term offsets end behind the positions");
        if (term_pos_off[term_n_pos] > 0 && !term_alt) return api_fail(FMX_E_ARG, "bad arguments");
    }
    WhereArgs args;
    fmx::LineView view;
    bool done = false;
    if ((rc = where_call_args(idx, n, n_terms, query_off, term_kind, q, where_of, line_lo, line_hi, val_off, term_status, &args, &view, &done)) ||
        done)
        return rc;
    // ONE batch: the terms in front, the value patterns behind them, position by position
    std::vector<uint16_t> all_alt;
    std::vector<int32_t> all_pos{0}, all_pat{0};
    auto append = [&](const uint16_t *a, const int32_t *pos, const int32_t *off, int32_t count) {
        for (int32_t i = 0; i < count; ++i) {
            for (int32_t j = off[i]; j < off[i + 1]; ++j) {
                all_alt.insert(all_alt.end(), a + pos[j], a + pos[j + 1]);
                all_pos.push_back((int32_t)all_alt.size());
            }
            all_pat.push_back((int32_t)all_pos.size() - 1);
        }
    };
    if ((int64_t)(n_terms > 0 ? term_pos_off[term_n_pos] : 0) + pos_off[n_pos] > INT32_MAX)
        return api_fail(FMX_E_ARG, "more than 2^31 - 1 alternatives in one batch");
    if (n_terms > 0) append(term_alt, term_pos_off, term_off, n_terms);
    append(alt, pos_off, pat_off, n);
    all_alt.push_back(0);  // (never an empty array)
    const fmx::ValuesBatch batch{all_alt.data(), all_pos.data(), (int32_t)all_pos.size() - 1, all_pat.data(), n_terms, n, max_ranges};
    return fmx::values_between_call(idx, batch, stop, n_stop, max_len, where_between, &args, val_off, counts, text_off, chars, occurrences, status,
                                    kept, term_status);
    });
}

}  // extern "C"
