// fmx_range_api.cpp — QUERY TERMS ON THE NUMBER BEHIND A PATTERN (include/fmx.h "THE LINES THAT MATCH A QUERY WITH TERMS ON NUMBERS",
// "THE HITS WHOSE NUMBER LIES IN A RANGE"; latency_ms >= 500): the device stage fmx_hits_in_number_range_dev and the host forms
// fmx_match_query_number_batch / fmx_match_query_number_class_batch.  Of a handle this file sees what fmx::line_view and
// fmx::text_view hand out.  The host forms run the packed sequence of fmx_api.cpp up to the stage of this file (fmx::hits_stage_call
// over a batch of terms and no value patterns, as fmx_line_histogram_batch does); the stage is fmx::query_lines_stage with the
// terms' ranges in its filter (fmx_host_stage.hpp: the number filter over the terms' hits, ONE 8-byte read and wait for the kept
// total, the lines of the queries over what is kept), then ONE more read and wait for the number of lines, which sizes the result.
// Only the lines and the small per-term arrays come down: the hits and their text do not.
#include "fmx_hit_range.hpp"
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

#include <cstdlib>

namespace {

using fmx::api_fail;
using fmx::guarded;

int check_range_arrays(int32_t n, const int32_t *term_len, int32_t frac_digits) {
    switch (fmx::fm_range_args_bad(n, term_len, frac_digits)) {
        case 0: return FMX_OK;
        case 1: return api_fail(FMX_E_ARG, "frac_digits is outside [0, 9]");
        default: return api_fail(FMX_E_ARG, "a term_len is negative");
    }
}

// what the host forms' stage needs of the call's arguments, and what it leaves for the call's end
struct QueryNumberArgs {
    fmx::HitsFilter filter;
    int32_t max_lines;
    std::vector<int32_t> term_len, kept, not_number, overflow, line_count;
    std::vector<int64_t> line_off;
    void *lines = nullptr;  // malloc'ed to the number of lines; the caller's once the call has synchronised
    ~QueryNumberArgs() { free(lines); }
};

// q > 0 queries over the n_terms > 0 terms of the batch (no value patterns)
int query_number_stage(const fmx::HitsBetween &h, void *arg) {
    QueryNumberArgs &a = *static_cast<QueryNumberArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const size_t q = (size_t)a.filter.q;
    if (h.term_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one batch");
    int64_t *d_line_off = nullptr;
    int32_t *d_lines = nullptr, *d_lcnt = nullptr;
    int rc;
    if ((rc = h.block(h.call, q * 4 + 8, reinterpret_cast<void **>(&d_lcnt))) ||
        (rc = fmx::query_lines_stage(h, a.filter, &d_line_off, &d_lines, d_lcnt, a.max_lines)))
        return rc;
    int64_t n_out = 0;
    FMX_HIP_TRY(hipMemcpyAsync(&n_out, d_line_off + q, 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipStreamSynchronize(st));
    if (n_out > 0) {
        if (!(a.lines = malloc((size_t)n_out * 4))) return api_fail(FMX_E_NOMEM, "out of host memory for " + std::to_string(n_out) + " lines");
        FMX_HIP_TRY(hipMemcpyAsync(a.lines, d_lines, (size_t)n_out * 4, hipMemcpyDeviceToHost, st));
    }
    FMX_HIP_TRY(hipMemcpyAsync(a.line_off.data(), d_line_off, (q + 1) * 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipMemcpyAsync(a.line_count.data(), d_lcnt, q * 4, hipMemcpyDeviceToHost, st));
    return FMX_OK;
}

// the outputs of the host forms
struct QueryNumberOut {
    int64_t *line_off;
    int32_t **lines;
    int32_t *line_count, *occurrences, *kept, *not_number, *overflow, *status;
};

template <class T>
void copy_out(T *to, const std::vector<T> &from, size_t count) {
    for (size_t i = 0; i < count && to; ++i) to[i] = from[i];
}

// behind the checks of the batch itself: the rest of the checks, the call, the hand-over.  `batch` holds the n terms and no value
// pattern; term_len[t] = the length of term t in characters.
int query_number_call(const fmx_index *idx, const fmx::ValuesBatch &batch, const int64_t *num_lo, const int64_t *num_hi, int32_t frac_digits,
                      const int32_t *query_off, const uint8_t *term_kind, int32_t q, int32_t max_lines, const QueryNumberOut &out) {
    const int32_t n = batch.n_terms;
    fmx::LineView view;
    fmx::TextView text;
    int rc;
    if (frac_digits < 0 || frac_digits > fmx::kNumFracMax) return api_fail(FMX_E_ARG, "frac_digits is outside [0, 9]");
    if ((rc = fmx::check_query_arrays(n, q, query_off, term_kind)) || (rc = fmx::line_view(idx, &view)) || (rc = fmx::text_view(idx, &text)))
        return rc;
    if (!view.table) return fmx::no_line_table();
    if ((rc = fmx::check_query_key_width(q, view.count, query_off))) return rc;
    if (n == 0 || q == 0) {  // (queries without terms: no lines; nothing is searched)
        for (int32_t i = 0; i <= q; ++i) out.line_off[i] = 0;
        fmx::zero(out.line_count, (size_t)q);
        return FMX_OK;
    }
    QueryNumberArgs a;
    for (int32_t t = 0; t < n; ++t) a.term_len.push_back(batch.pat_off[t + 1] - batch.pat_off[t]);  // (a class position is a character)
    a.kept.assign((size_t)n, 0);
    a.not_number.assign((size_t)n, 0);
    a.overflow.assign((size_t)n, 0);
    a.line_off.assign((size_t)q + 1, 0);
    a.line_count.assign((size_t)q, 0);
    a.max_lines = max_lines;
    a.filter = fmx::HitsFilter{query_off, term_kind, q, nullptr, 0, INT32_MAX, false, {}};
    const bool ranged = fmx::number_terms_ranged(n, num_lo);
    a.filter.number.num_lo = num_lo;
    a.filter.number.num_hi = num_hi;
    a.filter.number.term_len = a.term_len.data();
    a.filter.number.frac_digits = frac_digits;
    a.filter.number.ranged = ranged;
    a.filter.number.kept = a.kept.data();
    a.filter.number.not_number = a.not_number.data();
    a.filter.number.overflow = a.overflow.data();
    std::vector<int32_t> occurrences((size_t)n, 0), status((size_t)n, 0);
    if ((rc = fmx::hits_stage_call(idx, batch, query_number_stage, &a, nullptr, nullptr, occurrences.data(), status.data()))) return rc;
    // (the call has synchronised: from here on the answer is the caller's)
    if (!ranged) a.kept = occurrences;  // every term is a plain string term: every hit passes
    for (int32_t t = 0; t < n && !text.extract; ++t)  // (a batch without hits ran no stage that would have said so)
        if (num_lo[t] >= 0) status[(size_t)t] = FMX_ST_NOT_ENABLED;
    copy_out(out.line_off, a.line_off, (size_t)q + 1);
    copy_out(out.line_count, a.line_count, (size_t)q);
    copy_out(out.occurrences, occurrences, (size_t)n);
    copy_out(out.status, status, (size_t)n);
    copy_out(out.kept, a.kept, (size_t)n);
    copy_out(out.not_number, a.not_number, (size_t)n);
    copy_out(out.overflow, a.overflow, (size_t)n);
    *out.lines = static_cast<int32_t *>(a.lines);
    a.lines = nullptr;
    return FMX_OK;
}

// num_lo == NULL && num_hi == NULL: the unranged call's answer, array for array; every hit of every term passes
template <class Call>
int unranged_call(int32_t n, const QueryNumberOut &out, Call call) {
    std::vector<int32_t> occurrences((size_t)(n > 0 ? n : 0), 0);
    int32_t *occ = out.occurrences ? out.occurrences : occurrences.data();
    if (const int rc = call(occ)) return rc;
    for (int32_t t = 0; t < n && out.kept; ++t) out.kept[t] = occ[t];
    fmx::zero(out.not_number, (size_t)(n > 0 ? n : 0));
    fmx::zero(out.overflow, (size_t)(n > 0 ? n : 0));
    return FMX_OK;
}

}  // namespace

extern "C" {

size_t fmx_hits_in_number_range_scratch_bytes(int32_t n, int64_t n_hits) { return fmx::hits_in_number_range_scratch_bytes(n, n_hits); }

int fmx_hits_in_number_range_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const int64_t *num_lo, const int64_t *num_hi,
                                 int32_t frac_digits, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, int64_t *d_kept_off,
                                 int32_t *d_kept_locs, int32_t *d_kept, int32_t *d_not_number, int32_t *d_overflow, int32_t *d_status, void *d_ws,
                                 size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || n_hits < 0 || !d_kept_off || (n > 0 && (!term_len || !num_lo || !num_hi || !d_hit_off)) ||
        (n > 0 && n_hits > 0 && (!d_locs || !d_kept_locs)))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    int rc = check_range_arrays(n, term_len, frac_digits);
    if (rc) return rc;
    fmx::LineView view;
    fmx::TextView text;
    if ((rc = fmx::line_view(idx, &view)) || (rc = fmx::text_view(idx, &text))) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0 || n_hits == 0) {  // (the offsets and the counters are zeroed, nothing else is written)
        FMX_HIP_TRY(hipMemsetAsync(d_kept_off, 0, ((size_t)n + 1) * sizeof(int64_t), st));
        for (int32_t *p : {d_kept, d_not_number, d_overflow})
            if (p && n > 0) FMX_HIP_TRY(hipMemsetAsync(p, 0, (size_t)n * 4, st));
        return FMX_OK;
    }
    if (!d_ws || ws_bytes < fmx::hits_in_number_range_scratch_bytes(n, n_hits))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_hits_in_number_range_scratch_bytes");
    const fmx::NumberRangeOut out{d_kept_off, d_kept_locs, d_kept, d_not_number, d_overflow, d_status};
    return fmx::number_range_run(idx, view.n_cu, text, n, term_len, num_lo, num_hi, frac_digits, d_hit_off, d_locs, n_hits, out, d_ws, ws_bytes,
                                 stream);
    });
}

int fmx_match_query_number_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const int64_t *num_lo,
                                 const int64_t *num_hi, int32_t frac_digits, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                 int32_t max_lines, int64_t *line_off, int32_t **lines, int32_t *line_count, int32_t *occurrences, int32_t *kept,
                                 int32_t *not_number, int32_t *overflow, int32_t *status) {
    return guarded([&]() -> int {
    if (lines) *lines = nullptr;
    if ((num_lo == nullptr) != (num_hi == nullptr)) return api_fail(FMX_E_ARG, "one of num_lo and num_hi is NULL and the other is not");
    const QueryNumberOut out{line_off, lines, line_count, occurrences, kept, not_number, overflow, status};
    if (!num_lo)
        return unranged_call(n, out, [&](int32_t *occ) {
            return fmx_match_query_batch(idx, pat, pat_off, n, query_off, term_kind, q, max_lines, line_off, lines, line_count, occ, status);
        });
    if (!idx || n < 0 || q < 0 || !line_off || !lines || !query_off || (n > 0 && (!pat_off || !term_kind)))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (const int rc = fmx::check_literal_batches(pat_off, n, nullptr, 0)) return rc;
    const fmx::ValuesBatch batch{pat, nullptr, 0, pat_off, n, 0, 0};
    return query_number_call(idx, batch, num_lo, num_hi, frac_digits, query_off, term_kind, q, max_lines, out);
    });
}

int fmx_match_query_number_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                       int32_t n, int32_t max_ranges, const int64_t *num_lo, const int64_t *num_hi, int32_t frac_digits,
                                       const int32_t *query_off, const uint8_t *term_kind, int32_t q, int32_t max_lines, int64_t *line_off,
                                       int32_t **lines, int32_t *line_count, int32_t *occurrences, int32_t *kept, int32_t *not_number,
                                       int32_t *overflow, int32_t *status) {
    return guarded([&]() -> int {
    if (lines) *lines = nullptr;
    if ((num_lo == nullptr) != (num_hi == nullptr)) return api_fail(FMX_E_ARG, "one of num_lo and num_hi is NULL and the other is not");
    const QueryNumberOut out{line_off, lines, line_count, occurrences, kept, not_number, overflow, status};
    if (!num_lo)
        return unranged_call(n, out, [&](int32_t *occ) {
            return fmx_match_query_class_batch(idx, alt, pos_off, n_pos, pat_off, n, max_ranges, query_off, term_kind, q, max_lines, line_off, lines,
                                               line_count, occ, status);
        });
    if (!idx || n < 0 || n_pos < 0 || q < 0 || !line_off || !lines || !query_off || !pos_off || !pat_off || (n > 0 && !term_kind) || max_ranges < 1 ||
        max_ranges > FMX_CLASS_RANGES_MAX)
        return api_fail(FMX_E_ARG, "bad arguments");
    if (const int rc = fmx::check_class_batches(alt, pos_off, n_pos, pat_off, n, nullptr, nullptr, 0, nullptr, 0)) return rc;
    const fmx::ValuesBatch batch{alt, pos_off, n_pos, pat_off, n, 0, max_ranges};
    return query_number_call(idx, batch, num_lo, num_hi, frac_digits, query_off, term_kind, q, max_lines, out);
    });
}

}  // extern "C"
