// fmx_host_stage.cpp — what the where, histogram and stats forms run on the device inside their stage of the packed host sequence
// (fmx_host_stage.hpp): the lines of the queries from the terms' hits (fmx_query_lines.hip's launcher), then the value patterns' hits
// that lie in them and in the window of lines (fmx_hit_filter.hip's launcher); in front of the lines of the queries, where a term
// is ranged, the terms' hits whose number lies in the term's range (fmx_hit_range.hip's launchers around the packed extract).
#include "fmx_device.hpp"
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

namespace fmx {

int check_query_key_width(int32_t q, int32_t count, const int32_t *query_off) {
    const int32_t bits = fm_query_key_width(q, count, query_lines_max_terms(q, query_off));
    if (bits > 64) return api_fail(FMX_E_ARG, "the key query | line | term would take " + std::to_string(bits) + " bits (at most 64)");
    return FMX_OK;
}

int number_range_run(const ::fmx_index *idx, int n_cu, const TextView &text, int32_t n, const int32_t *term_len, const int64_t *num_lo,
                     const int64_t *num_hi, int32_t frac_digits, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits,
                     const NumberRangeOut &out, void *ws, size_t ws_bytes, void *stream) {
    ValuesWindows w;
    if (!range_windows(ws, ws_bytes, n, n_hits, &w))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_hits_in_number_range_scratch_bytes");
    int e = launch_range_windows(text.text_len, n_cu, n, term_len, num_lo, num_hi, d_hit_off, d_locs, n_hits, ws, ws_bytes, stream);
    if (e) return api_fail(FMX_E_HIP, std::string("windows of ranged hits: ") + hipGetErrorString((hipError_t)e));
    if (text.extract)
        if (const int rc = extract_windows(idx, w, (int32_t)n_hits, stream)) return rc;
    e = launch_range_keep(n_cu, n, text.extract, FMX_ST_NOT_ENABLED, frac_digits, d_hit_off, d_locs, n_hits, out.kept_off, out.kept_locs, out.kept,
                          out.not_number, out.overflow, out.status, ws, ws_bytes, stream);
    if (e) return api_fail(FMX_E_HIP, std::string("hits in number range: ") + hipGetErrorString((hipError_t)e));
    return FMX_OK;
}

// the terms' hits that pass the number filter, as (*d_off: n_terms + 1, *d_locs, *n_hits = the kept total, read with ONE 8-byte copy
// and wait); the counters go to the host arrays of f.number on the way.  h.n_terms > 0 and a term has a hit.
static int number_terms_stage(const HitsBetween &h, const NumberTerms &f, const int64_t **d_off, const int32_t **d_locs, int64_t *n_hits) {
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const size_t nt = (size_t)h.n_terms;
    TextView text;
    int64_t *d_koff = nullptr;
    int32_t *d_kept_locs = nullptr, *d_counters = nullptr;
    void *ws = nullptr;
    const size_t ws_bytes = hits_in_number_range_scratch_bytes(h.n_terms, h.term_hits);
    int rc;
    if ((rc = text_view(h.idx, &text)) || (rc = h.block(h.call, (nt + 1) * 8, reinterpret_cast<void **>(&d_koff))) ||
        (rc = h.block(h.call, (size_t)h.term_hits * 4 + 8, reinterpret_cast<void **>(&d_kept_locs))) ||
        (rc = h.block(h.call, 3 * nt * 4, reinterpret_cast<void **>(&d_counters))) || (rc = h.block(h.call, ws_bytes, &ws)))
        return rc;
    const NumberRangeOut out{d_koff, d_kept_locs, d_counters, d_counters + nt, d_counters + 2 * nt, h.term_status};
    if ((rc = number_range_run(h.idx, h.view->n_cu, text, h.n_terms, f.term_len, f.num_lo, f.num_hi, f.frac_digits, h.hit_off, h.locs, h.term_hits,
                               out, ws, ws_bytes, h.stream)))
        return rc;
    if (f.kept) FMX_HIP_TRY(hipMemcpyAsync(f.kept, out.kept, nt * 4, hipMemcpyDeviceToHost, st));
    if (f.not_number) FMX_HIP_TRY(hipMemcpyAsync(f.not_number, out.not_number, nt * 4, hipMemcpyDeviceToHost, st));
    if (f.overflow) FMX_HIP_TRY(hipMemcpyAsync(f.overflow, out.overflow, nt * 4, hipMemcpyDeviceToHost, st));
    int64_t kept_total = 0;
    FMX_HIP_TRY(hipMemcpyAsync(&kept_total, d_koff + nt, 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipStreamSynchronize(st));
    *d_off = d_koff;
    *d_locs = d_kept_locs;
    *n_hits = kept_total;
    return FMX_OK;
}

int query_lines_stage(const HitsBetween &h, const HitsFilter &f, int64_t **d_line_off, int32_t **d_lines, int32_t *d_line_count,
                      int32_t max_lines) {
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    int rc;
    if ((rc = check_query_key_width(f.q, h.view->count, f.query_off)) ||
        (rc = h.block(h.call, ((size_t)f.q + 1) * 8, reinterpret_cast<void **>(d_line_off))))
        return rc;
    const int64_t *t_off = h.hit_off;
    const int32_t *t_locs = h.locs;
    int64_t t_hits = h.term_hits;
    if (f.number.ranged && h.n_terms > 0 && h.term_hits > 0 && (rc = number_terms_stage(h, f.number, &t_off, &t_locs, &t_hits))) return rc;
    if (h.n_terms > 0 && t_hits > 0) {
        const size_t ws_bytes = query_lines_scratch_bytes(h.n_terms, f.q, t_hits);
        void *ws = nullptr;
        if ((rc = h.block(h.call, (size_t)t_hits * 4, reinterpret_cast<void **>(d_lines))) || (rc = h.block(h.call, ws_bytes, &ws))) return rc;
        const int e = launch_query_lines(h.view->table, h.view->count, h.view->n_cu, h.n_terms, f.q, f.query_off, f.term_kind, t_off, t_locs, t_hits,
                                         max_lines, *d_line_off, *d_lines, d_line_count, ws, ws_bytes, st);
        if (e) return api_fail(FMX_E_HIP, std::string("lines of queries: ") + hipGetErrorString((hipError_t)e));
    } else {  // (terms without hits: no query has a line)
        FMX_HIP_TRY(hipMemsetAsync(*d_line_off, 0, ((size_t)f.q + 1) * sizeof(int64_t), st));
        if (d_line_count) FMX_HIP_TRY(hipMemsetAsync(d_line_count, 0, (size_t)f.q * 4, st));
    }
    return FMX_OK;
}

int hits_in_lines_stage(const HitsBetween &h, const HitsFilter &f, int64_t *kept_off, int32_t *kept_locs) {
    int64_t *d_line_off = nullptr;
    int32_t *d_lines = nullptr;
    int rc;
    if (f.filters && f.q > 0 && (rc = query_lines_stage(h, f, &d_line_off, &d_lines, nullptr))) return rc;
    // the value patterns' part of the packed block: hit_off + n_terms starts at term_hits, not at 0; the slots are all `total`
    const size_t ws_bytes = hits_in_lines_scratch_bytes(h.n, h.total);
    void *ws = nullptr;
    if ((rc = h.block(h.call, ws_bytes, &ws))) return rc;
    const int e = launch_hits_in_lines(f.filters ? h.view->table : nullptr, h.view->count, h.view->n_cu, h.n, f.where_of, d_line_off, d_lines,
                                       f.line_lo, f.line_hi, h.hit_off + h.n_terms, h.locs, h.total, kept_off, kept_locs, ws, ws_bytes, h.stream);
    if (e) return api_fail(FMX_E_HIP, std::string("hits in lines: ") + hipGetErrorString((hipError_t)e));
    return FMX_OK;
}

int kept_hits_stage(const HitsBetween &h, const HitsFilter &f, const int64_t **d_off, const int32_t **d_locs, int64_t *n_hits) {
    *d_off = h.hit_off + h.n_terms;
    *d_locs = h.locs;
    *n_hits = h.total;
    if (!f.filters) return FMX_OK;
    const int64_t value_hits = h.total - h.term_hits;
    int64_t *d_koff = nullptr;
    int32_t *d_kept = nullptr;
    int rc;
    if ((rc = h.block(h.call, ((size_t)h.n + 1) * 8, reinterpret_cast<void **>(&d_koff))) ||
        (rc = h.block(h.call, (size_t)value_hits * 4 + 8, reinterpret_cast<void **>(&d_kept))) || (rc = hits_in_lines_stage(h, f, d_koff, d_kept)))
        return rc;
    *d_off = d_koff;
    *d_locs = d_kept;
    *n_hits = value_hits;  // (kept_off[n] <= value_hits: the slots behind are ignored)
    return FMX_OK;
}

}  // namespace fmx
