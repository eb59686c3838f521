// fmx_host_stage.cpp — what the where, histogram and stats forms run on the device inside their stage of the packed host sequence
// (fmx_host_stage.hpp): the lines of the queries from the terms' hits (fmx_query_lines.hip's launcher), then the value patterns' hits
// that lie in them and in the window of lines (fmx_hit_filter.hip's launcher); in front of the lines of the queries, where a term
// is ranged, the terms' hits whose number lies in the term's range (fmx_hit_range.hip's launchers around the packed extract).
// Behind them what the numbers, top and keyed forms share: the report of a HIP error, the groups of hits (stage b), the statistics
// arrays and the packed result of a stage, and the keyed forms' plumbing and front half (fmx_by_api.cpp, fmx_by_hist_api.cpp).
#include "fmx_device.hpp"
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

#include <cstring>

namespace fmx {

int hip_fail(const char *what, int e) { return api_fail(FMX_E_HIP, std::string(what) + ": " + hipGetErrorString((hipError_t)e)); }

int status_all(const HitsBetween &h, int32_t value, const char *what) {
    const int e = launch_values_status_all(h.view->n_cu, h.status, h.n, value, h.stream);
    return e ? hip_fail(what, e) : FMX_OK;
}

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
    if (e) return hip_fail("windows of ranged hits", e);
    if (text.extract)
        if (const int rc = extract_windows(idx, w, (int32_t)n_hits, stream)) return rc;
    e = launch_range_keep(n_cu, n, text.extract, FMX_ST_NOT_ENABLED, frac_digits, d_hit_off, d_locs, n_hits, out.kept_off, out.kept_locs, out.kept,
                          out.not_number, out.overflow, out.status, ws, ws_bytes, stream);
    if (e) return hip_fail("hits in number range", e);
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
        if (e) return hip_fail("lines of queries", e);
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
    if (e) return hip_fail("hits in lines", e);
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

int values_groups_run(const ::fmx_index *idx, const LineView &view, const TextView &text, int32_t n, const int32_t *term_len, const uint16_t *stop,
                      int32_t n_stop, int32_t max_len, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, int64_t *d_val_off,
                      int32_t *d_count, int64_t *d_text_off, int32_t *d_group_of_hit, int32_t *d_status, void *ws, size_t ws_bytes, void *stream) {
    ValuesWindows w;
    if (ws_bytes < values_groups_of_hits_scratch_bytes(n, n_hits, max_len) || !values_windows(ws, ws_bytes, n, n_hits, max_len, &w))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_values_of_hits_groups_scratch_bytes");
    int e = launch_values_ranges(text.text_len, view.n_cu, n, term_len, stop, n_stop, max_len, d_hit_off, d_locs, n_hits, ws, ws_bytes, stream);
    if (e) return hip_fail("windows of hits", e);
    if (const int rc = extract_windows(idx, w, (int32_t)n_hits, stream)) return rc;
    e = launch_values_groups_of_hits(view.n_cu, n, n_stop, max_len, n_hits, d_hit_off, d_val_off, d_count, d_text_off, d_status, d_group_of_hit, ws,
                                     ws_bytes, stream);
    return e ? hip_fail("groups of hits", e) : FMX_OK;
}

int stat_rows_blocks(const HitsBetween &h, const StatRows *wanted, size_t cells, size_t P, int32_t n, StatRows *d) {
    *d = StatRows{};
    const StatRows &w = wanted ? *wanted : *d;
    auto room = [&](const void *want, size_t bytes, auto **out) -> int {
        return !wanted || want ? h.block(h.call, bytes + 8, reinterpret_cast<void **>(out)) : FMX_OK;
    };
    const size_t per_pattern = (size_t)n * 4;
    int rc;
    if ((rc = room(w.count, cells * 4, &d->count)) || (rc = room(w.sum_lo, cells * 8, &d->sum_lo)) || (rc = room(w.sum_hi, cells * 8, &d->sum_hi)) ||
        (rc = room(w.min, cells * 8, &d->min)) || (rc = room(w.max, cells * 8, &d->max)) || (P > 0 && (rc = room(w.pct, cells * P * 8, &d->pct))) ||
        (rc = room(w.no_key, per_pattern, &d->no_key)) || (rc = room(w.not_number, per_pattern, &d->not_number)) ||
        (rc = room(w.overflow, per_pattern, &d->overflow)))
        return rc;
    return FMX_OK;
}

// f(array of a, array of b, bytes) over the nine arrays; the first HIP error ends it
template <class F>
static int stat_rows_each(const StatRows &a, const StatRows &b, size_t cells, size_t P, int32_t n, F &&f) {
    const size_t per_pattern = (size_t)n * 4;
    FMX_HIP_TRY(f(a.count, b.count, cells * 4));
    FMX_HIP_TRY(f(a.sum_lo, b.sum_lo, cells * 8));
    FMX_HIP_TRY(f(a.sum_hi, b.sum_hi, cells * 8));
    FMX_HIP_TRY(f(a.min, b.min, cells * 8));
    FMX_HIP_TRY(f(a.max, b.max, cells * 8));
    FMX_HIP_TRY(f(a.pct, b.pct, cells * P * 8));
    FMX_HIP_TRY(f(a.no_key, b.no_key, per_pattern));
    FMX_HIP_TRY(f(a.not_number, b.not_number, per_pattern));
    FMX_HIP_TRY(f(a.overflow, b.overflow, per_pattern));
    return FMX_OK;
}

int stat_rows_down(const StatRows &host, const StatRows &d, size_t cells, size_t P, int32_t n, void *stream) {
    return stat_rows_each(host, d, cells, P, n, [&](void *to, const void *from, size_t bytes) -> hipError_t {
        return to && bytes > 0 ? hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)) : hipSuccess;
    });
}

int stat_rows_zero(const StatRows &d, size_t cells, size_t P, int32_t n, void *stream) {
    return stat_rows_each(d, d, cells, P, n, [&](void *p, const void *, size_t bytes) -> hipError_t {
        return p && bytes > 0 ? hipMemsetAsync(p, 0, bytes, static_cast<hipStream_t>(stream)) : hipSuccess;
    });
}

bool PackedResult::alloc(std::initializer_list<size_t> bytes) {
    size_t total = 0;
    at.clear();
    for (const size_t b : bytes) {
        at.push_back(total);
        total += (b + 7) / 8 * 8;
    }
    p = static_cast<uint8_t *>(calloc(total + 8, 1));
    return p != nullptr;
}

void keyed_null_results(const KeyedCall &c) {
    for (void **p : {(void **)c.text_off, (void **)c.chars, (void **)c.count, (void **)c.sum_lo, (void **)c.sum_hi, (void **)c.min, (void **)c.max,
                     (void **)c.pct})
        if (p) *p = nullptr;
}

bool keyed_results_missing(const KeyedCall &c) {
    return !c.text_off || !c.chars || !c.count || !c.sum_lo || !c.sum_hi || !c.min || !c.max || !c.pct;
}

StatRows keyed_host_rows(KeyedArgs &a, size_t first) {
    const PackedResult &r = a.result;
    return StatRows{r.region<int32_t>(first),     r.region<uint64_t>(first + 1), r.region<uint64_t>(first + 2),
                    r.region<int64_t>(first + 3), r.region<int64_t>(first + 4),  r.region<int64_t>(first + 5),
                    a.no_key.data(),              a.not_number.data(),           a.overflow.data()};
}

void keyed_hand_over(const KeyedCall &c, KeyedArgs &a, size_t first) {
    const StatRows s = keyed_host_rows(a, first + 2);
    *c.text_off = a.result.region<int64_t>(first);
    *c.chars = a.result.region<uint16_t>(first + 1);
    *c.count = s.count;
    *c.sum_lo = s.sum_lo;
    *c.sum_hi = s.sum_hi;
    *c.min = s.min;
    *c.max = s.max;
    *c.pct = s.pct;
    a.result.release();
}

int keyed_call_checks(const KeyedCall &c) {
    int rc;
    if ((rc = check_values_shape(c.stop, c.n_stop, c.max_len)) || (rc = check_numbers_shape(c.frac_digits, c.permille, c.n_permille)) ||
        (rc = check_by_of(c.n, c.by_of, c.m)) || (rc = check_query_arrays(c.n_terms, c.q, c.query_off, c.term_kind)) ||
        (rc = check_where_of(c.m, c.key_where_of, c.q)) || (rc = check_where_of(c.n, c.where_of, c.q)))
        return rc;
    return FMX_OK;
}

int keyed_call_views(const ::fmx_index *idx, TextView *text) {
    LineView view;
    int rc;
    if ((rc = line_view(idx, &view)) || (rc = text_view(idx, text))) return rc;
    return view.table ? FMX_OK : no_line_table();
}

bool keyed_call_fill(const KeyedCall &c, int32_t line_lo, int32_t line_hi, KeyedArgs *a) {
    if (c.n == 0) {  // nothing is searched: no groups, no rows, the terms are not judged
        zero(c.term_status, (size_t)c.n_terms);
        return false;
    }
    keyed_args_fill(c, line_lo, line_hi, a);
    return true;
}

void keyed_args_fill(const KeyedCall &c, int32_t line_lo, int32_t line_hi, KeyedArgs *a) {
    const int32_t all = c.m + c.n;
    a->m = c.m;
    a->n = c.n;
    a->by_of = c.by_of;
    a->where_all.assign(c.key_where_of, c.key_where_of + c.m);
    a->where_all.insert(a->where_all.end(), c.where_of, c.where_of + c.n);
    a->filter = HitsFilter{c.query_off, c.term_kind, c.q, a->where_all.data(), line_lo, line_hi,
                           hits_filter_asked(all, a->where_all.data(), line_lo, line_hi)};
    a->stop = c.stop;
    a->n_stop = c.n_stop;
    a->max_len = c.max_len;
    a->frac_digits = c.frac_digits;
    a->permille = c.permille;
    a->P = c.n_permille;
    a->kept_off.assign((size_t)all + 1, 0);
    a->val_off.assign((size_t)c.m + 2, 0);
    a->no_key.assign((size_t)c.n, 0);
    a->not_number.assign((size_t)c.n, 0);
    a->overflow.assign((size_t)c.n, 0);
}

template <class T>
static void copy_out(T *to, const T *from, size_t count) {
    if (to && count > 0) memcpy(to, from, count * sizeof(T));
}

int keyed_call_run(const ::fmx_index *idx, const KeyedCall &c, const ValuesBatch &batch, ValuesBetweenFn stage, void *arg, const KeyedArgs &a) {
    const size_t m = (size_t)c.m, n = (size_t)c.n;
    std::vector<int32_t> occ(m + n, 0), st_all(m + n, 0), kept_all(m + n, 0);
    if (const int rc = hits_stage_call(idx, batch, stage, arg, occ.data(), st_all.data(), nullptr, c.term_status)) return rc;
    kept_of(a.kept_off.data(), c.m + c.n, kept_all.data());
    copy_out(c.key_occurrences, occ.data(), m);
    copy_out(c.occurrences, occ.data() + m, n);
    copy_out(c.key_status, st_all.data(), m);
    copy_out(c.status, st_all.data() + m, n);
    copy_out(c.key_kept, kept_all.data(), m);
    copy_out(c.kept, kept_all.data() + m, n);
    copy_out(c.no_key, a.no_key.data(), n);
    copy_out(c.not_number, a.not_number.data(), n);
    copy_out(c.overflow, a.overflow.data(), n);
    return FMX_OK;
}

// m key patterns and n number patterns (h.n = m + n value patterns) behind n_terms filter terms
int keyed_front_stage(const HitsBetween &h, KeyedArgs &a, const char *what, KeyedFront *f, bool *done) {
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const int32_t m = a.m, n = a.n;
    *done = true;
    if (h.total - h.term_hits == 0)  // (no key or number pattern has a hit: nothing runs on the device)
        return a.text.extract ? FMX_OK : status_all(h, FMX_ST_NOT_ENABLED, what);
    int rc;
    const int64_t *d_off = nullptr;
    const int32_t *d_locs = nullptr;
    int64_t slots = 0;
    if ((rc = kept_hits_stage(h, a.filter, &d_off, &d_locs, &slots))) return rc;
    FMX_HIP_TRY(hipMemcpyAsync(a.kept_off.data(), d_off, ((size_t)h.n + 1) * 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipStreamSynchronize(st));
    if (!a.text.extract) return status_all(h, FMX_ST_NOT_ENABLED, what);
    const int64_t key_end = a.kept_off[(size_t)m], K = key_end - a.kept_off[0], N = a.kept_off[(size_t)m + n] - key_end;
    f->K = K;
    f->N = N;
    if (K == 0) {  // (no line has a key: every kept number hit is no_key, nothing beyond the filter runs)
        kept_of(a.kept_off.data() + m, n, a.no_key.data());
        return FMX_OK;
    }
    if ((rc = check_values_hits(K > N ? K : N, a.max_len))) return rc;
    auto block = [&](size_t bytes, auto **out) -> int { return h.block(h.call, bytes + 8, reinterpret_cast<void **>(out)); };
    // the two parts of the kept block, each with offsets of its own that start at 0 (the host has them: no kernel): stage a then
    // sorts the K key hits and the caller's stage the N number hits, not every slot from the terms' first hit on
    a.part_off.resize((size_t)h.n + 2);
    for (int32_t k = 0; k <= m; ++k) a.part_off[(size_t)k] = a.kept_off[(size_t)k] - a.kept_off[0];
    for (int32_t i = 0; i <= n; ++i) a.part_off[(size_t)m + 1 + i] = a.kept_off[(size_t)m + i] - key_end;
    int64_t *d_part_off = nullptr;
    if ((rc = block(((size_t)h.n + 2) * 8, &d_part_off))) return rc;
    FMX_HIP_TRY(hipMemcpyAsync(d_part_off, a.part_off.data(), ((size_t)h.n + 2) * 8, hipMemcpyHostToDevice, st));
    f->key_off = d_part_off;
    f->num_off = d_part_off + m + 1;
    f->key_locs = d_locs + a.kept_off[0];
    f->num_locs = d_locs + key_end;
    // stage a over the keys' part of the kept hits
    int64_t *d_val_off = nullptr;
    void *ws_a = nullptr;
    const size_t a_bytes = first_hits_scratch_bytes(m, K);
    f->b_bytes = values_groups_of_hits_scratch_bytes(m, K, a.max_len);
    if ((rc = block(((size_t)m + 1) * 8, &f->first_off)) || (rc = block((size_t)K * 4, &f->first_lines)) ||
        (rc = block((size_t)K * 4, &f->first_locs)) || (rc = block(a_bytes, &ws_a)))
        return rc;
    int e = launch_first_hits(h.view->table, h.view->count, a.text.text_len, h.view->n_cu, m, f->key_off, f->key_locs, K, f->first_off, f->first_lines,
                              f->first_locs, ws_a, a_bytes, st);
    if (e) return hip_fail("first hits of lines", e);
    // stage b over the first hits (at most K of them: the slots behind first_off[m] are no hits)
    if ((rc = block(((size_t)m + 2) * 8, &d_val_off)) || (rc = block((size_t)K * 4, &f->lines)) || (rc = block(((size_t)K + 1) * 8, &f->text_off)) ||
        (rc = block((size_t)K * 4, &f->group)) || (rc = block(f->b_bytes, &f->ws_b)) ||
        (rc = values_groups_run(h.idx, *h.view, a.text, m, a.term_len.data(), a.stop, a.n_stop, a.max_len, f->first_off, f->first_locs, K, d_val_off,
                                f->lines, f->text_off, f->group, h.status, f->ws_b, f->b_bytes, st)))
        return rc;
    // ONE read: the m + 1 group offsets and, behind them, the units of the groups' text (text_off[G], picked on the device)
    e = launch_values_groups_units(d_val_off, m, f->text_off, d_val_off + m + 1, st);
    if (e) return hip_fail(what, e);
    FMX_HIP_TRY(hipMemcpyAsync(a.val_off.data(), d_val_off, ((size_t)m + 2) * 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipStreamSynchronize(st));
    *done = false;
    return FMX_OK;
}

// n > 0 value patterns behind n_terms filter terms
int groups_front_stage(const HitsBetween &h, GroupsArgs &a, bool units, const char *what, GroupsFront *f, bool *done) {
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const int32_t n = h.n;
    *done = true;
    if (h.total - h.term_hits == 0)  // (no value pattern has a hit: nothing runs on the device)
        return a.text.extract ? FMX_OK : status_all(h, FMX_ST_NOT_ENABLED, what);
    int rc;
    const int64_t *d_off = nullptr;
    const int32_t *d_locs = nullptr;
    int64_t slots = 0;
    if ((rc = kept_hits_stage(h, a.filter, &d_off, &d_locs, &slots))) return rc;
    FMX_HIP_TRY(hipMemcpyAsync(a.kept_off.data(), d_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipStreamSynchronize(st));
    if (!a.text.extract) return status_all(h, FMX_ST_NOT_ENABLED, what);
    const int64_t K = a.kept_off[(size_t)n] - a.kept_off[0];
    f->K = K;
    if (K == 0) return FMX_OK;  // (no hit is kept: no groups)
    if (K > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    auto block = [&](size_t bytes, auto **out) -> int { return h.block(h.call, bytes + 8, reinterpret_cast<void **>(out)); };
    // the kept hits with offsets of their own that start at 0 (the host has them: no kernel), so that the values stage and the
    // sorts of the caller's stage run over the K kept hits, not over every slot from the terms' first hit on
    for (int32_t i = 0; i <= n; ++i) a.part_off[(size_t)i] = a.kept_off[(size_t)i] - a.kept_off[0];
    int64_t *d_part_off = nullptr, *d_val_off = nullptr;
    f->b_bytes = fmx_values_of_hits_groups_scratch_bytes(n, K, a.max_len);
    if ((rc = block(((size_t)n + 1) * 8, &d_part_off)) || (rc = block(((size_t)n + 2) * 8, &d_val_off)) || (rc = block((size_t)K * 4, &f->count)) ||
        (rc = block(((size_t)K + 1) * 8, &f->text_off)) || (rc = block((size_t)K * 4, &f->group)) || (rc = block(f->b_bytes, &f->ws_b)))
        return rc;
    FMX_HIP_TRY(hipMemcpyAsync(d_part_off, a.part_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    f->part_off = d_part_off;
    f->locs = d_locs + a.kept_off[0];
    if ((rc = fmx_values_of_hits_groups_dev(h.idx, n, a.term_len.data(), a.stop, a.n_stop, a.max_len, d_part_off, f->locs, K, d_val_off, f->count,
                                            f->text_off, f->group, h.status, f->ws_b, f->b_bytes, st)))
        return rc;
    if (units)
        if (const int e = launch_values_groups_units(d_val_off, n, f->text_off, d_val_off + n + 1, st)) return hip_fail(what, e);
    FMX_HIP_TRY(hipMemcpyAsync(a.val_off.data(), d_val_off, ((size_t)n + (units ? 2 : 1)) * 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipStreamSynchronize(st));
    *done = false;
    return FMX_OK;
}

}  // namespace fmx
