// fmx_by_hist_api.cpp — STATISTICS OF THE NUMBER BEHIND A PATTERN, BY THE VALUE OF A FIELD OF THE SAME LINE, PER BUCKET OF LINES
// (include/fmx.h "STATISTICS BY KEY PER BUCKET"; fmx_by_hist.hpp has the definition): the device stage
// fmx_numbers_by_key_buckets_dev over fmx_by_hist.hip's launchers with the packed extract between them, and the host forms
// fmx_number_stats_by_histogram_batch / fmx_number_stats_by_histogram_class_batch.  Of a handle this file sees what fmx::line_view
// and fmx::text_view hand out; a host form runs the packed sequence of fmx_api.cpp up to the stage of this file
// (fmx::hits_stage_call) over ONE merged batch terms | key patterns | number patterns, then the filter with the edges' span as its
// window (fmx::kept_hits_stage), stage a over the keys' part, stage b, ONE read of the m + 1 group offsets and the size of the
// groups' text, which sizes the key rows and the cells, the new stage over the numbers' part, the fill of the groups' text and the
// gather of the key rows' text.  Its waits are fmx_number_stats_by_batch's, plus the 8-byte read of the rows' text length.
#include "fmx_by_hist.hpp"
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

namespace {

using fmx::api_fail;
using fmx::guarded;
using fmx::no_line_table;
using fmx::zero;

int hip_fail(const char *what, int e) { return api_fail(FMX_E_HIP, std::string(what) + ": " + hipGetErrorString((hipError_t)e)); }

int check_values_shape(const uint16_t *stop, int32_t n_stop, int32_t max_len) {
    if (max_len < 1 || max_len > fmx::kValuesMaxLen) return api_fail(FMX_E_ARG, "max_len is outside [1, 64]");
    if (n_stop < 0 || n_stop > fmx::kValuesMaxStop || (n_stop > 0 && !stop)) return api_fail(FMX_E_ARG, "the stop set is outside [0, 64] code units");
    return FMX_OK;
}
int check_hits(int64_t n_hits, int32_t max_len) {
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    if (n_hits * max_len > fmx::kValuesMaxUnits) return api_fail(FMX_E_ARG, "the windows of the hits hold more than 2^35 code units");
    return FMX_OK;
}
int check_term_len(int32_t n, const int32_t *term_len) {
    for (int32_t i = 0; i < n; ++i)
        if (term_len[i] < 0) return api_fail(FMX_E_ARG, "term_len[" + std::to_string(i) + "] is negative");
    return FMX_OK;
}
int check_numbers_shape(int32_t frac_digits, const int32_t *permille, int32_t n_permille) {
    if (frac_digits < 0 || frac_digits > fmx::kNumFracMax) return api_fail(FMX_E_ARG, "frac_digits is outside [0, 9]");
    switch (fmx::fm_num_permille_bad(permille, n_permille)) {
        case 0: return FMX_OK;
        case 1: return api_fail(FMX_E_ARG, "n_permille is outside [0, 16]");
        default: return api_fail(FMX_E_ARG, "a permille is outside [0, 1000]");
    }
}
// the edges (none at all: one bucket, every line), top and the cells they allow, from the arguments alone
int check_cut(int32_t n, const int32_t *edges, int32_t n_edges, int32_t top, int32_t n_permille, int32_t *B) {
    if (edges || n_edges != 0)
        if (const int rc = fmx::check_edges_array(edges, n_edges)) return rc;
    *B = edges ? n_edges - 1 : 1;
    switch (fmx::fm_bh_args_bad(n, top, *B, n_permille)) {
        case 0: return FMX_OK;
        case 1: return api_fail(FMX_E_ARG, "top is outside [1, 65536]");
        case 2: return api_fail(FMX_E_ARG, "more than 2^27 cells in one call (number patterns * (top + 1) * buckets)");
        default: return api_fail(FMX_E_ARG, "more than 2^27 percentiles in one call (cells * n_permille)");
    }
}
// the key rows and the cells of a call from the key patterns' group offsets (fm_bh_shape_bad's rules as messages)
int check_groups(int32_t n, const int32_t *by_of, int32_t m, const int64_t *val_off, int32_t top, int32_t B, int32_t n_permille,
                 int64_t *key_row_off, int64_t *cell_off) {
    switch (fmx::fm_bh_shape_bad(n, by_of, m, val_off, top, B, n_permille, key_row_off, cell_off, nullptr)) {
        case 0: return FMX_OK;
        case 1: return api_fail(FMX_E_ARG, "number patterns without a key pattern (m == 0 with n > 0)");
        case 2: return api_fail(FMX_E_ARG, "a by_of entry is outside 0 .. m - 1");
        case 3: return api_fail(FMX_E_ARG, "val_off does not start at 0 or decreases");
        case 6: return api_fail(FMX_E_ARG, "more than 2^31 - 1 groups in one call");
        default: return api_fail(FMX_E_ARG, "top is outside [1, 65536] or the call has more than 2^27 cells or percentiles");
    }
}

struct Cells {
    int32_t *count;
    uint64_t *sum_lo, *sum_hi;
    int64_t *min, *max, *pct;
    int32_t *no_key, *not_number, *overflow;
};
struct FirstHits {
    const int64_t *off;
    const int32_t *lines, *group, *group_lines;
};
struct KeyRows {
    int64_t *off;
    int32_t *group, *lines;
    int64_t *cell_off;
};
struct Cut {
    const int32_t *edges;
    int32_t n_edges, top;
};

// the new stage behind the arguments' checks: the ranks and the key rows, the windows and codes, the windows' text, the cells
// (n > 0, m > 0, an index with extraction; n_hits == 0: the key rows alone)
int cells_impl(const fmx_index *idx, const fmx::LineView &view, const fmx::TextView &text, int32_t n, const int32_t *term_len, const int32_t *by_of,
               int32_t m, const int64_t *val_off, const Cut &cut, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits,
               const FirstHits &f, int32_t frac_digits, const int32_t *permille, int32_t P, const KeyRows &k, const Cells &c, int32_t *d_status,
               void *ws, size_t ws_bytes, hipStream_t st) {
    int e = fmx::launch_by_hist_codes(view.table, view.count, text.text_len, view.n_cu, n, term_len, by_of, m, val_off, cut.top, cut.edges,
                                      cut.n_edges, d_hit_off, d_locs, n_hits, f.off, f.lines, f.group, f.group_lines, permille, P, k.off, k.group,
                                      k.lines, k.cell_off, ws, ws_bytes, st);
    if (e) return hip_fail("key rows and codes of hits", e);
    if (n_hits == 0) return FMX_OK;
    fmx::ValuesWindows w;
    if (!fmx::numbers_by_key_buckets_windows(ws, ws_bytes, n, m, val_off[m], n_hits, cut.n_edges, P, &w))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_numbers_by_key_buckets_scratch_bytes");
    if (const int rc = fmx::extract_windows(idx, w, (int32_t)n_hits, st)) return rc;
    e = fmx::launch_by_hist_cells(view.n_cu, n, by_of, m, val_off, cut.top, cut.n_edges, d_hit_off, n_hits, frac_digits, P, c.count, c.sum_lo,
                                  c.sum_hi, c.min, c.max, c.pct, c.no_key, c.not_number, c.overflow, d_status, ws, ws_bytes, st);
    if (e) return hip_fail("numbers by key per bucket", e);
    return FMX_OK;
}

// ---- the host form --------------------------------------------------------------------------------------------------------------------
// the ONE allocation of the answer: key_row_lines | key_row_group | text_off | chars | count | sum_lo | sum_hi | min | max | pct, each
// at a multiple of 8
struct Result {
    uint8_t *p = nullptr;
    size_t lines = 0, group = 0, text_off = 0, chars = 0, count = 0, sum_lo = 0, sum_hi = 0, min = 0, max = 0, pct = 0, total = 0;
    ~Result() { free(p); }
    bool alloc(size_t R, size_t units, size_t cells, size_t P) {
        size_t at = 0;
        auto take = [&](size_t bytes) {
            const size_t here = at;
            at += (bytes + 7) / 8 * 8;
            return here;
        };
        lines = take(R * 4);
        group = take(R * 4);
        text_off = take((R + 1) * 8);
        chars = take(units * 2 + 2);
        count = take(cells * 4);
        sum_lo = take(cells * 8);
        sum_hi = take(cells * 8);
        min = take(cells * 8);
        max = take(cells * 8);
        pct = take(cells * P * 8);
        total = at + 8;
        p = static_cast<uint8_t *>(calloc(total, 1));
        return p != nullptr;
    }
};

struct ByHistArgs {
    int32_t m = 0, n = 0;
    const int32_t *by_of = nullptr;
    fmx::HitsFilter filter{};
    Cut cut{};
    int32_t B = 1;
    std::vector<int32_t> where_all, term_len;  // m + n each: the key patterns', then the number patterns'
    const uint16_t *stop = nullptr;
    int32_t n_stop = 0, max_len = 0, frac_digits = 0;
    const int32_t *permille = nullptr;
    int32_t P = 0;
    fmx::TextView text{};
    // what the stage leaves (host; arrived when the call has synchronised)
    std::vector<int64_t> kept_off, val_off, key_row_off, cell_off;  // m + n + 1, m + 2 (the units of the groups' text behind), m + 1, n + 1
    std::vector<int64_t> part_off;                                  // the key part's and the number part's own offsets
    std::vector<int32_t> no_key, not_number, overflow;              // n each
    Result result;
};

int status_all(const fmx::HitsBetween &h, int32_t value) {
    const int e = fmx::launch_values_status_all(h.view->n_cu, h.status, h.n, value, h.stream);
    return e ? hip_fail("numbers by key per bucket", e) : FMX_OK;
}

// m key patterns and n number patterns (h.n = m + n value patterns) behind n_terms filter terms
int by_hist_stage(const fmx::HitsBetween &h, void *arg) {
    ByHistArgs &a = *static_cast<ByHistArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const int32_t m = a.m, n = a.n;
    if (h.total - h.term_hits == 0)  // (no key or number pattern has a hit: nothing runs on the device)
        return a.text.extract ? FMX_OK : status_all(h, FMX_ST_NOT_ENABLED);
    int rc;
    const int64_t *d_off = nullptr;
    const int32_t *d_locs = nullptr;
    int64_t slots = 0;
    if ((rc = fmx::kept_hits_stage(h, a.filter, &d_off, &d_locs, &slots))) return rc;
    FMX_HIP_TRY(hipMemcpyAsync(a.kept_off.data(), d_off, ((size_t)h.n + 1) * 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipStreamSynchronize(st));
    if (!a.text.extract) return status_all(h, FMX_ST_NOT_ENABLED);
    const int64_t key_end = a.kept_off[(size_t)m], all_end = a.kept_off[(size_t)m + n];
    const int64_t K = key_end - a.kept_off[0], N = all_end - key_end;
    if (K == 0) {  // (no line has a key: every kept number hit is no_key, nothing beyond the filter runs)
        for (int32_t i = 0; i < n; ++i) a.no_key[(size_t)i] = (int32_t)(a.kept_off[(size_t)m + i + 1] - a.kept_off[(size_t)m + i]);
        return FMX_OK;
    }
    if ((rc = check_hits(K > N ? K : N, a.max_len))) return rc;
    auto block = [&](size_t bytes, auto **out) -> int { return h.block(h.call, bytes + 8, reinterpret_cast<void **>(out)); };
    // the two parts of the kept block, each with offsets of its own that start at 0 (the host has them: no kernel)
    a.part_off.resize((size_t)h.n + 2);
    for (int32_t k = 0; k <= m; ++k) a.part_off[(size_t)k] = a.kept_off[(size_t)k] - a.kept_off[0];
    for (int32_t i = 0; i <= n; ++i) a.part_off[(size_t)m + 1 + i] = a.kept_off[(size_t)m + i] - key_end;
    int64_t *d_part_off = nullptr;
    if ((rc = block(((size_t)h.n + 2) * 8, &d_part_off))) return rc;
    FMX_HIP_TRY(hipMemcpyAsync(d_part_off, a.part_off.data(), ((size_t)h.n + 2) * 8, hipMemcpyHostToDevice, st));
    const int64_t *d_key_off = d_part_off, *d_num_off = d_part_off + m + 1;
    const int32_t *d_key_locs = d_locs + a.kept_off[0], *d_num_locs = d_locs + key_end;
    // stage a over the keys' part of the kept hits
    int64_t *d_first_off = nullptr, *d_val_off = nullptr, *d_text_off = nullptr;
    int32_t *d_first_lines = nullptr, *d_first_locs = nullptr, *d_lines = nullptr, *d_group = nullptr;
    void *ws_a = nullptr, *ws_b = nullptr;
    const size_t a_bytes = fmx::first_hits_scratch_bytes(m, K), b_bytes = fmx_values_of_hits_groups_scratch_bytes(m, K, a.max_len);
    if ((rc = block(((size_t)m + 1) * 8, &d_first_off)) || (rc = block((size_t)K * 4, &d_first_lines)) || (rc = block((size_t)K * 4, &d_first_locs)) ||
        (rc = block(a_bytes, &ws_a)))
        return rc;
    int e = fmx::launch_first_hits(h.view->table, h.view->count, a.text.text_len, h.view->n_cu, m, d_key_off, d_key_locs, K, d_first_off, d_first_lines,
                                   d_first_locs, ws_a, a_bytes, st);
    if (e) return hip_fail("first hits of lines", e);
    // stage b over the first hits (at most K of them: the slots behind first_off[m] are no hits)
    if ((rc = block(((size_t)m + 2) * 8, &d_val_off)) || (rc = block((size_t)K * 4, &d_lines)) || (rc = block(((size_t)K + 1) * 8, &d_text_off)) ||
        (rc = block((size_t)K * 4, &d_group)) || (rc = block(b_bytes, &ws_b)) ||
        (rc = fmx_values_of_hits_groups_dev(h.idx, m, a.term_len.data(), a.stop, a.n_stop, a.max_len, d_first_off, d_first_locs, K, d_val_off, d_lines,
                                            d_text_off, d_group, h.status, ws_b, b_bytes, st)))
        return rc;
    // ONE read: the m + 1 group offsets and, behind them, the units of the groups' text (text_off[G], picked on the device)
    e = fmx::launch_values_groups_units(d_val_off, m, d_text_off, d_val_off + m + 1, st);
    if (e) return hip_fail("numbers by key per bucket", e);
    FMX_HIP_TRY(hipMemcpyAsync(a.val_off.data(), d_val_off, ((size_t)m + 2) * 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipStreamSynchronize(st));
    if ((rc = check_groups(n, a.by_of, m, a.val_off.data(), a.cut.top, a.B, a.P, a.key_row_off.data(), a.cell_off.data()))) return rc;
    const size_t G = (size_t)a.val_off[(size_t)m], R = (size_t)a.key_row_off[(size_t)m], cells = (size_t)a.cell_off[(size_t)n], P = (size_t)a.P;
    const int64_t units = a.val_off[(size_t)m + 1];
    // the ranks, the key rows, the codes and the cells over the numbers' part
    Cells d{};
    KeyRows kr{};
    void *ws_c = nullptr;
    const size_t c_bytes = fmx::numbers_by_key_buckets_scratch_bytes(n, m, (int64_t)G, N, a.cut.n_edges, a.P);
    if ((rc = block(R * 4, &kr.group)) || (rc = block(R * 4, &kr.lines)) || (rc = block(cells * 4, &d.count)) || (rc = block(cells * 8, &d.sum_lo)) ||
        (rc = block(cells * 8, &d.sum_hi)) || (rc = block(cells * 8, &d.min)) || (rc = block(cells * 8, &d.max)) ||
        (P > 0 && (rc = block(cells * P * 8, &d.pct))) || (rc = block((size_t)n * 4, &d.no_key)) || (rc = block((size_t)n * 4, &d.not_number)) ||
        (rc = block((size_t)n * 4, &d.overflow)) || (rc = block(c_bytes, &ws_c)) ||
        (rc = cells_impl(h.idx, *h.view, a.text, n, a.term_len.data() + m, a.by_of, m, a.val_off.data(), a.cut, d_num_off, d_num_locs, N,
                         FirstHits{d_first_off, d_first_lines, d_group, d_lines}, a.frac_digits, a.permille, a.P, kr, d,
                         h.status ? h.status + m : nullptr, ws_c, c_bytes, st)))
        return rc;
    // the text of ALL groups on the device, the text of the key rows alone on the way down
    uint16_t *d_chars = nullptr, *d_row_chars = nullptr;
    int64_t *d_row_text_off = nullptr;
    void *ws_g = nullptr;
    const size_t g_bytes = fmx::values_gather_rows_scratch_bytes(m, (int64_t)R);
    if ((rc = block((size_t)units * 2, &d_chars)) || (rc = block((size_t)units * 2, &d_row_chars)) || (rc = block((R + 1) * 8, &d_row_text_off)) ||
        (rc = block(g_bytes, &ws_g)))
        return rc;
    if (units > 0 && (rc = fmx_values_fill_dev(h.idx, (int64_t)G, d_text_off, d_chars, ws_b, b_bytes, st))) return rc;
    e = fmx::launch_values_gather_rows(h.view->n_cu, m, a.val_off.data(), a.cut.top, units, kr.group, d_text_off, d_chars, d_row_text_off, d_row_chars,
                                       ws_g, g_bytes, st);
    if (e) return hip_fail("text of the key rows", e);
    int64_t row_units = 0;  // ONE 8-byte read: the packed length of the key rows' text sizes the allocation
    FMX_HIP_TRY(hipMemcpyAsync(&row_units, d_row_text_off + R, 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipStreamSynchronize(st));
    if (!a.result.alloc(R, (size_t)row_units, cells, P)) return api_fail(FMX_E_NOMEM, "out of host memory for " + std::to_string(cells) + " cells");
    uint8_t *out = a.result.p;
    auto down = [&](void *host, const void *dev, size_t bytes) -> hipError_t {
        return bytes > 0 ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    FMX_HIP_TRY(down(out + a.result.lines, kr.lines, R * 4));
    FMX_HIP_TRY(down(out + a.result.group, kr.group, R * 4));
    FMX_HIP_TRY(down(out + a.result.text_off, d_row_text_off, (R + 1) * 8));
    FMX_HIP_TRY(down(out + a.result.chars, d_row_chars, (size_t)row_units * 2));
    if (N == 0) return FMX_OK;  // (no number hit is kept: the key rows with zero cells — the allocation is zeroed)
    FMX_HIP_TRY(down(out + a.result.count, d.count, cells * 4));
    FMX_HIP_TRY(down(out + a.result.sum_lo, d.sum_lo, cells * 8));
    FMX_HIP_TRY(down(out + a.result.sum_hi, d.sum_hi, cells * 8));
    FMX_HIP_TRY(down(out + a.result.min, d.min, cells * 8));
    FMX_HIP_TRY(down(out + a.result.max, d.max, cells * 8));
    FMX_HIP_TRY(down(out + a.result.pct, d.pct, cells * P * 8));
    FMX_HIP_TRY(down(a.no_key.data(), d.no_key, (size_t)n * 4));
    FMX_HIP_TRY(down(a.not_number.data(), d.not_number, (size_t)n * 4));
    FMX_HIP_TRY(down(a.overflow.data(), d.overflow, (size_t)n * 4));
    return FMX_OK;
}

template <class T>
void copy_out(T *to, const T *from, size_t count) {
    if (to && count > 0) memcpy(to, from, count * sizeof(T));
}

// what the two host forms take besides their patterns, and what they hand back
struct ByHistCall {
    int32_t m, n;
    const int32_t *by_of;
    int32_t n_terms;
    const int32_t *query_off;
    const uint8_t *term_kind;
    int32_t q;
    const int32_t *key_where_of, *where_of, *edges;
    int32_t n_edges, top;
    const uint16_t *stop;
    int32_t n_stop, max_len, frac_digits;
    const int32_t *permille;
    int32_t n_permille;
    int32_t *n_groups;
    int64_t *key_row_off;
    int32_t **key_row_lines, **key_row_group;
    int64_t **text_off;
    uint16_t **chars;
    int64_t *cell_off;
    int32_t **count;
    uint64_t **sum_lo, **sum_hi;
    int64_t **min, **max, **pct;
    int32_t *no_key, *not_number, *overflow, *occurrences, *kept, *status, *key_occurrences, *key_kept, *key_status, *term_status;
};

bool results_missing(const ByHistCall &c) {
    return !c.key_row_off || !c.cell_off || !c.key_row_lines || !c.key_row_group || !c.text_off || !c.chars || !c.count || !c.sum_lo || !c.sum_hi ||
           !c.min || !c.max || !c.pct;
}
void null_results(const ByHistCall &c) {
    for (void **p : {(void **)c.key_row_lines, (void **)c.key_row_group, (void **)c.text_off, (void **)c.chars, (void **)c.count, (void **)c.sum_lo,
                     (void **)c.sum_hi, (void **)c.min, (void **)c.max, (void **)c.pct})
        *p = nullptr;
}

// the checks of the HOST arrays both forms share (behind their own batches'), the handle's views and the empty call; *done: answered
int by_hist_call_args(const fmx_index *idx, const ByHistCall &c, ByHistArgs *a, bool *done) {
    int rc;
    if ((rc = check_values_shape(c.stop, c.n_stop, c.max_len)) || (rc = check_numbers_shape(c.frac_digits, c.permille, c.n_permille)) ||
        (rc = fmx::check_by_of(c.n, c.by_of, c.m)) || (rc = fmx::check_query_arrays(c.n_terms, c.q, c.query_off, c.term_kind)) ||
        (rc = fmx::check_where_of(c.m, c.key_where_of, c.q)) || (rc = fmx::check_where_of(c.n, c.where_of, c.q)) ||
        (rc = check_cut(c.n, c.edges, c.n_edges, c.top, c.n_permille, &a->B)))
        return rc;
    fmx::LineView view;
    if ((rc = fmx::line_view(idx, &view)) || (rc = fmx::text_view(idx, &a->text))) return rc;
    if (!view.table) return no_line_table();  // (keys are per line)
    null_results(c);
    zero(c.n_groups, (size_t)c.m);
    zero(c.key_row_off, (size_t)c.m + 1);
    zero(c.cell_off, (size_t)c.n + 1);
    *done = c.n == 0;
    if (c.n == 0) {  // nothing is searched: no key rows, no cells, the terms are not judged
        zero(c.term_status, (size_t)c.n_terms);
        return FMX_OK;
    }
    const int32_t all = c.m + c.n;
    // the window of the filter is the span of the edges: every kept hit has a bucket
    const int32_t lo = c.edges ? c.edges[0] : 0, hi = c.edges ? c.edges[c.n_edges - 1] : INT32_MAX;
    a->m = c.m;
    a->n = c.n;
    a->by_of = c.by_of;
    a->where_all.assign(c.key_where_of, c.key_where_of + c.m);
    a->where_all.insert(a->where_all.end(), c.where_of, c.where_of + c.n);
    a->filter = fmx::HitsFilter{c.query_off, c.term_kind, c.q, a->where_all.data(), lo, hi, fmx::hits_filter_asked(all, a->where_all.data(), lo, hi)};
    a->cut = Cut{c.edges, c.edges ? c.n_edges : 0, c.top};
    a->stop = c.stop;
    a->n_stop = c.n_stop;
    a->max_len = c.max_len;
    a->frac_digits = c.frac_digits;
    a->permille = c.permille;
    a->P = c.n_permille;
    a->kept_off.assign((size_t)all + 1, 0);
    a->val_off.assign((size_t)c.m + 2, 0);
    a->key_row_off.assign((size_t)c.m + 1, 0);
    a->cell_off.assign((size_t)c.n + 1, 0);
    a->no_key.assign((size_t)c.n, 0);
    a->not_number.assign((size_t)c.n, 0);
    a->overflow.assign((size_t)c.n, 0);
    return FMX_OK;
}

// the call over the merged batch terms | key patterns | number patterns, and the answer into the caller's arrays
int by_hist_call_run(const fmx_index *idx, const ByHistCall &c, const fmx::ValuesBatch &batch, ByHistArgs &a) {
    const int32_t m = c.m, n = c.n, all = m + n;
    std::vector<int32_t> occ((size_t)all, 0), st_all((size_t)all, 0), kept_all((size_t)all, 0);
    if (const int rc = fmx::hits_stage_call(idx, batch, by_hist_stage, &a, occ.data(), st_all.data(), nullptr, c.term_status)) return rc;
    fmx::kept_of(a.kept_off.data(), all, kept_all.data());
    copy_out(c.key_occurrences, occ.data(), (size_t)m);
    copy_out(c.occurrences, occ.data() + m, (size_t)n);
    copy_out(c.key_status, st_all.data(), (size_t)m);
    copy_out(c.status, st_all.data() + m, (size_t)n);
    copy_out(c.key_kept, kept_all.data(), (size_t)m);
    copy_out(c.kept, kept_all.data() + m, (size_t)n);
    copy_out(c.no_key, a.no_key.data(), (size_t)n);
    copy_out(c.not_number, a.not_number.data(), (size_t)n);
    copy_out(c.overflow, a.overflow.data(), (size_t)n);
    for (int32_t k = 0; k < m && c.n_groups; ++k) c.n_groups[k] = (int32_t)(a.val_off[(size_t)k + 1] - a.val_off[(size_t)k]);
    if (a.result.p) {  // the ONE allocation: freed with fmx_free_buffer((uint8_t *)*key_row_lines)
        copy_out(c.key_row_off, a.key_row_off.data(), (size_t)m + 1);
        copy_out(c.cell_off, a.cell_off.data(), (size_t)n + 1);
        uint8_t *out = a.result.p;
        const Result &r = a.result;
        *c.key_row_lines = reinterpret_cast<int32_t *>(out + r.lines);
        *c.key_row_group = reinterpret_cast<int32_t *>(out + r.group);
        *c.text_off = reinterpret_cast<int64_t *>(out + r.text_off);
        *c.chars = reinterpret_cast<uint16_t *>(out + r.chars);
        *c.count = reinterpret_cast<int32_t *>(out + r.count);
        *c.sum_lo = reinterpret_cast<uint64_t *>(out + r.sum_lo);
        *c.sum_hi = reinterpret_cast<uint64_t *>(out + r.sum_hi);
        *c.min = reinterpret_cast<int64_t *>(out + r.min);
        *c.max = reinterpret_cast<int64_t *>(out + r.max);
        *c.pct = reinterpret_cast<int64_t *>(out + r.pct);
        a.result.p = nullptr;
    }
    return FMX_OK;
}

}  // namespace

extern "C" {

size_t fmx_numbers_by_key_buckets_scratch_bytes(int32_t n, int32_t m, int64_t n_groups, int64_t n_hits, int32_t n_edges, int32_t n_permille) {
    return fmx::numbers_by_key_buckets_scratch_bytes(n, m, n_groups, n_hits, n_edges, n_permille);
}

int fmx_numbers_by_key_buckets_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const int32_t *by_of, int32_t m, const int64_t *val_off,
                                   int32_t top, const int32_t *edges, int32_t n_edges, const int64_t *d_hit_off, const int32_t *d_locs,
                                   int64_t n_hits, const int64_t *d_first_off, const int32_t *d_first_lines, const int32_t *d_group_of_first,
                                   const int32_t *d_group_lines, int32_t frac_digits, const int32_t *permille, int32_t n_permille,
                                   int64_t *d_key_row_off, int32_t *d_key_row_group, int32_t *d_key_row_lines, int64_t *d_cell_off, int32_t *d_count,
                                   uint64_t *d_sum_lo, uint64_t *d_sum_hi, int64_t *d_min, int64_t *d_max, int64_t *d_pct, int32_t *d_no_key,
                                   int32_t *d_not_number, int32_t *d_overflow, int32_t *d_status, void *d_ws, size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || m < 0 || n_hits < 0 || n_edges < 0 ||
        (n > 0 && (!d_hit_off || !term_len || !by_of || !val_off || !d_key_row_off || !d_cell_off || !d_first_off || !d_count)) ||
        (n > 0 && n_hits > 0 && !d_locs))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    int rc;
    int32_t B = 1;
    if ((rc = check_numbers_shape(frac_digits, permille, n_permille)) || (rc = check_term_len(n, term_len)) ||
        (rc = check_cut(n, edges, n_edges, top, n_permille, &B)))
        return rc;
    if (n > 0 && m <= 0) return api_fail(FMX_E_ARG, "number patterns without a key pattern (m == 0 with n > 0)");
    std::vector<int64_t> key_row_off((size_t)m + 1, 0), cell_off((size_t)n + 1, 0);
    if (n > 0 && (rc = check_groups(n, by_of, m, val_off, top, B, n_permille, key_row_off.data(), cell_off.data()))) return rc;
    fmx::LineView view;
    fmx::TextView text;
    if ((rc = fmx::line_view(idx, &view)) || (rc = fmx::text_view(idx, &text))) return rc;
    if (!view.table) return no_line_table();
    if (n == 0) return FMX_OK;
    const int64_t G = val_off[m];
    const size_t cells = (size_t)cell_off[(size_t)n], P = (size_t)n_permille;
    if (G > 0 && (!d_group_lines || !d_key_row_group || !d_key_row_lines || (n_hits > 0 && (!d_first_lines || !d_group_of_first))))
        return api_fail(FMX_E_ARG, "bad arguments");
    const bool runs = n_hits > 0 && text.extract;  // (else: the key rows alone, the cells and the per-pattern counters zeroed)
    const int64_t H = runs ? n_hits : 0;
    if (!d_ws || ws_bytes < fmx::numbers_by_key_buckets_scratch_bytes(n, m, G, H, edges ? n_edges : 0, n_permille))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_numbers_by_key_buckets_scratch_bytes");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Cells c{d_count, d_sum_lo, d_sum_hi, d_min, d_max, n_permille > 0 ? d_pct : nullptr, d_no_key, d_not_number, d_overflow};
    rc = cells_impl(idx, view, text, n, term_len, by_of, m, val_off, Cut{edges, edges ? n_edges : 0, top}, d_hit_off, d_locs, H,
                    FirstHits{d_first_off, d_first_lines, d_group_of_first, d_group_lines}, frac_digits, permille, n_permille,
                    KeyRows{d_key_row_off, d_key_row_group, d_key_row_lines, d_cell_off}, c, d_status, d_ws, ws_bytes, st);
    if (rc || runs) return rc;
    FMX_HIP_TRY(hipMemsetAsync(c.count, 0, cells * 4, st));
    for (void *p : {(void *)c.sum_lo, (void *)c.sum_hi, (void *)c.min, (void *)c.max})
        if (p) FMX_HIP_TRY(hipMemsetAsync(p, 0, cells * 8, st));
    if (c.pct && P > 0) FMX_HIP_TRY(hipMemsetAsync(c.pct, 0, cells * P * 8, st));
    for (int32_t *p : {c.no_key, c.not_number, c.overflow})
        if (p) FMX_HIP_TRY(hipMemsetAsync(p, 0, (size_t)n * 4, st));
    if (n_hits > 0) {  // (an index without extraction)
        const int e = fmx::launch_values_status_all(view.n_cu, d_status, n, FMX_ST_NOT_ENABLED, st);
        if (e) return hip_fail("numbers by key per bucket", e);
    }
    return FMX_OK;
    });
}

int fmx_number_stats_by_histogram_batch(const fmx_index *idx, const uint16_t *key_pat, const int32_t *key_off, int32_t m, const uint16_t *pat,
                                        const int32_t *pat_off, int32_t n, const int32_t *by_of, const uint16_t *term_pat, const int32_t *term_off,
                                        int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q, const int32_t *key_where_of,
                                        const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t top, const uint16_t *stop,
                                        int32_t n_stop, int32_t max_len, int32_t frac_digits, const int32_t *permille, int32_t n_permille,
                                        int32_t *n_groups, int64_t *key_row_off, int32_t **key_row_lines, int32_t **key_row_group, int64_t **text_off,
                                        uint16_t **chars, int64_t *cell_off, int32_t **count, uint64_t **sum_lo, uint64_t **sum_hi, int64_t **min,
                                        int64_t **max, int64_t **pct, int32_t *no_key, int32_t *not_number, int32_t *overflow, int32_t *occurrences,
                                        int32_t *kept, int32_t *status, int32_t *key_occurrences, int32_t *key_kept, int32_t *key_status,
                                        int32_t *term_status) {
    return guarded([&]() -> int {
    const ByHistCall c{m, n, by_of, n_terms, query_off, term_kind, q, key_where_of, where_of, edges, n_edges, top, stop, n_stop, max_len, frac_digits,
                       permille, n_permille, n_groups, key_row_off, key_row_lines, key_row_group, text_off, chars, cell_off, count, sum_lo, sum_hi,
                       min, max, pct, no_key, not_number, overflow, occurrences, kept, status, key_occurrences, key_kept, key_status, term_status};
    if (!idx || m < 0 || n < 0 || n_terms < 0 || q < 0 || n_edges < 0 || results_missing(c) || (m > 0 && (!key_off || !key_where_of)) ||
        (n > 0 && (!pat_off || !where_of || !by_of)) || (n_terms > 0 && !term_off))
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_literal_batches(pat_off, n, term_off, n_terms)) || (m > 0 && (rc = fmx::check_offsets(key_off, m, "key pattern")))) return rc;
    ByHistArgs a;
    bool done = false;
    if ((rc = by_hist_call_args(idx, c, &a, &done)) || done) return rc;
    // ONE batch of value patterns: the key patterns, the number patterns behind them
    const int32_t all = m + n;
    std::vector<uint16_t> both;
    std::vector<int32_t> both_off((size_t)all + 1, 0);
    for (int32_t k = 0; k < m; ++k) {
        if (key_off[k + 1] > key_off[k] && !key_pat) return api_fail(FMX_E_ARG, "bad arguments");
        both.insert(both.end(), key_pat + key_off[k], key_pat + key_off[k + 1]);
        both_off[(size_t)k + 1] = (int32_t)both.size();
        a.term_len.push_back(key_off[k + 1] - key_off[k]);
    }
    for (int32_t i = 0; i < n; ++i) {
        if (pat_off[i + 1] > pat_off[i] && !pat) return api_fail(FMX_E_ARG, "bad arguments");
        both.insert(both.end(), pat + pat_off[i], pat + pat_off[i + 1]);
        both_off[(size_t)m + i + 1] = (int32_t)both.size();
        a.term_len.push_back(pat_off[i + 1] - pat_off[i]);
    }
    both.push_back(0);
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_literal_batch(both.data(), both_off.data(), all, term_pat, term_off, n_terms, &merged, &batch))) return rc;
    return by_hist_call_run(idx, c, batch, a);
    });
}

int fmx_number_stats_by_histogram_class_batch(const fmx_index *idx, const uint16_t *key_alt, const int32_t *key_pos_off, int32_t key_n_pos,
                                              const int32_t *key_off, int32_t m, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                              const int32_t *pat_off, int32_t n, const int32_t *by_of, const uint16_t *term_alt,
                                              const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off, int32_t n_terms,
                                              int32_t max_ranges, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                              const int32_t *key_where_of, const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t top,
                                              const uint16_t *stop, int32_t n_stop, int32_t max_len, int32_t frac_digits, const int32_t *permille,
                                              int32_t n_permille, int32_t *n_groups, int64_t *key_row_off, int32_t **key_row_lines,
                                              int32_t **key_row_group, int64_t **text_off, uint16_t **chars, int64_t *cell_off, int32_t **count,
                                              uint64_t **sum_lo, uint64_t **sum_hi, int64_t **min, int64_t **max, int64_t **pct, int32_t *no_key,
                                              int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept, int32_t *status,
                                              int32_t *key_occurrences, int32_t *key_kept, int32_t *key_status, int32_t *term_status) {
    return guarded([&]() -> int {
    const ByHistCall c{m, n, by_of, n_terms, query_off, term_kind, q, key_where_of, where_of, edges, n_edges, top, stop, n_stop, max_len, frac_digits,
                       permille, n_permille, n_groups, key_row_off, key_row_lines, key_row_group, text_off, chars, cell_off, count, sum_lo, sum_hi,
                       min, max, pct, no_key, not_number, overflow, occurrences, kept, status, key_occurrences, key_kept, key_status, term_status};
    if (!idx || m < 0 || n < 0 || n_pos < 0 || key_n_pos < 0 || n_terms < 0 || term_n_pos < 0 || q < 0 || n_edges < 0 || results_missing(c) ||
        !pos_off || !pat_off || !key_pos_off || !key_off || (m > 0 && !key_where_of) || (n > 0 && (!where_of || !by_of)) ||
        (n_terms > 0 && (!term_pos_off || !term_off)) || max_ranges < 1 || max_ranges > FMX_CLASS_RANGES_MAX)
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    // the key patterns are judged as the number patterns are: the terms' slot of the check takes them
    if ((rc = fmx::check_class_batches(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms)) ||
        (rc = fmx::check_class_batches(key_alt, key_pos_off, key_n_pos, key_off, m, nullptr, nullptr, 0, nullptr, 0)))
        return rc;
    ByHistArgs a;
    bool done = false;
    if ((rc = by_hist_call_args(idx, c, &a, &done)) || done) return rc;
    // ONE batch of value patterns, position by position: the key patterns, the number patterns behind them; then the terms in front
    fmx::MergedBatch both, merged;
    fmx::ValuesBatch both_batch, batch;
    if ((rc = fmx::merge_class_batch(alt, pos_off, n_pos, pat_off, n, key_alt, key_pos_off, key_n_pos, key_off, m, max_ranges, &both, &both_batch)) ||
        (rc = fmx::merge_class_batch(both.chars.data(), both.pos.data(), (int32_t)both.pos.size() - 1, both.off.data(), m + n, term_alt, term_pos_off,
                                     term_n_pos, term_off, n_terms, max_ranges, &merged, &batch)))
        return rc;
    for (int32_t k = 0; k < m; ++k) a.term_len.push_back(key_off[k + 1] - key_off[k]);  // (a position is a character)
    for (int32_t i = 0; i < n; ++i) a.term_len.push_back(pat_off[i + 1] - pat_off[i]);
    return by_hist_call_run(idx, c, batch, a);
    });
}

}  // extern "C"
