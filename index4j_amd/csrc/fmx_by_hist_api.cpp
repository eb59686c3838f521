// fmx_by_hist_api.cpp — STATISTICS OF THE NUMBER BEHIND A PATTERN, BY THE VALUE OF A FIELD OF THE SAME LINE, PER BUCKET OF LINES
// (include/fmx.h "STATISTICS BY KEY PER BUCKET"; fmx_by_hist.hpp has the definition): the device stage
// fmx_numbers_by_key_buckets_dev over fmx_by_hist.hip's launchers with the packed extract between them, and the host forms
// fmx_number_stats_by_histogram_batch / fmx_number_stats_by_histogram_class_batch.  Of a handle this file sees what fmx::line_view
// and fmx::text_view hand out; a host form runs the packed sequence of fmx_api.cpp up to the stage of this file
// (fmx::hits_stage_call) over ONE merged batch terms | key patterns | number patterns (fmx::merge_keyed_*_batch), then the keyed
// front half of the host-stage layer with the edges' span as the filter's window (fmx::keyed_front_stage: the filter, stage a,
// stage b, ONE read of the group offsets and the units of the groups' text), which sizes the key rows and the cells, the new stage
// over the numbers' part, the fill of the groups' text and the gather of the key rows' text.  Its waits are
// fmx_number_stats_by_batch's, plus the 8-byte read of the rows' text length.  The checks, the statistics arrays, the packed result
// and the call plumbing are that layer's too (fmx_host_stage.hpp); this file keeps the cut into key rows and cells and the new stage.
#include "fmx_by_hist.hpp"
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

#include <cstring>

namespace {

using fmx::api_fail;
using fmx::guarded;
using fmx::hip_fail;
using fmx::no_line_table;
using fmx::zero;

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

using Cells = fmx::StatRows;
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
// the regions of the ONE allocation of the answer
enum { kRowLines, kRowGroup, kTextOff, kChars, kCount, kSumLo, kSumHi, kMin, kMax, kPct };

struct ByHistArgs : fmx::KeyedArgs {
    Cut cut{};
    int32_t B = 1;
    std::vector<int64_t> key_row_off, cell_off;  // m + 1, n + 1
};

// the keyed front half, the new stage over the numbers' part, the text of the key rows
int by_hist_stage(const fmx::HitsBetween &h, void *arg) {
    ByHistArgs &a = *static_cast<ByHistArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const int32_t m = a.m, n = a.n;
    fmx::KeyedFront f{};
    bool done = false;
    int rc;
    if ((rc = fmx::keyed_front_stage(h, a, "numbers by key per bucket", &f, &done)) || done) return rc;
    // (the group offsets size the key rows and the cells)
    if ((rc = check_groups(n, a.by_of, m, a.val_off.data(), a.cut.top, a.B, a.P, a.key_row_off.data(), a.cell_off.data()))) return rc;
    const size_t G = (size_t)a.val_off[(size_t)m], R = (size_t)a.key_row_off[(size_t)m], cells = (size_t)a.cell_off[(size_t)n], P = (size_t)a.P;
    const int64_t units = a.val_off[(size_t)m + 1];
    auto block = [&](size_t bytes, auto **out) -> int { return h.block(h.call, bytes + 8, reinterpret_cast<void **>(out)); };
    // the ranks, the key rows, the codes and the cells over the numbers' part
    Cells d;
    KeyRows kr{};
    void *ws_c = nullptr;
    const size_t c_bytes = fmx::numbers_by_key_buckets_scratch_bytes(n, m, (int64_t)G, f.N, a.cut.n_edges, a.P);
    if ((rc = block(R * 4, &kr.group)) || (rc = block(R * 4, &kr.lines)) || (rc = fmx::stat_rows_blocks(h, nullptr, cells, P, n, &d)) ||
        (rc = block(c_bytes, &ws_c)) ||
        (rc = cells_impl(h.idx, *h.view, a.text, n, a.term_len.data() + m, a.by_of, m, a.val_off.data(), a.cut, f.num_off, f.num_locs, f.N,
                         FirstHits{f.first_off, f.first_lines, f.group, f.lines}, a.frac_digits, a.permille, a.P, kr, d,
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
    if (units > 0 && (rc = fmx_values_fill_dev(h.idx, (int64_t)G, f.text_off, d_chars, f.ws_b, f.b_bytes, st))) return rc;
    const int e = fmx::launch_values_gather_rows(h.view->n_cu, m, a.val_off.data(), a.cut.top, units, kr.group, f.text_off, d_chars, d_row_text_off,
                                                 d_row_chars, ws_g, g_bytes, st);
    if (e) return hip_fail("text of the key rows", e);
    int64_t row_units = 0;  // ONE 8-byte read: the packed length of the key rows' text sizes the allocation
    FMX_HIP_TRY(hipMemcpyAsync(&row_units, d_row_text_off + R, 8, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipStreamSynchronize(st));
    if (!a.result.alloc({R * 4, R * 4, (R + 1) * 8, (size_t)row_units * 2 + 2, cells * 4, cells * 8, cells * 8, cells * 8, cells * 8, cells * P * 8}))
        return api_fail(FMX_E_NOMEM, "out of host memory for " + std::to_string(cells) + " cells");
    auto down = [&](size_t region, const void *dev, size_t bytes) -> hipError_t {
        return bytes > 0 ? hipMemcpyAsync(a.result.region<uint8_t>(region), dev, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    FMX_HIP_TRY(down(kRowLines, kr.lines, R * 4));
    FMX_HIP_TRY(down(kRowGroup, kr.group, R * 4));
    FMX_HIP_TRY(down(kTextOff, d_row_text_off, (R + 1) * 8));
    FMX_HIP_TRY(down(kChars, d_row_chars, (size_t)row_units * 2));
    if (f.N == 0) return FMX_OK;  // (no number hit is kept: the key rows with zero cells — the allocation is zeroed)
    return fmx::stat_rows_down(fmx::keyed_host_rows(a, kCount), d, cells, P, n, st);
}

// what the two host forms take besides their patterns, and what they hand back
struct ByHistCall : fmx::KeyedCall {
    const int32_t *edges;
    int32_t n_edges, top;
    int32_t *n_groups;
    int64_t *key_row_off;
    int32_t **key_row_lines, **key_row_group;
    int64_t *cell_off;
};

bool results_missing(const ByHistCall &c) {
    return !c.key_row_off || !c.cell_off || !c.key_row_lines || !c.key_row_group || fmx::keyed_results_missing(c);
}

// the checks of the HOST arrays both forms share (behind their own batches'), the handle's views and the empty call; *done: answered
int by_hist_call_args(const fmx_index *idx, const ByHistCall &c, ByHistArgs *a, bool *done) {
    int rc;
    if ((rc = fmx::keyed_call_checks(c)) || (rc = check_cut(c.n, c.edges, c.n_edges, c.top, c.n_permille, &a->B)) ||
        (rc = fmx::keyed_call_views(idx, &a->text)))
        return rc;
    *c.key_row_lines = *c.key_row_group = nullptr;
    fmx::keyed_null_results(c);
    zero(c.n_groups, (size_t)c.m);
    zero(c.key_row_off, (size_t)c.m + 1);
    zero(c.cell_off, (size_t)c.n + 1);
    // the window of the filter is the span of the edges: every kept hit has a bucket
    *done = !fmx::keyed_call_fill(c, c.edges ? c.edges[0] : 0, c.edges ? c.edges[c.n_edges - 1] : INT32_MAX, a);
    a->cut = Cut{c.edges, c.edges ? c.n_edges : 0, c.top};
    a->key_row_off.assign((size_t)c.m + 1, 0);
    a->cell_off.assign((size_t)c.n + 1, 0);
    return FMX_OK;
}

// the call over the merged batch terms | key patterns | number patterns, and the answer into the caller's arrays
int by_hist_call_run(const fmx_index *idx, const ByHistCall &c, const fmx::ValuesBatch &batch, ByHistArgs &a) {
    if (const int rc = fmx::keyed_call_run(idx, c, batch, by_hist_stage, &a, a)) return rc;
    for (int32_t k = 0; k < c.m && c.n_groups; ++k) c.n_groups[k] = (int32_t)(a.val_off[(size_t)k + 1] - a.val_off[(size_t)k]);
    if (a.result.p) {  // the ONE allocation: freed with fmx_free_buffer((uint8_t *)*key_row_lines)
        memcpy(c.key_row_off, a.key_row_off.data(), ((size_t)c.m + 1) * 8);
        memcpy(c.cell_off, a.cell_off.data(), ((size_t)c.n + 1) * 8);
        *c.key_row_lines = a.result.region<int32_t>(kRowLines);
        *c.key_row_group = a.result.region<int32_t>(kRowGroup);
        fmx::keyed_hand_over(c, a, kTextOff);
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
    if ((rc = fmx::check_numbers_shape(frac_digits, permille, n_permille)) || (rc = fmx::check_term_len(n, term_len)) ||
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
    if ((rc = fmx::stat_rows_zero(c, cells, P, n, st))) return rc;
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
    const ByHistCall c{{m, n, by_of, n_terms, query_off, term_kind, q, key_where_of, where_of, stop, n_stop, max_len, frac_digits, permille, n_permille,
                        text_off, chars, count, sum_lo, sum_hi, min, max, pct, no_key, not_number, overflow, occurrences, kept, status,
                        key_occurrences, key_kept, key_status, term_status},
                       edges, n_edges, top, n_groups, key_row_off, key_row_lines, key_row_group, cell_off};
    if (!idx || m < 0 || n < 0 || n_terms < 0 || q < 0 || n_edges < 0 || results_missing(c) || (m > 0 && (!key_off || !key_where_of)) ||
        (n > 0 && (!pat_off || !where_of || !by_of)) || (n_terms > 0 && !term_off))
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_literal_batches(pat_off, n, term_off, n_terms)) || (m > 0 && (rc = fmx::check_offsets(key_off, m, "key pattern")))) return rc;
    ByHistArgs a;
    bool done = false;
    if ((rc = by_hist_call_args(idx, c, &a, &done)) || done) return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_keyed_literal_batch(key_pat, key_off, m, pat, pat_off, n, term_pat, term_off, n_terms, &merged, &batch, &a.term_len))) return rc;
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
    const ByHistCall c{{m, n, by_of, n_terms, query_off, term_kind, q, key_where_of, where_of, stop, n_stop, max_len, frac_digits, permille, n_permille,
                        text_off, chars, count, sum_lo, sum_hi, min, max, pct, no_key, not_number, overflow, occurrences, kept, status,
                        key_occurrences, key_kept, key_status, term_status},
                       edges, n_edges, top, n_groups, key_row_off, key_row_lines, key_row_group, cell_off};
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
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_keyed_class_batch(key_alt, key_pos_off, key_n_pos, key_off, m, alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off,
                                           term_n_pos, term_off, n_terms, max_ranges, &merged, &batch, &a.term_len)))
        return rc;
    return by_hist_call_run(idx, c, batch, a);
    });
}

}  // extern "C"
