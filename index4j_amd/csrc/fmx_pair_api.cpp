// fmx_pair_api.cpp — STATISTICS AND LINE COUNTS BY THE VALUES OF TWO FIELDS OF THE SAME LINE (include/fmx.h "STATISTICS BY TWO KEYS";
// fmx_hit_pairs.hpp has the definition): the join stage fmx_pairs_of_first_hits_dev over the launcher of fmx_hit_pairs.hip, and the
// host forms fmx_number_stats_by_pair_batch / fmx_number_stats_by_pair_class_batch.  A host form is fmx_by_api.cpp's with one stage
// and one read more: the merged batch terms | key patterns | number patterns, the keyed front half of the host-stage layer
// (fmx::keyed_front_stage), the join over its first hits and groups, ONE read of the c + 1 pair offsets, which sizes the rows, and
// stage c (fmx_numbers_by_key_dev, unchanged) over the joined lists with the pairs for key patterns.  n == 0 is a call of its own
// here: the pairs and their lines (count by a, b), no number stage.
#include "fmx_hit_pairs.hpp"
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

#include <cstring>

namespace {

using fmx::api_fail;
using fmx::guarded;
using fmx::hip_fail;
using fmx::zero;

// fm_pair_args_bad's rules as messages
int check_pairs(int32_t m, const int64_t *val_off, int32_t c, const int32_t *pair_a, const int32_t *pair_b, int64_t n_slots) {
    switch (fmx::fm_pair_args_bad(m, val_off, c, pair_a, pair_b, n_slots, nullptr, nullptr)) {
        case 0: return FMX_OK;
        case 1: return api_fail(FMX_E_ARG, "pairs without a key pattern (m == 0 with n_pairs > 0)");
        case 2: return api_fail(FMX_E_ARG, "a pair_a or pair_b entry is outside 0 .. m - 1");
        case 3: return api_fail(FMX_E_ARG, "val_off starts below 0, decreases or holds more than 2^31 - 1 groups of one key pattern");
        case 4: return api_fail(FMX_E_ARG, "more than 2^31 - 1 slots in one call");
        default: return api_fail(FMX_E_ARG, "the key pair | group of a | group of b would take more than 64 bits");
    }
}

// the rows of a call from the pair offsets (fm_by_rows_bad's rules with the pairs for key patterns, as messages)
int check_pair_rows(int32_t n, const int32_t *by_of, int32_t c, const int64_t *pair_off, int32_t n_permille, int64_t *row_off) {
    switch (fmx::fm_by_rows_bad(n, by_of, c, pair_off, n_permille, row_off, nullptr)) {
        case 0: return FMX_OK;
        case 1: return api_fail(FMX_E_ARG, "number patterns without a pair (n_pairs == 0 with n > 0)");
        case 2: return api_fail(FMX_E_ARG, "a by_of entry is outside 0 .. n_pairs - 1");
        case 3: return api_fail(FMX_E_ARG, "pair_off starts below 0 or decreases");
        case 4: return api_fail(FMX_E_ARG, "more than 2^27 rows in one call (the pairs of by_of[i], over the number patterns)");
        default: return api_fail(FMX_E_ARG, "more than 2^27 percentiles in one call (rows * n_permille)");
    }
}

// ---- the host form --------------------------------------------------------------------------------------------------------------------
// the regions of the ONE allocation of the answer
enum { kLines, kTextOff, kChars, kCount, kSumLo, kSumHi, kMin, kMax, kPct, kPairA, kPairB, kPairLines };

struct PairArgs : fmx::KeyedArgs {
    int32_t c = 0;
    const int32_t *pair_a = nullptr, *pair_b = nullptr;
    std::vector<int64_t> pair_off, row_off;  // c + 1, n + 1
};

// the keyed front half, the join, the groups' lines and text, the pairs, stage c over the joined lists
int pair_stage(const fmx::HitsBetween &h, void *arg) {
    PairArgs &a = *static_cast<PairArgs *>(arg);
    const hipStream_t st = static_cast<hipStream_t>(h.stream);
    const int32_t m = a.m, n = a.n, c = a.c;
    fmx::KeyedFront f{};
    bool done = false;
    int rc;
    if ((rc = fmx::keyed_front_stage(h, a, "numbers by pair", &f, &done)) || done) return rc;
    auto block = [&](size_t bytes, auto **out) -> int { return h.block(h.call, bytes + 8, reinterpret_cast<void **>(out)); };
    // the join: the kept hits of the a-sides bound their first hits (the host has them without a read)
    int64_t n_slots = 0;
    for (int32_t j = 0; j < c; ++j) n_slots += a.kept_off[(size_t)a.pair_a[j] + 1] - a.kept_off[(size_t)a.pair_a[j]];
    if ((rc = check_pairs(m, a.val_off.data(), c, a.pair_a, a.pair_b, n_slots))) return rc;
    int64_t *d_pair_off = nullptr, *d_joined_off = nullptr;
    int32_t *d_group_a = nullptr, *d_group_b = nullptr, *d_pair_lines = nullptr, *d_joined_lines = nullptr, *d_joined_group = nullptr;
    if (c > 0 && n_slots > 0) {
        void *ws_j = nullptr;
        const size_t S = (size_t)n_slots, j_bytes = fmx::pairs_of_first_hits_scratch_bytes(m, c, n_slots);
        if ((rc = block(((size_t)c + 1) * 8, &d_pair_off)) || (rc = block(((size_t)c + 1) * 8, &d_joined_off)) || (rc = block(S * 4, &d_group_a)) ||
            (rc = block(S * 4, &d_group_b)) || (rc = block(S * 4, &d_pair_lines)) || (rc = block(S * 4, &d_joined_lines)) ||
            (rc = block(S * 4, &d_joined_group)) || (rc = block(j_bytes, &ws_j)))
            return rc;
        const int e = fmx::launch_pairs_of_first_hits(h.view->n_cu, m, a.val_off.data(), c, a.pair_a, a.pair_b, f.first_off, f.first_lines, f.group, n_slots,
                                                      d_pair_off, d_group_a, d_group_b, d_pair_lines, d_joined_off, d_joined_lines, d_joined_group, ws_j,
                                                      j_bytes, st);
        if (e) return hip_fail("pairs of first hits", e);
        // ONE read: the c + 1 pair offsets size the rows
        FMX_HIP_TRY(hipMemcpyAsync(a.pair_off.data(), d_pair_off, ((size_t)c + 1) * 8, hipMemcpyDeviceToHost, st));
        FMX_HIP_TRY(hipStreamSynchronize(st));
    }
    const size_t pairs = (size_t)a.pair_off[(size_t)c];
    if (pairs == 0)  // (no line has a pair key: every kept number hit is no_key, no row)
        fmx::kept_of(a.kept_off.data() + m, n, a.no_key.data());
    else if ((rc = check_pair_rows(n, a.by_of, c, a.pair_off.data(), a.P, a.row_off.data())))
        return rc;
    const size_t G = (size_t)a.val_off[(size_t)m], units = (size_t)a.val_off[(size_t)m + 1], R = (size_t)a.row_off[(size_t)n], P = (size_t)a.P;
    if (!a.result.alloc({G * 4, (G + 1) * 8, units * 2 + 2, R * 4, R * 8, R * 8, R * 8, R * 8, R * P * 8, pairs * 4, pairs * 4, pairs * 4}))
        return api_fail(FMX_E_NOMEM, "out of host memory for " + std::to_string(G) + " groups and " + std::to_string(pairs) + " pairs");
    if (units > 0) {
        uint16_t *d_chars = nullptr;
        if ((rc = block(units * 2, &d_chars))) return rc;
        const int e = fmx::launch_values_fill(h.view->n_cu, (int64_t)G, f.text_off, d_chars, f.ws_b, st);
        if (e) return hip_fail("k_val_fill launch", e);
        FMX_HIP_TRY(hipMemcpyAsync(a.result.region<uint16_t>(kChars), d_chars, units * 2, hipMemcpyDeviceToHost, st));
    }
    FMX_HIP_TRY(hipMemcpyAsync(a.result.region<int32_t>(kLines), f.lines, G * 4, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipMemcpyAsync(a.result.region<int64_t>(kTextOff), f.text_off, (G + 1) * 8, hipMemcpyDeviceToHost, st));
    if (pairs == 0) return FMX_OK;
    FMX_HIP_TRY(hipMemcpyAsync(a.result.region<int32_t>(kPairA), d_group_a, pairs * 4, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipMemcpyAsync(a.result.region<int32_t>(kPairB), d_group_b, pairs * 4, hipMemcpyDeviceToHost, st));
    FMX_HIP_TRY(hipMemcpyAsync(a.result.region<int32_t>(kPairLines), d_pair_lines, pairs * 4, hipMemcpyDeviceToHost, st));
    if (n == 0 || f.N == 0) return FMX_OK;  // (the pivot alone, or no number hit is kept: zero rows — the allocation is zeroed)
    // stage c over the joined lists: the pairs are its key patterns, pair_off its group offsets
    fmx::StatRows d;
    void *ws_c = nullptr;
    int64_t *d_row_off = nullptr;
    const size_t c_bytes = fmx::numbers_by_key_scratch_bytes(n, f.N, a.P);
    if ((rc = fmx::stat_rows_blocks(h, nullptr, R, P, n, &d)) || (rc = block(((size_t)n + 1) * 8, &d_row_off)) || (rc = block(c_bytes, &ws_c)) ||
        (rc = fmx_numbers_by_key_dev(h.idx, n, a.term_len.data() + m, a.by_of, c, a.pair_off.data(), f.num_off, f.num_locs, f.N, d_joined_off,
                                     d_joined_lines, d_joined_group, a.frac_digits, a.permille, a.P, d_row_off, d.count, d.sum_lo, d.sum_hi, d.min, d.max,
                                     d.pct, d.no_key, d.not_number, d.overflow, h.status ? h.status + m : nullptr, ws_c, c_bytes, st)))
        return rc;
    return fmx::stat_rows_down(fmx::keyed_host_rows(a, kCount), d, R, P, n, st);
}

// what the two host forms take besides their patterns, and what they hand back
struct PairCall : fmx::KeyedCall {
    int32_t n_pairs;
    const int32_t *pair_a, *pair_b;
    int32_t line_lo, line_hi;
    int64_t *val_off;
    int32_t **lines;
    int64_t *pair_off;
    int32_t **pair_group_a, **pair_group_b, **pair_lines;
    int64_t *row_off;
};

void null_results(const PairCall &c) {
    for (int32_t **p : {c.lines, c.pair_group_a, c.pair_group_b, c.pair_lines})
        if (p) *p = nullptr;
    fmx::keyed_null_results(c);
}
bool results_missing(const PairCall &c) {
    return !c.val_off || !c.row_off || !c.pair_off || !c.lines || !c.pair_group_a || !c.pair_group_b || !c.pair_lines || fmx::keyed_results_missing(c);
}

// the checks of the HOST arrays both forms share (behind their own batches'), the handle's views, *a from c; *done: a call without
// a key pattern (and so without a pair and a number pattern) is answered, nothing is searched
int pair_call_args(const fmx_index *idx, const PairCall &c, PairArgs *a, bool *done) {
    int rc;
    if ((rc = fmx::check_values_shape(c.stop, c.n_stop, c.max_len)) || (rc = fmx::check_numbers_shape(c.frac_digits, c.permille, c.n_permille)) ||
        (rc = check_pairs(c.m, nullptr, c.n_pairs, c.pair_a, c.pair_b, 0)) ||
        (rc = check_pair_rows(c.n, c.by_of, c.n_pairs, nullptr, c.n_permille, nullptr)) ||
        (rc = fmx::check_query_arrays(c.n_terms, c.q, c.query_off, c.term_kind)) || (rc = fmx::check_where_of(c.m, c.key_where_of, c.q)) ||
        (rc = fmx::check_where_of(c.n, c.where_of, c.q)))
        return rc;
    if (c.line_lo < 0 || c.line_hi < c.line_lo) return api_fail(FMX_E_ARG, "the window of lines is not 0 <= line_lo <= line_hi");
    if ((rc = fmx::keyed_call_views(idx, &a->text))) return rc;
    zero(c.val_off, (size_t)c.m + 1);
    zero(c.pair_off, (size_t)c.n_pairs + 1);
    zero(c.row_off, (size_t)c.n + 1);
    if (c.m == 0) {
        zero(c.term_status, (size_t)c.n_terms);
        *done = true;
        return FMX_OK;
    }
    fmx::keyed_args_fill(c, c.line_lo, c.line_hi, a);
    a->c = c.n_pairs;
    a->pair_a = c.pair_a;
    a->pair_b = c.pair_b;
    a->pair_off.assign((size_t)c.n_pairs + 1, 0);
    a->row_off.assign((size_t)c.n + 1, 0);
    return FMX_OK;
}

// the call over the merged batch terms | key patterns | number patterns, and the answer into the caller's arrays
int pair_call_run(const fmx_index *idx, const PairCall &c, const fmx::ValuesBatch &batch, PairArgs &a) {
    if (const int rc = fmx::keyed_call_run(idx, c, batch, pair_stage, &a, a)) return rc;
    memcpy(c.val_off, a.val_off.data(), ((size_t)c.m + 1) * 8);
    memcpy(c.pair_off, a.pair_off.data(), ((size_t)c.n_pairs + 1) * 8);
    memcpy(c.row_off, a.row_off.data(), ((size_t)c.n + 1) * 8);
    if (a.result.p) {  // the ONE allocation: freed with fmx_free_buffer((uint8_t *)*lines)
        *c.lines = a.result.region<int32_t>(kLines);
        *c.pair_group_a = a.result.region<int32_t>(kPairA);
        *c.pair_group_b = a.result.region<int32_t>(kPairB);
        *c.pair_lines = a.result.region<int32_t>(kPairLines);
        fmx::keyed_hand_over(c, a, kTextOff);
    }
    return FMX_OK;
}

}  // namespace

extern "C" {

size_t fmx_pairs_of_first_hits_scratch_bytes(int32_t m, int32_t n_pairs, int64_t n_slots) {
    return fmx::pairs_of_first_hits_scratch_bytes(m, n_pairs, n_slots);
}

int fmx_pairs_of_first_hits_dev(const fmx_index *idx, int32_t m, const int64_t *val_off, int32_t n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                                const int64_t *d_first_off, const int32_t *d_first_lines, const int32_t *d_group_of_first, int64_t n_slots,
                                int64_t *d_pair_off, int32_t *d_pair_group_a, int32_t *d_pair_group_b, int32_t *d_pair_lines, int64_t *d_joined_off,
                                int32_t *d_joined_lines, int32_t *d_joined_group, void *d_ws, size_t ws_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || m < 0 || n_pairs < 0 || (n_pairs > 0 && (!val_off || !pair_a || !pair_b || !d_first_off || !d_pair_off || !d_joined_off)) ||
        (n_pairs > 0 && n_slots > 0 &&
         (!d_first_lines || !d_group_of_first || !d_pair_group_a || !d_pair_group_b || !d_pair_lines || !d_joined_lines || !d_joined_group)))
        return api_fail(FMX_E_ARG, "bad arguments");
    if (const int rc = check_pairs(m, val_off, n_pairs, pair_a, pair_b, n_slots)) return rc;
    if (n_pairs > 0 && n_slots > 0 && (!d_ws || ws_bytes < fmx::pairs_of_first_hits_scratch_bytes(m, n_pairs, n_slots)))
        return api_fail(FMX_E_ARG, "the workspace is smaller than fmx_pairs_of_first_hits_scratch_bytes");
    fmx::LineView view;
    if (const int rc = fmx::line_view(idx, &view)) return rc;
    if (n_pairs == 0) return FMX_OK;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_slots == 0) {
        FMX_HIP_TRY(hipMemsetAsync(d_pair_off, 0, ((size_t)n_pairs + 1) * 8, st));
        FMX_HIP_TRY(hipMemsetAsync(d_joined_off, 0, ((size_t)n_pairs + 1) * 8, st));
        return FMX_OK;
    }
    const int e = fmx::launch_pairs_of_first_hits(view.n_cu, m, val_off, n_pairs, pair_a, pair_b, d_first_off, d_first_lines, d_group_of_first, n_slots,
                                                  d_pair_off, d_pair_group_a, d_pair_group_b, d_pair_lines, d_joined_off, d_joined_lines, d_joined_group,
                                                  d_ws, ws_bytes, st);
    return e ? hip_fail("pairs of first hits", e) : FMX_OK;
    });
}

int fmx_number_stats_by_pair_batch(const fmx_index *idx, const uint16_t *key_pat, const int32_t *key_off, int32_t m, const uint16_t *pat,
                                   const int32_t *pat_off, int32_t n, const int32_t *by_of, int32_t n_pairs, const int32_t *pair_a,
                                   const int32_t *pair_b, const uint16_t *term_pat, const int32_t *term_off, int32_t n_terms, const int32_t *query_off,
                                   const uint8_t *term_kind, int32_t q, const int32_t *key_where_of, const int32_t *where_of, int32_t line_lo,
                                   int32_t line_hi, const uint16_t *stop, int32_t n_stop, int32_t max_len, int32_t frac_digits, const int32_t *permille,
                                   int32_t n_permille, int64_t *val_off, int32_t **lines, int64_t **text_off, uint16_t **chars, int64_t *pair_off,
                                   int32_t **pair_group_a, int32_t **pair_group_b, int32_t **pair_lines, int64_t *row_off, int32_t **count,
                                   uint64_t **sum_lo, uint64_t **sum_hi, int64_t **min, int64_t **max, int64_t **pct, int32_t *no_key,
                                   int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept, int32_t *status,
                                   int32_t *key_occurrences, int32_t *key_kept, int32_t *key_status, int32_t *term_status) {
    return guarded([&]() -> int {
    const PairCall c{{m, n, by_of, n_terms, query_off, term_kind, q, key_where_of, where_of, stop, n_stop, max_len, frac_digits, permille, n_permille,
                      text_off, chars, count, sum_lo, sum_hi, min, max, pct, no_key, not_number, overflow, occurrences, kept, status, key_occurrences,
                      key_kept, key_status, term_status},
                     n_pairs, pair_a, pair_b, line_lo, line_hi, val_off, lines, pair_off, pair_group_a, pair_group_b, pair_lines, row_off};
    null_results(c);
    if (!idx || m < 0 || n < 0 || n_pairs < 0 || n_terms < 0 || q < 0 || results_missing(c) || (m > 0 && (!key_off || !key_where_of)) ||
        (n > 0 && (!pat_off || !where_of || !by_of)) || (n_pairs > 0 && (!pair_a || !pair_b)) || (n_terms > 0 && !term_off))
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    if ((rc = fmx::check_literal_batches(pat_off, n, term_off, n_terms)) || (m > 0 && (rc = fmx::check_offsets(key_off, m, "key pattern")))) return rc;
    PairArgs a;
    bool done = false;
    if ((rc = pair_call_args(idx, c, &a, &done)) || done) return rc;
    const int32_t no_off[1] = {0};  // (a call without a number pattern may leave their offsets out)
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_keyed_literal_batch(key_pat, key_off, m, pat, n > 0 ? pat_off : no_off, n, term_pat, term_off, n_terms, &merged, &batch,
                                             &a.term_len)))
        return rc;
    return pair_call_run(idx, c, batch, a);
    });
}

int fmx_number_stats_by_pair_class_batch(const fmx_index *idx, const uint16_t *key_alt, const int32_t *key_pos_off, int32_t key_n_pos,
                                         const int32_t *key_off, int32_t m, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                         const int32_t *pat_off, int32_t n, const int32_t *by_of, int32_t n_pairs, const int32_t *pair_a,
                                         const int32_t *pair_b, const uint16_t *term_alt, const int32_t *term_pos_off, int32_t term_n_pos,
                                         const int32_t *term_off, int32_t n_terms, int32_t max_ranges, const int32_t *query_off,
                                         const uint8_t *term_kind, int32_t q, const int32_t *key_where_of, const int32_t *where_of, int32_t line_lo,
                                         int32_t line_hi, const uint16_t *stop, int32_t n_stop, int32_t max_len, int32_t frac_digits,
                                         const int32_t *permille, int32_t n_permille, int64_t *val_off, int32_t **lines, int64_t **text_off,
                                         uint16_t **chars, int64_t *pair_off, int32_t **pair_group_a, int32_t **pair_group_b, int32_t **pair_lines,
                                         int64_t *row_off, int32_t **count, uint64_t **sum_lo, uint64_t **sum_hi, int64_t **min, int64_t **max,
                                         int64_t **pct, int32_t *no_key, int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept,
                                         int32_t *status, int32_t *key_occurrences, int32_t *key_kept, int32_t *key_status, int32_t *term_status) {
    return guarded([&]() -> int {
    const PairCall c{{m, n, by_of, n_terms, query_off, term_kind, q, key_where_of, where_of, stop, n_stop, max_len, frac_digits, permille, n_permille,
                      text_off, chars, count, sum_lo, sum_hi, min, max, pct, no_key, not_number, overflow, occurrences, kept, status, key_occurrences,
                      key_kept, key_status, term_status},
                     n_pairs, pair_a, pair_b, line_lo, line_hi, val_off, lines, pair_off, pair_group_a, pair_group_b, pair_lines, row_off};
    null_results(c);
    if (!idx || m < 0 || n < 0 || n_pairs < 0 || n_pos < 0 || key_n_pos < 0 || n_terms < 0 || term_n_pos < 0 || q < 0 || results_missing(c) ||
        !pos_off || !pat_off || !key_pos_off || !key_off || (m > 0 && !key_where_of) || (n > 0 && (!where_of || !by_of)) ||
        (n_pairs > 0 && (!pair_a || !pair_b)) || (n_terms > 0 && (!term_pos_off || !term_off)) || max_ranges < 1 || max_ranges > FMX_CLASS_RANGES_MAX)
        return api_fail(FMX_E_ARG, "bad arguments");
    int rc;
    // the key patterns are judged as the number patterns are: the terms' slot of the check takes them
    if ((rc = fmx::check_class_batches(alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off, term_n_pos, term_off, n_terms)) ||
        (rc = fmx::check_class_batches(key_alt, key_pos_off, key_n_pos, key_off, m, nullptr, nullptr, 0, nullptr, 0)))
        return rc;
    PairArgs a;
    bool done = false;
    if ((rc = pair_call_args(idx, c, &a, &done)) || done) return rc;
    fmx::MergedBatch merged;
    fmx::ValuesBatch batch;
    if ((rc = fmx::merge_keyed_class_batch(key_alt, key_pos_off, key_n_pos, key_off, m, alt, pos_off, n_pos, pat_off, n, term_alt, term_pos_off,
                                           term_n_pos, term_off, n_terms, max_ranges, &merged, &batch, &a.term_len)))
        return rc;
    return pair_call_run(idx, c, batch, a);
    });
}

}  // extern "C"
