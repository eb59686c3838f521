// by_hist_hostsim.cpp — TEST-ONLY host build of the device code of "statistics of the number behind a pattern, by the value of a
// field of the same line, per bucket of lines" (fmx_numbers_by_key_buckets_dev): index4j_amd/csrc/fmx_by_hist.hpp's fm_bh_code,
// fm_bh_args_bad and fm_bh_shape_bad — with fmx_value_hist.hpp's rank functions, fmx_hit_by.hpp's fm_by_find and fm_by_row_pattern,
// fmx_line_hist.hpp's buckets and fmx_hit_numbers.hpp's parser, segments and sums — driven by a mirror of the stage with the lanes
// run one after the other, the tile loop included: std::stable_sort for rocPRIM's sorts, running sums for its scans.  Stages a and b
// (the first lines of every key pattern, the group of every first hit, the groups' offsets and lines) are handed in: their mirror is
// tests/by_key_hostsim.cpp.  The windows' text is cut from the TEXT the caller hands in.  Every cell is checked here against values
// kept hit by hit in 128-bit arithmetic, by the definition and without a sort; exit status 6 where one differs.  g++ compiles the
// headers' functions as plain C++, so the CPU suite checks the source of those FUNCTIONS
// (tests/test_number_stats_by_histogram_cpu.py); the kernels' own route runs in tests/test_gpu_number_stats_by_histogram.py only.
// Never part of libfmx.so.
//
// A stand-alone program:
//   by_hist_hostsim self          the per-item functions and the host checks at their edges; exit status 4 where one fails
//   by_hist_hostsim run IN OUT    IN   int64 {m, n, n_hits, count, max_fences, n_edges, top, P, frac_digits, text_len, F, G}, int32 T[count],
//                                      int32 term_len[n], int32 by_of[n], int64 hit_off[n + 1] (hit_off[0] may be non-zero),
//                                      int32 locs[n_hits], int32 edges[n_edges], int32 permille[P], int64 first_off[m + 1],
//                                      int32 first_lines[F], int32 group_of_first[F], int64 val_off[m + 1], int32 group_lines[G],
//                                      uint16 text[text_len]
//                                 OUT  int64 key_row_off[m + 1], int32 key_row_group[R], int32 key_row_lines[R], int64 cell_off[n + 1],
//                                      int32 count[cells], uint64 sum_lo[cells], uint64 sum_hi[cells], int64 min[cells], int64 max[cells],
//                                      int64 pct[cells * P], int32 no_key[n], int32 not_number[n], int32 overflow[n]
#include "../index4j_amd/csrc/fmx_by_hist.hpp"
#include "../index4j_amd/csrc/fmx_hit_filter.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

using namespace fmx;

namespace {

template <class T>
bool get(FILE *f, std::vector<T> &v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}
template <class T>
void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int g_failed = 0;
#define EXPECT(cond)                                           \
    do {                                                       \
        if (!(cond)) {                                         \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
            g_failed = 1;                                      \
        }                                                      \
    } while (0)

void self_checks() {
    {  // the code: rank | bucket, the pattern's own "other", and what has no cell
        const int32_t rank_of_group[] = {9, 9, 1, 0, 3, 2, 3};  // (the groups of a key pattern at g0 = 2: ranks 1, 0, 3, 2, 3 with top = 3)
        const int32_t group_of_first[] = {0, 1, 2, 3, 4, -1, 5};
        const int32_t top = 3, B = 4, C = 16;
        EXPECT(fm_bh_code(rank_of_group, group_of_first, 0, 2, 5, top, 0, B, C) == 1 * B + 0);
        EXPECT(fm_bh_code(rank_of_group, group_of_first, 1, 2, 5, top, 3, B, C) == 0 * B + 3);
        EXPECT(fm_bh_code(rank_of_group, group_of_first, 2, 2, 5, top, 2, B, C) == 3 * B + 2);   // rank top = "other"
        EXPECT(fm_bh_code(rank_of_group, group_of_first, 3, 2, 5, top, 1, B, C) == 2 * B + 1);
        EXPECT(fm_bh_code(rank_of_group, group_of_first, -1, 2, 5, top, 1, B, C) == C);          // no key
        EXPECT(fm_bh_code(rank_of_group, group_of_first, 0, 2, 5, top, B, B, C) == C);           // no bucket
        EXPECT(fm_bh_code(rank_of_group, group_of_first, 5, 2, 5, top, 1, B, C) == C);           // a first hit without a group
        EXPECT(fm_bh_code(rank_of_group, group_of_first, 6, 2, 5, top, 1, B, C) == C);           // a group outside the pattern's
        // R_k folds the pattern's own other: two groups, top = 3 -> rows = 2; a rank of 3 (never stored for them) would fold to 2
        const int32_t two[] = {1, 0}, folded[] = {3, 0}, first2[] = {0, 1};
        EXPECT(fm_bh_code(two, first2, 0, 0, 2, top, 0, B, C) == 1 * B && fm_bh_code(folded, first2, 0, 0, 2, top, 1, B, C) == 2 * B + 1);
        // one bucket (no edges)
        EXPECT(fm_bh_code(rank_of_group, group_of_first, 2, 2, 5, top, 0, 1, 4) == 3 && fm_bh_code(rank_of_group, group_of_first, 1, 2, 5, top, 0, 1, 4) == 0);
    }
    {  // the shape from the arguments alone
        EXPECT(fm_bh_args_bad(1, 0, 1, 0) == 1 && fm_bh_args_bad(1, 65537, 1, 0) == 1 && fm_bh_args_bad(1, 1, 1, 0) == 0);
        EXPECT(fm_bh_args_bad(1, 65536, 1, 0) == 0 && fm_bh_args_bad(0, 65536, 1 << 30, 16) == 0);
        EXPECT(fm_bh_args_bad(1, 1, (int32_t)(kHistCellsMax / 2), 0) == 0 && fm_bh_args_bad(1, 1, (int32_t)(kHistCellsMax / 2) + 1, 0) == 2);
        EXPECT(fm_bh_args_bad(1, 1, (int32_t)(kHistCellsMax / 2), 1) == 0 && fm_bh_args_bad(1, 1, (int32_t)(kHistCellsMax / 2), 2) == 3);
        EXPECT(fm_bh_args_bad(0x7fffffff, 65536, 0x7fffffff, 16) == 2);  // (no overflow of the product)
    }
    {  // ... and with the groups: the key rows, the cells, the code space
        const int32_t by_of[] = {1, 0, 1}, bad[] = {0, 2, 0}, neg[] = {-1, 0, 0};
        const int64_t val_off[] = {0, 2, 9}, down[] = {0, 3, 2}, from1[] = {1, 2, 9}, none[] = {0, 0, 0};
        int64_t key_row_off[3], cell_off[4];
        int32_t C = 0;
        EXPECT(fm_bh_shape_bad(3, by_of, 2, val_off, 3, 4, 2, key_row_off, cell_off, &C) == 0);
        EXPECT(key_row_off[0] == 0 && key_row_off[1] == 2 && key_row_off[2] == 5);
        EXPECT(cell_off[0] == 0 && cell_off[1] == 16 && cell_off[2] == 28 && cell_off[3] == 44 && C == 16);
        EXPECT(fm_bh_shape_bad(3, by_of, 2, val_off, 100, 1, 0, key_row_off, cell_off, &C) == 0 && key_row_off[2] == 9 && cell_off[3] == 19 && C == 8);
        EXPECT(fm_bh_shape_bad(3, by_of, 2, none, 5, 3, 0, key_row_off, cell_off, &C) == 0 && key_row_off[2] == 0 && cell_off[3] == 9 && C == 3);
        EXPECT(fm_bh_shape_bad(3, by_of, 0, val_off, 3, 1, 0, nullptr, nullptr, nullptr) == 1 && fm_bh_shape_bad(3, nullptr, 2, val_off, 3, 1, 0, nullptr, nullptr, nullptr) == 1);
        EXPECT(fm_bh_shape_bad(3, bad, 2, val_off, 3, 1, 0, nullptr, nullptr, nullptr) == 2 && fm_bh_shape_bad(3, neg, 2, val_off, 3, 1, 0, nullptr, nullptr, nullptr) == 2);
        EXPECT(fm_bh_shape_bad(3, by_of, 2, down, 3, 1, 0, nullptr, nullptr, nullptr) == 3 && fm_bh_shape_bad(3, by_of, 2, from1, 3, 1, 0, nullptr, nullptr, nullptr) == 3);
        EXPECT(fm_bh_shape_bad(3, by_of, 2, nullptr, 3, 1, 0, nullptr, nullptr, nullptr) == 3);
        const int64_t many[] = {0, 1, (int64_t)1 << 31};
        EXPECT(fm_bh_shape_bad(3, by_of, 2, many, 3, 1, 0, nullptr, nullptr, nullptr) == 6);
        EXPECT(fm_bh_shape_bad(3, by_of, 2, val_off, 0, 1, 0, nullptr, nullptr, nullptr) == 7 && fm_bh_shape_bad(3, by_of, 2, val_off, 3, 0, 0, nullptr, nullptr, nullptr) == 7);
        EXPECT(fm_bh_shape_bad(0, nullptr, 0, nullptr, 1, 1, 0, nullptr, cell_off, &C) == 0 && cell_off[0] == 0 && C == 1);
    }
}

struct In {
    int64_t m, n, n_hits, count, max_fences, n_edges, top, P, frac_digits, text_len, F, G;
    std::vector<int32_t> T, term_len, by_of, locs, edges, permille, first_lines, group_of_first, group_lines;
    std::vector<int64_t> hit_off, first_off, val_off;
    std::vector<uint16_t> text;
};

typedef unsigned __int128 u128;

int run(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) return 2;
    In a;
    std::vector<int64_t> head;
    if (!get(f, head, 12)) return 2;
    a.m = head[0], a.n = head[1], a.n_hits = head[2], a.count = head[3], a.max_fences = head[4], a.n_edges = head[5], a.top = head[6];
    a.P = head[7], a.frac_digits = head[8], a.text_len = head[9], a.F = head[10], a.G = head[11];
    if (!get(f, a.T, (size_t)a.count) || !get(f, a.term_len, (size_t)a.n) || !get(f, a.by_of, (size_t)a.n) || !get(f, a.hit_off, (size_t)a.n + 1) ||
        !get(f, a.locs, (size_t)a.n_hits) || !get(f, a.edges, (size_t)a.n_edges) || !get(f, a.permille, (size_t)a.P) ||
        !get(f, a.first_off, (size_t)a.m + 1) || !get(f, a.first_lines, (size_t)a.F) || !get(f, a.group_of_first, (size_t)a.F) ||
        !get(f, a.val_off, (size_t)a.m + 1) || !get(f, a.group_lines, (size_t)a.G) || !get(f, a.text, (size_t)a.text_len))
        return 2;
    fclose(f);
    const int32_t m = (int32_t)a.m, n = (int32_t)a.n, count = (int32_t)a.count, text_len = (int32_t)a.text_len, top = (int32_t)a.top;
    const int32_t P = (int32_t)a.P, n_edges = (int32_t)a.n_edges, B = n_edges > 0 ? n_edges - 1 : 1;
    const int64_t n_hits = a.n_hits, G = a.G;
    if (n_edges > 0 && fm_hist_edges_bad(a.edges.data(), n_edges)) return 5;
    std::vector<int64_t> key_row_off((size_t)m + 1, 0), cell_off((size_t)n + 1, 0);
    int32_t C = 1;
    if (fm_bh_shape_bad(n, a.by_of.data(), m, a.val_off.data(), top, B, P, key_row_off.data(), cell_off.data(), &C) || a.val_off[(size_t)m] != G) return 5;
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, (int32_t)a.max_fences, n_fences);
    std::vector<int32_t> fence((size_t)n_fences);
    for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = a.T[(size_t)((int64_t)j << shift)];

    // ---- 1. rank: k_bh_rank_keys, the stable sort, k_bh_ranks ----
    const int64_t R = key_row_off[(size_t)m];
    std::vector<uint64_t> rkey((size_t)G);
    std::vector<uint32_t> rgroup((size_t)G);
    for (int64_t g = 0; g < G; ++g) {
        const int32_t c = a.group_lines[(size_t)g];
        rkey[(size_t)g] = fm_vh_rank_key(fm_hit_pattern(a.val_off.data(), m, g), c < 0 ? 0 : c);
        rgroup[(size_t)g] = (uint32_t)g;
    }
    std::stable_sort(rgroup.begin(), rgroup.end(), [&](uint32_t x, uint32_t y) { return rkey[x] < rkey[y]; });
    std::vector<int32_t> rank_of_group((size_t)G, -1), key_row_group((size_t)R, -1), key_row_lines((size_t)R, -1);
    for (int64_t j = 0; j < G; ++j) {
        const uint64_t key = rkey[rgroup[(size_t)j]];
        const int32_t k = fm_vh_rank_key_pattern(key);
        const int64_t g = rgroup[(size_t)j], first = a.val_off[(size_t)k];
        const int32_t rank = fm_vh_rank(j, first, top);
        rank_of_group[(size_t)g] = rank;
        if (rank < top) {
            const int64_t row = key_row_off[(size_t)k] + rank;
            if (row >= key_row_off[(size_t)k + 1]) return 6;
            key_row_group[(size_t)row] = (int32_t)(g - first);
            key_row_lines[(size_t)row] = fm_vh_rank_key_count(key);
        }
    }

    // ---- 2. codes: k_bh_codes' tile loop, one lane after the other; 3. the parse ----
    const int32_t code_bits = fm_num_code_bits(C);
    const uint64_t no_hit = fm_hist_key(n, 0, code_bits);
    const int64_t *hit_off = a.hit_off.data();
    const int64_t first = fm_filter_slot(hit_off[0], n_hits), total = fm_filter_slot(hit_off[n], n_hits);
    std::vector<uint64_t> ckey((size_t)n_hits, ~(uint64_t)0), cval((size_t)n_hits, 0);
    std::vector<int32_t> bucket_of((size_t)n_hits, -1);  // (for the hit-by-hit check)
    for (int64_t tile = 0; tile < n_hits; tile += kLocateAllTile) {
        for (int32_t lane = 0; lane < kLocateAllTile; ++lane) {
            const int64_t t = tile + lane;
            if (tile >= total || tile + kLocateAllTile <= first) {
                if (t < n_hits) ckey[(size_t)t] = no_hit;
                continue;
            }
            const HitTile h = fm_hit_tile(hit_off, n, tile, total);
            if (t >= first && t <= h.tile_last) {
                const int32_t p = h.p_lo + fm_hit_pattern(hit_off + h.p_lo, h.slice_count, t);
                const int32_t loc = a.locs[(size_t)t];
                int32_t s, e;
                fm_val_window(loc, a.term_len[(size_t)p], kNumWindow, text_len, s, e);
                const int32_t k = a.by_of[(size_t)p], L = fm_line_of(a.T.data(), count, fence.data(), n_fences, shift, loc);
                const int32_t bucket = n_edges > 0 ? fm_hist_bucket(a.edges.data(), n_edges, L) : 0;
                const int64_t found = fm_by_find(a.first_lines.data(), a.first_off[(size_t)k], a.first_off[(size_t)k + 1], L), g0 = a.val_off[(size_t)k];
                const int32_t code = fm_bh_code(rank_of_group.data(), a.group_of_first.data(), found, g0, a.val_off[(size_t)k + 1] - g0, top, bucket, B, C);
                int64_t v;
                const int32_t kind = fm_num_parse(a.text.data() + s, e - s, (int32_t)a.frac_digits, v);
                ckey[(size_t)t] = fm_hist_key(p, fm_num_code(code, C, kind), code_bits);
                cval[(size_t)t] = (uint64_t)v;
                bucket_of[(size_t)t] = bucket;
            } else if (t < n_hits) {
                ckey[(size_t)t] = no_hit;
            }
        }
    }
    for (int64_t t = 0; t < n_hits; ++t)
        if (ckey[(size_t)t] == ~(uint64_t)0) return 6;  // a slot no lane stored

    // ---- the two stable sorts and the two running sums ----
    std::vector<size_t> order((size_t)n_hits);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return cval[x] < cval[y]; });
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return ckey[x] < ckey[y]; });
    std::vector<uint64_t> skey((size_t)n_hits), sval((size_t)n_hits), scan_lo((size_t)n_hits), scan_hi((size_t)n_hits);
    for (size_t i = 0; i < order.size(); ++i) {
        skey[i] = ckey[order[i]];
        sval[i] = cval[order[i]];
        scan_lo[i] = (i ? scan_lo[i - 1] : 0) + fm_num_low(sval[i]);
        scan_hi[i] = (i ? scan_hi[i - 1] : 0) + fm_num_high(sval[i]);
    }

    // ---- 4. cells and tails ----
    const int64_t cells = cell_off[(size_t)n];
    std::vector<int32_t> cnt((size_t)cells), no_key((size_t)n), nn((size_t)n), ov((size_t)n);
    std::vector<uint64_t> sum_lo((size_t)cells), sum_hi((size_t)cells);
    std::vector<int64_t> vmin((size_t)cells), vmax((size_t)cells), pct((size_t)(cells * P));
    for (int64_t i = 0; i < cells; ++i) {
        const int32_t p = fm_by_row_pattern(cell_off.data(), n, i);
        int64_t lo;
        const int64_t c = fm_num_segment(skey.data(), hit_off, n_hits, first, p, (int32_t)(i - cell_off[(size_t)p]), code_bits, lo);
        cnt[(size_t)i] = (int32_t)c;
        vmin[(size_t)i] = c > 0 ? (int64_t)sval[(size_t)lo] : 0;
        vmax[(size_t)i] = c > 0 ? (int64_t)sval[(size_t)(lo + c - 1)] : 0;
        fm_num_sum128(fm_num_scan_between(scan_lo.data(), lo, c), fm_num_scan_between(scan_hi.data(), lo, c), sum_lo[(size_t)i], sum_hi[(size_t)i]);
        for (int32_t j = 0; j < P; ++j)
            pct[(size_t)(i * P + j)] = c > 0 ? (int64_t)sval[(size_t)(lo + fm_num_pct_index(a.permille[(size_t)j], c))] : 0;
    }
    for (int32_t p = 0; p < n; ++p) {
        no_key[(size_t)p] = fm_hist_count(skey.data(), hit_off, n_hits, first, p, C, code_bits);
        nn[(size_t)p] = fm_hist_count(skey.data(), hit_off, n_hits, first, p, C + kNumNotNumber, code_bits);
        ov[(size_t)p] = fm_hist_count(skey.data(), hit_off, n_hits, first, p, C + kNumOverflow, code_bits);
    }

    // ---- the check: every cell against values kept hit by hit, by the definition (no sort, no rank table, no code) ----
    {
        // the key row of group g of key pattern k by counting: the groups with more lines, and the earlier ones with as many
        auto row_of = [&](int32_t k, int32_t g) -> int64_t {
            const int64_t g0 = a.val_off[(size_t)k], g1 = a.val_off[(size_t)k + 1];
            int64_t ahead = 0;
            for (int64_t x = g0; x < g1; ++x)
                if (a.group_lines[(size_t)x] > a.group_lines[(size_t)(g0 + g)] || (a.group_lines[(size_t)x] == a.group_lines[(size_t)(g0 + g)] && x < g0 + g))
                    ++ahead;
            const int64_t rows = std::min<int64_t>(top, g1 - g0);
            return std::min(ahead, rows);
        };
        std::vector<u128> w_sum((size_t)cells, 0);
        std::vector<int64_t> w_cnt((size_t)cells, 0), w_min((size_t)cells, 0), w_max((size_t)cells, 0);
        std::vector<std::vector<int64_t>> w_vals((size_t)cells);
        std::vector<int64_t> w_nk((size_t)n, 0), w_nn((size_t)n, 0), w_ov((size_t)n, 0);
        for (int32_t p = 0; p < n; ++p) {
            const int32_t k = a.by_of[(size_t)p];
            for (int64_t t = fm_filter_slot(hit_off[p], n_hits); t < fm_filter_slot(hit_off[p + 1], n_hits); ++t) {
                const int32_t loc = a.locs[(size_t)t];
                const int32_t L = (int32_t)(std::lower_bound(a.T.begin(), a.T.end(), loc) - a.T.begin());
                int32_t b = 0;
                if (n_edges > 0) {
                    b = -1;
                    for (int32_t x = 0; x < B; ++x)
                        if (a.edges[(size_t)x] <= L && L < a.edges[(size_t)x + 1]) b = x;
                }
                int64_t at = -1;
                for (int64_t x = a.first_off[(size_t)k]; x < a.first_off[(size_t)k + 1]; ++x)
                    if (a.first_lines[(size_t)x] == L) at = x;
                const int32_t g = at >= 0 ? a.group_of_first[(size_t)at] : -1;
                if (at < 0 || b < 0 || g < 0 || g >= a.val_off[(size_t)k + 1] - a.val_off[(size_t)k]) {
                    ++w_nk[(size_t)p];
                    continue;
                }
                int32_t s, e;
                fm_val_window(loc, a.term_len[(size_t)p], kNumWindow, text_len, s, e);
                int64_t v;
                const int32_t kind = fm_num_parse(a.text.data() + s, e - s, (int32_t)a.frac_digits, v);
                if (kind == kNumNotNumber) {
                    ++w_nn[(size_t)p];
                } else if (kind == kNumOverflow) {
                    ++w_ov[(size_t)p];
                } else {
                    const size_t c = (size_t)(cell_off[(size_t)p] + row_of(k, g) * B + b);
                    if ((int64_t)c >= cell_off[(size_t)p + 1]) return 6;
                    w_min[c] = w_cnt[c] ? std::min(w_min[c], v) : v;
                    w_max[c] = w_cnt[c] ? std::max(w_max[c], v) : v;
                    ++w_cnt[c];
                    w_sum[c] += (u128)(uint64_t)v;
                    w_vals[c].push_back(v);
                }
            }
        }
        for (int64_t i = 0; i < cells; ++i) {
            const size_t c = (size_t)i;
            const u128 got = ((u128)sum_hi[c] << 64) | sum_lo[c];
            if (cnt[c] != w_cnt[c] || vmin[c] != w_min[c] || vmax[c] != w_max[c] || got != w_sum[c]) {
                fprintf(stderr, "cell %lld differs: count %d, hit by hit %lld\n", (long long)i, cnt[c], (long long)w_cnt[c]);
                return 6;
            }
            std::sort(w_vals[c].begin(), w_vals[c].end());
            for (int32_t j = 0; j < P; ++j) {
                const int64_t cc = w_cnt[c], rank = ((int64_t)a.permille[(size_t)j] * cc + 999) / 1000;
                const int64_t want = cc ? w_vals[c][(size_t)((rank < 1 ? 1 : rank) - 1)] : 0;
                if (pct[(size_t)(i * P + j)] != want) return 6;
            }
        }
        for (int32_t p = 0; p < n; ++p)
            if (no_key[(size_t)p] != w_nk[(size_t)p] || nn[(size_t)p] != w_nn[(size_t)p] || ov[(size_t)p] != w_ov[(size_t)p]) return 6;
        // the key rows: descending lines, ties by group index, each group once
        for (int32_t k = 0; k < m; ++k)
            for (int64_t r = key_row_off[(size_t)k]; r < key_row_off[(size_t)k + 1]; ++r) {
                if (row_of(k, key_row_group[(size_t)r]) != r - key_row_off[(size_t)k]) return 6;
                if (key_row_lines[(size_t)r] != a.group_lines[(size_t)(a.val_off[(size_t)k] + key_row_group[(size_t)r])]) return 6;
            }
    }

    FILE *o = fopen(out_path, "wb");
    if (!o) return 2;
    put(o, key_row_off);
    put(o, key_row_group);
    put(o, key_row_lines);
    put(o, cell_off);
    put(o, cnt);
    put(o, sum_lo);
    put(o, sum_hi);
    put(o, vmin);
    put(o, vmax);
    put(o, pct);
    put(o, no_key);
    put(o, nn);
    put(o, ov);
    fclose(o);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "self")) {
        self_checks();
        return g_failed ? 4 : 0;
    }
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    fprintf(stderr, "usage: by_hist_hostsim self | run IN OUT\n");
    return 1;
}
