// fmx_by_hist.hip — packed hits of number patterns, behind stages a and b of "stats ... by" over the key patterns' hits ->
// STATISTICS OF THE NUMBER BEHIND EACH HIT BY THE KEY OF ITS LINE, PER BUCKET OF LINES (fmx_numbers_by_key_buckets_dev,
// fmx_number_stats_by_histogram_batch; fmx_by_hist.hpp has the definition and the per-item functions).  The windows' text is the
// packed extract's, which the C-ABI layer runs between launch_by_hist_codes and launch_by_hist_cells over the ranges the former
// leaves in the workspace.
//
// Lanes go to groups, slots, cells or patterns' tails, never to patterns' hits:
//   k_bh_rank_keys    a lane per group: its key pattern (fm_hit_pattern over val_off) and the key pattern | INT32_MAX - lines; the
//                     payload is the group's index
//   rocPRIM           ONE stable radix_sort_pairs over the G groups and 31 + fm_bits(m) bits
//   k_bh_ranks        a lane per sorted group: rank_of_group = min(sorted index - val_off[k], top); a rank below top also stores the
//                     key row's group and lines
//   k_bh_codes        a lane per packed number slot, k_by_ranges' tile loop with k_num_ranges' edges: the window [s, e), the line
//                     (fm_line_of over the fences in LDS), the bucket (fm_hist_bucket; up to kHistEdgesLds edges in LDS, more in HBM,
//                     none: bucket 0), ONE lower bound in the first lines of its key pattern (fm_by_find), the code (fm_bh_code)
//   (packed extract, launch_numbers_sorted: k_num_parse, the two stable sorts, the two running sums — fmx_hit_numbers.hip's own)
//   k_bh_cells        a lane per PACKED cell: its pattern off cell_off (fm_by_row_pattern), fm_num_segment's two lower bounds, then
//                     count, min, max, the 128-bit sum and the percentiles as k_by_rows reads them
//   k_bh_tails        a lane per number pattern: no_key, not_number and overflow
// Integers only, no atomics: the result does not depend on the order the lanes run in.  LDS of k_bh_codes: 16 KiB slice + 16 KiB
// fences + 16 KiB edges, as k_vh_keys.  Nothing here looks at the image, so this file is compiled once.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <cstring>
#include <vector>

#include "fmx_by_hist.hpp"
#include "fmx_hit_filter.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_bh_codes: a tile of kLocateAllTile slots per round
constexpr int kFlatBlock = 256;  // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

__global__ __launch_bounds__(kFlatBlock) void k_bh_rank_keys(const int64_t *__restrict__ val_off, int32_t m, const int32_t *__restrict__ lines,
                                                             int64_t G, uint64_t *__restrict__ keys, uint32_t *__restrict__ group) {
    for (int64_t g = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; g < G; g += (int64_t)gridDim.x * kFlatBlock) {
        const int32_t c = lines[g];
        keys[g] = fm_vh_rank_key(fm_hit_pattern(val_off, m, g), c < 0 ? 0 : c);
        group[g] = (uint32_t)g;
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_bh_ranks(const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ sgroup,
                                                         const int64_t *__restrict__ val_off, const int64_t *__restrict__ key_row_off, int64_t G,
                                                         int32_t top, int32_t *__restrict__ rank_of_group, int32_t *__restrict__ key_row_group,
                                                         int32_t *__restrict__ key_row_lines) {
    for (int64_t j = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; j < G; j += (int64_t)gridDim.x * kFlatBlock) {
        const uint64_t key = skeys[j];
        const int32_t k = fm_vh_rank_key_pattern(key);
        const int64_t g = sgroup[j], first = val_off[k];
        const int32_t rank = fm_vh_rank(j, first, top);
        rank_of_group[g] = rank;
        if (rank < top) {
            const int64_t row = key_row_off[k] + rank;
            key_row_group[row] = (int32_t)(g - first);
            key_row_lines[row] = fm_vh_rank_key_count(key);
        }
    }
}

// n_edges == 0: no edges (B = 1), every slot lies in bucket 0.  by_of (n), val_off (m + 1), first_off (m + 1), first_lines /
// group_of_first: the key patterns' first hits of lines and their groups (stages a, b)
__global__ __launch_bounds__(kKeyBlock) void k_bh_codes(const int32_t *__restrict__ T, int32_t count, int32_t n_fences, int32_t shift,
                                                        const int64_t *__restrict__ hit_off, int32_t n, const int32_t *__restrict__ locs,
                                                        int64_t n_hits, const int32_t *__restrict__ term_len, int32_t text_len,
                                                        const int32_t *__restrict__ edges, int32_t n_edges, const int32_t *__restrict__ by_of,
                                                        const int64_t *__restrict__ val_off, const int64_t *__restrict__ first_off,
                                                        const int32_t *__restrict__ first_lines, const int32_t *__restrict__ group_of_first,
                                                        const int32_t *__restrict__ rank_of_group, int32_t top, int32_t B, int32_t C,
                                                        int32_t code_bits, int32_t *__restrict__ start, int32_t *__restrict__ stop,
                                                        uint64_t *__restrict__ keys) {
    __shared__ int64_t s_off[kLocateAllSlice];
    __shared__ int32_t s_fence[kLineFences];
    __shared__ int32_t s_edge[kHistEdgesLds];
    const bool bucketed = n_edges > 0;                              // (workgroup-uniform)
    const bool edges_in_lds = bucketed && n_edges <= kHistEdgesLds;  // (workgroup-uniform)
    for (int32_t j = threadIdx.x; j < n_fences; j += kKeyBlock) s_fence[j] = T[(int64_t)j << shift];
    if (edges_in_lds)
        for (int32_t j = threadIdx.x; j < n_edges; j += kKeyBlock) s_edge[j] = edges[j];
    __syncthreads();
    const int32_t *edge = edges_in_lds ? s_edge : edges;
    const uint64_t no_hit = fm_hist_key(n, 0, code_bits);
    const int64_t first = fm_filter_slot(hit_off[0], n_hits), total = fm_filter_slot(hit_off[n], n_hits);
    for (int64_t tile = (int64_t)blockIdx.x * kLocateAllTile; tile < n_hits; tile += (int64_t)gridDim.x * kLocateAllTile) {
        const int64_t t = tile + threadIdx.x;
        if (tile >= total || tile + kLocateAllTile <= first) {  // a tile of slots behind or in front of the hits (workgroup-uniform)
            if (t < n_hits) {
                keys[t] = no_hit;
                start[t] = stop[t] = 0;
            }
            continue;
        }
        const HitTile h = fm_hit_tile(hit_off, n, tile, total);
        bool in_lds;
        const int64_t *slice = fm_hit_tile_slice<kKeyBlock>(s_off, hit_off, h, in_lds);
        if (t >= first && t <= h.tile_last) {
            const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
            const int32_t loc = locs[t];
            int32_t s, e;
            fm_val_window(loc, term_len[p], kNumWindow, text_len, s, e);
            start[t] = s;
            stop[t] = e;
            const int32_t k = by_of[p], L = fm_line_of(T, count, s_fence, n_fences, shift, loc);
            const int32_t bucket = bucketed ? fm_hist_bucket(edge, n_edges, L) : 0;
            const int64_t found = fm_by_find(first_lines, first_off[k], first_off[k + 1], L), g0 = val_off[k];
            keys[t] = fm_hist_key(p, fm_bh_code(rank_of_group, group_of_first, found, g0, val_off[k + 1] - g0, top, bucket, B, C), code_bits);
        } else if (t < n_hits) {
            keys[t] = no_hit;
            start[t] = stop[t] = 0;
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

struct CellOut {
    int32_t *count;
    uint64_t *sum_lo, *sum_hi;
    int64_t *min, *max, *pct;
};

// cell_off: n + 1 (the workspace's copy); cells = cell_off[n]
__global__ __launch_bounds__(kFlatBlock) void k_bh_cells(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ values,
                                                         const uint64_t *__restrict__ scan_lo, const uint64_t *__restrict__ scan_hi,
                                                         const int64_t *__restrict__ hit_off, int32_t n, int64_t n_hits,
                                                         const int64_t *__restrict__ cell_off, int64_t cells, int32_t code_bits,
                                                         const int32_t *__restrict__ permille, int32_t P, CellOut out) {
    const int64_t first = fm_filter_slot(hit_off[0], n_hits);
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < cells; i += (int64_t)gridDim.x * kFlatBlock) {
        const int32_t p = fm_by_row_pattern(cell_off, n, i);
        int64_t lo;
        const int64_t c = fm_num_segment(keys, hit_off, n_hits, first, p, (int32_t)(i - cell_off[p]), code_bits, lo);
        out.count[i] = (int32_t)c;
        if (out.min) out.min[i] = c > 0 ? (int64_t)values[lo] : 0;
        if (out.max) out.max[i] = c > 0 ? (int64_t)values[lo + c - 1] : 0;
        if (out.sum_lo || out.sum_hi) {
            uint64_t s_lo, s_hi;
            fm_num_sum128(fm_num_scan_between(scan_lo, lo, c), fm_num_scan_between(scan_hi, lo, c), s_lo, s_hi);
            if (out.sum_lo) out.sum_lo[i] = s_lo;
            if (out.sum_hi) out.sum_hi[i] = s_hi;
        }
        if (out.pct)
            for (int32_t j = 0; j < P; ++j) out.pct[i * P + j] = c > 0 ? (int64_t)values[lo + fm_num_pct_index(permille[j], c)] : 0;
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_bh_tails(const uint64_t *__restrict__ keys, const int64_t *__restrict__ hit_off, int32_t n,
                                                         int64_t n_hits, int32_t C, int32_t code_bits, int32_t *__restrict__ no_key,
                                                         int32_t *__restrict__ not_number, int32_t *__restrict__ overflow) {
    const int64_t first = fm_filter_slot(hit_off[0], n_hits);
    for (int64_t p = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kFlatBlock) {
        if (no_key) no_key[p] = fm_hist_count(keys, hit_off, n_hits, first, (int32_t)p, C, code_bits);
        if (not_number) not_number[p] = fm_hist_count(keys, hit_off, n_hits, first, (int32_t)p, C + kNumNotNumber, code_bits);
        if (overflow) overflow[p] = fm_hist_count(keys, hit_off, n_hits, first, (int32_t)p, C + kNumOverflow, code_bits);
    }
}

// the regions of the caller's workspace, each a multiple of 256 bytes.  tables: edges (n_edges ints), term_len (n), permille (P),
// by_of (n) — one copy.  The numbers stage's sorts go a -> b (by value), b -> a (by key); the running sums land in val_b and key_b.
struct ByHistWs {
    size_t start, stop, win_off, piece_off, win_status, extract, extract_bytes, win, key_a, key_b, val_a, val_b, tables, tables_bytes, t_len,
        t_permille, t_by_of, val_off, key_row_off, cell_off, rank_a, rank_b, group_a, group_b, rank_of_group, tmp, tmp_bytes, total;
};
ByHistWs by_hist_ws(int32_t n, int32_t m, int64_t G, int64_t n_hits, int32_t n_edges, int32_t P) {
    ByHistWs w{};
    const size_t H = (size_t)n_hits;
    size_t rank_tmp = 0;
    (void)rocprim::radix_sort_pairs(nullptr, rank_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                    (uint32_t *)nullptr, (size_t)G, 0u, 62u);
    const size_t num_tmp = n_hits > 0 ? numbers_sorted_tmp_bytes(n_hits) : 0;
    w.tmp_bytes = pad256(rank_tmp > num_tmp ? rank_tmp : num_tmp);
    w.t_len = (size_t)n_edges * 4;
    w.t_permille = w.t_len + (size_t)n * 4;
    w.t_by_of = w.t_permille + (size_t)P * 4;
    w.tables_bytes = w.t_by_of + (size_t)n * 4;
    w.extract_bytes = n_hits > 0 ? extract_packed_scratch_bytes((int32_t)n_hits) : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.start = take(H * 4);
    w.stop = take(H * 4);
    w.win_off = take((H + 1) * 8);
    w.piece_off = take((H + 1) * 8);
    w.win_status = take(H * 4);
    w.extract = take(w.extract_bytes);
    w.win = take(H * (size_t)kNumWindow * 2 + 8);
    w.key_a = take(H * 8);
    w.key_b = take(H * 8);
    w.val_a = take(H * 8);
    w.val_b = take(H * 8);
    w.tables = take(w.tables_bytes);
    w.val_off = take(((size_t)m + 1) * 8);
    w.key_row_off = take(((size_t)m + 1) * 8);
    w.cell_off = take(((size_t)n + 1) * 8);
    w.rank_a = take((size_t)G * 8);
    w.rank_b = take((size_t)G * 8);
    w.group_a = take((size_t)G * 4);
    w.group_b = take((size_t)G * 4);
    w.rank_of_group = take((size_t)G * 4);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}
bool shape_ok(int32_t n, int32_t m, int64_t G, int64_t n_hits, int32_t n_edges, int32_t P) {
    return n > 0 && m > 0 && G >= 0 && G <= 0x7fffffff && n_hits >= 0 && n_hits <= 0x7fffffff && (n_edges == 0 || n_edges >= 2) && P >= 0 &&
           P <= kNumPermilleMax;
}

template <class T>
T *region(void *ws, size_t off) {
    return reinterpret_cast<T *>(static_cast<uint8_t *>(ws) + off);
}

// what the three launchers agree on: the checks of the small host arrays and the layout
struct Shape {
    std::vector<int64_t> key_row_off, cell_off;
    int32_t B = 1, C = 1;
    ByHistWs w{};
};
bool shape_of(int32_t n, const int32_t *by_of, int32_t m, const int64_t *val_off, int32_t top, const int32_t *edges, int32_t n_edges,
              int64_t n_hits, const int32_t *permille, int32_t P, const void *ws, size_t ws_bytes, Shape *s) {
    if (n <= 0 || m <= 0 || !val_off || !shape_ok(n, m, val_off[m], n_hits, n_edges, P) || fm_num_permille_bad(permille, P)) return false;
    if (n_edges > 0 && fm_hist_edges_bad(edges, n_edges)) return false;
    s->B = n_edges > 0 ? n_edges - 1 : 1;
    s->key_row_off.assign((size_t)m + 1, 0);
    s->cell_off.assign((size_t)n + 1, 0);
    if (fm_bh_shape_bad(n, by_of, m, val_off, top, s->B, P, s->key_row_off.data(), s->cell_off.data(), &s->C)) return false;
    s->w = by_hist_ws(n, m, val_off[m], n_hits, n_edges, P);
    return ws && ws_bytes >= s->w.total;
}

}  // namespace

size_t numbers_by_key_buckets_scratch_bytes(int32_t n, int32_t m, int64_t n_groups, int64_t n_hits, int32_t n_edges, int32_t n_permille) {
    return shape_ok(n, m, n_groups, n_hits, n_edges, n_permille) ? by_hist_ws(n, m, n_groups, n_hits, n_edges, n_permille).total : 0;
}

bool numbers_by_key_buckets_windows(void *ws, size_t ws_bytes, int32_t n, int32_t m, int64_t n_groups, int64_t n_hits, int32_t n_edges,
                                    int32_t n_permille, ValuesWindows *out) {
    if (!ws || n_hits <= 0 || !shape_ok(n, m, n_groups, n_hits, n_edges, n_permille)) return false;
    const ByHistWs w = by_hist_ws(n, m, n_groups, n_hits, n_edges, n_permille);
    if (ws_bytes < w.total) return false;
    out->start = region<int32_t>(ws, w.start);
    out->stop = region<int32_t>(ws, w.stop);
    out->status = region<int32_t>(ws, w.win_status);
    out->text_off = region<int64_t>(ws, w.win_off);
    out->piece_off = region<int64_t>(ws, w.piece_off);
    out->chars = region<uint16_t>(ws, w.win);
    out->scratch = region<uint8_t>(ws, w.extract);
    out->scratch_bytes = w.extract_bytes;
    return true;
}

int launch_by_hist_codes(const int32_t *T, int32_t count, int32_t text_len, int n_cu, int32_t n, const int32_t *term_len, const int32_t *by_of,
                         int32_t m, const int64_t *val_off, int32_t top, const int32_t *edges, int32_t n_edges, const int64_t *hit_off,
                         const int32_t *locs, int64_t n_hits, const int64_t *first_off, const int32_t *first_lines, const int32_t *group_of_first,
                         const int32_t *group_lines, const int32_t *permille, int32_t n_permille, int64_t *key_row_off_out,
                         int32_t *key_row_group, int32_t *key_row_lines, int64_t *cell_off_out, void *ws, size_t ws_bytes, void *stream) {
    Shape s;
    if (!shape_of(n, by_of, m, val_off, top, edges, n_edges, n_hits, permille, n_permille, ws, ws_bytes, &s) || count < 0 || !T || !term_len)
        return (int)hipErrorInvalidValue;
    const int64_t G = val_off[m];
    if (G > 0 && (!group_lines || !key_row_group || !key_row_lines)) return (int)hipErrorInvalidValue;
    if (n_hits > 0 && (!hit_off || !locs || !first_off || (G > 0 && (!first_lines || !group_of_first)))) return (int)hipErrorInvalidValue;
    const ByHistWs &w = s.w;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    // the tables.  The runtime has read these blocks when the copies return (a copy from pageable host memory is staged before the
    // call comes back).
    std::vector<uint8_t> host(w.tables_bytes + 4, 0);
    if (n_edges > 0) memcpy(host.data(), edges, (size_t)n_edges * 4);
    memcpy(host.data() + w.t_len, term_len, (size_t)n * 4);
    if (n_permille > 0) memcpy(host.data() + w.t_permille, permille, (size_t)n_permille * 4);
    memcpy(host.data() + w.t_by_of, by_of, (size_t)n * 4);
    int64_t *d_val_off = region<int64_t>(ws, w.val_off), *d_key_row_off = region<int64_t>(ws, w.key_row_off);
    const size_t key_bytes = ((size_t)m + 1) * 8, cell_bytes = ((size_t)n + 1) * 8;
#define FMX_BH_CHECK(call) \
    if (hipError_t e_ = (call); e_ != hipSuccess) return (int)e_
    FMX_BH_CHECK(hipMemcpyAsync(region<uint8_t>(ws, w.tables), host.data(), w.tables_bytes, hipMemcpyHostToDevice, st));
    FMX_BH_CHECK(hipMemcpyAsync(d_val_off, val_off, key_bytes, hipMemcpyHostToDevice, st));
    FMX_BH_CHECK(hipMemcpyAsync(d_key_row_off, s.key_row_off.data(), key_bytes, hipMemcpyHostToDevice, st));
    FMX_BH_CHECK(hipMemcpyAsync(region<uint8_t>(ws, w.cell_off), s.cell_off.data(), cell_bytes, hipMemcpyHostToDevice, st));
    if (key_row_off_out) FMX_BH_CHECK(hipMemcpyAsync(key_row_off_out, s.key_row_off.data(), key_bytes, hipMemcpyHostToDevice, st));
    if (cell_off_out) FMX_BH_CHECK(hipMemcpyAsync(cell_off_out, s.cell_off.data(), cell_bytes, hipMemcpyHostToDevice, st));
    int32_t unused = 1, group_grid = 1, key_grid = 1;
    int32_t *rank_of_group = region<int32_t>(ws, w.rank_of_group);
    if (G > 0) {
        uint64_t *rank_a = region<uint64_t>(ws, w.rank_a), *rank_b = region<uint64_t>(ws, w.rank_b);
        uint32_t *group_a = region<uint32_t>(ws, w.group_a), *group_b = region<uint32_t>(ws, w.group_b);
        size_t tmp_bytes = w.tmp_bytes;
        hit_lines_geometry(G, n_cu, &unused, &group_grid);
        hipLaunchKernelGGL(k_bh_rank_keys, dim3((unsigned)group_grid), dim3(kFlatBlock), 0, st, d_val_off, m, group_lines, G, rank_a, group_a);
        FMX_BH_CHECK(hipGetLastError());
        FMX_BH_CHECK(rocprim::radix_sort_pairs(region<uint8_t>(ws, w.tmp), tmp_bytes, rank_a, rank_b, group_a, group_b, (size_t)G, 0u,
                                               (unsigned)fm_vh_rank_key_width(m), st));
        hipLaunchKernelGGL(k_bh_ranks, dim3((unsigned)group_grid), dim3(kFlatBlock), 0, st, rank_b, group_b, d_val_off, d_key_row_off, G, top,
                           rank_of_group, key_row_group, key_row_lines);
        FMX_BH_CHECK(hipGetLastError());
    }
#undef FMX_BH_CHECK
    if (n_hits == 0) return 0;  // (no number hit: the key rows alone)
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, kLineFences, n_fences);
    hit_lines_geometry(n_hits, n_cu, &key_grid, &unused);
    hipLaunchKernelGGL(k_bh_codes, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, T, count, n_fences, shift, hit_off, n, locs, n_hits,
                       region<const int32_t>(ws, w.tables + w.t_len), text_len, region<const int32_t>(ws, w.tables), n_edges,
                       region<const int32_t>(ws, w.tables + w.t_by_of), d_val_off, first_off, first_lines, group_of_first, rank_of_group, top, s.B,
                       s.C, fm_num_code_bits(s.C), region<int32_t>(ws, w.start), region<int32_t>(ws, w.stop), region<uint64_t>(ws, w.key_a));
    return (int)hipGetLastError();
}

int launch_by_hist_cells(int n_cu, int32_t n, const int32_t *by_of, int32_t m, const int64_t *val_off, int32_t top, int32_t n_edges,
                         const int64_t *hit_off, int64_t n_hits, int32_t frac_digits, int32_t n_permille, int32_t *count, uint64_t *sum_lo,
                         uint64_t *sum_hi, int64_t *min, int64_t *max, int64_t *pct, int32_t *no_key, int32_t *not_number, int32_t *overflow,
                         int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    if (n <= 0 || m <= 0 || n_hits <= 0 || !val_off || !shape_ok(n, m, val_off[m], n_hits, n_edges, n_permille) || frac_digits < 0 ||
        frac_digits > kNumFracMax || !count || !hit_off)
        return (int)hipErrorInvalidValue;
    Shape s;
    s.B = n_edges > 0 ? n_edges - 1 : 1;
    s.cell_off.assign((size_t)n + 1, 0);
    if (fm_bh_shape_bad(n, by_of, m, val_off, top, s.B, n_permille, nullptr, s.cell_off.data(), &s.C)) return (int)hipErrorInvalidValue;
    const ByHistWs w = by_hist_ws(n, m, val_off[m], n_hits, n_edges, n_permille);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t *key_a = region<uint64_t>(ws, w.key_a), *key_b = region<uint64_t>(ws, w.key_b);
    uint64_t *val_a = region<uint64_t>(ws, w.val_a), *val_b = region<uint64_t>(ws, w.val_b);
    if (const int e = launch_numbers_sorted(n_cu, n, n_hits, s.C, frac_digits, region<const int64_t>(ws, w.win_off), region<const uint16_t>(ws, w.win),
                                            region<const int32_t>(ws, w.win_status), key_a, key_b, val_a, val_b, sum_lo || sum_hi, status,
                                            region<uint8_t>(ws, w.tmp), w.tmp_bytes, stream))
        return e;
    const int64_t cells = s.cell_off[(size_t)n];
    const int32_t code_bits = fm_num_code_bits(s.C);
    int32_t unused = 1, cell_grid = 1, pat_grid = 1;
    hit_lines_geometry(cells, n_cu, &unused, &cell_grid);
    hit_lines_geometry(n, n_cu, &unused, &pat_grid);
    hipLaunchKernelGGL(k_bh_cells, dim3((unsigned)cell_grid), dim3(kFlatBlock), 0, st, key_a, val_a, val_b, key_b, hit_off, n, n_hits,
                       region<const int64_t>(ws, w.cell_off), cells, code_bits, region<const int32_t>(ws, w.tables + w.t_permille), n_permille,
                       CellOut{count, sum_lo, sum_hi, min, max, n_permille > 0 ? pct : nullptr});
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (no_key || not_number || overflow) {
        hipLaunchKernelGGL(k_bh_tails, dim3((unsigned)pat_grid), dim3(kFlatBlock), 0, st, key_a, hit_off, n, n_hits, s.C, code_bits, no_key,
                           not_number, overflow);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    }
    return 0;
}

}  // namespace fmx
