// fmx_line_hist.hip — MATCHING LINES AND HITS PER BUCKET OF LINES (fmx_lines_histogram_dev, fmx_hits_histogram_dev;
// fmx_line_hist.hpp has the definitions): the timeline of a log search — what the line, query and sequence stages and the hit
// filter leave on the device, turned into rows x B counters, so that only the counters come down.
//
// LINES per bucket (packed ascending lists in, q x B counters out): no lane walks a list.
//   k_hist_ranks     a lane per (list, edge): ONE lower bound of the edge in its list — q x n_edges short searches; a list of
//                    10^7 lines costs what a list of 10 costs
//   k_hist_diffs     a lane per (list, bucket): the difference of two neighbouring ranks
// HITS per bucket (packed hits in SA-row order in, n x B counters out): every stage hands lanes to SLOTS or to COUNTERS, never to
// patterns, so ONE pattern with millions of hits uses the whole device.
//   k_hist_keys      a lane per packed slot: its pattern (fm_hit_pattern over an LDS slice of hit_off: fm_hit_tile /
//                    fm_hit_tile_slice, as k_hit_line_keys), its line (fm_line_of: the first levels over the fences staged in LDS),
//                    its bucket (fm_hist_bucket: an upper bound over the edges, staged in LDS where they are at most
//                    kHistEdgesLds, searched in HBM otherwise — correct, not tuned), the key pattern | bucket; a slot that is no
//                    hit gets the pattern n, which sorts last
//   rocPRIM          ONE device-wide radix sort of the keys over the bits in use, fm_bits(n) + fm_bits(B): usually one or two
//                    passes (not a segmented sort, for the reason fmx_hit_lines.hip gives)
//   k_hist_counts    a lane per (pattern, bucket): two lower bounds in the pattern's part of the sorted keys
// Integers only, no atomics: the result does not depend on the order the lanes run in.  Nothing here looks at the image, so this
// file is compiled once.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "fmx_hit_filter.hpp"
#include "fmx_line_hist.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_hist_keys: a tile of kLocateAllTile hits per round; 16 + 16 + 16 KiB of LDS: three workgroups per CU
constexpr int kFlatBlock = 256;  // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

__global__ __launch_bounds__(kFlatBlock) void k_hist_ranks(const int64_t *__restrict__ line_off, const int32_t *__restrict__ lines, int32_t q,
                                                           const int32_t *__restrict__ edges, int32_t n_edges, int64_t *__restrict__ rank) {
    const int64_t items = (int64_t)q * n_edges;
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < items; i += (int64_t)gridDim.x * kFlatBlock) {
        const int64_t Q = i / n_edges;
        const int32_t e = (int32_t)(i - Q * n_edges);
        const int64_t lo = line_off[Q], hi = line_off[Q + 1];
        rank[i] = hi > lo ? fm_hist_rank(lines, lo, hi, edges[e]) : lo;
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_hist_diffs(const int64_t *__restrict__ rank, int32_t q, int32_t n_edges, int32_t *__restrict__ hist) {
    const int32_t B = n_edges - 1;
    const int64_t items = (int64_t)q * B;
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < items; i += (int64_t)gridDim.x * kFlatBlock) {
        const int64_t Q = i / B, at = Q * n_edges + (i - Q * B);
        hist[i] = fm_hist_between(rank[at], rank[at + 1]);
    }
}

__global__ __launch_bounds__(kKeyBlock) void k_hist_keys(const int32_t *__restrict__ T, int32_t count, int32_t n_fences, int32_t shift,
                                                         const int64_t *__restrict__ hit_off, int32_t n, const int32_t *__restrict__ locs,
                                                         int64_t n_hits, const int32_t *__restrict__ edges, int32_t n_edges,
                                                         int32_t bucket_bits, uint64_t *__restrict__ keys) {
    __shared__ int64_t s_off[kLocateAllSlice];
    __shared__ int32_t s_fence[kLineFences];
    __shared__ int32_t s_edge[kHistEdgesLds];
    for (int32_t j = threadIdx.x; j < n_fences; j += kKeyBlock) s_fence[j] = T[(int64_t)j << shift];
    const bool edges_in_lds = n_edges <= kHistEdgesLds;  // (workgroup-uniform)
    if (edges_in_lds)
        for (int32_t j = threadIdx.x; j < n_edges; j += kKeyBlock) s_edge[j] = edges[j];
    __syncthreads();
    const int32_t *edge = edges_in_lds ? s_edge : edges;
    const uint64_t no_hit = fm_hist_key(n, 0, bucket_bits);
    const int64_t first = fm_filter_slot(hit_off[0], n_hits), total = fm_filter_slot(hit_off[n], n_hits);
    for (int64_t tile = (int64_t)blockIdx.x * kLocateAllTile; tile < n_hits; tile += (int64_t)gridDim.x * kLocateAllTile) {
        const int64_t t = tile + threadIdx.x;
        if (tile >= total || tile + kLocateAllTile <= first) {  // a tile of slots behind or in front of the hits (workgroup-uniform)
            if (t < n_hits) keys[t] = no_hit;
            continue;
        }
        const HitTile h = fm_hit_tile(hit_off, n, tile, total);
        bool in_lds;
        const int64_t *slice = fm_hit_tile_slice<kKeyBlock>(s_off, hit_off, h, in_lds);
        if (t >= first && t <= h.tile_last) {
            const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
            const int32_t L = fm_line_of(T, count, s_fence, n_fences, shift, locs[t]);
            keys[t] = fm_hist_key(p, fm_hist_bucket(edge, n_edges, L), bucket_bits);
        } else if (t < n_hits) {
            keys[t] = no_hit;
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_hist_counts(const uint64_t *__restrict__ keys, const int64_t *__restrict__ hit_off, int32_t n,
                                                            int64_t n_hits, int32_t B, int32_t bucket_bits, int32_t *__restrict__ hist) {
    const int64_t items = (int64_t)n * B, first = fm_filter_slot(hit_off[0], n_hits);
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < items; i += (int64_t)gridDim.x * kFlatBlock) {
        const int64_t p = i / B;
        hist[i] = fm_hist_count(keys, hit_off, n_hits, first, (int32_t)p, (int32_t)(i - p * B), bucket_bits);
    }
}

// the regions of the caller's workspace, each a multiple of 256 bytes
struct LinesHistWs {
    size_t edges, rank, total;
};
LinesHistWs lines_hist_ws(int32_t q, int32_t n_edges) {
    LinesHistWs w{};
    w.edges = 0;
    w.rank = pad256((size_t)n_edges * 4);
    w.total = w.rank + pad256((size_t)q * (size_t)n_edges * 8);
    return w;
}
struct HitsHistWs {
    size_t edges, keys_a, keys_b, tmp, tmp_bytes, total;
};
HitsHistWs hits_hist_ws(int64_t n_hits, int32_t n_edges) {
    HitsHistWs w{};
    size_t sort_tmp = 0;
    (void)rocprim::radix_sort_keys(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n_hits, 0u, 59u);
    w.tmp_bytes = pad256(sort_tmp);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.edges = take((size_t)n_edges * 4);
    w.keys_a = take((size_t)n_hits * 8);
    w.keys_b = take((size_t)n_hits * 8);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}

bool shape_ok(int32_t rows, int32_t n_edges) { return rows > 0 && n_edges >= 2 && (int64_t)rows * (n_edges - 1) <= kHistCellsMax; }

}  // namespace

size_t lines_histogram_scratch_bytes(int32_t q, int32_t n_edges) { return shape_ok(q, n_edges) ? lines_hist_ws(q, n_edges).total : 0; }

size_t hits_histogram_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_edges) {
    if (!shape_ok(n, n_edges) || n_hits <= 0 || n_hits > 0x7fffffff) return 0;
    return hits_hist_ws(n_hits, n_edges).total;
}

int launch_lines_histogram(int n_cu, int32_t q, const int64_t *line_off, const int32_t *lines, const int32_t *edges, int32_t n_edges,
                           int32_t *hist, void *ws, size_t ws_bytes, void *stream) {
    if (q <= 0) return 0;
    if (!shape_ok(q, n_edges) || fm_hist_edges_bad(edges, n_edges)) return (int)hipErrorInvalidValue;
    const LinesHistWs w = lines_hist_ws(q, n_edges);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *base = static_cast<uint8_t *>(ws);
    int32_t *d_edges = reinterpret_cast<int32_t *>(base + w.edges);
    int64_t *rank = reinterpret_cast<int64_t *>(base + w.rank);
    // (the runtime has read edges when the copy returns: a copy from pageable host memory is staged before the call comes back)
    if (hipError_t e = hipMemcpyAsync(d_edges, edges, (size_t)n_edges * 4, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    int32_t unused = 1, rank_grid = 1, diff_grid = 1;
    hit_lines_geometry((int64_t)q * n_edges, n_cu, &unused, &rank_grid);
    hit_lines_geometry((int64_t)q * (n_edges - 1), n_cu, &unused, &diff_grid);
    hipLaunchKernelGGL(k_hist_ranks, dim3((unsigned)rank_grid), dim3(kFlatBlock), 0, st, line_off, lines, q, d_edges, n_edges, rank);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hist_diffs, dim3((unsigned)diff_grid), dim3(kFlatBlock), 0, st, rank, q, n_edges, hist);
    return (int)hipGetLastError();
}

int launch_hits_histogram(const int32_t *T, int32_t count, int n_cu, int32_t n, const int64_t *hit_off, const int32_t *locs, int64_t n_hits,
                          const int32_t *edges, int32_t n_edges, int32_t *hist, void *ws, size_t ws_bytes, void *stream) {
    if (n <= 0 || n_hits <= 0) return 0;
    if (n_hits > 0x7fffffff || count < 0 || !T || !shape_ok(n, n_edges) || fm_hist_edges_bad(edges, n_edges)) return (int)hipErrorInvalidValue;
    const HitsHistWs w = hits_hist_ws(n_hits, n_edges);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *base = static_cast<uint8_t *>(ws);
    int32_t *d_edges = reinterpret_cast<int32_t *>(base + w.edges);
    uint64_t *keys_a = reinterpret_cast<uint64_t *>(base + w.keys_a), *keys_b = reinterpret_cast<uint64_t *>(base + w.keys_b);
    void *tmp = base + w.tmp;
    size_t tmp_bytes = w.tmp_bytes;
    if (hipError_t e = hipMemcpyAsync(d_edges, edges, (size_t)n_edges * 4, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, kLineFences, n_fences);
    const int32_t B = n_edges - 1, bucket_bits = fm_bits((uint32_t)B), key_bits = fm_hist_key_width(n, B);
    int32_t key_grid = 1, flat = 1, unused = 1, count_grid = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hit_lines_geometry((int64_t)n * B, n_cu, &unused, &count_grid);
    hipLaunchKernelGGL(k_hist_keys, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, T, count, n_fences, shift, hit_off, n, locs, n_hits,
                       d_edges, n_edges, bucket_bits, keys_a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::radix_sort_keys(tmp, tmp_bytes, keys_a, keys_b, (size_t)n_hits, 0u, (unsigned)key_bits, st); e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_hist_counts, dim3((unsigned)count_grid), dim3(kFlatBlock), 0, st, keys_b, hit_off, n, n_hits, B, bucket_bits, hist);
    return (int)hipGetLastError();
}

}  // namespace fmx
