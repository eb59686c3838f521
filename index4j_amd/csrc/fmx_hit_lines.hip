// fmx_hit_lines.hip — packed hits -> packed DISTINCT LINES (fmx_line_table_build, fmx_line_bounds_*, fmx_lines_of_hits_dev): what a
// log search asks of "all occurrences" (fmx_locate_all_*) — which lines hold the pattern, each once, in text order; how many; the
// first k.  The line table T is the sorted answer of locate() for the boundary character (fmx_device.hpp "THE LINE TABLE").
//
// Every stage hands lanes to HITS, never to patterns, so a batch of one pattern that matches everywhere uses the whole device:
//   k_hit_line_keys  a lane per packed hit: its pattern (fm_hit_pattern over an LDS slice of hit_off: the tile and its slice
//                    are k_locate_all's, fm_hit_tile / fm_hit_tile_slice), its line (fm_line_of: the first levels over the fences staged in LDS, the rest in HBM), the 64-bit
//                    key (pattern << line_bits) | line; a slot behind hit_off[n] gets the pattern n, which sorts last
//   rocPRIM          ONE device-wide radix sort of the keys over the bits in use (not a segmented sort: that would hand a
//                    pattern of 10^6 hits to one workgroup).  The keys of pattern p then lie at [hit_off[p], hit_off[p + 1])
//   k_line_heads     1 where a key differs from its predecessor; rocPRIM's exclusive scan numbers the distinct (pattern, line) pairs
//   k_line_counts    a lane per pattern: distinct lines = the difference of two scan entries; the count clamped to max_lines,
//                    whose exclusive scan is line_off
//   k_line_compact   a lane per sorted key: a head whose rank inside its pattern is below the limit stores its line
// No atomics: the result does not depend on the order the lanes run in.  Nothing here looks at the image, so this file is compiled
// once — not per image form like fmx_kernels.hip.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fmx_device.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;       // k_hit_line_keys: a tile of kLocateAllTile hits per round, 32 KiB of LDS: two workgroups per CU
constexpr int kFlatBlock = 256;       // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

int flat_grid(int64_t items, int n_cu) {
    int64_t blocks = (items + kFlatBlock - 1) / kFlatBlock;
    const int64_t cap = (int64_t)(n_cu > 0 ? n_cu : 256) * kHitLinesFlatGroupsPerCu;
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}

__global__ __launch_bounds__(kKeyBlock) void k_hit_line_keys(const int32_t *__restrict__ T, int32_t count, int32_t n_fences, int32_t shift,
                                                             int32_t line_bits, const int64_t *__restrict__ hit_off, int32_t n,
                                                             const int32_t *__restrict__ locs, int64_t n_hits,
                                                             uint64_t *__restrict__ keys) {
    __shared__ int64_t s_off[kLocateAllSlice];
    __shared__ int32_t s_fence[kLineFences];
    for (int32_t j = threadIdx.x; j < n_fences; j += kKeyBlock) s_fence[j] = T[(int64_t)j << shift];
    __syncthreads();
    const int64_t total = hit_off[n] < n_hits ? hit_off[n] : n_hits;  // (the caller holds n_hits >= hit_off[n]; nothing is read beyond either)
    for (int64_t tile = (int64_t)blockIdx.x * kLocateAllTile; tile < n_hits; tile += (int64_t)gridDim.x * kLocateAllTile) {
        const int64_t t = tile + threadIdx.x;
        if (tile >= total) {  // a tile of slots behind the hits (workgroup-uniform)
            if (t < n_hits) keys[t] = fm_line_key(n, 0, line_bits);
            continue;
        }
        const HitTile h = fm_hit_tile(hit_off, n, tile, total);
        bool in_lds;
        const int64_t *slice = fm_hit_tile_slice<kKeyBlock>(s_off, hit_off, h, in_lds);
        if (t <= h.tile_last) {
            const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
            keys[t] = fm_line_key(p, fm_line_of(T, count, s_fence, n_fences, shift, locs[t]), line_bits);
        } else if (t < n_hits) {
            keys[t] = fm_line_key(n, 0, line_bits);
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

// head[i] for the sorted keys, and head[n_hits] = 0: the exclusive scan then leaves the number of all pairs there
__global__ __launch_bounds__(kFlatBlock) void k_line_heads(const uint64_t *__restrict__ keys, int64_t n_hits, int32_t n, int32_t line_bits,
                                                           int32_t *__restrict__ head) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i <= n_hits; i += (int64_t)gridDim.x * kFlatBlock)
        head[i] = i < n_hits && fm_line_head(keys, i, n, line_bits) ? 1 : 0;
}

// pos = the exclusive scan of head.  The keys of pattern p are [hit_off[p], hit_off[p + 1]) of the sorted order.
__global__ __launch_bounds__(kFlatBlock) void k_line_counts(const int64_t *__restrict__ hit_off, const int32_t *__restrict__ pos, int32_t n,
                                                            int64_t n_hits, int32_t max_lines, int32_t *__restrict__ line_count,
                                                            int64_t *__restrict__ stored) {
    const int64_t p = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x;
    if (p > n) return;
    int64_t c = 0;
    if (p < n) {
        const int64_t a = hit_off[p] < n_hits ? hit_off[p] : n_hits, b = hit_off[p + 1] < n_hits ? hit_off[p + 1] : n_hits;
        c = b > a ? pos[b] - pos[a] : 0;
        if (line_count) line_count[p] = (int32_t)c;
        if (max_lines > 0 && c > max_lines) c = max_lines;
    }
    stored[p] = c;  // (stored[n] = 0: the exclusive scan leaves the batch's total in line_off[n])
}

__global__ __launch_bounds__(kFlatBlock) void k_line_compact(const uint64_t *__restrict__ keys, const int32_t *__restrict__ pos,
                                                             const int64_t *__restrict__ hit_off, const int64_t *__restrict__ line_off,
                                                             int64_t n_hits, int32_t n, int32_t line_bits, int32_t max_lines,
                                                             int32_t *__restrict__ lines) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < n_hits; i += (int64_t)gridDim.x * kFlatBlock) {
        if (!fm_line_head(keys, i, n, line_bits)) continue;
        const int32_t p = fm_line_key_pattern(keys[i], line_bits);
        const int64_t first = hit_off[p] < n_hits ? hit_off[p] : n_hits;
        const int32_t rank = pos[i] - pos[first];
        if (max_lines > 0 && rank >= max_lines) continue;
        lines[line_off[p] + rank] = fm_line_key_line(keys[i], line_bits);
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_line_bounds(const int32_t *__restrict__ T, int32_t count, int64_t n_lines, int32_t text_len,
                                                            const int32_t *__restrict__ ids, int32_t n, int32_t *__restrict__ start,
                                                            int32_t *__restrict__ stop) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kFlatBlock) {
        int32_t a, b;
        fm_line_bounds(T, count, n_lines, text_len, ids[i], a, b);
        start[i] = a;
        stop[i] = b;
    }
}

__global__ void k_line_total(const int32_t *__restrict__ T, int32_t count, int32_t text_len, int64_t *__restrict__ n_lines) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_lines = fm_line_total(T, count, text_len);
}

// the regions of the caller's workspace, each a multiple of 256 bytes
struct LinesWs {
    size_t keys_a, keys_b, head, pos, stored, tmp, tmp_bytes, total;
};
LinesWs lines_ws(int32_t n, int64_t n_hits) {
    LinesWs w{};
    size_t sort_tmp = 0, scan32 = 0, scan64 = 0;
    (void)rocprim::radix_sort_keys(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n_hits, 0u, 62u);
    (void)rocprim::exclusive_scan(nullptr, scan32, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, (size_t)n_hits + 1,
                                  rocprim::plus<int32_t>());
    (void)rocprim::exclusive_scan(nullptr, scan64, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)n + 1,
                                  rocprim::plus<int64_t>());
    w.tmp_bytes = pad256(sort_tmp > scan32 ? (sort_tmp > scan64 ? sort_tmp : scan64) : (scan32 > scan64 ? scan32 : scan64));
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.keys_a = take((size_t)n_hits * 8);
    w.keys_b = take((size_t)n_hits * 8);
    w.head = take(((size_t)n_hits + 1) * 4);
    w.pos = take(((size_t)n_hits + 1) * 4);
    w.stored = take(((size_t)n + 1) * 8);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}

}  // namespace

size_t lines_of_hits_scratch_bytes(int32_t n, int64_t n_hits) {
    if (n <= 0 || n_hits <= 0 || n_hits > 0x7fffffff) return 0;
    return lines_ws(n, n_hits).total;
}

void hit_lines_geometry(int64_t n_hits, int n_cu, int32_t *key_grid, int32_t *flat_grid_out) {
    const int64_t tiles = (n_hits + kLocateAllTile - 1) / kLocateAllTile, cap = (int64_t)(n_cu > 0 ? n_cu : 256) * kHitLinesKeyGroupsPerCu;
    *key_grid = (int32_t)(tiles < 1 ? 1 : tiles < cap ? tiles : cap);
    *flat_grid_out = flat_grid(n_hits + 1, n_cu);
}

int launch_lines_of_hits(const int32_t *T, int32_t count, int n_cu, int32_t n, const int64_t *hit_off, const int32_t *locs, int64_t n_hits,
                         int32_t max_lines, int64_t *line_off, int32_t *lines, int32_t *line_count, void *ws, size_t ws_bytes,
                         void *stream) {
    if (n <= 0 || n_hits <= 0) return 0;
    if (n_hits > 0x7fffffff || count < 0) return (int)hipErrorInvalidValue;
    const LinesWs w = lines_ws(n, n_hits);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *base = static_cast<uint8_t *>(ws);
    uint64_t *keys_a = reinterpret_cast<uint64_t *>(base + w.keys_a), *keys_b = reinterpret_cast<uint64_t *>(base + w.keys_b);
    int32_t *head = reinterpret_cast<int32_t *>(base + w.head), *pos = reinterpret_cast<int32_t *>(base + w.pos);
    int64_t *stored = reinterpret_cast<int64_t *>(base + w.stored);
    void *tmp = base + w.tmp;
    size_t tmp_bytes = w.tmp_bytes;
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, kLineFences, n_fences);
    const int32_t line_bits = fm_bits((uint32_t)count), key_bits = fm_bits((uint32_t)n) + line_bits;
    int32_t key_grid = 1, flat = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hipLaunchKernelGGL(k_hit_line_keys, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, T, count, n_fences, shift, line_bits, hit_off, n,
                       locs, n_hits, keys_a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::radix_sort_keys(tmp, tmp_bytes, keys_a, keys_b, (size_t)n_hits, 0u, (unsigned)key_bits, st); e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_line_heads, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, keys_b, n_hits, n, line_bits, head);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, head, pos, (int32_t)0, (size_t)n_hits + 1, rocprim::plus<int32_t>(), st);
        e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_line_counts, dim3((unsigned)(((int64_t)n + 1 + kFlatBlock - 1) / kFlatBlock)), dim3(kFlatBlock), 0, st, hit_off, pos, n,
                       n_hits, max_lines, line_count, stored);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, stored, line_off, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st);
        e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_line_compact, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, keys_b, pos, hit_off, line_off, n_hits, n, line_bits,
                       max_lines, lines);
    return (int)hipGetLastError();
}

// the line table: `count` positions sorted ascending as int32 (a derailed walk of quirk Q1 may answer anything), then the lines
size_t line_table_scratch_bytes(int32_t count) {
    size_t tmp = 0;
    (void)rocprim::radix_sort_keys(nullptr, tmp, (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)(count > 0 ? count : 1));
    return pad256(tmp);
}
int launch_line_table(const int32_t *locs, int32_t count, int32_t text_len, int32_t *T, int64_t *n_lines, void *scratch, size_t scratch_bytes,
                      void *stream) {
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (count > 0) {
        if (scratch_bytes < line_table_scratch_bytes(count)) return (int)hipErrorInvalidValue;
        if (hipError_t e = rocprim::radix_sort_keys(scratch, scratch_bytes, locs, T, (size_t)count, 0u, 32u, st); e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_line_total, dim3(1), dim3(64), 0, st, T, count, text_len, n_lines);
    return (int)hipGetLastError();
}

int launch_line_bounds(const int32_t *T, int32_t count, int64_t n_lines, int32_t text_len, int n_cu, const int32_t *ids, int32_t n,
                       int32_t *start, int32_t *stop, void *stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_line_bounds, dim3((unsigned)flat_grid(n, n_cu)), dim3(kFlatBlock), 0, static_cast<hipStream_t>(stream), T, count,
                       n_lines, text_len, ids, n, start, stop);
    return (int)hipGetLastError();
}

}  // namespace fmx
