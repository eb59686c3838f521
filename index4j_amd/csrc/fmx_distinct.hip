// fmx_distinct.hip — THE DISTINCT VALUES OF A FIELD PER BUCKET OF LINES (fmx_values_distinct_histogram_dev; fmx_distinct.hpp has
// the definitions): "dc(field) over time" and "values seen for the first time" off the groups the values stage gave the kept hits.
// n * B pairs of ints are the answer, whatever the number of groups is; no group's text is looked at.
//
// Lanes go to slots and counters, never to patterns:
//   k_dv_keys     a lane per packed slot, k_vh_keys' tile loop: its pattern (fm_hit_tile / fm_hit_tile_slice / fm_hit_pattern), its
//                 line (fm_line_of over the fences staged in LDS), its bucket (fm_hist_bucket over the edges, staged in LDS where
//                 they are at most kHistEdgesLds, searched in HBM otherwise; no edges: bucket 0, no line is looked up), the key
//                 pattern | group | bucket; a slot that is no hit, a hit in no bucket and a hit without a group get the pattern n
//   rocPRIM       ONE radix_sort_keys over the n_hits slots and the bits in use (fm_dv_key_width)
//   k_dv_heads    a lane per sorted slot: the head of a run of equal keys becomes (pattern | bucket) << 1 | not first, every other
//                 slot the pattern n
//   rocPRIM       ONE radix_sort_keys over the n_hits slots and the fm_dv_head_key_width bits in use: a few passes
//   k_dv_counts   a lane per counter (pattern, bucket): three lower bounds over all slots
// Integers only, no atomics: the result does not depend on the order the lanes run in.  LDS of k_dv_keys: 16 KiB slice + 16 KiB
// fences + 16 KiB edges, as k_vh_keys; a workgroup of 1,024 lanes is 4 of a SIMD's 8 waves: two workgroups per CU.  Nothing here
// is tuned (v1): the block sizes and the grids are the hits histogram's, and the second sort runs over every slot, not over the
// heads alone.  Nothing looks at the image, so this file is compiled once.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "fmx_distinct.hpp"
#include "fmx_hit_filter.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_dv_keys: a tile of kLocateAllTile hits per round
constexpr int kFlatBlock = 256;  // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

// T == nullptr: no edges (B = 1), every hit lies in bucket 0
__global__ __launch_bounds__(kKeyBlock) void k_dv_keys(const int32_t *__restrict__ T, int32_t count, int32_t n_fences, int32_t shift,
                                                       const int64_t *__restrict__ hit_off, int32_t n, const int32_t *__restrict__ locs,
                                                       int64_t n_hits, const int32_t *__restrict__ edges, int32_t n_edges, int32_t B,
                                                       const int64_t *__restrict__ val_off, const int32_t *__restrict__ group_of_hit,
                                                       int32_t group_bits, int32_t bucket_bits, uint64_t *__restrict__ keys) {
    __shared__ int64_t s_off[kLocateAllSlice];
    __shared__ int32_t s_fence[kLineFences];
    __shared__ int32_t s_edge[kHistEdgesLds];
    const bool binned = T != nullptr;                                 // (workgroup-uniform)
    const bool edges_in_lds = binned && n_edges <= kHistEdgesLds;     // (workgroup-uniform)
    if (binned)
        for (int32_t j = threadIdx.x; j < n_fences; j += kKeyBlock) s_fence[j] = T[(int64_t)j << shift];
    if (edges_in_lds)
        for (int32_t j = threadIdx.x; j < n_edges; j += kKeyBlock) s_edge[j] = edges[j];
    __syncthreads();
    const int32_t *edge = edges_in_lds ? s_edge : edges;
    const uint64_t no_hit = fm_dv_key(n, 0, 0, group_bits, bucket_bits);
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
            int32_t bucket = 0;
            if (binned) bucket = fm_hist_bucket(edge, n_edges, fm_line_of(T, count, s_fence, n_fences, shift, locs[t]));
            keys[t] = fm_dv_hit_key(n, p, val_off[p + 1] - val_off[p], group_of_hit[t], bucket, B, group_bits, bucket_bits);
        } else if (t < n_hits) {
            keys[t] = no_hit;
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_dv_heads(const uint64_t *__restrict__ skeys, int64_t n_hits, int32_t n, int32_t group_bits,
                                                         int32_t bucket_bits, uint64_t *__restrict__ heads) {
    for (int64_t j = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; j < n_hits; j += (int64_t)gridDim.x * kFlatBlock)
        heads[j] = fm_dv_head_of(skeys, j, n, group_bits, bucket_bits);
}

__global__ __launch_bounds__(kFlatBlock) void k_dv_counts(const uint64_t *__restrict__ heads, int64_t n_hits, int32_t n, int32_t B,
                                                          int32_t bucket_bits, int32_t *__restrict__ distinct, int32_t *__restrict__ first_seen) {
    const int64_t items = (int64_t)n * B;
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < items; i += (int64_t)gridDim.x * kFlatBlock) {
        const int32_t p = (int32_t)(i / B);
        int32_t d, f;
        fm_dv_counts(heads, n_hits, p, (int32_t)(i - (int64_t)p * B), bucket_bits, d, f);
        distinct[i] = d;
        first_seen[i] = f;
    }
}

// the regions of the caller's workspace, each a multiple of 256 bytes
struct DistinctWs {
    size_t val_off, edges, keys_a, keys_b, heads_a, heads_b, tmp, tmp_bytes, total;
};
DistinctWs distinct_ws(int32_t n, int64_t n_hits, int32_t n_edges) {
    DistinctWs w{};
    size_t key_tmp = 0;
    (void)rocprim::radix_sort_keys(nullptr, key_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n_hits, 0u, 64u);
    w.tmp_bytes = pad256(key_tmp);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.val_off = take(((size_t)n + 1) * 8);
    w.edges = take((size_t)n_edges * 4);
    w.keys_a = take((size_t)n_hits * 8);
    w.keys_b = take((size_t)n_hits * 8);
    w.heads_a = take((size_t)n_hits * 8);
    w.heads_b = take((size_t)n_hits * 8);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}
bool shape_ok(int32_t n, int64_t G, int64_t n_hits, int32_t n_edges) {
    return n > 0 && G >= 0 && G <= 0x7fffffff && n_hits > 0 && n_hits <= 0x7fffffff && (n_edges == 0 || n_edges >= 2);
}

}  // namespace

size_t values_distinct_histogram_scratch_bytes(int32_t n, int64_t n_groups, int64_t n_hits, int32_t n_edges) {
    return shape_ok(n, n_groups, n_hits, n_edges) ? distinct_ws(n, n_hits, n_edges).total : 0;
}

int launch_values_distinct_histogram(const int32_t *T, int32_t count, int n_cu, int32_t n, const int64_t *val_off, const int32_t *edges,
                                     int32_t n_edges, const int64_t *hit_off, const int32_t *locs, int64_t n_hits, const int32_t *group_of_hit,
                                     int32_t *distinct, int32_t *first_seen, void *ws, size_t ws_bytes, void *stream) {
    if (n <= 0 || n_hits <= 0) return 0;
    const int32_t B = n_edges > 0 ? n_edges - 1 : 1;
    if (!val_off || !shape_ok(n, val_off[n], n_hits, n_edges) || (n_edges > 0 && (!T || count < 0 || fm_hist_edges_bad(edges, n_edges))))
        return (int)hipErrorInvalidValue;
    int64_t max_groups = 0;
    if (fm_dv_shape_bad(n, val_off, B, &max_groups)) return (int)hipErrorInvalidValue;
    const DistinctWs w = distinct_ws(n, n_hits, n_edges);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *base = static_cast<uint8_t *>(ws);
    int64_t *d_val_off = reinterpret_cast<int64_t *>(base + w.val_off);
    int32_t *d_edges = reinterpret_cast<int32_t *>(base + w.edges);
    uint64_t *keys_a = reinterpret_cast<uint64_t *>(base + w.keys_a), *keys_b = reinterpret_cast<uint64_t *>(base + w.keys_b);
    uint64_t *heads_a = reinterpret_cast<uint64_t *>(base + w.heads_a), *heads_b = reinterpret_cast<uint64_t *>(base + w.heads_b);
    void *tmp = base + w.tmp;
    // (the runtime has read the host arrays when a copy returns: a copy from pageable host memory is staged before the call comes back)
    if (hipError_t e = hipMemcpyAsync(d_val_off, val_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    if (n_edges > 0)
        if (hipError_t e = hipMemcpyAsync(d_edges, edges, (size_t)n_edges * 4, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    int32_t unused = 1, key_grid = 1, slot_grid = 1, count_grid = 1;
    int32_t n_fences = 0;
    const int32_t shift = n_edges > 0 ? fm_line_fence_shift(count, kLineFences, n_fences) : 0;
    const int32_t group_bits = fm_bits((uint32_t)max_groups), bucket_bits = fm_bits((uint32_t)B);
    hit_lines_geometry(n_hits, n_cu, &key_grid, &slot_grid);
    hit_lines_geometry((int64_t)n * B, n_cu, &unused, &count_grid);
    hipLaunchKernelGGL(k_dv_keys, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, n_edges > 0 ? T : nullptr, count, n_fences, shift, hit_off, n,
                       locs, n_hits, d_edges, n_edges, B, d_val_off, group_of_hit, group_bits, bucket_bits, keys_a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    size_t tmp_bytes = w.tmp_bytes;
    if (hipError_t e = rocprim::radix_sort_keys(tmp, tmp_bytes, keys_a, keys_b, (size_t)n_hits, 0u, (unsigned)fm_dv_key_width(n, max_groups, B), st);
        e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_dv_heads, dim3((unsigned)slot_grid), dim3(kFlatBlock), 0, st, keys_b, n_hits, n, group_bits, bucket_bits, heads_a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    tmp_bytes = w.tmp_bytes;
    if (hipError_t e = rocprim::radix_sort_keys(tmp, tmp_bytes, heads_a, heads_b, (size_t)n_hits, 0u, (unsigned)fm_dv_head_key_width(n, B), st);
        e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_dv_counts, dim3((unsigned)count_grid), dim3(kFlatBlock), 0, st, heads_b, n_hits, n, B, bucket_bits, distinct, first_seen);
    return (int)hipGetLastError();
}

}  // namespace fmx
