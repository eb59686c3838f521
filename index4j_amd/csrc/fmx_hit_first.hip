// fmx_hit_first.hip — packed hits -> THE FIRST HIT OF EVERY LINE (fmx_first_hits_of_lines_dev; fmx_hit_by.hpp has the definition and
// the per-item functions): per pattern its distinct lines ascending, each with the smallest text position of a hit on it.  It is the
// join of "stats ... by key": the key of a line is the value behind that hit, and a number hit of the same line finds it by one
// lower bound in these lines.
//
// Every stage hands lanes to HITS, never to patterns:
//   k_first_keys    a lane per packed slot: its pattern (fm_hit_pattern over an LDS slice of hit_off: fm_hit_tile /
//                   fm_hit_tile_slice, as k_hit_line_keys) and the key (pattern << pos_bits) | position; a slot in front of
//                   hit_off[0] or behind hit_off[m] gets the pattern m, which sorts last
//   rocPRIM         ONE device-wide radix sort of the keys over the bits in use: the hits of pattern p then lie at
//                   [hit_off[p], hit_off[p + 1]) - hit_off[0], ascending by position, so their lines never decrease
//   k_first_lines   a lane per sorted slot: its line (fm_line_of: the first levels over the fences staged in LDS)
//   k_first_heads   1 where a sorted hit's pattern or line differs from its predecessor's; rocPRIM's exclusive scan numbers the
//                   (pattern, line) pairs
//   k_first_store   a head stores its line and its position; a lane per pattern reads first_off off the scan
// No atomics: the result does not depend on the order the lanes run in.  Nothing here looks at the image, so this file is compiled
// once, like fmx_hit_lines.hip.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fmx_hit_by.hpp"
#include "fmx_hit_filter.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_first_keys (the slice, 16 KiB) and k_first_lines (the fences, 16 KiB)
constexpr int kFlatBlock = 256;  // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

__global__ __launch_bounds__(kKeyBlock) void k_first_keys(const int64_t *__restrict__ hit_off, int32_t m, const int32_t *__restrict__ locs,
                                                          int64_t n_hits, int32_t pos_bits, uint64_t *__restrict__ keys) {
    __shared__ int64_t s_off[kLocateAllSlice];
    const uint64_t no_hit = fm_first_key(m, 0, pos_bits);
    const int64_t first = fm_filter_slot(hit_off[0], n_hits), total = fm_filter_slot(hit_off[m], n_hits);
    for (int64_t tile = (int64_t)blockIdx.x * kLocateAllTile; tile < n_hits; tile += (int64_t)gridDim.x * kLocateAllTile) {
        const int64_t t = tile + threadIdx.x;
        if (tile >= total || tile + kLocateAllTile <= first) {  // a tile of slots behind or in front of the hits (workgroup-uniform)
            if (t < n_hits) keys[t] = no_hit;
            continue;
        }
        const HitTile h = fm_hit_tile(hit_off, m, tile, total);
        bool in_lds;
        const int64_t *slice = fm_hit_tile_slice<kKeyBlock>(s_off, hit_off, h, in_lds);
        if (t >= first && t <= h.tile_last)
            keys[t] = fm_first_key(h.p_lo + fm_hit_pattern(slice, h.slice_count, t), locs[t], pos_bits);
        else if (t < n_hits)
            keys[t] = no_hit;
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

__global__ __launch_bounds__(kKeyBlock) void k_first_lines(const int32_t *__restrict__ T, int32_t count, int32_t n_fences, int32_t shift,
                                                           const uint64_t *__restrict__ keys, int64_t n_hits, int32_t m, int32_t pos_bits,
                                                           int32_t *__restrict__ line_of) {
    __shared__ int32_t s_fence[kLineFences];
    for (int32_t j = threadIdx.x; j < n_fences; j += kKeyBlock) s_fence[j] = T[(int64_t)j << shift];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kKeyBlock + threadIdx.x; i < n_hits; i += (int64_t)gridDim.x * kKeyBlock) {
        const uint64_t key = keys[i];
        line_of[i] = fm_first_key_pattern(key, pos_bits) < m ? fm_line_of(T, count, s_fence, n_fences, shift, fm_first_key_loc(key, pos_bits)) : 0;
    }
}

// head[i] for the sorted slots, and head[n_hits] = 0: the exclusive scan then leaves the number of all pairs there
__global__ __launch_bounds__(kFlatBlock) void k_first_heads(const uint64_t *__restrict__ keys, const int32_t *__restrict__ line_of,
                                                            int64_t n_hits, int32_t m, int32_t pos_bits, int32_t *__restrict__ head) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i <= n_hits; i += (int64_t)gridDim.x * kFlatBlock)
        head[i] = i < n_hits && fm_first_head(keys, line_of, i, m, pos_bits) ? 1 : 0;
}

// pos = the exclusive scan of head.  The sorted slots of pattern p are [slot(hit_off[p]), slot(hit_off[p + 1])) - slot(hit_off[0]).
__global__ __launch_bounds__(kFlatBlock) void k_first_store(const uint64_t *__restrict__ keys, const int32_t *__restrict__ line_of,
                                                            const int32_t *__restrict__ head, const int32_t *__restrict__ pos,
                                                            const int64_t *__restrict__ hit_off, int64_t n_hits, int32_t m, int32_t pos_bits,
                                                            int64_t *__restrict__ first_off, int32_t *__restrict__ first_lines,
                                                            int32_t *__restrict__ first_locs) {
    const int64_t lane = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x, lanes = (int64_t)gridDim.x * kFlatBlock;
    for (int64_t i = lane; i < n_hits; i += lanes)
        if (head[i]) {
            first_lines[pos[i]] = line_of[i];
            first_locs[pos[i]] = fm_first_key_loc(keys[i], pos_bits);
        }
    const int64_t first = fm_filter_slot(hit_off[0], n_hits);
    for (int64_t p = lane; p <= m; p += lanes) {
        const int64_t at = fm_filter_slot(hit_off[p], n_hits);
        first_off[p] = pos[(at < first ? first : at) - first];
    }
}

// the regions of the caller's workspace, each a multiple of 256 bytes
struct FirstWs {
    size_t keys_a, keys_b, line_of, head, pos, tmp, tmp_bytes, total;
};
FirstWs first_ws(int64_t n_hits) {
    FirstWs w{};
    const size_t H = (size_t)n_hits;
    size_t sort_tmp = 0, scan32 = 0;
    (void)rocprim::radix_sort_keys(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, H, 0u, 63u);
    (void)rocprim::exclusive_scan(nullptr, scan32, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, H + 1, rocprim::plus<int32_t>());
    w.tmp_bytes = pad256(sort_tmp > scan32 ? sort_tmp : scan32);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.keys_a = take(H * 8);
    w.keys_b = take(H * 8);
    w.line_of = take(H * 4);
    w.head = take((H + 1) * 4);
    w.pos = take((H + 1) * 4);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}

}  // namespace

size_t first_hits_scratch_bytes(int32_t m, int64_t n_hits) {
    if (m <= 0 || n_hits <= 0 || n_hits > 0x7fffffff) return 0;
    return first_ws(n_hits).total;
}

int launch_first_hits(const int32_t *T, int32_t count, int32_t text_len, int n_cu, int32_t m, const int64_t *hit_off, const int32_t *locs,
                      int64_t n_hits, int64_t *first_off, int32_t *first_lines, int32_t *first_locs, void *ws, size_t ws_bytes, void *stream) {
    if (m <= 0 || n_hits <= 0 || n_hits > 0x7fffffff || count < 0 || text_len < 0 || !T) return (int)hipErrorInvalidValue;
    const FirstWs w = first_ws(n_hits);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *base = static_cast<uint8_t *>(ws);
    uint64_t *keys_a = reinterpret_cast<uint64_t *>(base + w.keys_a), *keys_b = reinterpret_cast<uint64_t *>(base + w.keys_b);
    int32_t *line_of = reinterpret_cast<int32_t *>(base + w.line_of), *head = reinterpret_cast<int32_t *>(base + w.head);
    int32_t *pos = reinterpret_cast<int32_t *>(base + w.pos);
    void *tmp = base + w.tmp;
    size_t tmp_bytes = w.tmp_bytes;
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, kLineFences, n_fences);
    const int32_t pos_bits = fm_bits((uint32_t)text_len), key_bits = fm_bits((uint32_t)m) + pos_bits;
    int32_t key_grid = 1, flat = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
#define FMX_FIRST_CHECK(call) \
    if (hipError_t e_ = (call); e_ != hipSuccess) return (int)e_
    hipLaunchKernelGGL(k_first_keys, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, hit_off, m, locs, n_hits, pos_bits, keys_a);
    FMX_FIRST_CHECK(hipGetLastError());
    FMX_FIRST_CHECK(rocprim::radix_sort_keys(tmp, tmp_bytes, keys_a, keys_b, (size_t)n_hits, 0u, (unsigned)key_bits, st));
    hipLaunchKernelGGL(k_first_lines, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, T, count, n_fences, shift, keys_b, n_hits, m, pos_bits,
                       line_of);
    FMX_FIRST_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_first_heads, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, keys_b, line_of, n_hits, m, pos_bits, head);
    FMX_FIRST_CHECK(hipGetLastError());
    FMX_FIRST_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, head, pos, (int32_t)0, (size_t)n_hits + 1, rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(k_first_store, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, keys_b, line_of, head, pos, hit_off, n_hits, m, pos_bits,
                       first_off, first_lines, first_locs);
#undef FMX_FIRST_CHECK
    return (int)hipGetLastError();
}

}  // namespace fmx
