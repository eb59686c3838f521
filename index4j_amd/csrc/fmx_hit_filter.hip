// fmx_hit_filter.hip — packed hits -> THE PACKED HITS THAT LIE IN GIVEN LINES (fmx_hits_in_lines_dev; fmx_hit_filter.hpp has the keep
// rule): the stage that lets the line, sequence and values stages run on "the hits of pattern i inside the lines of query w and
// inside a window of lines" — count by block id WHERE the line holds `terminating`.  The output is the packed format the input has.
//
// Every stage hands lanes to HITS, never to patterns:
//   k_hit_keep_flags  a lane per packed slot: its pattern (fm_hit_pattern over an LDS slice of hit_off: fm_hit_tile /
//                     fm_hit_tile_slice, as k_hit_line_keys), its line (fm_line_of: the first levels over the fences staged in LDS),
//                     the window, ONE lower bound in the line list of the pattern's query; flag 1 = kept.  Slots in front of
//                     hit_off[0] and behind hit_off[n] get 0.
//   rocPRIM           the exclusive scan of the flags: where each kept hit goes — the order they had
//   k_hit_keep_store  a lane per slot stores a kept hit; a lane per pattern reads kept_off off the scan (launch_hit_keep_store: also
//                     the store of fmx_hit_range.hip, which makes its flags from the number behind a hit)
// Integers only, no atomics: the result does not depend on the order the lanes run in.  Nothing here looks at the image, so this
// file is compiled once.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "fmx_hit_filter.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_hit_keep_flags: a tile of kLocateAllTile hits per round, 32 KiB of LDS: two workgroups per CU
constexpr int kFlatBlock = 256;  // the element-wise kernel
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

// T == nullptr: no line table and nothing to filter by (the launcher has seen to that) — every hit is kept
__global__ __launch_bounds__(kKeyBlock) void k_hit_keep_flags(const int32_t *__restrict__ T, int32_t count, int32_t n_fences, int32_t shift,
                                                              const int64_t *__restrict__ hit_off, int32_t n,
                                                              const int32_t *__restrict__ locs, int64_t n_hits,
                                                              const int32_t *__restrict__ where_of, const int64_t *__restrict__ line_off,
                                                              const int32_t *__restrict__ lines, int32_t line_lo, int32_t line_hi,
                                                              int32_t *__restrict__ flag) {
    __shared__ int64_t s_off[kLocateAllSlice];
    __shared__ int32_t s_fence[kLineFences];
    for (int32_t j = threadIdx.x; j < n_fences; j += kKeyBlock) s_fence[j] = T[(int64_t)j << shift];
    __syncthreads();
    const int64_t first = fm_filter_slot(hit_off[0], n_hits), total = fm_filter_slot(hit_off[n], n_hits);
    if (blockIdx.x == 0 && threadIdx.x == 0) flag[n_hits] = 0;  // (the scan then leaves the number of kept hits there)
    for (int64_t tile = (int64_t)blockIdx.x * kLocateAllTile; tile < n_hits; tile += (int64_t)gridDim.x * kLocateAllTile) {
        const int64_t t = tile + threadIdx.x;
        if (tile >= total || tile + kLocateAllTile <= first) {  // a tile of slots behind or in front of the hits (workgroup-uniform)
            if (t < n_hits) flag[t] = 0;
            continue;
        }
        const HitTile h = fm_hit_tile(hit_off, n, tile, total);
        bool in_lds;
        const int64_t *slice = fm_hit_tile_slice<kKeyBlock>(s_off, hit_off, h, in_lds);
        if (t >= first && t <= h.tile_last) {
            bool keep = true;
            if (T) {
                const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
                keep = fm_filter_keep(fm_line_of(T, count, s_fence, n_fences, shift, locs[t]), line_lo, line_hi, where_of[p], line_off, lines);
            }
            flag[t] = keep ? 1 : 0;
        } else if (t < n_hits) {
            flag[t] = 0;
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

// pos = the exclusive scan of flag (n_hits + 1 entries)
__global__ __launch_bounds__(kFlatBlock) void k_hit_keep_store(const int32_t *__restrict__ flag, const int32_t *__restrict__ pos,
                                                               const int64_t *__restrict__ hit_off, int32_t n,
                                                               const int32_t *__restrict__ locs, int64_t n_hits,
                                                               int64_t *__restrict__ kept_off, int32_t *__restrict__ kept_locs) {
    const int64_t lane = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x, lanes = (int64_t)gridDim.x * kFlatBlock;
    for (int64_t i = lane; i < n_hits; i += lanes)
        if (flag[i]) kept_locs[pos[i]] = locs[i];
    for (int64_t p = lane; p <= n; p += lanes) kept_off[p] = fm_filter_kept_off(hit_off, pos, n_hits, (int32_t)p);
}

// the regions of the caller's workspace, each a multiple of 256 bytes
struct FilterWs {
    size_t where_of, flag, pos, tmp, tmp_bytes, total;
};
FilterWs filter_ws(int32_t n, int64_t n_hits) {
    FilterWs w{};
    size_t scan32 = 0;
    (void)rocprim::exclusive_scan(nullptr, scan32, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, (size_t)n_hits + 1,
                                  rocprim::plus<int32_t>());
    w.tmp_bytes = pad256(scan32);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.where_of = take((size_t)n * 4);
    w.flag = take(((size_t)n_hits + 1) * 4);
    w.pos = take(((size_t)n_hits + 1) * 4);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}

}  // namespace

size_t hits_in_lines_scratch_bytes(int32_t n, int64_t n_hits) {
    if (n <= 0 || n_hits <= 0 || n_hits > 0x7fffffff) return 0;
    return filter_ws(n, n_hits).total;
}

int launch_hits_in_lines(const int32_t *T, int32_t count, int n_cu, int32_t n, const int32_t *where_of, const int64_t *line_off,
                         const int32_t *lines, int32_t line_lo, int32_t line_hi, const int64_t *hit_off, const int32_t *locs, int64_t n_hits,
                         int64_t *kept_off, int32_t *kept_locs, void *ws, size_t ws_bytes, void *stream) {
    if (n <= 0 || n_hits <= 0) return 0;
    if (n_hits > 0x7fffffff || count < 0) return (int)hipErrorInvalidValue;
    const FilterWs w = filter_ws(n, n_hits);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *base = static_cast<uint8_t *>(ws);
    int32_t *d_where = reinterpret_cast<int32_t *>(base + w.where_of);
    int32_t *flag = reinterpret_cast<int32_t *>(base + w.flag), *pos = reinterpret_cast<int32_t *>(base + w.pos);
    void *tmp = base + w.tmp;
    size_t tmp_bytes = w.tmp_bytes;
    // (the runtime has read where_of when the copy returns: a copy from pageable host memory is staged before the call comes back)
    if (hipError_t e = hipMemcpyAsync(d_where, where_of, (size_t)n * 4, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    int32_t n_fences = 0;
    const int32_t shift = T ? fm_line_fence_shift(count, kLineFences, n_fences) : 0;
    int32_t key_grid = 1, flat = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hipLaunchKernelGGL(k_hit_keep_flags, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, T, count, n_fences, shift, hit_off, n, locs, n_hits,
                       d_where, line_off, lines, line_lo, line_hi, flag);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, flag, pos, (int32_t)0, (size_t)n_hits + 1, rocprim::plus<int32_t>(), st);
        e != hipSuccess)
        return (int)e;
    return launch_hit_keep_store(flat, flag, pos, hit_off, n, locs, n_hits, kept_off, kept_locs, stream);
}

int launch_hit_keep_store(int32_t flat_grid, const int32_t *flag, const int32_t *pos, const int64_t *hit_off, int32_t n, const int32_t *locs,
                          int64_t n_hits, int64_t *kept_off, int32_t *kept_locs, void *stream) {
    hipLaunchKernelGGL(k_hit_keep_store, dim3((unsigned)flat_grid), dim3(kFlatBlock), 0, static_cast<hipStream_t>(stream), flag, pos, hit_off, n,
                       locs, n_hits, kept_off, kept_locs);
    return (int)hipGetLastError();
}

}  // namespace fmx
