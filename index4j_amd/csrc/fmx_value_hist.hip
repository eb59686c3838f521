// fmx_value_hist.hip — THE TOP VALUES OF A FIELD PER BUCKET OF LINES (fmx_values_top_histogram_dev, fmx_values_gather_rows_dev;
// fmx_value_hist.hpp has the definitions): the stacked timeline of a log search — the groups of the values stage ranked by count on
// the device, the kept hits binned by (pattern, rank, bucket), and the text of the selected groups alone gathered for the way down.
//
// Lanes go to groups, slots, counters or code units, never to patterns:
//   k_vh_rank_keys   a lane per group: its pattern (fm_hit_pattern over val_off) and the key pattern | INT32_MAX - count; the
//                    payload is the group's index
//   rocPRIM          ONE stable radix_sort_pairs over the G groups and the bits in use, 31 + fm_bits(n)
//   k_vh_ranks       a lane per sorted group: rank_of_group = min(sorted index - val_off[pattern], top); a rank below top also stores
//                    the row's group and count
//   k_vh_keys        a lane per packed slot, k_hist_keys' tile loop: its pattern (fm_hit_tile / fm_hit_tile_slice / fm_hit_pattern),
//                    its line (fm_line_of over the fences staged in LDS), its bucket (fm_hist_bucket over the edges, staged in LDS
//                    where they are at most kHistEdgesLds, searched in HBM otherwise; no edges: bucket 0, no line is looked up),
//                    its code (the rank of its group), the key pattern | code | bucket; a slot that is no hit gets the pattern n
//   rocPRIM          ONE radix_sort_keys over the n_hits slots and the bits in use (fm_vh_key_width)
//   k_vh_counts      a lane per counter, (row, bucket) or (pattern, other, bucket): two lower bounds inside its pattern's slots
// and for the text of the rows (fmx_values_gather_rows_dev):
//   k_vh_row_lengths a lane per row: the length of its group's text; rocPRIM: an exclusive scan over R + 1
//   k_vh_row_sources a lane per row: the group its text comes from
//   k_vh_gather      a lane per code unit of the packed rows: its row (one search in the scanned offsets), one unit copied
// Integers only, no atomics: the result does not depend on the order the lanes run in.  LDS of k_vh_keys: 16 KiB slice + 16 KiB
// fences + 16 KiB edges, as k_hist_keys: three workgroups per CU.  Nothing here is tuned (v1): the block sizes and the grids are
// the hits histogram's.  Nothing looks at the image, so this file is compiled once.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fmx_hit_filter.hpp"
#include "fmx_plan.hpp"
#include "fmx_value_hist.hpp"

#include <vector>

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_vh_keys: a tile of kLocateAllTile hits per round
constexpr int kFlatBlock = 256;  // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

__global__ __launch_bounds__(kFlatBlock) void k_vh_rank_keys(const int64_t *__restrict__ val_off, int32_t n, const int32_t *__restrict__ count,
                                                             int64_t G, uint64_t *__restrict__ keys, uint32_t *__restrict__ group) {
    for (int64_t g = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; g < G; g += (int64_t)gridDim.x * kFlatBlock) {
        const int32_t c = count[g];
        keys[g] = fm_vh_rank_key(fm_hit_pattern(val_off, n, g), c < 0 ? 0 : c);
        group[g] = (uint32_t)g;
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_vh_ranks(const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ sgroup,
                                                         const int64_t *__restrict__ val_off, const int64_t *__restrict__ row_off, int64_t G,
                                                         int32_t top, int32_t *__restrict__ rank_of_group, int32_t *__restrict__ row_group,
                                                         int32_t *__restrict__ row_count) {
    for (int64_t j = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; j < G; j += (int64_t)gridDim.x * kFlatBlock) {
        const uint64_t key = skeys[j];
        const int32_t p = fm_vh_rank_key_pattern(key);
        const int64_t g = sgroup[j], first = val_off[p];
        const int32_t rank = fm_vh_rank(j, first, top);
        rank_of_group[g] = rank;
        if (rank < top) {
            const int64_t row = row_off[p] + rank;
            row_group[row] = (int32_t)(g - first);
            row_count[row] = fm_vh_rank_key_count(key);
        }
    }
}

// T == nullptr: no edges (B = 1), every hit lies in bucket 0
__global__ __launch_bounds__(kKeyBlock) void k_vh_keys(const int32_t *__restrict__ T, int32_t count, int32_t n_fences, int32_t shift,
                                                       const int64_t *__restrict__ hit_off, int32_t n, const int32_t *__restrict__ locs,
                                                       int64_t n_hits, const int32_t *__restrict__ edges, int32_t n_edges,
                                                       const int64_t *__restrict__ val_off, const int32_t *__restrict__ rank_of_group,
                                                       const int32_t *__restrict__ group_of_hit, int32_t top, int32_t code_bits,
                                                       int32_t bucket_bits, uint64_t *__restrict__ keys) {
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
    const uint64_t no_hit = fm_vh_key(n, 0, 0, code_bits, bucket_bits);
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
            const int64_t g0 = val_off[p];
            keys[t] = fm_vh_key(p, fm_vh_code(rank_of_group, g0, val_off[p + 1] - g0, group_of_hit[t], top), bucket, code_bits, bucket_bits);
        } else if (t < n_hits) {
            keys[t] = no_hit;
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_vh_counts(const uint64_t *__restrict__ keys, const int64_t *__restrict__ hit_off, int32_t n,
                                                          int64_t n_hits, const int64_t *__restrict__ row_off, int64_t R, int32_t B, int32_t top,
                                                          int32_t code_bits, int32_t bucket_bits, int32_t *__restrict__ hist,
                                                          int32_t *__restrict__ other) {
    const int64_t items = (R + n) * B, first = fm_filter_slot(hit_off[0], n_hits);
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < items; i += (int64_t)gridDim.x * kFlatBlock) {
        int32_t p, code, b;
        fm_vh_counter(row_off, n, R, B, top, i, p, code, b);
        const int32_t c = fm_vh_count(keys, hit_off, n_hits, first, p, code, b, code_bits, bucket_bits);
        if (i < R * B)
            hist[i] = c;
        else
            other[i - R * B] = c;
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_vh_row_lengths(const int64_t *__restrict__ row_src, const int64_t *__restrict__ text_off, int64_t R,
                                                               int64_t *__restrict__ len) {
    for (int64_t r = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; r <= R; r += (int64_t)gridDim.x * kFlatBlock)
        len[r] = r < R ? text_off[row_src[r] + 1] - text_off[row_src[r]] : 0;
}

__global__ __launch_bounds__(kFlatBlock) void k_vh_gather(const int64_t *__restrict__ row_src, const int64_t *__restrict__ text_off,
                                                          const uint16_t *__restrict__ chars, int64_t R, const int64_t *__restrict__ row_text_off,
                                                          uint16_t *__restrict__ row_chars) {
    const int64_t units = row_text_off[R];
    for (int64_t u = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; u < units; u += (int64_t)gridDim.x * kFlatBlock) {
        const int64_t r = fm_vh_unit_row(row_text_off, R, u);
        row_chars[u] = chars[text_off[row_src[r]] + (u - row_text_off[r])];
    }
}

// a lane per row: the group a row's text comes from, val_off[pattern] + row_group
__global__ __launch_bounds__(kFlatBlock) void k_vh_row_sources(const int64_t *__restrict__ val_off, const int64_t *__restrict__ row_off, int32_t n,
                                                               const int32_t *__restrict__ row_group, int64_t R, int64_t *__restrict__ row_src) {
    for (int64_t r = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; r < R; r += (int64_t)gridDim.x * kFlatBlock)
        row_src[r] = val_off[fm_hit_pattern(row_off, n, r)] + row_group[r];
}

// one lane: the code units of all groups' text, text_off[val_off[n]], where the host reads it with the group offsets
__global__ void k_vh_units(const int64_t *__restrict__ val_off, int32_t n, const int64_t *__restrict__ text_off, int64_t *__restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = text_off[val_off[n]];
}

// the regions of the caller's workspace, each a multiple of 256 bytes
struct ValueHistWs {
    size_t val_off, row_off, edges, rank_keys_a, rank_keys_b, group_a, group_b, rank_of_group, keys_a, keys_b, tmp, tmp_bytes, total;
};
ValueHistWs value_hist_ws(int32_t n, int64_t G, int64_t n_hits, int32_t n_edges) {
    ValueHistWs w{};
    size_t rank_tmp = 0, key_tmp = 0;
    (void)rocprim::radix_sort_pairs(nullptr, rank_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                    (uint32_t *)nullptr, (size_t)G, 0u, 62u);
    (void)rocprim::radix_sort_keys(nullptr, key_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n_hits, 0u, 64u);
    w.tmp_bytes = pad256(rank_tmp > key_tmp ? rank_tmp : key_tmp);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.val_off = take(((size_t)n + 1) * 8);
    w.row_off = take(((size_t)n + 1) * 8);
    w.edges = take((size_t)n_edges * 4);
    w.rank_keys_a = take((size_t)G * 8);
    w.rank_keys_b = take((size_t)G * 8);
    w.group_a = take((size_t)G * 4);
    w.group_b = take((size_t)G * 4);
    w.rank_of_group = take((size_t)G * 4);
    w.keys_a = take((size_t)n_hits * 8);
    w.keys_b = take((size_t)n_hits * 8);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}
bool shape_ok(int32_t n, int64_t G, int64_t n_hits, int32_t n_edges) {
    return n > 0 && G >= 0 && G <= 0x7fffffff && n_hits > 0 && n_hits <= 0x7fffffff && (n_edges == 0 || n_edges >= 2);
}

struct GatherWs {
    size_t val_off, row_off, src, len, tmp, tmp_bytes, total;
};
GatherWs gather_ws(int32_t n, int64_t R) {
    GatherWs w{};
    size_t scan_tmp = 0;
    (void)rocprim::exclusive_scan(nullptr, scan_tmp, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)R + 1, rocprim::plus<int64_t>());
    w.tmp_bytes = pad256(scan_tmp);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.val_off = take(((size_t)n + 1) * 8);
    w.row_off = take(((size_t)n + 1) * 8);
    w.src = take((size_t)R * 8);
    w.len = take(((size_t)R + 1) * 8);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}

}  // namespace

size_t values_top_histogram_scratch_bytes(int32_t n, int64_t n_groups, int64_t n_hits, int32_t n_edges) {
    return shape_ok(n, n_groups, n_hits, n_edges) ? value_hist_ws(n, n_groups, n_hits, n_edges).total : 0;
}

int launch_values_top_histogram(const int32_t *T, int32_t count, int n_cu, int32_t n, const int64_t *val_off, int32_t top, const int32_t *edges,
                                int32_t n_edges, const int64_t *hit_off, const int32_t *locs, int64_t n_hits, const int32_t *group_count,
                                const int32_t *group_of_hit, int64_t *row_off_out, int32_t *row_group, int32_t *row_count, int32_t *hist,
                                int32_t *other, void *ws, size_t ws_bytes, void *stream) {
    if (n <= 0 || n_hits <= 0) return 0;
    const int32_t B = n_edges > 0 ? n_edges - 1 : 1;
    if (!val_off || !shape_ok(n, val_off[n], n_hits, n_edges) || (n_edges > 0 && (!T || count < 0 || fm_hist_edges_bad(edges, n_edges))))
        return (int)hipErrorInvalidValue;
    std::vector<int64_t> row_off((size_t)n + 1, 0);
    if (fm_vh_shape_bad(n, val_off, top, B, row_off.data())) return (int)hipErrorInvalidValue;
    const int64_t G = val_off[n], R = row_off[(size_t)n];
    const ValueHistWs w = value_hist_ws(n, G, n_hits, n_edges);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *base = static_cast<uint8_t *>(ws);
    int64_t *d_val_off = reinterpret_cast<int64_t *>(base + w.val_off), *d_row_off = reinterpret_cast<int64_t *>(base + w.row_off);
    int32_t *d_edges = reinterpret_cast<int32_t *>(base + w.edges), *rank_of_group = reinterpret_cast<int32_t *>(base + w.rank_of_group);
    uint64_t *rank_a = reinterpret_cast<uint64_t *>(base + w.rank_keys_a), *rank_b = reinterpret_cast<uint64_t *>(base + w.rank_keys_b);
    uint32_t *group_a = reinterpret_cast<uint32_t *>(base + w.group_a), *group_b = reinterpret_cast<uint32_t *>(base + w.group_b);
    uint64_t *keys_a = reinterpret_cast<uint64_t *>(base + w.keys_a), *keys_b = reinterpret_cast<uint64_t *>(base + w.keys_b);
    void *tmp = base + w.tmp;
    size_t tmp_bytes = w.tmp_bytes;
    // (the runtime has read the host arrays when a copy returns: a copy from pageable host memory is staged before the call comes back;
    // row_off is this function's own vector, so its two copies are waited for by the same rule)
    const size_t off_bytes = ((size_t)n + 1) * 8;
    if (hipError_t e = hipMemcpyAsync(d_val_off, val_off, off_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    if (hipError_t e = hipMemcpyAsync(d_row_off, row_off.data(), off_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    if (hipError_t e = hipMemcpyAsync(row_off_out, row_off.data(), off_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    if (n_edges > 0)
        if (hipError_t e = hipMemcpyAsync(d_edges, edges, (size_t)n_edges * 4, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    int32_t unused = 1, group_grid = 1, key_grid = 1, count_grid = 1;
    if (G > 0) {
        hit_lines_geometry(G, n_cu, &unused, &group_grid);
        hipLaunchKernelGGL(k_vh_rank_keys, dim3((unsigned)group_grid), dim3(kFlatBlock), 0, st, d_val_off, n, group_count, G, rank_a, group_a);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
        if (hipError_t e = rocprim::radix_sort_pairs(tmp, tmp_bytes, rank_a, rank_b, group_a, group_b, (size_t)G, 0u,
                                                     (unsigned)fm_vh_rank_key_width(n), st);
            e != hipSuccess)
            return (int)e;
        hipLaunchKernelGGL(k_vh_ranks, dim3((unsigned)group_grid), dim3(kFlatBlock), 0, st, rank_b, group_b, d_val_off, d_row_off, G, top,
                           rank_of_group, row_group, row_count);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    }
    int32_t n_fences = 0;
    const int32_t shift = n_edges > 0 ? fm_line_fence_shift(count, kLineFences, n_fences) : 0;
    const int32_t code_bits = fm_bits((uint32_t)top), bucket_bits = fm_bits((uint32_t)B), key_bits = fm_vh_key_width(n, top, B);
    hit_lines_geometry(n_hits, n_cu, &key_grid, &unused);
    hit_lines_geometry((R + n) * B, n_cu, &unused, &count_grid);
    hipLaunchKernelGGL(k_vh_keys, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, n_edges > 0 ? T : nullptr, count, n_fences, shift, hit_off, n,
                       locs, n_hits, d_edges, n_edges, d_val_off, rank_of_group, group_of_hit, top, code_bits, bucket_bits, keys_a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    tmp_bytes = w.tmp_bytes;
    if (hipError_t e = rocprim::radix_sort_keys(tmp, tmp_bytes, keys_a, keys_b, (size_t)n_hits, 0u, (unsigned)key_bits, st); e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_vh_counts, dim3((unsigned)count_grid), dim3(kFlatBlock), 0, st, keys_b, hit_off, n, n_hits, d_row_off, R, B, top, code_bits,
                       bucket_bits, hist, other);
    return (int)hipGetLastError();
}

int launch_values_groups_units(const int64_t *val_off, int32_t n, const int64_t *text_off, int64_t *out, void *stream) {
    hipLaunchKernelGGL(k_vh_units, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), val_off, n, text_off, out);
    return (int)hipGetLastError();
}

size_t values_gather_rows_scratch_bytes(int32_t n, int64_t n_rows) {
    return n > 0 && n_rows > 0 && n_rows <= kHistCellsMax ? gather_ws(n, n_rows).total : 0;
}

int launch_values_gather_rows(int n_cu, int32_t n, const int64_t *val_off, int32_t top, int64_t max_units, const int32_t *row_group,
                              const int64_t *text_off, const uint16_t *chars, int64_t *row_text_off, uint16_t *row_chars, void *ws,
                              size_t ws_bytes, void *stream) {
    if (n <= 0) return 0;
    std::vector<int64_t> row_off((size_t)n + 1, 0);
    if (!val_off || max_units < 0 || fm_vh_shape_bad(n, val_off, top, 1, row_off.data())) return (int)hipErrorInvalidValue;
    const int64_t R = row_off[(size_t)n];
    if (R <= 0) return 0;
    if (R > kHistCellsMax) return (int)hipErrorInvalidValue;
    const GatherWs w = gather_ws(n, R);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *base = static_cast<uint8_t *>(ws);
    int64_t *d_val_off = reinterpret_cast<int64_t *>(base + w.val_off), *d_row_off = reinterpret_cast<int64_t *>(base + w.row_off);
    int64_t *src = reinterpret_cast<int64_t *>(base + w.src), *len = reinterpret_cast<int64_t *>(base + w.len);
    void *tmp = base + w.tmp;
    size_t tmp_bytes = w.tmp_bytes;
    const size_t off_bytes = ((size_t)n + 1) * 8;
    if (hipError_t e = hipMemcpyAsync(d_val_off, val_off, off_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    if (hipError_t e = hipMemcpyAsync(d_row_off, row_off.data(), off_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    int32_t unused = 1, row_grid = 1, unit_grid = 1;
    hit_lines_geometry(R, n_cu, &unused, &row_grid);
    hit_lines_geometry(max_units, n_cu, &unused, &unit_grid);
    hipLaunchKernelGGL(k_vh_row_sources, dim3((unsigned)row_grid), dim3(kFlatBlock), 0, st, d_val_off, d_row_off, n, row_group, R, src);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_vh_row_lengths, dim3((unsigned)row_grid), dim3(kFlatBlock), 0, st, src, text_off, R, len);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, len, row_text_off, (int64_t)0, (size_t)R + 1, rocprim::plus<int64_t>(), st);
        e != hipSuccess)
        return (int)e;
    if (max_units > 0) {
        hipLaunchKernelGGL(k_vh_gather, dim3((unsigned)unit_grid), dim3(kFlatBlock), 0, st, src, text_off, chars, R, row_text_off, row_chars);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    }
    return 0;
}

}  // namespace fmx
