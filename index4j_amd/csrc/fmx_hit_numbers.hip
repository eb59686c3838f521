// fmx_hit_numbers.hip — packed hits of a batch of patterns -> STATISTICS OF THE NUMBER BEHIND EACH HIT, PER BUCKET OF LINES
// (fmx_numbers_of_hits_dev, fmx_number_stats_where_batch; fmx_hit_numbers.hpp has the definition and the per-item functions).  The
// windows' text is the packed extract's (fmx_extract_packed.hip), which the C-ABI layer runs between launch_numbers_ranges and
// launch_numbers_rows over the ranges the former leaves in the workspace.
//
// Lanes go to slots or to counters, never to patterns:
//   k_num_ranges      a lane per packed slot, k_hist_keys' tile loop (fm_hit_tile / fm_hit_tile_slice / fm_hit_pattern; fences and
//                     up to kHistEdgesLds edges staged in LDS): the hit's window [s, e) and the key pattern | bucket (fm_line_of,
//                     fm_hist_bucket; no edges: the bucket 0); a slot that is no hit gets the pattern n and an empty window
//   (packed extract)  both of its stages over the n_hits windows, redo launch included: n_hits * 32 code units at most
//   k_num_parse       a lane per slot reads its window unit by unit up to the first that is no digit (neighbouring lanes read
//                     neighbouring windows of the packed text: a wave's reads fall into the cache lines its own lanes share)
//                     and stores the value and the key pattern | code; a window the extract ran literally hands its status to
//                     its pattern
//   rocPRIM           two stable radix_sort_pairs: by value over 63 bits, then by key over fm_num_key_width bits — the order
//                     (key, value); two inclusive scans of the values' halves over the sorted values
//   k_num_rows        a lane per (pattern, bucket): fm_num_segment's two lower bounds, then count, min (the first value), max (the
//                     last), the 128-bit sum off the scans, the P percentiles by index
//   k_num_tails       a lane per pattern: not_number and overflow, the same way
// GROUPED BY THE VALUE OF A FIELD (fmx_numbers_by_key_dev; fmx_hit_by.hpp has the definition): the same sequence with
//   k_by_ranges       in k_num_ranges' place: the code of a slot is the GROUP of its line's key — the hit's line (fm_line_of), ONE
//                     lower bound in the first lines of its key pattern by_of[p] (fm_by_find), that first hit's group — or B = no key
//   k_by_rows         a lane per PACKED row: its pattern off row_off (fm_by_row_pattern), then what k_num_rows stores
//   k_by_tails        a lane per pattern: no_key, not_number and overflow
// Integers only, no atomics: the result does not depend on the order the lanes run in.  Nothing here looks at the image, so this
// file is compiled once, like fmx_line_hist.hip.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "fmx_hit_by.hpp"
#include "fmx_hit_filter.hpp"
#include "fmx_hit_numbers.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_num_ranges: a tile of kLocateAllTile slots per round; 16 + 16 + 16 KiB of LDS
constexpr int kFlatBlock = 256;  // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

// T == nullptr: no edges, B = 1 and every hit lies in bucket 0
__global__ __launch_bounds__(kKeyBlock) void k_num_ranges(const int32_t *__restrict__ T, int32_t count, int32_t n_fences, int32_t shift,
                                                          const int64_t *__restrict__ hit_off, int32_t n, const int32_t *__restrict__ locs,
                                                          int64_t n_hits, const int32_t *__restrict__ term_len, int32_t text_len,
                                                          const int32_t *__restrict__ edges, int32_t n_edges, int32_t code_bits,
                                                          int32_t *__restrict__ start, int32_t *__restrict__ stop, uint64_t *__restrict__ keys) {
    __shared__ int64_t s_off[kLocateAllSlice];
    __shared__ int32_t s_fence[kLineFences];
    __shared__ int32_t s_edge[kHistEdgesLds];
    const bool bucketed = n_edges > 0;  // (workgroup-uniform)
    if (bucketed)
        for (int32_t j = threadIdx.x; j < n_fences; j += kKeyBlock) s_fence[j] = T[(int64_t)j << shift];
    const bool edges_in_lds = n_edges <= kHistEdgesLds;
    if (bucketed && edges_in_lds)
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
            const int32_t b = bucketed ? fm_hist_bucket(edge, n_edges, fm_line_of(T, count, s_fence, n_fences, shift, loc)) : 0;
            keys[t] = fm_hist_key(p, b, code_bits);
        } else if (t < n_hits) {
            keys[t] = no_hit;
            start[t] = stop[t] = 0;
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_num_parse(const int64_t *__restrict__ win_off, const uint16_t *__restrict__ win,
                                                          const int32_t *__restrict__ win_status, int64_t n_hits, int32_t n, int32_t B,
                                                          int32_t code_bits, int32_t frac_digits, uint64_t *__restrict__ keys,
                                                          uint64_t *__restrict__ values, int32_t *__restrict__ status) {
    for (int64_t t = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; t < n_hits; t += (int64_t)gridDim.x * kFlatBlock) {
        const uint64_t key = keys[t];
        const int32_t p = fm_hist_key_pattern(key, code_bits);
        if (p >= n) {
            values[t] = 0;
            continue;
        }
        const int64_t at = win_off[t];
        int64_t v;
        const int32_t kind = fm_num_parse(win + at, (int32_t)(win_off[t + 1] - at), frac_digits, v);
        keys[t] = fm_hist_key(p, fm_num_code(fm_hist_key_bucket(key, code_bits), B, kind), code_bits);
        values[t] = (uint64_t)v;
        // (a window the redo pass ran: the literal extract's status, by k_val_lengths' rule — every non-OK status here is the same
        // one, so the value does not depend on which lane stores last)
        const int32_t ws = win_status[t];
        if (status && ws != ST_OK) status[p] = ws;
    }
}

struct RowOut {
    int32_t *count;
    uint64_t *sum_lo, *sum_hi;
    int64_t *min, *max, *pct;
};

__global__ __launch_bounds__(kFlatBlock) void k_num_rows(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ values,
                                                         const uint64_t *__restrict__ scan_lo, const uint64_t *__restrict__ scan_hi,
                                                         const int64_t *__restrict__ hit_off, int32_t n, int64_t n_hits, int32_t B,
                                                         int32_t code_bits, const int32_t *__restrict__ permille, int32_t P, RowOut out) {
    const int64_t items = (int64_t)n * B, first = fm_filter_slot(hit_off[0], n_hits);
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < items; i += (int64_t)gridDim.x * kFlatBlock) {
        const int64_t p = i / B;
        int64_t lo;
        const int64_t c = fm_num_segment(keys, hit_off, n_hits, first, (int32_t)p, (int32_t)(i - p * B), code_bits, lo);
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

__global__ __launch_bounds__(kFlatBlock) void k_num_tails(const uint64_t *__restrict__ keys, const int64_t *__restrict__ hit_off, int32_t n,
                                                          int64_t n_hits, int32_t B, int32_t code_bits, int32_t *__restrict__ not_number,
                                                          int32_t *__restrict__ overflow) {
    const int64_t first = fm_filter_slot(hit_off[0], n_hits);
    for (int64_t p = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kFlatBlock) {
        if (not_number) not_number[p] = fm_hist_count(keys, hit_off, n_hits, first, (int32_t)p, B + kNumNotNumber, code_bits);
        if (overflow) overflow[p] = fm_hist_count(keys, hit_off, n_hits, first, (int32_t)p, B + kNumOverflow, code_bits);
    }
}

// by_of (n), first_off (m + 1), first_lines / group_of_first: the key patterns' first hits of lines and their groups (stages a, b)
__global__ __launch_bounds__(kKeyBlock) void k_by_ranges(const int32_t *__restrict__ T, int32_t count, int32_t n_fences, int32_t shift,
                                                         const int64_t *__restrict__ hit_off, int32_t n, const int32_t *__restrict__ locs,
                                                         int64_t n_hits, const int32_t *__restrict__ term_len, int32_t text_len,
                                                         const int32_t *__restrict__ by_of, const int64_t *__restrict__ first_off,
                                                         const int32_t *__restrict__ first_lines, const int32_t *__restrict__ group_of_first,
                                                         int32_t B, int32_t code_bits, int32_t *__restrict__ start, int32_t *__restrict__ stop,
                                                         uint64_t *__restrict__ keys) {
    __shared__ int64_t s_off[kLocateAllSlice];
    __shared__ int32_t s_fence[kLineFences];
    for (int32_t j = threadIdx.x; j < n_fences; j += kKeyBlock) s_fence[j] = T[(int64_t)j << shift];
    __syncthreads();
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
            const int32_t k = by_of[p];
            const int64_t found = fm_by_find(first_lines, first_off[k], first_off[k + 1], fm_line_of(T, count, s_fence, n_fences, shift, loc));
            keys[t] = fm_hist_key(p, fm_by_code(group_of_first, found, B), code_bits);
        } else if (t < n_hits) {
            keys[t] = no_hit;
            start[t] = stop[t] = 0;
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

// row_off: n + 1 (the workspace's copy); rows = row_off[n]
__global__ __launch_bounds__(kFlatBlock) void k_by_rows(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ values,
                                                        const uint64_t *__restrict__ scan_lo, const uint64_t *__restrict__ scan_hi,
                                                        const int64_t *__restrict__ hit_off, int32_t n, int64_t n_hits,
                                                        const int64_t *__restrict__ row_off, int64_t rows, int32_t code_bits,
                                                        const int32_t *__restrict__ permille, int32_t P, RowOut out) {
    const int64_t first = fm_filter_slot(hit_off[0], n_hits);
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < rows; i += (int64_t)gridDim.x * kFlatBlock) {
        const int32_t p = fm_by_row_pattern(row_off, n, i);
        int64_t lo;
        const int64_t c = fm_num_segment(keys, hit_off, n_hits, first, p, (int32_t)(i - row_off[p]), code_bits, lo);
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

__global__ __launch_bounds__(kFlatBlock) void k_by_tails(const uint64_t *__restrict__ keys, const int64_t *__restrict__ hit_off, int32_t n,
                                                         int64_t n_hits, int32_t B, int32_t code_bits, int32_t *__restrict__ no_key,
                                                         int32_t *__restrict__ not_number, int32_t *__restrict__ overflow) {
    const int64_t first = fm_filter_slot(hit_off[0], n_hits);
    for (int64_t p = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kFlatBlock) {
        if (no_key) no_key[p] = fm_hist_count(keys, hit_off, n_hits, first, (int32_t)p, B, code_bits);
        if (not_number) not_number[p] = fm_hist_count(keys, hit_off, n_hits, first, (int32_t)p, B + kNumNotNumber, code_bits);
        if (overflow) overflow[p] = fm_hist_count(keys, hit_off, n_hits, first, (int32_t)p, B + kNumOverflow, code_bits);
    }
}

struct LowHalf {
    __host__ __device__ uint64_t operator()(uint64_t v) const { return v & 0xffffffffu; }
};
struct HighHalf {
    __host__ __device__ uint64_t operator()(uint64_t v) const { return v >> 32; }
};

// the regions of the caller's workspace, each a multiple of 256 bytes.  tables: edges (n_edges ints), term_len (n), permille (P) —
// one copy.  The sorts go a -> b (by value), b -> a (by key); the running sums of the values in val_a land in val_b and key_b.
struct NumWs {
    size_t start, stop, win_off, piece_off, win_status, extract, extract_bytes, win, key_a, key_b, val_a, val_b, tables, tables_bytes, t_len,
        t_permille, tmp, tmp_bytes, total;
};
NumWs num_ws(int32_t n, int64_t n_hits, int32_t n_edges, int32_t P) {
    NumWs w{};
    const size_t H = (size_t)n_hits;
    size_t sort = 0, scan = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint64_t *)nullptr, (uint64_t *)nullptr, H,
                                    0u, 64u);
    (void)rocprim::inclusive_scan(nullptr, scan, rocprim::make_transform_iterator((const uint64_t *)nullptr, LowHalf()), (uint64_t *)nullptr, H,
                                  rocprim::plus<uint64_t>());
    w.tmp_bytes = pad256(std::max(sort, scan));
    w.t_len = (size_t)n_edges * 4;
    w.t_permille = w.t_len + (size_t)n * 4;
    w.tables_bytes = w.t_permille + (size_t)P * 4;
    w.extract_bytes = extract_packed_scratch_bytes((int32_t)n_hits);
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
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}

template <class T>
T *region(void *ws, size_t off) {
    return reinterpret_cast<T *>(static_cast<uint8_t *>(ws) + off);
}

}  // namespace

bool numbers_shape_ok(int32_t n, int64_t n_hits, int32_t n_edges, int32_t n_permille) {
    if (n <= 0 || n_hits <= 0 || n_hits > 0x7fffffff || n_edges < 0 || n_edges == 1 || n_permille < 0 || n_permille > kNumPermilleMax) return false;
    const int64_t cells = (int64_t)n * (n_edges > 0 ? n_edges - 1 : 1);
    return cells <= kHistCellsMax && cells * (n_permille > 0 ? n_permille : 1) <= kHistCellsMax;
}

size_t numbers_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_edges, int32_t n_permille) {
    return numbers_shape_ok(n, n_hits, n_edges, n_permille) ? num_ws(n, n_hits, n_edges, n_permille).total : 0;
}

bool numbers_windows(void *ws, size_t ws_bytes, int32_t n, int64_t n_hits, int32_t n_edges, int32_t n_permille, ValuesWindows *out) {
    if (!ws || !numbers_shape_ok(n, n_hits, n_edges, n_permille)) return false;
    const NumWs w = num_ws(n, n_hits, n_edges, n_permille);
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

int launch_numbers_ranges(const int32_t *T, int32_t count, int32_t text_len, int n_cu, int32_t n, const int32_t *term_len, const int64_t *hit_off,
                          const int32_t *locs, int64_t n_hits, const int32_t *edges, int32_t n_edges, const int32_t *permille, int32_t n_permille,
                          void *ws, size_t ws_bytes, void *stream) {
    if (!numbers_shape_ok(n, n_hits, n_edges, n_permille) || fm_num_permille_bad(permille, n_permille) || count < 0 || !term_len)
        return (int)hipErrorInvalidValue;
    if (n_edges > 0 && (!T || fm_hist_edges_bad(edges, n_edges))) return (int)hipErrorInvalidValue;
    const NumWs w = num_ws(n, n_hits, n_edges, n_permille);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    // the tables.  The runtime has read this block when the copy returns (a copy from pageable host memory is staged before the
    // call comes back).
    std::vector<uint8_t> host(w.tables_bytes + 4, 0);
    if (n_edges > 0) memcpy(host.data(), edges, (size_t)n_edges * 4);
    memcpy(host.data() + w.t_len, term_len, (size_t)n * 4);
    if (n_permille > 0) memcpy(host.data() + w.t_permille, permille, (size_t)n_permille * 4);
    if (hipError_t e = hipMemcpyAsync(region<uint8_t>(ws, w.tables), host.data(), w.tables_bytes, hipMemcpyHostToDevice, st); e != hipSuccess)
        return (int)e;
    int32_t n_fences = 0;
    const int32_t shift = n_edges > 0 ? fm_line_fence_shift(count, kLineFences, n_fences) : 0;
    const int32_t B = n_edges > 0 ? n_edges - 1 : 1;
    int32_t key_grid = 1, flat = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hipLaunchKernelGGL(k_num_ranges, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, n_edges > 0 ? T : nullptr, count, n_fences, shift, hit_off, n,
                       locs, n_hits, region<const int32_t>(ws, w.tables + w.t_len), text_len, region<const int32_t>(ws, w.tables), n_edges,
                       fm_num_code_bits(B), region<int32_t>(ws, w.start), region<int32_t>(ws, w.stop), region<uint64_t>(ws, w.key_a));
    return (int)hipGetLastError();
}

int launch_numbers_rows(int n_cu, int32_t n, const int64_t *hit_off, int64_t n_hits, int32_t n_edges, int32_t frac_digits, int32_t n_permille,
                        int32_t *count, uint64_t *sum_lo, uint64_t *sum_hi, int64_t *min, int64_t *max, int64_t *pct, int32_t *not_number,
                        int32_t *overflow, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    if (!numbers_shape_ok(n, n_hits, n_edges, n_permille) || frac_digits < 0 || frac_digits > kNumFracMax || !count) return (int)hipErrorInvalidValue;
    const NumWs w = num_ws(n, n_hits, n_edges, n_permille);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t *key_a = region<uint64_t>(ws, w.key_a), *key_b = region<uint64_t>(ws, w.key_b);
    uint64_t *val_a = region<uint64_t>(ws, w.val_a), *val_b = region<uint64_t>(ws, w.val_b);
    void *tmp = region<uint8_t>(ws, w.tmp);
    size_t tmp_bytes = w.tmp_bytes;
    const int32_t B = n_edges > 0 ? n_edges - 1 : 1, code_bits = fm_num_code_bits(B);
    const size_t H = (size_t)n_hits;
    int32_t unused = 1, flat = 1, row_grid = 1, pat_grid = 1;
    hit_lines_geometry(n_hits, n_cu, &unused, &flat);
    hit_lines_geometry((int64_t)n * B, n_cu, &unused, &row_grid);
    hit_lines_geometry(n, n_cu, &unused, &pat_grid);
    const dim3 fb(kFlatBlock);
#define FMX_NUM_CHECK(call) \
    if (hipError_t e_ = (call); e_ != hipSuccess) return (int)e_
    hipLaunchKernelGGL(k_num_parse, dim3((unsigned)flat), fb, 0, st, region<const int64_t>(ws, w.win_off), region<const uint16_t>(ws, w.win),
                       region<const int32_t>(ws, w.win_status), n_hits, n, B, code_bits, frac_digits, key_a, val_a, status);
    FMX_NUM_CHECK(hipGetLastError());
    // the order (key, value): stable passes, the least significant first
    FMX_NUM_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, val_a, val_b, key_a, key_b, H, 0u, 63u, st));
    FMX_NUM_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key_b, key_a, val_b, val_a, H, 0u, (unsigned)fm_num_key_width(n, B), st));
    uint64_t *scan_lo = val_b, *scan_hi = key_b;
    if (sum_lo || sum_hi) {
        FMX_NUM_CHECK(rocprim::inclusive_scan(tmp, tmp_bytes, rocprim::make_transform_iterator((const uint64_t *)val_a, LowHalf()), scan_lo, H,
                                              rocprim::plus<uint64_t>(), st));
        FMX_NUM_CHECK(rocprim::inclusive_scan(tmp, tmp_bytes, rocprim::make_transform_iterator((const uint64_t *)val_a, HighHalf()), scan_hi, H,
                                              rocprim::plus<uint64_t>(), st));
    }
    hipLaunchKernelGGL(k_num_rows, dim3((unsigned)row_grid), fb, 0, st, key_a, val_a, scan_lo, scan_hi, hit_off, n, n_hits, B, code_bits,
                       region<const int32_t>(ws, w.tables + w.t_permille), n_permille, RowOut{count, sum_lo, sum_hi, min, max, pct});
    FMX_NUM_CHECK(hipGetLastError());
    if (not_number || overflow) {
        hipLaunchKernelGGL(k_num_tails, dim3((unsigned)pat_grid), fb, 0, st, key_a, hit_off, n, n_hits, B, code_bits, not_number, overflow);
        FMX_NUM_CHECK(hipGetLastError());
    }
#undef FMX_NUM_CHECK
    return 0;
}

// ---- the parse, the two sorts and the two running sums alone, over the arrays of a stage that makes the codes and reads the cells
// itself (fmx_by_hist.hip): key_a / val_a leave sorted by (key, value), val_b and key_b hold the running sums of the values' halves --
size_t numbers_sorted_tmp_bytes(int64_t n_hits) {
    size_t sort = 0, scan = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                    (size_t)n_hits, 0u, 64u);
    (void)rocprim::inclusive_scan(nullptr, scan, rocprim::make_transform_iterator((const uint64_t *)nullptr, LowHalf()), (uint64_t *)nullptr,
                                  (size_t)n_hits, rocprim::plus<uint64_t>());
    return pad256(std::max(sort, scan));
}

int launch_numbers_sorted(int n_cu, int32_t n, int64_t n_hits, int32_t B, int32_t frac_digits, const int64_t *win_off, const uint16_t *win,
                          const int32_t *win_status, uint64_t *key_a, uint64_t *key_b, uint64_t *val_a, uint64_t *val_b, bool sums, int32_t *status,
                          void *tmp, size_t tmp_bytes, void *stream) {
    if (n <= 0 || n_hits <= 0 || n_hits > 0x7fffffff || B < 1 || frac_digits < 0 || frac_digits > kNumFracMax || !win_off || !win || !win_status ||
        !key_a || !key_b || !val_a || !val_b || !tmp || tmp_bytes < numbers_sorted_tmp_bytes(n_hits))
        return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int32_t code_bits = fm_num_code_bits(B);
    const size_t H = (size_t)n_hits;
    int32_t unused = 1, flat = 1;
    hit_lines_geometry(n_hits, n_cu, &unused, &flat);
#define FMX_NUM_CHECK(call) \
    if (hipError_t e_ = (call); e_ != hipSuccess) return (int)e_
    hipLaunchKernelGGL(k_num_parse, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, win_off, win, win_status, n_hits, n, B, code_bits, frac_digits,
                       key_a, val_a, status);
    FMX_NUM_CHECK(hipGetLastError());
    // the order (key, value): stable passes, the least significant first
    FMX_NUM_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, val_a, val_b, key_a, key_b, H, 0u, 63u, st));
    FMX_NUM_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key_b, key_a, val_b, val_a, H, 0u, (unsigned)fm_num_key_width(n, B), st));
    if (sums) {
        FMX_NUM_CHECK(rocprim::inclusive_scan(tmp, tmp_bytes, rocprim::make_transform_iterator((const uint64_t *)val_a, LowHalf()), val_b, H,
                                              rocprim::plus<uint64_t>(), st));
        FMX_NUM_CHECK(rocprim::inclusive_scan(tmp, tmp_bytes, rocprim::make_transform_iterator((const uint64_t *)val_a, HighHalf()), key_b, H,
                                              rocprim::plus<uint64_t>(), st));
    }
#undef FMX_NUM_CHECK
    return 0;
}

// ---- grouped by the value of a field: num_ws without edges, and behind it the tables by_of (n ints) and row_off (n + 1 int64) -----
namespace {
struct ByWs {
    NumWs num;
    size_t by_of, row_off, total;
};
ByWs by_ws(int32_t n, int64_t n_hits, int32_t P) {
    ByWs w{};
    w.num = num_ws(n, n_hits, 0, P);
    w.by_of = w.num.total;
    w.row_off = w.by_of + pad256((size_t)n * 4);
    w.total = w.row_off + pad256(((size_t)n + 1) * 8);
    return w;
}
bool by_shape_ok(int32_t n, int64_t n_hits, int32_t n_permille) {
    return n > 0 && n_hits > 0 && n_hits <= 0x7fffffff && n_permille >= 0 && n_permille <= kNumPermilleMax;
}
}  // namespace

size_t numbers_by_key_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_permille) {
    return by_shape_ok(n, n_hits, n_permille) ? by_ws(n, n_hits, n_permille).total : 0;
}

bool numbers_by_key_windows(void *ws, size_t ws_bytes, int32_t n, int64_t n_hits, int32_t n_permille, ValuesWindows *out) {
    if (!ws || !by_shape_ok(n, n_hits, n_permille)) return false;
    const ByWs b = by_ws(n, n_hits, n_permille);
    if (ws_bytes < b.total) return false;
    const NumWs &w = b.num;
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

int launch_numbers_by_key_ranges(const int32_t *T, int32_t count, int32_t text_len, int n_cu, int32_t n, const int32_t *term_len,
                                 const int32_t *by_of, int32_t m, const int64_t *val_off, const int64_t *hit_off, const int32_t *locs,
                                 int64_t n_hits, const int64_t *first_off, const int32_t *first_lines, const int32_t *group_of_first,
                                 const int32_t *permille, int32_t n_permille, int64_t *row_off_out, void *ws, size_t ws_bytes, void *stream) {
    if (!by_shape_ok(n, n_hits, n_permille) || fm_num_permille_bad(permille, n_permille) || count < 0 || !T || !term_len || !val_off ||
        !first_off || !first_lines || !group_of_first)
        return (int)hipErrorInvalidValue;
    std::vector<int64_t> row_off((size_t)n + 1, 0);
    int32_t B = 1;
    if (fm_by_rows_bad(n, by_of, m, val_off, n_permille, row_off.data(), &B)) return (int)hipErrorInvalidValue;
    const ByWs b = by_ws(n, n_hits, n_permille);
    const NumWs &w = b.num;
    if (!ws || ws_bytes < b.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    // the tables.  The runtime has read these blocks when the copies return (a copy from pageable host memory is staged before the
    // call comes back).
    std::vector<uint8_t> host(w.tables_bytes + 4, 0);
    memcpy(host.data() + w.t_len, term_len, (size_t)n * 4);
    if (n_permille > 0) memcpy(host.data() + w.t_permille, permille, (size_t)n_permille * 4);
#define FMX_BY_CHECK(call) \
    if (hipError_t e_ = (call); e_ != hipSuccess) return (int)e_
    FMX_BY_CHECK(hipMemcpyAsync(region<uint8_t>(ws, w.tables), host.data(), w.tables_bytes, hipMemcpyHostToDevice, st));
    FMX_BY_CHECK(hipMemcpyAsync(region<uint8_t>(ws, b.by_of), by_of, (size_t)n * 4, hipMemcpyHostToDevice, st));
    FMX_BY_CHECK(hipMemcpyAsync(region<uint8_t>(ws, b.row_off), row_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    if (row_off_out) FMX_BY_CHECK(hipMemcpyAsync(row_off_out, row_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
#undef FMX_BY_CHECK
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, kLineFences, n_fences);
    int32_t key_grid = 1, flat = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hipLaunchKernelGGL(k_by_ranges, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, T, count, n_fences, shift, hit_off, n, locs, n_hits,
                       region<const int32_t>(ws, w.tables + w.t_len), text_len, region<const int32_t>(ws, b.by_of), first_off, first_lines,
                       group_of_first, B, fm_num_code_bits(B), region<int32_t>(ws, w.start), region<int32_t>(ws, w.stop),
                       region<uint64_t>(ws, w.key_a));
    return (int)hipGetLastError();
}

int launch_numbers_by_key_rows(int n_cu, int32_t n, const int32_t *by_of, int32_t m, const int64_t *val_off, const int64_t *hit_off,
                               int64_t n_hits, int32_t frac_digits, int32_t n_permille, int32_t *count, uint64_t *sum_lo, uint64_t *sum_hi,
                               int64_t *min, int64_t *max, int64_t *pct, int32_t *no_key, int32_t *not_number, int32_t *overflow,
                               int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    if (!by_shape_ok(n, n_hits, n_permille) || frac_digits < 0 || frac_digits > kNumFracMax) return (int)hipErrorInvalidValue;
    std::vector<int64_t> row_off((size_t)n + 1, 0);
    int32_t B = 1;
    if (!val_off || fm_by_rows_bad(n, by_of, m, val_off, n_permille, row_off.data(), &B)) return (int)hipErrorInvalidValue;
    const int64_t rows = row_off[(size_t)n];
    if (rows > 0 && !count) return (int)hipErrorInvalidValue;
    const ByWs b = by_ws(n, n_hits, n_permille);
    const NumWs &w = b.num;
    if (!ws || ws_bytes < b.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t *key_a = region<uint64_t>(ws, w.key_a), *key_b = region<uint64_t>(ws, w.key_b);
    uint64_t *val_a = region<uint64_t>(ws, w.val_a), *val_b = region<uint64_t>(ws, w.val_b);
    void *tmp = region<uint8_t>(ws, w.tmp);
    size_t tmp_bytes = w.tmp_bytes;
    const int32_t code_bits = fm_num_code_bits(B);
    const size_t H = (size_t)n_hits;
    int32_t unused = 1, flat = 1, row_grid = 1, pat_grid = 1;
    hit_lines_geometry(n_hits, n_cu, &unused, &flat);
    hit_lines_geometry(rows, n_cu, &unused, &row_grid);
    hit_lines_geometry(n, n_cu, &unused, &pat_grid);
    const dim3 fb(kFlatBlock);
#define FMX_NUM_CHECK(call) \
    if (hipError_t e_ = (call); e_ != hipSuccess) return (int)e_
    hipLaunchKernelGGL(k_num_parse, dim3((unsigned)flat), fb, 0, st, region<const int64_t>(ws, w.win_off), region<const uint16_t>(ws, w.win),
                       region<const int32_t>(ws, w.win_status), n_hits, n, B, code_bits, frac_digits, key_a, val_a, status);
    FMX_NUM_CHECK(hipGetLastError());
    // the order (key, value): stable passes, the least significant first
    FMX_NUM_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, val_a, val_b, key_a, key_b, H, 0u, 63u, st));
    FMX_NUM_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key_b, key_a, val_b, val_a, H, 0u, (unsigned)fm_num_key_width(n, B), st));
    uint64_t *scan_lo = val_b, *scan_hi = key_b;
    if (rows > 0 && (sum_lo || sum_hi)) {
        FMX_NUM_CHECK(rocprim::inclusive_scan(tmp, tmp_bytes, rocprim::make_transform_iterator((const uint64_t *)val_a, LowHalf()), scan_lo, H,
                                              rocprim::plus<uint64_t>(), st));
        FMX_NUM_CHECK(rocprim::inclusive_scan(tmp, tmp_bytes, rocprim::make_transform_iterator((const uint64_t *)val_a, HighHalf()), scan_hi, H,
                                              rocprim::plus<uint64_t>(), st));
    }
    if (rows > 0) {
        hipLaunchKernelGGL(k_by_rows, dim3((unsigned)row_grid), fb, 0, st, key_a, val_a, scan_lo, scan_hi, hit_off, n, n_hits,
                           region<const int64_t>(ws, b.row_off), rows, code_bits, region<const int32_t>(ws, w.tables + w.t_permille), n_permille,
                           RowOut{count, sum_lo, sum_hi, min, max, n_permille > 0 ? pct : nullptr});
        FMX_NUM_CHECK(hipGetLastError());
    }
    if (no_key || not_number || overflow) {
        hipLaunchKernelGGL(k_by_tails, dim3((unsigned)pat_grid), fb, 0, st, key_a, hit_off, n, n_hits, B, code_bits, no_key, not_number, overflow);
        FMX_NUM_CHECK(hipGetLastError());
    }
#undef FMX_NUM_CHECK
    return 0;
}

}  // namespace fmx
