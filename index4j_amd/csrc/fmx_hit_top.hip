// fmx_hit_top.hip — packed hits of a batch of patterns -> THE LINES RANKED BY THE NUMBER BEHIND EACH HIT (fmx_top_lines_of_hits_dev,
// fmx_top_lines_where_batch; fmx_hit_top.hpp has the definition and the per-item functions).  The windows' text is the packed
// extract's (fmx_extract_packed.hip), which the C-ABI layer runs between launch_top_lines_windows and launch_top_lines_rows over the
// ranges the former leaves in the workspace.
//
// Lanes go to slots, keys or rows, never to patterns' hits or to lines:
//   k_top_keys        a lane per packed slot, k_first_keys' tile loop (fm_hit_tile / fm_hit_tile_slice / fm_hit_pattern): the hit's
//                     window [s, e) and the key (pattern << pos_bits) | position; a slot that is no hit gets the pattern n and an
//                     empty window
//   (packed extract)  both of its stages over the n_hits windows, redo launch included
//   k_top_parse       a lane per slot parses its window (fm_num_parse) and stores the ordered value u; a slot that does not parse
//                     gets the pattern n, and its reason goes into fm_range_tail's word of two halves
//   rocPRIM           ONE exclusive scan of those words in slot order (not_number and overflow of every pattern as differences), ONE
//                     radix sort of (key, u) over the bits in use: every pattern's parsing hits side by side, ascending by position
//   k_top_lines       a lane per sorted slot: its line (fm_line_of, the fences staged in LDS), the run key pattern | line and the
//                     pair {u, position}
//   rocPRIM           reduce_by_key over the runs of equal key with the minimum of {u, position}: a lane's work does not grow
//                     with the hits of one line — a run that spans tiles is folded by the look-back of the primitive
//   k_top_fill        the run keys' output holds the pattern n in front of the reduction, so what lies behind the runs is no candidate
//   k_top_cands       a lane per candidate slot: u and its own index; rocPRIM's stable sort by u (63 bits)
//   k_top_patterns    a lane per ranked slot: the pattern of its candidate; rocPRIM's stable sort over the pattern's bits
//   k_top_tails       a lane per pattern: its segment of the ranking (fm_top_segment), lines, rows, numbers and the two reasons
//   k_top_rows        a lane per row (i, j): rank first + j of the pattern's segment, or zeros
// Integers only, no atomics of its own: the result does not depend on the order the lanes run in (the minimum of a total order is
// the same however the reduction is cut).  Nothing here looks at the image, so this file is compiled once, like fmx_hit_numbers.hip.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cstring>
#include <vector>

#include "fmx_hit_filter.hpp"
#include "fmx_hit_top.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_top_keys (the slice, 16 KiB) and k_top_lines (the fences, 16 KiB)
constexpr int kFlatBlock = 256;  // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

__global__ __launch_bounds__(kKeyBlock) void k_top_keys(const int64_t *__restrict__ hit_off, int32_t n, const int32_t *__restrict__ locs,
                                                        int64_t n_hits, const int32_t *__restrict__ term_len, int32_t text_len,
                                                        int32_t pos_bits, int32_t *__restrict__ start, int32_t *__restrict__ stop,
                                                        uint64_t *__restrict__ keys) {
    __shared__ int64_t s_off[kLocateAllSlice];
    const uint64_t no_hit = fm_first_key(n, 0, pos_bits);
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
            keys[t] = fm_first_key(p, loc, pos_bits);
        } else if (t < n_hits) {
            keys[t] = no_hit;
            start[t] = stop[t] = 0;
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

// tail: n_hits + 1 words, tail[n_hits] = 0, so that the exclusive scan leaves every total
__global__ __launch_bounds__(kFlatBlock) void k_top_parse(const int64_t *__restrict__ win_off, const uint16_t *__restrict__ win,
                                                          const int32_t *__restrict__ win_status, int64_t n_hits, int32_t n,
                                                          int32_t pos_bits, int32_t frac_digits, const uint8_t *__restrict__ descending,
                                                          uint64_t *__restrict__ keys, uint64_t *__restrict__ u, uint64_t *__restrict__ tail,
                                                          int32_t *__restrict__ status) {
    const uint64_t no_hit = fm_first_key(n, 0, pos_bits);
    for (int64_t t = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; t <= n_hits; t += (int64_t)gridDim.x * kFlatBlock) {
        if (t == n_hits) {
            tail[t] = 0;
            continue;
        }
        const int32_t p = fm_first_key_pattern(keys[t], pos_bits);
        if (p >= n) {
            u[t] = 0;
            tail[t] = 0;
            continue;
        }
        const int64_t at = win_off[t];
        int64_t v;
        const int32_t kind = fm_num_parse(win + at, (int32_t)(win_off[t + 1] - at), frac_digits, v);
        if (kind != kNumOk) keys[t] = no_hit;
        u[t] = kind == kNumOk ? fm_top_ordered(v, descending[p] != 0) : 0;
        tail[t] = fm_range_tail(fm_top_tail_code(kind));
        // (a window the redo pass ran: the literal extract's status, by k_val_lengths' rule — every non-OK status here is the same
        // one, so the value does not depend on which lane stores last)
        const int32_t ws = win_status[t];
        if (status && ws != ST_OK) status[p] = ws;
    }
}

__global__ __launch_bounds__(kKeyBlock) void k_top_lines(const int32_t *__restrict__ T, int32_t count, int32_t n_fences, int32_t shift,
                                                         const uint64_t *__restrict__ keys, const uint64_t *__restrict__ u, int64_t n_hits,
                                                         int32_t n, int32_t pos_bits, uint64_t *__restrict__ run_key,
                                                         TopCand *__restrict__ cand) {
    __shared__ int32_t s_fence[kLineFences];
    for (int32_t j = threadIdx.x; j < n_fences; j += kKeyBlock) s_fence[j] = T[(int64_t)j << shift];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kKeyBlock + threadIdx.x; i < n_hits; i += (int64_t)gridDim.x * kKeyBlock) {
        const uint64_t key = keys[i];
        const int32_t p = fm_first_key_pattern(key, pos_bits);
        if (p < n) {
            const int32_t loc = fm_first_key_loc(key, pos_bits);
            run_key[i] = fm_top_line_key(p, fm_line_of(T, count, s_fence, n_fences, shift, loc));
            cand[i] = TopCand{u[i], (int64_t)loc};
        } else {
            run_key[i] = fm_top_line_key(n, 0);
            cand[i] = TopCand{0, 0};
        }
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_top_fill(uint64_t *__restrict__ out, int64_t count, uint64_t value) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kFlatBlock) out[i] = value;
}

__global__ __launch_bounds__(kFlatBlock) void k_top_cands(const uint64_t *__restrict__ cand_key, const TopCand *__restrict__ cand, int64_t n_hits,
                                                          int32_t n, uint64_t *__restrict__ cand_u, uint32_t *__restrict__ cand_idx) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < n_hits; i += (int64_t)gridDim.x * kFlatBlock) {
        cand_u[i] = fm_top_line_key_pattern(cand_key[i]) < n ? cand[i].u : 0;
        cand_idx[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_top_patterns(const uint64_t *__restrict__ cand_key, const uint32_t *__restrict__ ranked,
                                                             int64_t n_hits, uint32_t *__restrict__ pat) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < n_hits; i += (int64_t)gridDim.x * kFlatBlock)
        pat[i] = (uint32_t)fm_top_line_key_pattern(cand_key[ranked[i]]);
}

// seg: n + 1 entries of the workspace; tail_pos: the exclusive scan of the reasons' words, n_hits + 1 entries in slot order
__global__ __launch_bounds__(kFlatBlock) void k_top_tails(const uint32_t *__restrict__ pat, const uint64_t *__restrict__ tail_pos,
                                                          const int64_t *__restrict__ hit_off, int32_t n, int64_t n_hits, int32_t first,
                                                          int32_t top, int64_t *__restrict__ seg, int32_t *__restrict__ rows,
                                                          int32_t *__restrict__ lines, int32_t *__restrict__ numbers,
                                                          int32_t *__restrict__ not_number, int32_t *__restrict__ overflow) {
    for (int64_t p = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; p <= n; p += (int64_t)gridDim.x * kFlatBlock) {
        const int64_t lo = fm_top_segment(pat, n_hits, (int32_t)p);
        seg[p] = lo;
        if (p == n) continue;
        const int64_t count = fm_top_segment(pat, n_hits, (int32_t)p + 1) - lo;
        const int64_t a = fm_filter_slot(hit_off[p], n_hits), b = fm_filter_slot(hit_off[p + 1], n_hits);
        const int32_t nn = fm_range_not_number(tail_pos, a, b), ov = fm_range_overflow(tail_pos, a, b);
        rows[p] = fm_top_rows(count, first, top);
        if (lines) lines[p] = (int32_t)count;
        if (numbers) numbers[p] = (int32_t)(b - a) - nn - ov;
        if (not_number) not_number[p] = nn;
        if (overflow) overflow[p] = ov;
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_top_rows(const int64_t *__restrict__ seg, const uint32_t *__restrict__ ranked,
                                                         const uint64_t *__restrict__ cand_key, const TopCand *__restrict__ cand,
                                                         const uint8_t *__restrict__ descending, int32_t n, int32_t first, int32_t top,
                                                         int32_t *__restrict__ row_line, int64_t *__restrict__ row_value,
                                                         int32_t *__restrict__ row_loc) {
    const int64_t items = (int64_t)n * top;
    for (int64_t r = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; r < items; r += (int64_t)gridDim.x * kFlatBlock) {
        const int64_t p = r / top;
        const int64_t rank = (int64_t)first + (r - p * top), lo = seg[p];
        int32_t line = 0, loc = 0;
        int64_t value = 0;
        if (rank < seg[p + 1] - lo) {
            const uint32_t c = ranked[lo + rank];
            const TopCand best = cand[c];
            line = fm_top_line_key_line(cand_key[c]);
            loc = (int32_t)best.loc;
            value = fm_top_value(best.u, descending[p] != 0);
        }
        if (row_line) row_line[r] = line;
        if (row_value) row_value[r] = value;
        if (row_loc) row_loc[r] = loc;
    }
}

// the regions of the caller's workspace, each a multiple of 256 bytes.  tables: term_len (n ints), descending (n bytes) — one copy.
// The first sort goes (key_a, u_a) -> (key_b, u_b); the run keys and pairs lie in run_key / run_cand, the candidates in cand_key /
// cand; the ranking sorts (u_a, idx_a) -> (u_b, idx_b) by u, then (pat_a, idx_b) -> (pat_b, idx_a) by pattern.
struct TopWs {
    size_t start, stop, win_off, piece_off, win_status, extract, extract_bytes, win, key_a, key_b, u_a, u_b, tail, tail_pos, run_key, run_cand,
        cand_key, cand, runs, idx_a, idx_b, pat_a, pat_b, seg, tables, tables_bytes, t_desc, tmp, tmp_bytes, total;
    bool ok;
};
TopWs top_ws(int32_t n, int64_t n_hits) {
    TopWs w{};
    const size_t H = (size_t)n_hits;
    size_t sort64 = 0, sort_u = 0, sort_p = 0, scan = 0, reduce = 0;
    w.ok = rocprim::radix_sort_pairs(nullptr, sort64, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint64_t *)nullptr,
                                     (uint64_t *)nullptr, H, 0u, 64u) == hipSuccess &&
           rocprim::radix_sort_pairs(nullptr, sort_u, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                     (uint32_t *)nullptr, H, 0u, 64u) == hipSuccess &&
           rocprim::radix_sort_pairs(nullptr, sort_p, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                     (uint32_t *)nullptr, H, 0u, 32u) == hipSuccess &&
           rocprim::exclusive_scan(nullptr, scan, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, H + 1,
                                   rocprim::plus<uint64_t>()) == hipSuccess &&
           rocprim::reduce_by_key(nullptr, reduce, (const uint64_t *)nullptr, (const TopCand *)nullptr, H, (uint64_t *)nullptr, (TopCand *)nullptr,
                                  (int64_t *)nullptr, TopBetter()) == hipSuccess;
    size_t tmp = sort64;
    for (size_t b : {sort_u, sort_p, scan, reduce})
        if (b > tmp) tmp = b;
    w.tmp_bytes = pad256(tmp);
    w.t_desc = (size_t)n * 4;
    w.tables_bytes = w.t_desc + (size_t)n;
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
    w.u_a = take(H * 8);
    w.u_b = take(H * 8);
    w.tail = take((H + 1) * 8);
    w.tail_pos = take((H + 1) * 8);
    w.run_key = take(H * 8);
    w.run_cand = take(H * sizeof(TopCand));
    w.cand_key = take(H * 8);
    w.cand = take(H * sizeof(TopCand));
    w.runs = take(8);
    w.idx_a = take(H * 4);
    w.idx_b = take(H * 4);
    w.pat_a = take(H * 4);
    w.pat_b = take(H * 4);
    w.seg = take(((size_t)n + 1) * 8);
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

bool top_lines_shape_ok(int32_t n, int64_t n_hits, int32_t top) {
    return n > 0 && n_hits > 0 && n_hits <= 0x7fffffff && top >= 1 && (int64_t)n * top <= kHistCellsMax;
}

size_t top_lines_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t top) {
    if (!top_lines_shape_ok(n, n_hits, top)) return 0;
    const TopWs w = top_ws(n, n_hits);
    return w.ok ? w.total : 0;
}

bool top_lines_windows(void *ws, size_t ws_bytes, int32_t n, int64_t n_hits, int32_t top, ValuesWindows *out) {
    if (!ws || !top_lines_shape_ok(n, n_hits, top)) return false;
    const TopWs w = top_ws(n, n_hits);
    if (!w.ok || ws_bytes < w.total) return false;
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

int launch_top_lines_windows(int32_t text_len, int n_cu, int32_t n, const int32_t *term_len, const uint8_t *descending, const int64_t *hit_off,
                             const int32_t *locs, int64_t n_hits, int32_t top, void *ws, size_t ws_bytes, void *stream) {
    if (!top_lines_shape_ok(n, n_hits, top) || text_len < 0 || !term_len || !descending || !hit_off || !locs) return (int)hipErrorInvalidValue;
    for (int32_t i = 0; i < n; ++i)
        if (term_len[i] < 0) return (int)hipErrorInvalidValue;
    const TopWs w = top_ws(n, n_hits);
    if (!w.ok || !ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    // the tables.  The runtime has read this block when the copy returns (a copy from pageable host memory is staged before the
    // call comes back).
    std::vector<uint8_t> host(w.tables_bytes + 4, 0);
    memcpy(host.data(), term_len, (size_t)n * 4);
    for (int32_t i = 0; i < n; ++i) host[w.t_desc + (size_t)i] = descending[i] ? 1 : 0;
    if (hipError_t e = hipMemcpyAsync(region<uint8_t>(ws, w.tables), host.data(), w.tables_bytes, hipMemcpyHostToDevice, st); e != hipSuccess)
        return (int)e;
    int32_t key_grid = 1, flat = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hipLaunchKernelGGL(k_top_keys, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, hit_off, n, locs, n_hits, region<const int32_t>(ws, w.tables),
                       text_len, fm_bits((uint32_t)text_len), region<int32_t>(ws, w.start), region<int32_t>(ws, w.stop),
                       region<uint64_t>(ws, w.key_a));
    return (int)hipGetLastError();
}

int launch_top_lines_rows(const int32_t *T, int32_t count, int32_t text_len, int n_cu, int32_t n, const int64_t *hit_off, int64_t n_hits,
                          int32_t frac_digits, int32_t first, int32_t top, int32_t *rows, int32_t *row_line, int64_t *row_value, int32_t *row_loc,
                          int32_t *lines, int32_t *numbers, int32_t *not_number, int32_t *overflow, int32_t *status, void *ws, size_t ws_bytes,
                          void *stream) {
    if (!top_lines_shape_ok(n, n_hits, top) || frac_digits < 0 || frac_digits > kNumFracMax || first < 0 || count < 0 || text_len < 0 || !T ||
        !hit_off || !rows)
        return (int)hipErrorInvalidValue;
    const TopWs w = top_ws(n, n_hits);
    if (!w.ok || !ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t *key_a = region<uint64_t>(ws, w.key_a), *key_b = region<uint64_t>(ws, w.key_b);
    uint64_t *u_a = region<uint64_t>(ws, w.u_a), *u_b = region<uint64_t>(ws, w.u_b);
    uint64_t *tail = region<uint64_t>(ws, w.tail), *tail_pos = region<uint64_t>(ws, w.tail_pos);
    uint64_t *run_key = region<uint64_t>(ws, w.run_key), *cand_key = region<uint64_t>(ws, w.cand_key);
    TopCand *run_cand = region<TopCand>(ws, w.run_cand), *cand = region<TopCand>(ws, w.cand);
    uint32_t *idx_a = region<uint32_t>(ws, w.idx_a), *idx_b = region<uint32_t>(ws, w.idx_b);
    uint32_t *pat_a = region<uint32_t>(ws, w.pat_a), *pat_b = region<uint32_t>(ws, w.pat_b);
    int64_t *seg = region<int64_t>(ws, w.seg);
    const uint8_t *descending = region<const uint8_t>(ws, w.tables + w.t_desc);
    void *tmp = region<uint8_t>(ws, w.tmp);
    size_t tmp_bytes = w.tmp_bytes;
    const size_t H = (size_t)n_hits;
    const int32_t pos_bits = fm_bits((uint32_t)text_len), pat_bits = fm_bits((uint32_t)n);
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, kLineFences, n_fences);
    int32_t key_grid = 1, flat = 1, unused = 1, flat1 = 1, row_grid = 1, pat_grid = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hit_lines_geometry(n_hits + 1, n_cu, &unused, &flat1);
    hit_lines_geometry((int64_t)n * top, n_cu, &unused, &row_grid);
    hit_lines_geometry((int64_t)n + 1, n_cu, &unused, &pat_grid);
    const dim3 fb(kFlatBlock);
#define FMX_TOP_CHECK(call) \
    if (hipError_t e_ = (call); e_ != hipSuccess) return (int)e_
    hipLaunchKernelGGL(k_top_parse, dim3((unsigned)flat1), fb, 0, st, region<const int64_t>(ws, w.win_off), region<const uint16_t>(ws, w.win),
                       region<const int32_t>(ws, w.win_status), n_hits, n, pos_bits, frac_digits, descending, key_a, u_a, tail, status);
    FMX_TOP_CHECK(hipGetLastError());
    FMX_TOP_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, (const uint64_t *)tail, tail_pos, (uint64_t)0, H + 1, rocprim::plus<uint64_t>(), st));
    FMX_TOP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, (const uint64_t *)key_a, key_b, (const uint64_t *)u_a, u_b, H, 0u,
                                            (unsigned)(pat_bits + pos_bits), st));
    hipLaunchKernelGGL(k_top_lines, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, T, count, n_fences, shift, key_b, u_b, n_hits, n, pos_bits,
                       run_key, run_cand);
    FMX_TOP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_top_fill, dim3((unsigned)flat), fb, 0, st, cand_key, n_hits, fm_top_line_key(n, 0));
    FMX_TOP_CHECK(hipGetLastError());
    FMX_TOP_CHECK(rocprim::reduce_by_key(tmp, tmp_bytes, (const uint64_t *)run_key, (const TopCand *)run_cand, H, cand_key, cand,
                                         region<int64_t>(ws, w.runs), TopBetter(), rocprim::equal_to<uint64_t>(), st));
    // the candidates lie in (pattern, line) order: stable passes, the least significant first
    hipLaunchKernelGGL(k_top_cands, dim3((unsigned)flat), fb, 0, st, cand_key, cand, n_hits, n, u_a, idx_a);
    FMX_TOP_CHECK(hipGetLastError());
    FMX_TOP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, (const uint64_t *)u_a, u_b, (const uint32_t *)idx_a, idx_b, H, 0u, 63u, st));
    hipLaunchKernelGGL(k_top_patterns, dim3((unsigned)flat), fb, 0, st, cand_key, idx_b, n_hits, pat_a);
    FMX_TOP_CHECK(hipGetLastError());
    FMX_TOP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, (const uint32_t *)pat_a, pat_b, (const uint32_t *)idx_b, idx_a, H, 0u,
                                            (unsigned)pat_bits, st));
    hipLaunchKernelGGL(k_top_tails, dim3((unsigned)pat_grid), fb, 0, st, pat_b, tail_pos, hit_off, n, n_hits, first, top, seg, rows, lines, numbers,
                       not_number, overflow);
    FMX_TOP_CHECK(hipGetLastError());
    if (row_line || row_value || row_loc) {
        hipLaunchKernelGGL(k_top_rows, dim3((unsigned)row_grid), fb, 0, st, seg, idx_a, cand_key, cand, descending, n, first, top, row_line,
                           row_value, row_loc);
        FMX_TOP_CHECK(hipGetLastError());
    }
#undef FMX_TOP_CHECK
    return 0;
}

}  // namespace fmx
