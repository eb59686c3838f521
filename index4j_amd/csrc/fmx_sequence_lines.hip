// fmx_sequence_lines.hip — packed hits of a batch of TERMS -> the packed LINES of each SEQUENCE (fmx_sequence_lines_of_hits_dev,
// fmx_match_sequence_batch): the n patterns are terms, cut into q sequences by query_off; a line belongs to a sequence iff it holds
// hits of its terms in order, inside the line, without overlap (fmx_device.hpp "A SEQUENCE OF TERMS IN ORDER": grep 'A.*B').  The
// chaining happens in HBM on the sorted positions of the hits; only the answer comes down.
//
// Lanes go to HITS in every stage but one, so ONE sequence over terms that match everywhere uses the whole device:
//   k_seq_keys      a lane per packed hit, k_query_line_keys' tile loop (fm_hit_tile / fm_hit_tile_slice / fm_hit_pattern for the
//                   term); the 64-bit key term | position (signed order); a slot behind hit_off[n] gets the term n: last
//   rocPRIM         ONE device-wide radix sort of the keys over the bits in use: term t's positions stand ascending in
//                   [hit_off[t], hit_off[t + 1]) — the offsets of the packed layout, no new offsets array
//   k_seq_positions a lane per sorted key: its position as an int32, so that the probes of the next stage read 4-byte entries
//   k_seq_chain     a lane per sorted hit, the fences of the line table in LDS: a hit of a term that is not its sequence's first,
//                   and a first-term hit that is not its line's first, get flag 0; a head runs the earliest-fit walk (fm_seq_chain:
//                   one lower bound per further term, inside that term's segment) and stores flag, line and the chain's end
//   rocPRIM         an exclusive scan of the flags over n_hits + 1
//   k_seq_counts    a lane per sequence: line_count = scan[hit_off[f + 1]] - scan[hit_off[f]], f its first term — hit_off is the
//                   group boundary, no search; clamped to max_lines; an exclusive scan of that is line_off
//   k_seq_compact   a lane per sorted hit: a flagged one whose rank inside its sequence is below the limit stores its line and,
//                   if asked, its span {position, chain's end}; the heads of a term are ascending, so are the lines
// No atomics of ours, integer arithmetic only: the result does not depend on the order the lanes run in.  Nothing here looks at
// the image, so this file is compiled once, like fmx_query_lines.hip.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cstring>
#include <vector>

#include "fmx_device.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_seq_keys (the slice, 16 KiB) and k_seq_chain (the fences, 16 KiB)
constexpr int kFlatBlock = 256;  // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

__global__ __launch_bounds__(kKeyBlock) void k_seq_keys(const int64_t *__restrict__ hit_off, int32_t n, const int32_t *__restrict__ locs,
                                                        int64_t n_hits, uint64_t *__restrict__ keys) {
    __shared__ int64_t s_off[kLocateAllSlice];
    const uint64_t behind = fm_seq_key(n, 0);
    const int64_t total = hit_off[n] < n_hits ? hit_off[n] : n_hits;  // (the caller holds n_hits >= hit_off[n]; nothing is read beyond either)
    for (int64_t tile = (int64_t)blockIdx.x * kLocateAllTile; tile < n_hits; tile += (int64_t)gridDim.x * kLocateAllTile) {
        const int64_t t = tile + threadIdx.x;
        if (tile >= total) {  // a tile of slots behind the hits (workgroup-uniform)
            if (t < n_hits) keys[t] = behind;
            continue;
        }
        const HitTile h = fm_hit_tile(hit_off, n, tile, total);
        bool in_lds;
        const int64_t *slice = fm_hit_tile_slice<kKeyBlock>(s_off, hit_off, h, in_lds);
        if (t <= h.tile_last)
            keys[t] = fm_seq_key(h.p_lo + fm_hit_pattern(slice, h.slice_count, t), locs[t]);
        else if (t < n_hits)
            keys[t] = behind;
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_seq_positions(const uint64_t *__restrict__ keys, int64_t n_hits, int32_t *__restrict__ pos) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < n_hits; i += (int64_t)gridDim.x * kFlatBlock)
        pos[i] = fm_seq_key_loc(keys[i]);
}

// flag[i] for the sorted hits, 0 for the slots behind them up to flag[n_hits]: the exclusive scan runs over n_hits + 1
__global__ __launch_bounds__(kKeyBlock) void k_seq_chain(const int32_t *__restrict__ T, int32_t count, int64_t n_lines, int32_t text_len,
                                                         int32_t n_fences, int32_t shift, const uint64_t *__restrict__ keys,
                                                         const int32_t *__restrict__ pos, const int64_t *__restrict__ hit_off, int32_t n,
                                                         const int32_t *__restrict__ term_seq, const int32_t *__restrict__ query_off,
                                                         const int32_t *__restrict__ term_len, int64_t n_hits, int32_t *__restrict__ flag,
                                                         int32_t *__restrict__ line_of, int32_t *__restrict__ end_of) {
    __shared__ int32_t s_fence[kLineFences];
    for (int32_t j = threadIdx.x; j < n_fences; j += kKeyBlock) s_fence[j] = T[(int64_t)j << shift];
    __syncthreads();
    const int64_t total = hit_off[n] < n_hits ? hit_off[n] : n_hits;
    for (int64_t i = (int64_t)blockIdx.x * kKeyBlock + threadIdx.x; i <= n_hits; i += (int64_t)gridDim.x * kKeyBlock) {
        int32_t f = 0;
        if (i < total) {
            const int32_t t = fm_seq_key_term(keys[i]);
            int32_t line = 0, end = 0;
            if (t < n) f = fm_seq_flag(pos, i, t, hit_off, total, term_seq, query_off, term_len, T, count, n_lines, text_len, s_fence, n_fences, shift, line, end);
            if (f) {
                line_of[i] = line;
                end_of[i] = end;
            }
        }
        flag[i] = f;
    }
}

// scan = the exclusive scan of flag.  The heads of sequence Q are among the sorted hits of its first term f: [hit_off[f], hit_off[f + 1]).
__global__ __launch_bounds__(kFlatBlock) void k_seq_counts(const int32_t *__restrict__ scan, const int64_t *__restrict__ hit_off, int32_t n,
                                                           int64_t n_hits, int32_t q, const int32_t *__restrict__ query_off, int32_t max_lines,
                                                           int32_t *__restrict__ line_count, int32_t *__restrict__ seq_base,
                                                           int64_t *__restrict__ stored) {
    const int64_t total = hit_off[n] < n_hits ? hit_off[n] : n_hits;
    for (int64_t seq = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; seq <= q; seq += (int64_t)gridDim.x * kFlatBlock) {
        int64_t c = 0;
        if (seq < q) {
            const int32_t f = query_off[seq];
            int32_t base = 0;
            if (f < query_off[seq + 1]) {  // (a sequence without terms has no lines)
                const int64_t a = hit_off[f] < total ? hit_off[f] : total, b = hit_off[f + 1] < total ? hit_off[f + 1] : total;
                base = scan[a];
                c = scan[b] - base;
            }
            seq_base[seq] = base;
            if (line_count) line_count[seq] = (int32_t)c;
            if (max_lines > 0 && c > max_lines) c = max_lines;
        }
        stored[seq] = c;  // (stored[q] = 0: the exclusive scan leaves the batch's total in line_off[q])
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_seq_compact(const uint64_t *__restrict__ keys, const int32_t *__restrict__ pos,
                                                            const int32_t *__restrict__ flag, const int32_t *__restrict__ scan,
                                                            const int32_t *__restrict__ line_of, const int32_t *__restrict__ end_of,
                                                            const int32_t *__restrict__ term_seq, const int32_t *__restrict__ seq_base,
                                                            const int64_t *__restrict__ line_off, int64_t n_hits, int32_t max_lines,
                                                            int32_t *__restrict__ lines, int32_t *__restrict__ spans) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < n_hits; i += (int64_t)gridDim.x * kFlatBlock) {
        if (!flag[i]) continue;  // (a flagged hit's term is below n)
        const int32_t seq = term_seq[fm_seq_key_term(keys[i])];
        const int32_t rank = scan[i] - seq_base[seq];
        if (max_lines > 0 && rank >= max_lines) continue;
        const int64_t at = line_off[seq] + rank;
        lines[at] = line_of[i];
        if (spans) {
            spans[2 * at] = pos[i];
            spans[2 * at + 1] = end_of[i];
        }
    }
}

// the regions of the caller's workspace, each a multiple of 256 bytes.  tables: term_seq (n ints), query_off (q + 1), term_len (n)
// — what the call derives from its host arrays, one copy.
struct SeqWs {
    size_t keys_a, keys_b, pos, flag, scan, line, end, stored, seq_base, tables, tables_bytes, tmp, tmp_bytes, total;
    size_t t_query_off, t_term_len;  // inside `tables` (term_seq at 0)
};
SeqWs seq_ws(int32_t n, int32_t q, int64_t n_hits) {
    SeqWs w{};
    size_t sort_tmp = 0, scan32 = 0, scan64 = 0;
    (void)rocprim::radix_sort_keys(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n_hits, 0u, 64u);
    (void)rocprim::exclusive_scan(nullptr, scan32, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, (size_t)n_hits + 1,
                                  rocprim::plus<int32_t>());
    (void)rocprim::exclusive_scan(nullptr, scan64, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)q + 1,
                                  rocprim::plus<int64_t>());
    size_t tmp = sort_tmp > scan32 ? sort_tmp : scan32;
    if (scan64 > tmp) tmp = scan64;
    w.tmp_bytes = pad256(tmp);
    w.t_query_off = (size_t)n * 4;
    w.t_term_len = w.t_query_off + ((size_t)q + 1) * 4;
    w.tables_bytes = w.t_term_len + (size_t)n * 4;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.keys_a = take((size_t)n_hits * 8);
    w.keys_b = take((size_t)n_hits * 8);
    w.pos = take((size_t)n_hits * 4);
    w.flag = take(((size_t)n_hits + 1) * 4);
    w.scan = take(((size_t)n_hits + 1) * 4);
    w.line = take((size_t)n_hits * 4);
    w.end = take((size_t)n_hits * 4);
    w.stored = take(((size_t)q + 1) * 8);
    w.seq_base = take(((size_t)q + 1) * 4);
    w.tables = take(w.tables_bytes);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}

}  // namespace

size_t sequence_lines_scratch_bytes(int32_t n, int32_t q, int64_t n_hits) {
    if (n <= 0 || q <= 0 || n_hits <= 0 || n_hits > 0x7fffffff) return 0;
    return seq_ws(n, q, n_hits).total;
}

int launch_sequence_lines(const int32_t *T, int32_t count, int64_t n_lines, int32_t text_len, int n_cu, int32_t n, int32_t q,
                          const int32_t *query_off, const int32_t *term_len, const int64_t *hit_off, const int32_t *locs, int64_t n_hits,
                          int32_t max_lines, int64_t *line_off, int32_t *lines, int32_t *line_count, int32_t *spans, void *ws, size_t ws_bytes,
                          void *stream) {
    if (n <= 0 || q <= 0 || n_hits <= 0) return 0;
    if (n_hits > 0x7fffffff || count < 0) return (int)hipErrorInvalidValue;
    const SeqWs w = seq_ws(n, q, n_hits);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const int32_t key_bits = fm_seq_key_width(n);  // at most 31 + 32
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *base = static_cast<uint8_t *>(ws);
    // the tables: the sequence of every term, the terms of every sequence, the lengths.  The runtime has read this block when the
    // copy returns (a copy from pageable host memory is staged before the call comes back).
    std::vector<uint8_t> host(w.tables_bytes);
    {
        int32_t *term_seq = reinterpret_cast<int32_t *>(host.data());
        memcpy(host.data() + w.t_query_off, query_off, ((size_t)q + 1) * 4);
        memcpy(host.data() + w.t_term_len, term_len, (size_t)n * 4);
        for (int32_t i = 0; i < q; ++i)
            for (int32_t t = query_off[i]; t < query_off[i + 1]; ++t) term_seq[t] = i;
    }
    if (hipError_t e = hipMemcpyAsync(base + w.tables, host.data(), w.tables_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    const int32_t *d_term_seq = reinterpret_cast<const int32_t *>(base + w.tables);
    const int32_t *d_query_off = reinterpret_cast<const int32_t *>(base + w.tables + w.t_query_off);
    const int32_t *d_term_len = reinterpret_cast<const int32_t *>(base + w.tables + w.t_term_len);
    uint64_t *keys_a = reinterpret_cast<uint64_t *>(base + w.keys_a), *keys_b = reinterpret_cast<uint64_t *>(base + w.keys_b);
    int32_t *pos = reinterpret_cast<int32_t *>(base + w.pos);
    int32_t *flag = reinterpret_cast<int32_t *>(base + w.flag), *scan = reinterpret_cast<int32_t *>(base + w.scan);
    int32_t *line_of = reinterpret_cast<int32_t *>(base + w.line), *end_of = reinterpret_cast<int32_t *>(base + w.end);
    int64_t *stored = reinterpret_cast<int64_t *>(base + w.stored);
    int32_t *seq_base = reinterpret_cast<int32_t *>(base + w.seq_base);
    void *tmp = base + w.tmp;
    size_t tmp_bytes = w.tmp_bytes;
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, kLineFences, n_fences);
    int32_t key_grid = 1, flat = 1, unused = 1, seq_grid = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hit_lines_geometry(q, n_cu, &unused, &seq_grid);  // (the element-wise grid over q + 1 items)
    hipLaunchKernelGGL(k_seq_keys, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, hit_off, n, locs, n_hits, keys_a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::radix_sort_keys(tmp, tmp_bytes, keys_a, keys_b, (size_t)n_hits, 0u, (unsigned)key_bits, st); e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_seq_positions, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, keys_b, n_hits, pos);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_seq_chain, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, T, count, n_lines, text_len, n_fences, shift, keys_b, pos,
                       hit_off, n, d_term_seq, d_query_off, d_term_len, n_hits, flag, line_of, end_of);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, flag, scan, (int32_t)0, (size_t)n_hits + 1, rocprim::plus<int32_t>(), st);
        e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_seq_counts, dim3((unsigned)seq_grid), dim3(kFlatBlock), 0, st, scan, hit_off, n, n_hits, q, d_query_off, max_lines,
                       line_count, seq_base, stored);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, stored, line_off, (int64_t)0, (size_t)q + 1, rocprim::plus<int64_t>(), st);
        e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_seq_compact, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, keys_b, pos, flag, scan, line_of, end_of, d_term_seq, seq_base,
                       line_off, n_hits, max_lines, lines, spans);
    return (int)hipGetLastError();
}

}  // namespace fmx
