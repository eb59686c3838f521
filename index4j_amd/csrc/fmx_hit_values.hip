// fmx_hit_values.hip — packed hits of a batch of patterns -> the distinct VALUES that follow each pattern, with their counts
// (fmx_values_of_hits_dev / fmx_values_fill_dev, fmx_field_values_batch; grep -o 'blk_[^ ]*' | sort | uniq -c).  fmx_hit_values.hpp
// has the definition and the per-item functions; the windows' text is the packed extract's (fmx_extract_packed.hip), which the
// C-ABI layer runs between launch_values_ranges and launch_values_groups over the ranges the former leaves in the workspace.
//
// Lanes go to hits, runs or groups throughout:
//   k_val_ranges      a lane per packed hit, k_seq_keys' tile loop (fm_hit_tile / fm_hit_tile_slice / fm_hit_pattern): the hit's
//                     pattern and its window [s, e); a slot behind hit_off[n] gets the pattern n and an empty window
//   (packed extract)  both of its stages over the n_hits windows, redo launch included: n_hits * max_len code units at most
//   k_val_lengths     a lane per hit, the stop set in LDS (a bitmap over the 65,536 code units, or the sorted units): the length
//                     of the hit's value; a window the extract ran literally hands its status to its pattern
//   k_val_run_flags   a lane per hit: 1 where (pattern, length, code units) differ from the predecessor's in the packed order
//   rocPRIM           an exclusive scan of the flags over n_hits + 1: a run's number, and R behind the last
//   k_val_run_starts  a lane per hit: a flagged one stores its index as its run's start; run r's weight is start[r + 1] - start[r]
//   rocPRIM           stable radix_sort_pairs over n_hits slots (R is not known on the host: the slots behind the runs sort last),
//                     keys made by k_val_length_keys (7 bits), k_val_chunk_keys (64 bits, the last chunk first) and
//                     k_val_pattern_keys (the bits of n), the payload the run's number
//   k_val_heads       a lane per sorted slot: head = its (pattern, length, code units) differ from the slot's in front; its
//                     weight; its length where it is a head
//   rocPRIM           three exclusive scans over n_hits + 1: the group ids, the weights, the lengths
//   k_val_groups      a head stores where its group starts, its text_off and where its code units lie
//   k_val_counts      a lane per group: the difference of the weight scan over its slots
//   k_val_offsets     a lane per pattern: val_off[p] = the group id at the first sorted slot whose pattern is not below p
//   k_val_fill        a lane per group: the representative's code units into the caller's array
// and, only in launch_values_groups_of_hits (fmx_values_of_hits_groups_dev: the keys of "stats ... by", fmx_hit_by.hpp):
//   k_val_run_groups  a lane per sorted slot: the group of its run, off the scan of the heads
//   k_val_hit_groups  a lane per hit: its run off the scan of the run flags, that run's group, counted from its pattern's first
// The grouping is exact for hits in any order — runs only shorten the sort — so these hits need not stand in SA-row order.
// No atomics, integer arithmetic only: the result does not depend on the order the lanes run in.  Nothing here looks at the
// image, so this file is compiled once, like fmx_sequence_lines.hip.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "fmx_hit_values.hpp"
#include "fmx_plan.hpp"

// the LDS form of the stop set: 0 = a bitmap over the 65,536 code units (8 KiB, one read per unit), 1 = the sorted units (128
// bytes, a binary search per unit) — an A/B of the build (EXTRA_DEFS), the results do not differ
#if !defined(FMX_VALUES_STOP_LIST)
#define FMX_VALUES_STOP_LIST 0
#endif

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_val_ranges (the slice, 16 KiB) and k_val_lengths (the stop set, 8 KiB)
constexpr int kFlatBlock = 256;  // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

__global__ __launch_bounds__(kKeyBlock) void k_val_ranges(const int64_t *__restrict__ hit_off, int32_t n, const int32_t *__restrict__ locs,
                                                          int64_t n_hits, const int32_t *__restrict__ term_len, int32_t max_len,
                                                          int32_t text_len, int32_t *__restrict__ pat, int32_t *__restrict__ start,
                                                          int32_t *__restrict__ stop) {
    __shared__ int64_t s_off[kLocateAllSlice];
    const int64_t total = hit_off[n] < n_hits ? hit_off[n] : n_hits;  // (nothing is read beyond either)
    for (int64_t tile = (int64_t)blockIdx.x * kLocateAllTile; tile < n_hits; tile += (int64_t)gridDim.x * kLocateAllTile) {
        const int64_t t = tile + threadIdx.x;
        if (tile >= total) {  // a tile of slots behind the hits (workgroup-uniform)
            if (t < n_hits) {
                pat[t] = n;
                start[t] = stop[t] = 0;
            }
            continue;
        }
        const HitTile h = fm_hit_tile(hit_off, n, tile, total);
        bool in_lds;
        const int64_t *slice = fm_hit_tile_slice<kKeyBlock>(s_off, hit_off, h, in_lds);
        if (t <= h.tile_last) {
            const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
            int32_t s, e;
            fm_val_window(locs[t], term_len[p], max_len, text_len, s, e);
            pat[t] = p;
            start[t] = s;
            stop[t] = e;
        } else if (t < n_hits) {
            pat[t] = n;
            start[t] = stop[t] = 0;
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

// stop: the n_stop units of the set, sorted ascending (the workspace's copy)
template <bool kBitmap>
__global__ __launch_bounds__(kKeyBlock) void k_val_lengths(const uint16_t *__restrict__ stop, int32_t n_stop, const int32_t *__restrict__ pat,
                                                           int32_t n, const int64_t *__restrict__ win_off, const uint16_t *__restrict__ win,
                                                           const int32_t *__restrict__ win_status, int64_t n_hits,
                                                           int32_t *__restrict__ vlen, int32_t *__restrict__ status) {
    __shared__ uint32_t s_set[kBitmap ? kStopBitmapWords : kValuesMaxStop / 2];
    if (kBitmap) {
        for (int32_t j = threadIdx.x; j < kStopBitmapWords; j += kKeyBlock) s_set[j] = 0;
        __syncthreads();
        if (threadIdx.x == 0)  // (one lane: two units may share a word)
            for (int32_t j = 0; j < n_stop; ++j) s_set[stop[j] >> 5] |= 1u << (stop[j] & 31);
    } else {
        uint16_t *list = reinterpret_cast<uint16_t *>(s_set);
        for (int32_t j = threadIdx.x; j < n_stop; j += kKeyBlock) list[j] = stop[j];
    }
    __syncthreads();
    for (int64_t t = (int64_t)blockIdx.x * kKeyBlock + threadIdx.x; t < n_hits; t += (int64_t)gridDim.x * kKeyBlock) {
        const int32_t p = pat[t];
        if (p >= n) {
            vlen[t] = 0;
            continue;
        }
        const int64_t at = win_off[t];
        vlen[t] = fm_val_length<kBitmap>(win + at, (int32_t)(win_off[t + 1] - at), s_set, n_stop);
        const int32_t ws = win_status[t];
        // (a window the redo pass ran: the literal extract's status.)  Several lanes may store to one status[p], and the value does
        // not depend on which of them is last: every non-OK status here is ST_JAVA_AIOOBE.  A window is [s, e) with 0 <= s <= e <=
        // textLength < ix.length on an index with extraction (one without never gets here: fmx_values_of_hits_dev answers
        // ST_NOT_ENABLED for all patterns itself), so fm_extract_packed_status is ST_OK for it, and of fm_extract's statuses
        // neither the range checks (FM:566-576), nor ST_DEST_TOO_SMALL (dst_len = e - s, offset 0), nor the destination index
        // (remaining - 1 in [0, dst_len)) can fire; what is left is the status of an LF-step, and fm_lf_step and what it calls set
        // no other than ST_JAVA_AIOOBE.
        if (status && ws != ST_OK) status[p] = ws;
    }
}

// flag[i] for the hits, 0 for the slots behind them up to flag[n_hits]: the exclusive scan runs over n_hits + 1
__global__ __launch_bounds__(kFlatBlock) void k_val_run_flags(const int32_t *__restrict__ pat, int32_t n, const int32_t *__restrict__ vlen,
                                                              const int64_t *__restrict__ win_off, const uint16_t *__restrict__ win,
                                                              int64_t n_hits, int32_t *__restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i <= n_hits; i += (int64_t)gridDim.x * kFlatBlock) {
        int32_t f = 0;
        if (i < n_hits && pat[i] < n)
            f = i == 0 || pat[i - 1] != pat[i] || !fm_val_same(win + win_off[i - 1], vlen[i - 1], win + win_off[i], vlen[i]);
        flag[i] = f;
    }
}

// run_start[r] = the first hit of run r; run_start[R] = the hits in use (R = scan[n_hits])
__global__ __launch_bounds__(kFlatBlock) void k_val_run_starts(const int32_t *__restrict__ flag, const int32_t *__restrict__ scan,
                                                               const int64_t *__restrict__ hit_off, int32_t n, int64_t n_hits,
                                                               int32_t *__restrict__ run_start) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i <= n_hits; i += (int64_t)gridDim.x * kFlatBlock) {
        if (i == n_hits)
            run_start[scan[n_hits]] = (int32_t)(hit_off[n] < n_hits ? hit_off[n] : n_hits);
        else if (flag[i])
            run_start[scan[i]] = (int32_t)i;
    }
}

// slot j holds run j; the key of the first pass is the length (a slot behind the runs: anything, the last pass sends it to the end)
__global__ __launch_bounds__(kFlatBlock) void k_val_length_keys(const int32_t *__restrict__ scan, const int32_t *__restrict__ run_start,
                                                                const int32_t *__restrict__ vlen, int64_t n_hits, uint32_t *__restrict__ perm,
                                                                uint32_t *__restrict__ keys) {
    const int32_t R = scan[n_hits];
    for (int64_t j = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; j < n_hits; j += (int64_t)gridDim.x * kFlatBlock) {
        perm[j] = (uint32_t)j;
        keys[j] = j < R ? (uint32_t)vlen[run_start[j]] : 0u;
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_val_chunk_keys(const int32_t *__restrict__ scan, const int32_t *__restrict__ run_start,
                                                               const int32_t *__restrict__ vlen, const int64_t *__restrict__ win_off,
                                                               const uint16_t *__restrict__ win, int64_t n_hits, int32_t chunk,
                                                               const uint32_t *__restrict__ perm, uint64_t *__restrict__ keys) {
    const uint32_t R = (uint32_t)scan[n_hits];
    for (int64_t j = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; j < n_hits; j += (int64_t)gridDim.x * kFlatBlock) {
        const uint32_t r = perm[j];
        uint64_t key = 0;
        if (r < R) {
            const int32_t h = run_start[r];
            key = fm_val_chunk_key(win + win_off[h], vlen[h], chunk);
        }
        keys[j] = key;
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_val_pattern_keys(const int32_t *__restrict__ scan, const int32_t *__restrict__ run_start,
                                                                 const int32_t *__restrict__ pat, int32_t n, int64_t n_hits,
                                                                 const uint32_t *__restrict__ perm, uint32_t *__restrict__ keys) {
    const uint32_t R = (uint32_t)scan[n_hits];
    for (int64_t j = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; j < n_hits; j += (int64_t)gridDim.x * kFlatBlock) {
        const uint32_t r = perm[j];
        keys[j] = r < R ? (uint32_t)pat[run_start[r]] : (uint32_t)n;
    }
}

// skeys: the sorted slots' patterns (n behind the runs).  head, weight, hlen: n_hits + 1 entries each (the scans' inputs).
__global__ __launch_bounds__(kFlatBlock) void k_val_heads(const uint32_t *__restrict__ skeys, const uint32_t *__restrict__ perm, int32_t n,
                                                          const int32_t *__restrict__ run_start, const int32_t *__restrict__ vlen,
                                                          const int64_t *__restrict__ win_off, const uint16_t *__restrict__ win,
                                                          int64_t n_hits, int32_t *__restrict__ head, int32_t *__restrict__ weight,
                                                          int64_t *__restrict__ hlen) {
    for (int64_t j = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; j <= n_hits; j += (int64_t)gridDim.x * kFlatBlock) {
        int32_t f = 0, w = 0;
        int64_t len = 0;
        if (j < n_hits && skeys[j] < (uint32_t)n) {
            const uint32_t r = perm[j];
            const int32_t h = run_start[r];
            w = run_start[r + 1] - h;
            f = 1;
            if (j > 0 && skeys[j - 1] == skeys[j]) {
                const int32_t g = run_start[perm[j - 1]];
                f = !fm_val_same(win + win_off[g], vlen[g], win + win_off[h], vlen[h]);
            }
            if (f) len = vlen[h];
        }
        head[j] = f;
        weight[j] = w;
        hlen[j] = len;
    }
}

// a head stores its group's first slot, its offset into the answer's text and where its code units lie; the lane behind the last
// slot closes both lists (group_start[G] = n_hits: the weights behind the runs are 0)
__global__ __launch_bounds__(kFlatBlock) void k_val_groups(const int32_t *__restrict__ head, const int32_t *__restrict__ hscan,
                                                           const int64_t *__restrict__ lscan, const uint32_t *__restrict__ perm,
                                                           const int32_t *__restrict__ run_start, const int64_t *__restrict__ win_off,
                                                           const uint16_t *__restrict__ win, int64_t n_hits, int32_t *__restrict__ group_start,
                                                           int64_t *__restrict__ text_off, const uint16_t **__restrict__ group_src) {
    for (int64_t j = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; j <= n_hits; j += (int64_t)gridDim.x * kFlatBlock) {
        if (j == n_hits) {
            group_start[hscan[j]] = (int32_t)n_hits;
            text_off[hscan[j]] = lscan[j];
        } else if (head[j]) {
            const int32_t g = hscan[j];
            group_start[g] = (int32_t)j;
            text_off[g] = lscan[j];
            group_src[g] = win + win_off[run_start[perm[j]]];
        }
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_val_counts(const int32_t *__restrict__ hscan, const int32_t *__restrict__ wscan,
                                                           const int32_t *__restrict__ group_start, int64_t n_hits, int32_t *__restrict__ count) {
    const int32_t G = hscan[n_hits];
    for (int64_t g = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; g < G; g += (int64_t)gridDim.x * kFlatBlock)
        count[g] = wscan[group_start[g + 1]] - wscan[group_start[g]];
}

__global__ __launch_bounds__(kFlatBlock) void k_val_offsets(const uint32_t *__restrict__ skeys, const int32_t *__restrict__ hscan, int32_t n,
                                                            int64_t n_hits, int64_t *__restrict__ val_off) {
    for (int64_t p = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; p <= n; p += (int64_t)gridDim.x * kFlatBlock)
        val_off[p] = hscan[fm_val_lower_bound(skeys, n_hits, (uint32_t)p)];
}

__global__ __launch_bounds__(kFlatBlock) void k_val_fill(const uint16_t *const *__restrict__ group_src, const int64_t *__restrict__ text_off,
                                                         int64_t G, uint16_t *__restrict__ chars) {
    for (int64_t g = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; g < G; g += (int64_t)gridDim.x * kFlatBlock) {
        const int64_t at = text_off[g];
        const int32_t len = (int32_t)(text_off[g + 1] - at);
        const uint16_t *src = group_src[g];
        for (int32_t k = 0; k < len; ++k) chars[at + k] = src[k];
    }
}

// THE GROUP OF EVERY HIT (launch_values_groups_of_hits): sorted slot j holds run perm[j], and its group is the number of heads up to
// and including it, less one — hscan is exclusive.  perm is a permutation of the slots, so every run is stored by one lane.
__global__ __launch_bounds__(kFlatBlock) void k_val_run_groups(const uint32_t *__restrict__ skeys, const uint32_t *__restrict__ perm, int32_t n,
                                                               const int32_t *__restrict__ head, const int32_t *__restrict__ hscan,
                                                               int64_t n_hits, int32_t *__restrict__ run_group) {
    for (int64_t j = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; j < n_hits; j += (int64_t)gridDim.x * kFlatBlock)
        if (skeys[j] < (uint32_t)n) run_group[perm[j]] = hscan[j] + head[j] - 1;
}

// a lane per hit: its run is the number of run flags up to and including it, less one (scan is exclusive over n_hits + 1, so that
// number is scan[i + 1]); its group counts from its pattern's first group.  A slot that is no hit gets -1.
__global__ __launch_bounds__(kFlatBlock) void k_val_hit_groups(const int32_t *__restrict__ pat, int32_t n, const int32_t *__restrict__ scan,
                                                               const int32_t *__restrict__ run_group, const int64_t *__restrict__ val_off,
                                                               int64_t n_hits, int32_t *__restrict__ group_of_hit) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < n_hits; i += (int64_t)gridDim.x * kFlatBlock) {
        const int32_t p = pat[i];
        group_of_hit[i] = p < n ? (int32_t)(run_group[scan[i + 1] - 1] - val_off[p]) : -1;
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_val_status_all(int32_t *__restrict__ status, int32_t n, int32_t value) {
    for (int64_t p = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kFlatBlock) status[p] = value;
}

// the regions of the caller's workspace, each a multiple of 256 bytes.  group_src stands first: fmx_values_fill_dev finds it
// without knowing the batch.  tables: term_len (n ints), then the stop set's units sorted (kValuesMaxStop) — one copy.
// key32_a / key32_b (the length and the pattern pass) lie in key64_a / key64_b (the chunk passes between them); head lies in flag
// (dead once the runs' starts are stored).
struct ValWs {
    size_t group_src, pat, start, stop, win_off, piece_off, win_status, extract, extract_bytes, win, vlen, flag, scan, run_start, perm_a, perm_b,
        key64_a, key64_b, weight, hlen, hscan, wscan, lscan, group_start, tables, tables_bytes, t_stop, tmp, tmp_bytes, total;
};
ValWs val_ws(int32_t n, int64_t n_hits, int32_t max_len) {
    ValWs w{};
    const size_t H = (size_t)n_hits;
    size_t s64 = 0, s32 = 0, c32 = 0, c64 = 0;
    (void)rocprim::radix_sort_pairs(nullptr, s64, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                    H, 0u, 64u);
    (void)rocprim::radix_sort_pairs(nullptr, s32, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                    H, 0u, 32u);
    (void)rocprim::exclusive_scan(nullptr, c32, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, H + 1, rocprim::plus<int32_t>());
    (void)rocprim::exclusive_scan(nullptr, c64, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, H + 1, rocprim::plus<int64_t>());
    w.tmp_bytes = pad256(std::max(std::max(s64, s32), std::max(c32, c64)));
    w.t_stop = (size_t)n * 4;
    w.tables_bytes = w.t_stop + kValuesMaxStop * 2;
    w.extract_bytes = extract_packed_scratch_bytes((int32_t)n_hits);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.group_src = take(H * 8);
    w.pat = take(H * 4);
    w.start = take(H * 4);
    w.stop = take(H * 4);
    w.win_off = take((H + 1) * 8);
    w.piece_off = take((H + 1) * 8);
    w.win_status = take(H * 4);
    w.extract = take(w.extract_bytes);
    w.win = take(H * (size_t)max_len * 2 + 8);
    w.vlen = take(H * 4);
    w.flag = take((H + 1) * 4);
    w.scan = take((H + 1) * 4);
    w.run_start = take((H + 1) * 4);
    w.perm_a = take(H * 4);
    w.perm_b = take(H * 4);
    w.key64_a = take(H * 8);
    w.key64_b = take(H * 8);
    w.weight = take((H + 1) * 4);
    w.hlen = take((H + 1) * 8);
    w.hscan = take((H + 1) * 4);
    w.wscan = take((H + 1) * 4);
    w.lscan = take((H + 1) * 8);
    w.group_start = take((H + 1) * 4);
    w.tables = take(w.tables_bytes);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}
bool shape_ok(int32_t n, int64_t n_hits, int32_t max_len) {
    return n > 0 && n_hits > 0 && n_hits <= 0x7fffffff && max_len >= 1 && max_len <= kValuesMaxLen && n_hits * max_len <= kValuesMaxUnits;
}

template <class T>
T *region(void *ws, size_t off) {
    return reinterpret_cast<T *>(static_cast<uint8_t *>(ws) + off);
}

}  // namespace

size_t values_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t max_len) {
    return shape_ok(n, n_hits, max_len) ? val_ws(n, n_hits, max_len).total : 0;
}

bool values_windows(void *ws, size_t ws_bytes, int32_t n, int64_t n_hits, int32_t max_len, ValuesWindows *out) {
    if (!ws || !shape_ok(n, n_hits, max_len)) return false;
    const ValWs w = val_ws(n, n_hits, max_len);
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

int launch_values_ranges(int32_t text_len, int n_cu, int32_t n, const int32_t *term_len, const uint16_t *stop, int32_t n_stop, int32_t max_len,
                         const int64_t *hit_off, const int32_t *locs, int64_t n_hits, void *ws, size_t ws_bytes, void *stream) {
    if (!shape_ok(n, n_hits, max_len) || n_stop < 0 || n_stop > kValuesMaxStop) return (int)hipErrorInvalidValue;
    const ValWs w = val_ws(n, n_hits, max_len);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    // the tables: the lengths and the stop set, sorted.  The runtime has read this block when the copy returns (a copy from
    // pageable host memory is staged before the call comes back).
    std::vector<uint8_t> host(w.tables_bytes, 0);
    memcpy(host.data(), term_len, (size_t)n * 4);
    if (n_stop > 0) {
        uint16_t *set = reinterpret_cast<uint16_t *>(host.data() + w.t_stop);
        memcpy(set, stop, (size_t)n_stop * 2);
        std::sort(set, set + n_stop);
    }
    if (hipError_t e = hipMemcpyAsync(region<uint8_t>(ws, w.tables), host.data(), w.tables_bytes, hipMemcpyHostToDevice, st); e != hipSuccess)
        return (int)e;
    int32_t key_grid = 1, flat = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hipLaunchKernelGGL(k_val_ranges, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, hit_off, n, locs, n_hits, region<const int32_t>(ws, w.tables),
                       max_len, text_len, region<int32_t>(ws, w.pat), region<int32_t>(ws, w.start), region<int32_t>(ws, w.stop));
    return (int)hipGetLastError();
}

namespace {

// the workspace of the twin that also stores the group of every hit: val_ws, and behind it run_group (a group per run)
size_t groups_of_hits_ws_total(const ValWs &w, int64_t n_hits) { return w.total + pad256(((size_t)n_hits + 1) * 4); }

// group_of_hit == nullptr: launch_values_groups as it always was (nothing behind w.total is touched)
int values_groups_impl(int n_cu, int32_t n, int32_t n_stop, int32_t max_len, int64_t n_hits, const int64_t *hit_off, int64_t *val_off,
                       int32_t *count, int64_t *text_off, int32_t *status, int32_t *group_of_hit, void *ws, size_t ws_bytes, void *stream) {
    if (!shape_ok(n, n_hits, max_len) || n_stop < 0 || n_stop > kValuesMaxStop) return (int)hipErrorInvalidValue;
    const ValWs w = val_ws(n, n_hits, max_len);
    if (!ws || ws_bytes < (group_of_hit ? groups_of_hits_ws_total(w, n_hits) : w.total)) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int32_t *pat = region<int32_t>(ws, w.pat), *win_status = region<int32_t>(ws, w.win_status);
    const int64_t *win_off = region<int64_t>(ws, w.win_off);
    const uint16_t *win = region<uint16_t>(ws, w.win), *d_stop = region<uint16_t>(ws, w.tables + w.t_stop);
    int32_t *vlen = region<int32_t>(ws, w.vlen), *flag = region<int32_t>(ws, w.flag), *scan = region<int32_t>(ws, w.scan);
    int32_t *run_start = region<int32_t>(ws, w.run_start), *head = flag, *weight = region<int32_t>(ws, w.weight);
    uint32_t *perm_a = region<uint32_t>(ws, w.perm_a), *perm_b = region<uint32_t>(ws, w.perm_b);
    uint64_t *key64_a = region<uint64_t>(ws, w.key64_a), *key64_b = region<uint64_t>(ws, w.key64_b);
    uint32_t *key32_a = region<uint32_t>(ws, w.key64_a), *key32_b = region<uint32_t>(ws, w.key64_b);
    int64_t *hlen = region<int64_t>(ws, w.hlen), *lscan = region<int64_t>(ws, w.lscan);
    int32_t *hscan = region<int32_t>(ws, w.hscan), *wscan = region<int32_t>(ws, w.wscan), *group_start = region<int32_t>(ws, w.group_start);
    const uint16_t **group_src = region<const uint16_t *>(ws, w.group_src);
    void *tmp = region<uint8_t>(ws, w.tmp);
    size_t tmp_bytes = w.tmp_bytes;
    int32_t key_grid = 1, flat = 1, unused = 1, pat_grid = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hit_lines_geometry(n, n_cu, &unused, &pat_grid);  // (the element-wise grid over n + 1 items)
    const dim3 fg((unsigned)flat), fb(kFlatBlock);
    const size_t H = (size_t)n_hits;
#define FMX_VAL_CHECK(call) \
    if (hipError_t e_ = (call); e_ != hipSuccess) return (int)e_
    hipLaunchKernelGGL(k_val_lengths<!FMX_VALUES_STOP_LIST>, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, d_stop, n_stop, pat, n, win_off, win,
                       win_status, n_hits, vlen, status);
    FMX_VAL_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_val_run_flags, fg, fb, 0, st, pat, n, vlen, win_off, win, n_hits, flag);
    FMX_VAL_CHECK(hipGetLastError());
    FMX_VAL_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, flag, scan, (int32_t)0, H + 1, rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(k_val_run_starts, fg, fb, 0, st, flag, scan, hit_off, n, n_hits, run_start);
    FMX_VAL_CHECK(hipGetLastError());
    // the exact grouping: stable passes, the least significant first
    hipLaunchKernelGGL(k_val_length_keys, fg, fb, 0, st, scan, run_start, vlen, n_hits, perm_a, key32_a);
    FMX_VAL_CHECK(hipGetLastError());
    FMX_VAL_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key32_a, key32_b, perm_a, perm_b, H, 0u, (unsigned)fm_bits(kValuesMaxLen), st));
    std::swap(perm_a, perm_b);
    for (int32_t c = fm_val_chunks(max_len) - 1; c >= 0; --c) {
        hipLaunchKernelGGL(k_val_chunk_keys, fg, fb, 0, st, scan, run_start, vlen, win_off, win, n_hits, c, perm_a, key64_a);
        FMX_VAL_CHECK(hipGetLastError());
        FMX_VAL_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key64_a, key64_b, perm_a, perm_b, H, 0u, 64u, st));
        std::swap(perm_a, perm_b);
    }
    hipLaunchKernelGGL(k_val_pattern_keys, fg, fb, 0, st, scan, run_start, pat, n, n_hits, perm_a, key32_a);
    FMX_VAL_CHECK(hipGetLastError());
    FMX_VAL_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key32_a, key32_b, perm_a, perm_b, H, 0u, (unsigned)fm_bits((uint32_t)n), st));
    std::swap(perm_a, perm_b);
    const uint32_t *skeys = key32_b;
    hipLaunchKernelGGL(k_val_heads, fg, fb, 0, st, skeys, perm_a, n, run_start, vlen, win_off, win, n_hits, head, weight, hlen);
    FMX_VAL_CHECK(hipGetLastError());
    FMX_VAL_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, head, hscan, (int32_t)0, H + 1, rocprim::plus<int32_t>(), st));
    FMX_VAL_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, weight, wscan, (int32_t)0, H + 1, rocprim::plus<int32_t>(), st));
    FMX_VAL_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, hlen, lscan, (int64_t)0, H + 1, rocprim::plus<int64_t>(), st));
    hipLaunchKernelGGL(k_val_groups, fg, fb, 0, st, head, hscan, lscan, perm_a, run_start, win_off, win, n_hits, group_start, text_off, group_src);
    FMX_VAL_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_val_counts, fg, fb, 0, st, hscan, wscan, group_start, n_hits, count);
    FMX_VAL_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_val_offsets, dim3((unsigned)pat_grid), fb, 0, st, skeys, hscan, n, n_hits, val_off);
    if (group_of_hit) {
        FMX_VAL_CHECK(hipGetLastError());
        int32_t *run_group = region<int32_t>(ws, w.total);
        hipLaunchKernelGGL(k_val_run_groups, fg, fb, 0, st, skeys, perm_a, n, head, hscan, n_hits, run_group);
        FMX_VAL_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_val_hit_groups, fg, fb, 0, st, pat, n, scan, run_group, val_off, n_hits, group_of_hit);
    }
#undef FMX_VAL_CHECK
    return (int)hipGetLastError();
}

}  // namespace

int launch_values_groups(int n_cu, int32_t n, int32_t n_stop, int32_t max_len, int64_t n_hits, const int64_t *hit_off,
                         int64_t *val_off, int32_t *count, int64_t *text_off, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    return values_groups_impl(n_cu, n, n_stop, max_len, n_hits, hit_off, val_off, count, text_off, status, nullptr, ws, ws_bytes, stream);
}

size_t values_groups_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t max_len) {
    return shape_ok(n, n_hits, max_len) ? groups_of_hits_ws_total(val_ws(n, n_hits, max_len), n_hits) : 0;
}

int launch_values_groups_of_hits(int n_cu, int32_t n, int32_t n_stop, int32_t max_len, int64_t n_hits, const int64_t *hit_off, int64_t *val_off,
                                 int32_t *count, int64_t *text_off, int32_t *status, int32_t *group_of_hit, void *ws, size_t ws_bytes,
                                 void *stream) {
    if (!group_of_hit) return (int)hipErrorInvalidValue;
    return values_groups_impl(n_cu, n, n_stop, max_len, n_hits, hit_off, val_off, count, text_off, status, group_of_hit, ws, ws_bytes, stream);
}

int launch_values_fill(int n_cu, int64_t groups, const int64_t *text_off, uint16_t *chars, const void *ws, void *stream) {
    if (groups <= 0) return 0;
    int32_t unused = 1, flat = 1;
    hit_lines_geometry(groups, n_cu, &unused, &flat);
    hipLaunchKernelGGL(k_val_fill, dim3((unsigned)flat), dim3(kFlatBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *const *>(ws), text_off, groups, chars);
    return (int)hipGetLastError();
}

int launch_values_status_all(int n_cu, int32_t *status, int32_t n, int32_t value, void *stream) {
    if (!status || n <= 0) return 0;
    int32_t unused = 1, flat = 1;
    hit_lines_geometry(n, n_cu, &unused, &flat);
    hipLaunchKernelGGL(k_val_status_all, dim3((unsigned)flat), dim3(kFlatBlock), 0, static_cast<hipStream_t>(stream), status, n, value);
    return (int)hipGetLastError();
}

}  // namespace fmx
