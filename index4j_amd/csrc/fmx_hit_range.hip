// fmx_hit_range.hip — packed hits of a batch of patterns -> THE PACKED HITS WHOSE NUMBER LIES IN A RANGE
// (fmx_hits_in_number_range_dev, fmx_match_query_number_batch; fmx_hit_range.hpp has the definition and the per-item functions).  The
// windows' text is the packed extract's (fmx_extract_packed.hip), which the C-ABI layer runs between launch_range_windows and
// launch_range_keep over the ranges the former leaves in the workspace.
//
// Lanes go to slots, never to patterns:
//   k_range_windows   a lane per packed slot, k_num_ranges' tile loop (fm_hit_tile / fm_hit_tile_slice / fm_hit_pattern; 16 KiB of
//                     LDS for the slice of hit_off, no fences: no line is asked for): the slot's pattern and its window [s, e).  A
//                     slot of an UNRANGED pattern, a slot in front of hit_off[0] and a slot behind hit_off[n] get an empty window
//                     (the pattern n for a slot that is no hit): the packed extract walks nothing for them, so a call whose ranged
//                     terms are rare pays for those hits only
//   (packed extract)  both of its stages over the n_hits windows, redo launch included: 32 code units per hit of a ranged pattern
//   k_range_flags     a lane per slot: unranged — keep; ranged — fm_range_code (fm_num_parse and the two comparisons; neighbouring
//                     lanes read neighbouring windows of the packed text, as k_num_parse); the flag of the compaction and the
//                     word of the two reasons; a window the extract ran literally hands its status to its pattern
//   rocPRIM           two exclusive scans over n_hits + 1 entries: of the flags (where each kept hit goes), of the reasons' words
//   k_hit_keep_store  fmx_hit_filter.hip's stable store through launch_hit_keep_store: kept_locs and kept_off
//   k_range_tails     a lane per pattern: kept, not_number and overflow off the scans at hit_off[p] / hit_off[p + 1]
// Integers only, no atomics: the result does not depend on the order the lanes run in.  Nothing here looks at the image, so this
// file is compiled once, like fmx_hit_numbers.hip.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <cstring>
#include <vector>

#include "fmx_hit_range.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_range_windows: a tile of kLocateAllTile slots per round; 16 KiB of LDS
constexpr int kFlatBlock = 256;  // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

__global__ __launch_bounds__(kKeyBlock) void k_range_windows(const int64_t *__restrict__ hit_off, int32_t n, const int32_t *__restrict__ locs,
                                                             int64_t n_hits, const int32_t *__restrict__ term_len,
                                                             const int64_t *__restrict__ num_lo, int32_t text_len,
                                                             int32_t *__restrict__ pattern, int32_t *__restrict__ start,
                                                             int32_t *__restrict__ stop) {
    __shared__ int64_t s_off[kLocateAllSlice];
    const int64_t first = fm_filter_slot(hit_off[0], n_hits), total = fm_filter_slot(hit_off[n], n_hits);
    for (int64_t tile = (int64_t)blockIdx.x * kLocateAllTile; tile < n_hits; tile += (int64_t)gridDim.x * kLocateAllTile) {
        const int64_t t = tile + threadIdx.x;
        if (tile >= total || tile + kLocateAllTile <= first) {  // a tile of slots behind or in front of the hits (workgroup-uniform)
            if (t < n_hits) {
                pattern[t] = n;
                start[t] = stop[t] = 0;
            }
            continue;
        }
        const HitTile h = fm_hit_tile(hit_off, n, tile, total);
        bool in_lds;
        const int64_t *slice = fm_hit_tile_slice<kKeyBlock>(s_off, hit_off, h, in_lds);
        if (t >= first && t <= h.tile_last) {
            const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
            int32_t s = 0, e = 0;
            if (fm_range_ranged(num_lo[p])) fm_val_window(locs[t], term_len[p], kNumWindow, text_len, s, e);
            pattern[t] = p;
            start[t] = s;
            stop[t] = e;
        } else if (t < n_hits) {
            pattern[t] = n;
            start[t] = stop[t] = 0;
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

// extract == false (an index built without extraction): no window has text — a ranged pattern keeps nothing
__global__ __launch_bounds__(kFlatBlock) void k_range_flags(const int32_t *__restrict__ pattern, const int64_t *__restrict__ win_off,
                                                            const uint16_t *__restrict__ win, const int32_t *__restrict__ win_status,
                                                            int64_t n_hits, int32_t n, bool extract, int32_t frac_digits,
                                                            const int64_t *__restrict__ num_lo, const int64_t *__restrict__ num_hi,
                                                            int32_t *__restrict__ flag, uint64_t *__restrict__ tail,
                                                            int32_t *__restrict__ status) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // (the scans then leave the totals there)
        flag[n_hits] = 0;
        tail[n_hits] = 0;
    }
    for (int64_t t = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; t < n_hits; t += (int64_t)gridDim.x * kFlatBlock) {
        const int32_t p = pattern[t];
        int32_t code = kRangeOutside;
        if (p < n) {
            const int64_t lo = num_lo[p];
            if (!fm_range_ranged(lo)) {
                code = kRangeKeep;
            } else if (extract) {
                const int64_t at = win_off[t];
                code = fm_range_code(win + at, (int32_t)(win_off[t + 1] - at), frac_digits, lo, num_hi[p]);
                // (a window the redo pass ran: the literal extract's status, by k_num_parse's rule — every non-OK status here is the
                // same one, so the value does not depend on which lane stores last)
                const int32_t ws = win_status[t];
                if (status && ws != ST_OK) status[p] = ws;
            }
        }
        flag[t] = code == kRangeKeep ? 1 : 0;
        tail[t] = fm_range_tail(code);
    }
}

// pos, tail_pos = the exclusive scans of flag and tail (n_hits + 1 entries each)
__global__ __launch_bounds__(kFlatBlock) void k_range_tails(const int32_t *__restrict__ pos, const uint64_t *__restrict__ tail_pos,
                                                            const int64_t *__restrict__ hit_off, int32_t n, int64_t n_hits,
                                                            const int64_t *__restrict__ num_lo, bool extract, int32_t not_enabled,
                                                            int32_t *__restrict__ kept, int32_t *__restrict__ not_number,
                                                            int32_t *__restrict__ overflow, int32_t *__restrict__ status) {
    const int64_t first = fm_filter_slot(hit_off[0], n_hits);
    for (int64_t p = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kFlatBlock) {
        int64_t a = fm_filter_slot(hit_off[p], n_hits), b = fm_filter_slot(hit_off[p + 1], n_hits);
        a = a < first ? first : a;
        b = b < a ? a : b;
        if (kept) kept[p] = pos[b] - pos[a];
        if (not_number) not_number[p] = fm_range_not_number(tail_pos, a, b);
        if (overflow) overflow[p] = fm_range_overflow(tail_pos, a, b);
        if (!extract && status && fm_range_ranged(num_lo[p])) status[p] = not_enabled;
    }
}

// the regions of the caller's workspace, each a multiple of 256 bytes.  tables: num_lo (n int64), num_hi (n int64), term_len (n
// ints) — one copy.
struct RangeWs {
    size_t tables, tables_bytes, t_hi, t_len, pattern, start, stop, win_off, piece_off, win_status, extract, extract_bytes, win, flag, pos, tail,
        tail_pos, tmp, tmp_bytes, total;
};
RangeWs range_ws(int32_t n, int64_t n_hits) {
    RangeWs w{};
    const size_t H = (size_t)n_hits;
    size_t scan32 = 0, scan64 = 0;
    (void)rocprim::exclusive_scan(nullptr, scan32, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, H + 1, rocprim::plus<int32_t>());
    (void)rocprim::exclusive_scan(nullptr, scan64, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, H + 1, rocprim::plus<uint64_t>());
    w.tmp_bytes = pad256(scan32 > scan64 ? scan32 : scan64);
    w.t_hi = (size_t)n * 8;
    w.t_len = w.t_hi + (size_t)n * 8;
    w.tables_bytes = w.t_len + (size_t)n * 4;
    w.extract_bytes = extract_packed_scratch_bytes((int32_t)n_hits);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.tables = take(w.tables_bytes);
    w.pattern = take(H * 4);
    w.start = take(H * 4);
    w.stop = take(H * 4);
    w.win_off = take((H + 1) * 8);
    w.piece_off = take((H + 1) * 8);
    w.win_status = take(H * 4);
    w.extract = take(w.extract_bytes);
    w.win = take(H * (size_t)kNumWindow * 2 + 8);
    w.flag = take((H + 1) * 4);
    w.pos = take((H + 1) * 4);
    w.tail = take((H + 1) * 8);
    w.tail_pos = take((H + 1) * 8);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}

bool range_shape_ok(int32_t n, int64_t n_hits) { return n > 0 && n_hits > 0 && n_hits <= 0x7fffffff; }

template <class T>
T *region(void *ws, size_t off) {
    return reinterpret_cast<T *>(static_cast<uint8_t *>(ws) + off);
}

}  // namespace

size_t hits_in_number_range_scratch_bytes(int32_t n, int64_t n_hits) { return range_shape_ok(n, n_hits) ? range_ws(n, n_hits).total : 0; }

bool range_windows(void *ws, size_t ws_bytes, int32_t n, int64_t n_hits, ValuesWindows *out) {
    if (!ws || !range_shape_ok(n, n_hits)) return false;
    const RangeWs w = range_ws(n, n_hits);
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

int launch_range_windows(int32_t text_len, int n_cu, int32_t n, const int32_t *term_len, const int64_t *num_lo, const int64_t *num_hi,
                         const int64_t *hit_off, const int32_t *locs, int64_t n_hits, void *ws, size_t ws_bytes, void *stream) {
    if (!range_shape_ok(n, n_hits) || !term_len || !num_lo || !num_hi || !hit_off || !locs || text_len < 0) return (int)hipErrorInvalidValue;
    const RangeWs w = range_ws(n, n_hits);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    // the tables.  The runtime has read this block when the copy returns (a copy from pageable host memory is staged before the
    // call comes back).
    std::vector<uint8_t> host(w.tables_bytes + 8, 0);
    memcpy(host.data(), num_lo, (size_t)n * 8);
    memcpy(host.data() + w.t_hi, num_hi, (size_t)n * 8);
    memcpy(host.data() + w.t_len, term_len, (size_t)n * 4);
    if (hipError_t e = hipMemcpyAsync(region<uint8_t>(ws, w.tables), host.data(), w.tables_bytes, hipMemcpyHostToDevice, st); e != hipSuccess)
        return (int)e;
    int32_t key_grid = 1, flat = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hipLaunchKernelGGL(k_range_windows, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, hit_off, n, locs, n_hits,
                       region<const int32_t>(ws, w.tables + w.t_len), region<const int64_t>(ws, w.tables), text_len, region<int32_t>(ws, w.pattern),
                       region<int32_t>(ws, w.start), region<int32_t>(ws, w.stop));
    return (int)hipGetLastError();
}

int launch_range_keep(int n_cu, int32_t n, bool extract, int32_t not_enabled, int32_t frac_digits, const int64_t *hit_off, const int32_t *locs,
                      int64_t n_hits, int64_t *kept_off, int32_t *kept_locs, int32_t *kept, int32_t *not_number, int32_t *overflow,
                      int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    if (!range_shape_ok(n, n_hits) || frac_digits < 0 || frac_digits > kNumFracMax || !hit_off || !locs || !kept_off || !kept_locs)
        return (int)hipErrorInvalidValue;
    const RangeWs w = range_ws(n, n_hits);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t *flag = region<int32_t>(ws, w.flag), *pos = region<int32_t>(ws, w.pos);
    uint64_t *tail = region<uint64_t>(ws, w.tail), *tail_pos = region<uint64_t>(ws, w.tail_pos);
    const int64_t *num_lo = region<const int64_t>(ws, w.tables), *num_hi = region<const int64_t>(ws, w.tables + w.t_hi);
    void *tmp = region<uint8_t>(ws, w.tmp);
    size_t tmp_bytes = w.tmp_bytes;
    int32_t unused = 1, flat = 1, pat_grid = 1;
    hit_lines_geometry(n_hits, n_cu, &unused, &flat);
    hit_lines_geometry(n, n_cu, &unused, &pat_grid);
    const dim3 fb(kFlatBlock);
#define FMX_RANGE_CHECK(call) \
    if (hipError_t e_ = (call); e_ != hipSuccess) return (int)e_
    hipLaunchKernelGGL(k_range_flags, dim3((unsigned)flat), fb, 0, st, region<const int32_t>(ws, w.pattern), region<const int64_t>(ws, w.win_off),
                       region<const uint16_t>(ws, w.win), region<const int32_t>(ws, w.win_status), n_hits, n, extract, frac_digits, num_lo, num_hi,
                       flag, tail, status);
    FMX_RANGE_CHECK(hipGetLastError());
    const size_t H1 = (size_t)n_hits + 1;
    FMX_RANGE_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, flag, pos, (int32_t)0, H1, rocprim::plus<int32_t>(), st));
    FMX_RANGE_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, tail, tail_pos, (uint64_t)0, H1, rocprim::plus<uint64_t>(), st));
    if (const int e = launch_hit_keep_store(flat, flag, pos, hit_off, n, locs, n_hits, kept_off, kept_locs, stream)) return e;
    if (kept || not_number || overflow || (!extract && status)) {
        hipLaunchKernelGGL(k_range_tails, dim3((unsigned)pat_grid), fb, 0, st, pos, tail_pos, hit_off, n, n_hits, num_lo, extract, not_enabled, kept,
                           not_number, overflow, status);
        FMX_RANGE_CHECK(hipGetLastError());
    }
#undef FMX_RANGE_CHECK
    return 0;
}

}  // namespace fmx
