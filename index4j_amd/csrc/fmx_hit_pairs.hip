// fmx_hit_pairs.hip — two first-hit lists joined through the line (fmx_pairs_of_first_hits_dev; fmx_hit_pairs.hpp has the definition
// and the per-item functions): per pair (pair_a[j], pair_b[j]) of key patterns the distinct pairs of groups (ga, gb) with their lines,
// and the JOINED LISTS — per pair the lines that have a pair key, ascending, each with the index of its pair — in the form of stage
// a's and b's answers, so that stage c (fmx_numbers_by_key_dev) runs over them unchanged.
//
// Every stage hands lanes to SLOTS (the first hits of the a-sides, pair after pair), to sorted slots, or to pairs of the call:
//   k_pair_lens     a lane per pair of the call: the first hits of its a-side; rocPRIM's exclusive scan makes slot_off (c + 1)
//   k_pair_keys     a lane per slot: its pair (fm_by_row_pattern over slot_off), its line, ONE lower bound in the b-side's first lines
//                   (fm_pair_slot_key) and the key pair | ga | gb; a slot without a partner or behind slot_off[c] gets the pair c
//   rocPRIM         ONE stable device-wide radix sort of (key, slot) over the bits in use
//   k_pair_heads    1 where a sorted slot's key differs from its predecessor's; rocPRIM's exclusive scan numbers the pairs
//   k_pair_store    a head stores ga, gb and the length of its run (an upper bound, no walk); a lane per pair of the call reads
//                   pair_off off the scan
//   k_pair_back     a lane per sorted slot: the index of its pair within pair j back to the slot it came from, and the slot's flag;
//                   rocPRIM's exclusive scan over the flags in slot order numbers the joined entries
//   k_pair_compact  a flagged slot stores its line and its pair's index; a lane per pair of the call reads joined_off off the scan
// No atomics: the result does not depend on the order the lanes run in.  Nothing here looks at the image or the line table, so this
// file is compiled once, like fmx_hit_first.hip.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fmx_hit_pairs.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kFlatBlock = 256;  // every kernel here is element-wise

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

// the tables of a call in the workspace: pair_a, pair_b (c ints each), val_off (m + 1)
struct PairTables {
    const int32_t *pair_a, *pair_b;
    const int64_t *val_off;
};

__global__ __launch_bounds__(kFlatBlock) void k_pair_lens(PairTables t, int32_t c, const int64_t *__restrict__ first_off, int64_t *__restrict__ len) {
    for (int64_t j = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; j <= c; j += (int64_t)gridDim.x * kFlatBlock)
        len[j] = j < c ? first_off[t.pair_a[j] + 1] - first_off[t.pair_a[j]] : 0;
}

__global__ __launch_bounds__(kFlatBlock) void k_pair_keys(PairTables t, int32_t c, const int64_t *__restrict__ slot_off,
                                                          const int64_t *__restrict__ first_off, const int32_t *__restrict__ first_lines,
                                                          const int32_t *__restrict__ group_of_first, int64_t n_slots, int32_t a_bits, int32_t b_bits,
                                                          uint64_t *__restrict__ keys, uint32_t *__restrict__ slots, int32_t *__restrict__ line_of) {
    const uint64_t no_pair = fm_pair_key(c, 0, 0, a_bits, b_bits);
    const int64_t real = slot_off[c];
    for (int64_t s = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; s < n_slots; s += (int64_t)gridDim.x * kFlatBlock) {
        uint64_t key = no_pair;
        int32_t line = 0;
        if (s < real) {
            const int32_t j = fm_by_row_pattern(slot_off, c, s), a = t.pair_a[j], b = t.pair_b[j];
            key = fm_pair_slot_key(first_lines, group_of_first, first_off[a] + (s - slot_off[j]), first_off[b], first_off[b + 1], j, c,
                                   t.val_off[a + 1] - t.val_off[a], t.val_off[b + 1] - t.val_off[b], a_bits, b_bits, &line);
        }
        keys[s] = key;
        slots[s] = (uint32_t)s;
        line_of[s] = line;
    }
}

// head[i] for the sorted slots, and head[n_slots] = 0: the exclusive scan then leaves the number of all pairs there
__global__ __launch_bounds__(kFlatBlock) void k_pair_heads(const uint64_t *__restrict__ keys, int64_t n_slots, int32_t c, int32_t a_bits, int32_t b_bits,
                                                           int32_t *__restrict__ head) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i <= n_slots; i += (int64_t)gridDim.x * kFlatBlock)
        head[i] = i < n_slots && fm_pair_head(keys, i, c, a_bits, b_bits) ? 1 : 0;
}

// pos = the exclusive scan of head
__global__ __launch_bounds__(kFlatBlock) void k_pair_store(const uint64_t *__restrict__ keys, const int32_t *__restrict__ head,
                                                           const int32_t *__restrict__ pos, int64_t n_slots, int32_t c, int32_t a_bits, int32_t b_bits,
                                                           int64_t *__restrict__ pair_off, int32_t *__restrict__ pair_group_a,
                                                           int32_t *__restrict__ pair_group_b, int32_t *__restrict__ pair_lines) {
    const int64_t lane = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x, lanes = (int64_t)gridDim.x * kFlatBlock;
    for (int64_t i = lane; i < n_slots; i += lanes)
        if (head[i]) {
            const uint64_t key = keys[i];
            pair_group_a[pos[i]] = fm_pair_key_a(key, a_bits, b_bits);
            pair_group_b[pos[i]] = fm_pair_key_b(key, b_bits);
            pair_lines[pos[i]] = (int32_t)fm_pair_run_length(keys, n_slots, i);
        }
    for (int64_t j = lane; j <= c; j += lanes) pair_off[j] = pos[fm_pair_first_slot(keys, n_slots, (int32_t)j, a_bits, b_bits)];
}

// pair_of[s] = the index of slot s's pair among the pairs of its j (a slot without a partner: untouched, its flag is 0);
// flag[n_slots] = 0: the exclusive scan then leaves the number of all joined entries there
__global__ __launch_bounds__(kFlatBlock) void k_pair_back(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ slots,
                                                          const int32_t *__restrict__ head, const int32_t *__restrict__ pos,
                                                          const int64_t *__restrict__ pair_off, int64_t n_slots, int32_t c, int32_t a_bits,
                                                          int32_t b_bits, int32_t *__restrict__ pair_of, int32_t *__restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i <= n_slots; i += (int64_t)gridDim.x * kFlatBlock) {
        if (i == n_slots) {
            flag[i] = 0;
            continue;
        }
        const int32_t j = fm_pair_key_pair(keys[i], a_bits, b_bits);
        const uint32_t s = slots[i];
        flag[s] = j < c ? 1 : 0;
        if (j < c) pair_of[s] = (int32_t)(pos[i] + head[i] - 1 - pair_off[j]);
    }
}

// at = the exclusive scan of flag, in slot order
__global__ __launch_bounds__(kFlatBlock) void k_pair_compact(const int32_t *__restrict__ flag, const int32_t *__restrict__ at,
                                                             const int32_t *__restrict__ line_of, const int32_t *__restrict__ pair_of,
                                                             const int64_t *__restrict__ slot_off, int64_t n_slots, int32_t c,
                                                             int64_t *__restrict__ joined_off, int32_t *__restrict__ joined_lines,
                                                             int32_t *__restrict__ joined_group) {
    const int64_t lane = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x, lanes = (int64_t)gridDim.x * kFlatBlock;
    for (int64_t s = lane; s < n_slots; s += lanes)
        if (flag[s]) {
            joined_lines[at[s]] = line_of[s];
            joined_group[at[s]] = pair_of[s];
        }
    for (int64_t j = lane; j <= c; j += lanes) {
        const int64_t first = slot_off[j];
        joined_off[j] = at[first < n_slots ? first : n_slots];
    }
}

// the regions of the caller's workspace, each a multiple of 256 bytes
struct PairWs {
    size_t pair_a, pair_b, val_off, len, slot_off, keys_a, keys_b, slots_a, slots_b, line_of, pair_of, head, pos, tmp, tmp_bytes, total;
};
PairWs pair_ws(int32_t m, int32_t c, int64_t n_slots) {
    PairWs w{};
    const size_t S = (size_t)n_slots, C = (size_t)c;
    size_t sort_tmp = 0, scan32 = 0, scan64 = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                    S, 0u, 64u);
    (void)rocprim::exclusive_scan(nullptr, scan32, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, S + 1, rocprim::plus<int32_t>());
    (void)rocprim::exclusive_scan(nullptr, scan64, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, C + 1, rocprim::plus<int64_t>());
    const size_t scan = scan32 > scan64 ? scan32 : scan64;
    w.tmp_bytes = pad256(sort_tmp > scan ? sort_tmp : scan);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.pair_a = take(C * 4);
    w.pair_b = take(C * 4);
    w.val_off = take(((size_t)m + 1) * 8);
    w.len = take((C + 1) * 8);
    w.slot_off = take((C + 1) * 8);
    w.keys_a = take(S * 8);
    w.keys_b = take(S * 8);
    w.slots_a = take(S * 4);
    w.slots_b = take(S * 4);
    w.line_of = take(S * 4);
    w.pair_of = take(S * 4);
    w.head = take((S + 1) * 4);
    w.pos = take((S + 1) * 4);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}

bool pair_shape_ok(int32_t m, int32_t c, int64_t n_slots) { return m > 0 && c > 0 && n_slots > 0 && n_slots <= 0x7fffffff; }

template <class T>
T *region(void *ws, size_t at) {
    return reinterpret_cast<T *>(static_cast<uint8_t *>(ws) + at);
}

}  // namespace

size_t pairs_of_first_hits_scratch_bytes(int32_t m, int32_t n_pairs, int64_t n_slots) {
    return pair_shape_ok(m, n_pairs, n_slots) ? pair_ws(m, n_pairs, n_slots).total : 0;
}

int launch_pairs_of_first_hits(int n_cu, int32_t m, const int64_t *val_off, int32_t c, const int32_t *pair_a, const int32_t *pair_b,
                               const int64_t *first_off, const int32_t *first_lines, const int32_t *group_of_first, int64_t n_slots,
                               int64_t *pair_off, int32_t *pair_group_a, int32_t *pair_group_b, int32_t *pair_lines, int64_t *joined_off,
                               int32_t *joined_lines, int32_t *joined_group, void *ws, size_t ws_bytes, void *stream) {
    int32_t a_bits = 1, b_bits = 1;
    if (!pair_shape_ok(m, c, n_slots) || !val_off || fm_pair_args_bad(m, val_off, c, pair_a, pair_b, n_slots, &a_bits, &b_bits))
        return (int)hipErrorInvalidValue;
    const PairWs w = pair_ws(m, c, n_slots);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const PairTables t{region<int32_t>(ws, w.pair_a), region<int32_t>(ws, w.pair_b), region<int64_t>(ws, w.val_off)};
    int64_t *len = region<int64_t>(ws, w.len), *slot_off = region<int64_t>(ws, w.slot_off);
    uint64_t *keys_a = region<uint64_t>(ws, w.keys_a), *keys_b = region<uint64_t>(ws, w.keys_b);
    uint32_t *slots_a = region<uint32_t>(ws, w.slots_a), *slots_b = region<uint32_t>(ws, w.slots_b);
    int32_t *line_of = region<int32_t>(ws, w.line_of), *pair_of = region<int32_t>(ws, w.pair_of);
    int32_t *head = region<int32_t>(ws, w.head), *pos = region<int32_t>(ws, w.pos);
    // behind the sort the unsorted keys are done with: their region holds the flags of the slots and the scan of the flags
    // (2 * (n_slots + 1) ints in n_slots * 8 bytes and the 256 spare bytes of every region)
    int32_t *flag = reinterpret_cast<int32_t *>(keys_a), *at = flag + (n_slots + 1);
    void *tmp = region<uint8_t>(ws, w.tmp);
    size_t tmp_bytes = w.tmp_bytes;
    const int32_t key_bits = fm_bits((uint32_t)c) + a_bits + b_bits;
    int32_t key_grid = 1, flat = 1;
    hit_lines_geometry(n_slots, n_cu, &key_grid, &flat);
#define FMX_PAIR_CHECK(call) \
    if (hipError_t e_ = (call); e_ != hipSuccess) return (int)e_
    // the tables.  The runtime has read these blocks when the copies return (a copy from pageable host memory is staged before the
    // call comes back).
    FMX_PAIR_CHECK(hipMemcpyAsync(region<uint8_t>(ws, w.pair_a), pair_a, (size_t)c * 4, hipMemcpyHostToDevice, st));
    FMX_PAIR_CHECK(hipMemcpyAsync(region<uint8_t>(ws, w.pair_b), pair_b, (size_t)c * 4, hipMemcpyHostToDevice, st));
    FMX_PAIR_CHECK(hipMemcpyAsync(region<uint8_t>(ws, w.val_off), val_off, ((size_t)m + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pair_lens, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, t, c, first_off, len);
    FMX_PAIR_CHECK(hipGetLastError());
    FMX_PAIR_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, len, slot_off, (int64_t)0, (size_t)c + 1, rocprim::plus<int64_t>(), st));
    hipLaunchKernelGGL(k_pair_keys, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, t, c, slot_off, first_off, first_lines, group_of_first, n_slots,
                       a_bits, b_bits, keys_a, slots_a, line_of);
    FMX_PAIR_CHECK(hipGetLastError());
    FMX_PAIR_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_a, keys_b, slots_a, slots_b, (size_t)n_slots, 0u, (unsigned)key_bits, st));
    hipLaunchKernelGGL(k_pair_heads, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, keys_b, n_slots, c, a_bits, b_bits, head);
    FMX_PAIR_CHECK(hipGetLastError());
    FMX_PAIR_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, head, pos, (int32_t)0, (size_t)n_slots + 1, rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(k_pair_store, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, keys_b, head, pos, n_slots, c, a_bits, b_bits, pair_off,
                       pair_group_a, pair_group_b, pair_lines);
    FMX_PAIR_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pair_back, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, keys_b, slots_b, head, pos, pair_off, n_slots, c, a_bits, b_bits,
                       pair_of, flag);
    FMX_PAIR_CHECK(hipGetLastError());
    FMX_PAIR_CHECK(rocprim::exclusive_scan(tmp, tmp_bytes, flag, at, (int32_t)0, (size_t)n_slots + 1, rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(k_pair_compact, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, flag, at, line_of, pair_of, slot_off, n_slots, c, joined_off,
                       joined_lines, joined_group);
#undef FMX_PAIR_CHECK
    return (int)hipGetLastError();
}

}  // namespace fmx
