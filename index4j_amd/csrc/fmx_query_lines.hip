// fmx_query_lines.hip — packed hits of a batch of TERMS -> the packed distinct LINES of each QUERY (fmx_query_lines_of_hits_dev,
// fmx_match_query_batch): the n patterns are terms, cut into q queries by query_off, each term ALL, ANY or NONE (fmx_device.hpp
// "A QUERY OF SEVERAL TERMS"); the lines of a query = those that hold every ALL term, one of the ANY terms if there are any, and
// no NONE term.  The set algebra happens in HBM on the sorted keys of the hits; only the answer comes down.
//
// Every stage hands lanes to HITS, to sorted keys or to (query, line) groups, never to queries or lines — ONE query whose terms
// match everywhere uses the whole device (k_query_counts alone has a lane per query: two binary searches each):
//   k_query_line_keys   a lane per packed hit, k_hit_line_keys' tile loop (fm_hit_tile / fm_hit_tile_slice / fm_hit_pattern for the
//                       term, fm_line_of over the fences in LDS for the line); the term's query from a per-term table in HBM; the
//                       64-bit key query | line | term index inside the query; a slot behind hit_off[n] gets the query q: last
//   rocPRIM             ONE device-wide radix sort of the keys over the bits in use
//   k_query_words       a lane per sorted key: a key that differs from its predecessor is a distinct (query, line, term) triple
//                       and contributes its kind's word (fm_query_word); a repeated key — the term's second hit on the line —
//                       contributes nothing
//   rocPRIM             reduce_by_key over the (query, line) part of the keys with fm_query_word_join: one head key and one word
//                       per group, and the number of groups (lanes per key: no lane walks a group)
//   k_query_flags       a lane per group: 1 where the word matches the query's n_all / n_any (fm_query_matches); an exclusive
//                       scan numbers the matching groups
//   k_query_counts      a lane per query: its groups by binary search in the head keys, line_count = the difference of two scan
//                       entries, clamped to max_lines; an exclusive scan of that is line_off
//   k_query_compact     a lane per group: a matching group whose rank inside its query is below the limit stores its line
// No atomics of ours, integer arithmetic only: the result does not depend on the order the lanes run in.  Nothing here looks at
// the image, so this file is compiled once, like fmx_hit_lines.hip.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cstring>
#include <vector>

#include "fmx_device.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

constexpr int kKeyBlock = 1024;  // k_query_line_keys: k_hit_line_keys' budget — fences 16 KiB + the slice 16 KiB: two workgroups per CU
constexpr int kFlatBlock = 256;  // the element-wise kernels
static_assert(kLocateAllTile == kKeyBlock, "a lane per hit of a tile");

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }

__global__ __launch_bounds__(kKeyBlock) void k_query_line_keys(const int32_t *__restrict__ T, int32_t count, int32_t n_fences, int32_t shift,
                                                               int32_t line_bits, int32_t term_bits, const int64_t *__restrict__ hit_off,
                                                               int32_t n, int32_t q, const int32_t *__restrict__ term_query,
                                                               const int32_t *__restrict__ query_off, const int32_t *__restrict__ locs,
                                                               int64_t n_hits, uint64_t *__restrict__ keys) {
    __shared__ int64_t s_off[kLocateAllSlice];
    __shared__ int32_t s_fence[kLineFences];
    for (int32_t j = threadIdx.x; j < n_fences; j += kKeyBlock) s_fence[j] = T[(int64_t)j << shift];
    __syncthreads();
    const uint64_t behind = fm_query_key(q, 0, 0, line_bits, term_bits);
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
        if (t <= h.tile_last) {
            const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
            const int32_t query = term_query[p];
            keys[t] = fm_query_key(query, fm_line_of(T, count, s_fence, n_fences, shift, locs[t]), p - query_off[query], line_bits, term_bits);
        } else if (t < n_hits) {
            keys[t] = behind;
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_query_words(const uint64_t *__restrict__ keys, int64_t n_hits, int32_t q, int32_t line_bits,
                                                            int32_t term_bits, const int32_t *__restrict__ query_off,
                                                            const uint8_t *__restrict__ term_kind, uint64_t *__restrict__ word) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; i < n_hits; i += (int64_t)gridDim.x * kFlatBlock)
        word[i] = fm_query_contribution(keys, i, q, line_bits, term_bits, query_off, term_kind);
}

struct SameGroup {
    int32_t term_bits;
    __host__ __device__ bool operator()(uint64_t a, uint64_t b) const { return (a >> term_bits) == (b >> term_bits); }
};
struct JoinWords {
    __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return fm_query_word_join(a, b); }
};

// flag[g] for the groups, 0 from *n_groups on up to flag[n_hits]: the exclusive scan then runs over a length the host knows
__global__ __launch_bounds__(kFlatBlock) void k_query_flags(const uint64_t *__restrict__ group_key, const uint64_t *__restrict__ group_word,
                                                            const size_t *__restrict__ n_groups, int64_t n_hits, int32_t q, int32_t line_bits,
                                                            int32_t term_bits, const int32_t *__restrict__ n_all,
                                                            const int32_t *__restrict__ n_any, int32_t *__restrict__ flag) {
    const int64_t groups = (int64_t)*n_groups < n_hits ? (int64_t)*n_groups : n_hits;
    for (int64_t g = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; g <= n_hits; g += (int64_t)gridDim.x * kFlatBlock) {
        int32_t f = 0;
        if (g < groups) {
            const int32_t query = fm_query_key_query(group_key[g], line_bits, term_bits);
            f = query < q && fm_query_matches(group_word[g], n_all[query], n_any[query]) ? 1 : 0;
        }
        flag[g] = f;
    }
}

// pos = the exclusive scan of flag.  The groups of query Q are [first_group(Q), first_group(Q + 1)) of the head keys.
__global__ __launch_bounds__(kFlatBlock) void k_query_counts(const uint64_t *__restrict__ group_key, const size_t *__restrict__ n_groups,
                                                             const int32_t *__restrict__ pos, int64_t n_hits, int32_t q, int32_t line_bits,
                                                             int32_t term_bits, int32_t max_lines, int32_t *__restrict__ line_count,
                                                             int32_t *__restrict__ query_base, int64_t *__restrict__ stored) {
    const int64_t groups = (int64_t)*n_groups < n_hits ? (int64_t)*n_groups : n_hits;
    for (int64_t query = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; query <= q; query += (int64_t)gridDim.x * kFlatBlock) {
        int64_t c = 0;
        if (query < q) {
            const int64_t a = fm_query_first_group(group_key, groups, (int32_t)query, line_bits, term_bits);
            const int64_t b = fm_query_first_group(group_key, groups, (int32_t)query + 1, line_bits, term_bits);
            c = pos[b] - pos[a];
            query_base[query] = pos[a];
            if (line_count) line_count[query] = (int32_t)c;
            if (max_lines > 0 && c > max_lines) c = max_lines;
        }
        stored[query] = c;  // (stored[q] = 0: the exclusive scan leaves the batch's total in line_off[q])
    }
}

__global__ __launch_bounds__(kFlatBlock) void k_query_compact(const uint64_t *__restrict__ group_key, const size_t *__restrict__ n_groups,
                                                              const int32_t *__restrict__ flag, const int32_t *__restrict__ pos,
                                                              const int32_t *__restrict__ query_base, const int64_t *__restrict__ line_off,
                                                              int64_t n_hits, int32_t line_bits, int32_t term_bits, int32_t max_lines,
                                                              int32_t *__restrict__ lines) {
    const int64_t groups = (int64_t)*n_groups < n_hits ? (int64_t)*n_groups : n_hits;
    for (int64_t g = (int64_t)blockIdx.x * kFlatBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kFlatBlock) {
        if (!flag[g]) continue;  // (a flagged group's query is below q)
        const int32_t query = fm_query_key_query(group_key[g], line_bits, term_bits);
        const int32_t rank = pos[g] - query_base[query];
        if (max_lines > 0 && rank >= max_lines) continue;
        lines[line_off[query] + rank] = fm_query_key_line(group_key[g], line_bits, term_bits);
    }
}

// the regions of the caller's workspace, each a multiple of 256 bytes.  keys_a: the unsorted keys, then the words of the sorted
// ones.  tables: term_query (n ints), query_off (q + 1), n_all (q), n_any (q), term_kind (n bytes) — what the call derives from
// its host arrays, one copy.
struct QueryWs {
    size_t keys_a, keys_b, group_key, group_word, flag, pos, stored, query_base, n_groups, tables, tables_bytes, tmp, tmp_bytes, total;
    size_t t_query_off, t_n_all, t_n_any, t_kind;  // inside `tables` (term_query at 0)
};
QueryWs query_ws(int32_t n, int32_t q, int64_t n_hits) {
    QueryWs w{};
    size_t sort_tmp = 0, reduce_tmp = 0, scan32 = 0, scan64 = 0;
    (void)rocprim::radix_sort_keys(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n_hits, 0u, 64u);
    (void)rocprim::reduce_by_key(nullptr, reduce_tmp, (const uint64_t *)nullptr, (const uint64_t *)nullptr, (size_t)n_hits, (uint64_t *)nullptr,
                                 (uint64_t *)nullptr, (size_t *)nullptr, JoinWords(), SameGroup{0});
    (void)rocprim::exclusive_scan(nullptr, scan32, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, (size_t)n_hits + 1,
                                  rocprim::plus<int32_t>());
    (void)rocprim::exclusive_scan(nullptr, scan64, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)q + 1,
                                  rocprim::plus<int64_t>());
    size_t tmp = sort_tmp > reduce_tmp ? sort_tmp : reduce_tmp;
    if (scan32 > tmp) tmp = scan32;
    if (scan64 > tmp) tmp = scan64;
    w.tmp_bytes = pad256(tmp);
    w.t_query_off = (size_t)n * 4;
    w.t_n_all = w.t_query_off + ((size_t)q + 1) * 4;
    w.t_n_any = w.t_n_all + (size_t)q * 4;
    w.t_kind = w.t_n_any + (size_t)q * 4;
    w.tables_bytes = w.t_kind + (size_t)n;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += pad256(bytes);
        return here;
    };
    w.keys_a = take((size_t)n_hits * 8);
    w.keys_b = take((size_t)n_hits * 8);
    w.group_key = take((size_t)n_hits * 8);
    w.group_word = take((size_t)n_hits * 8);
    w.flag = take(((size_t)n_hits + 1) * 4);
    w.pos = take(((size_t)n_hits + 1) * 4);
    w.stored = take(((size_t)q + 1) * 8);
    w.query_base = take(((size_t)q + 1) * 4);
    w.n_groups = take(sizeof(size_t));
    w.tables = take(w.tables_bytes);
    w.tmp = take(w.tmp_bytes);
    w.total = at;
    return w;
}

}  // namespace

size_t query_lines_scratch_bytes(int32_t n, int32_t q, int64_t n_hits) {
    if (n <= 0 || q <= 0 || n_hits <= 0 || n_hits > 0x7fffffff) return 0;
    return query_ws(n, q, n_hits).total;
}

int32_t query_lines_max_terms(int32_t q, const int32_t *query_off) {
    int32_t most = 0;
    for (int32_t i = 0; i < q; ++i)
        if (query_off[i + 1] - query_off[i] > most) most = query_off[i + 1] - query_off[i];
    return most;
}

int launch_query_lines(const int32_t *T, int32_t count, int n_cu, int32_t n, int32_t q, const int32_t *query_off, const uint8_t *term_kind,
                       const int64_t *hit_off, const int32_t *locs, int64_t n_hits, int32_t max_lines, int64_t *line_off, int32_t *lines,
                       int32_t *line_count, void *ws, size_t ws_bytes, void *stream) {
    if (n <= 0 || q <= 0 || n_hits <= 0) return 0;
    if (n_hits > 0x7fffffff || count < 0) return (int)hipErrorInvalidValue;
    const QueryWs w = query_ws(n, q, n_hits);
    if (!ws || ws_bytes < w.total) return (int)hipErrorInvalidValue;
    const int32_t line_bits = fm_bits((uint32_t)count), term_bits = fm_bits((uint32_t)query_lines_max_terms(q, query_off));
    const int32_t key_bits = fm_bits((uint32_t)q) + line_bits + term_bits;
    if (key_bits > 64) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t *base = static_cast<uint8_t *>(ws);
    // the tables: the query of every term, the terms of every query, how many of them are ALL and ANY, the kinds.  The runtime
    // has read this block when the copy returns (a copy from pageable host memory is staged before the call comes back).
    std::vector<uint8_t> host(w.tables_bytes);
    {
        int32_t *term_query = reinterpret_cast<int32_t *>(host.data()), *h_off = reinterpret_cast<int32_t *>(host.data() + w.t_query_off);
        int32_t *n_all = reinterpret_cast<int32_t *>(host.data() + w.t_n_all), *n_any = reinterpret_cast<int32_t *>(host.data() + w.t_n_any);
        memcpy(h_off, query_off, ((size_t)q + 1) * 4);
        memcpy(host.data() + w.t_kind, term_kind, (size_t)n);
        for (int32_t i = 0; i < q; ++i) {
            n_all[i] = n_any[i] = 0;
            for (int32_t t = query_off[i]; t < query_off[i + 1]; ++t) {
                term_query[t] = i;
                n_all[i] += term_kind[t] == kTermAll;
                n_any[i] += term_kind[t] == kTermAny;
            }
        }
    }
    if (hipError_t e = hipMemcpyAsync(base + w.tables, host.data(), w.tables_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return (int)e;
    const int32_t *d_term_query = reinterpret_cast<const int32_t *>(base + w.tables);
    const int32_t *d_query_off = reinterpret_cast<const int32_t *>(base + w.tables + w.t_query_off);
    const int32_t *d_n_all = reinterpret_cast<const int32_t *>(base + w.tables + w.t_n_all);
    const int32_t *d_n_any = reinterpret_cast<const int32_t *>(base + w.tables + w.t_n_any);
    const uint8_t *d_kind = base + w.tables + w.t_kind;
    uint64_t *keys_a = reinterpret_cast<uint64_t *>(base + w.keys_a), *keys_b = reinterpret_cast<uint64_t *>(base + w.keys_b);
    uint64_t *group_key = reinterpret_cast<uint64_t *>(base + w.group_key), *group_word = reinterpret_cast<uint64_t *>(base + w.group_word);
    int32_t *flag = reinterpret_cast<int32_t *>(base + w.flag), *pos = reinterpret_cast<int32_t *>(base + w.pos);
    int64_t *stored = reinterpret_cast<int64_t *>(base + w.stored);
    int32_t *query_base = reinterpret_cast<int32_t *>(base + w.query_base);
    size_t *n_groups = reinterpret_cast<size_t *>(base + w.n_groups);
    void *tmp = base + w.tmp;
    size_t tmp_bytes = w.tmp_bytes;
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, kLineFences, n_fences);
    int32_t key_grid = 1, flat = 1, unused = 1, query_grid = 1;
    hit_lines_geometry(n_hits, n_cu, &key_grid, &flat);
    hit_lines_geometry(q, n_cu, &unused, &query_grid);  // (the element-wise grid over q + 1 items)
    hipLaunchKernelGGL(k_query_line_keys, dim3((unsigned)key_grid), dim3(kKeyBlock), 0, st, T, count, n_fences, shift, line_bits, term_bits, hit_off,
                       n, q, d_term_query, d_query_off, locs, n_hits, keys_a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::radix_sort_keys(tmp, tmp_bytes, keys_a, keys_b, (size_t)n_hits, 0u, (unsigned)key_bits, st); e != hipSuccess)
        return (int)e;
    uint64_t *word = keys_a;  // (the unsorted keys are done with)
    hipLaunchKernelGGL(k_query_words, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, keys_b, n_hits, q, line_bits, term_bits, d_query_off, d_kind,
                       word);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::reduce_by_key(tmp, tmp_bytes, (const uint64_t *)keys_b, (const uint64_t *)word, (size_t)n_hits, group_key,
                                              group_word, n_groups, JoinWords(), SameGroup{term_bits}, st);
        e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_query_flags, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, group_key, group_word, n_groups, n_hits, q, line_bits,
                       term_bits, d_n_all, d_n_any, flag);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, flag, pos, (int32_t)0, (size_t)n_hits + 1, rocprim::plus<int32_t>(), st);
        e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_query_counts, dim3((unsigned)query_grid), dim3(kFlatBlock), 0, st, group_key, n_groups, pos, n_hits, q, line_bits,
                       term_bits, max_lines, line_count, query_base, stored);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, stored, line_off, (int64_t)0, (size_t)q + 1, rocprim::plus<int64_t>(), st);
        e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_query_compact, dim3((unsigned)flat), dim3(kFlatBlock), 0, st, group_key, n_groups, flag, pos, query_base, line_off, n_hits,
                       line_bits, term_bits, max_lines, lines);
    return (int)hipGetLastError();
}

}  // namespace fmx
