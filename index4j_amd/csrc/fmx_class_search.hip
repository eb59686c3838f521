// fmx_class_search.hip — patterns of character classes (fmx_class_*, fmx_*_class_batch): the backward search of FM:455-474 over
// a FRONTIER of SA ranges per pattern.  fmx_device.hpp ("CLASS SEARCH") has the contract and the per-candidate functions; here:
//
//   k_class_search        a team of kClassTeam lanes per pattern, patterns by a grid-stride loop; per position the alternatives are
//                         mapped, freed of code 0 and of duplicates and ordered by code, then a lane pair per (code, range)
//                         candidate makes the literal's two ranks and the survivors are appended by ballot and prefix popcount.
//                         Stage 1 (kFill = false) leaves each pattern's number of ranges, count and status; stage 2 runs the
//                         same search and stores the ranges at the pattern's offset.  No atomics.
//   k_class_gather        hit_off[i] = range_hit_off[range_off[i]]: the hit offsets of the patterns from those of their ranges
//   k_class_fold_status   status[i] |= the statuses of pattern i's ranges
//
// Compiled twice, like fmx_extract_packed.hip: as it stands (namespace fmx: the scans and the two small kernels, which look at no
// image, and the search over expanded images) and with -DFMX_COMPACT=1 -DFMX_KNS=fmxc (the search over compact images).
#include <hip/hip_runtime.h>

#include "fmx_device.hpp"
#include "fmx_options.hpp"
#include "fmx_plan.hpp"

#if !defined(FMX_KNS)
#define FMX_KNS fmx
#endif

#if !FMX_COMPACT
#include <rocprim/device/device_scan.hpp>

namespace fmx {
namespace {

__global__ __launch_bounds__(256) void k_class_gather(const int64_t *__restrict__ range_off, int32_t n, int64_t m,
                                                       const int64_t *__restrict__ range_hit_off, int64_t *__restrict__ hit_off) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    int64_t r = range_off[i];
    r = r < 0 ? 0 : (r > m ? m : r);  // (range_hit_off has m + 1 entries)
    hit_off[i] = range_hit_off[r];
}

__global__ __launch_bounds__(256) void k_class_fold_status(const int64_t *__restrict__ range_off, int32_t n, int64_t m,
                                                            const int32_t *__restrict__ range_status, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t a = range_off[i], b = range_off[i + 1];
    a = a < 0 ? 0 : a;
    b = b > m ? m : b;
    int32_t st = 0;
    for (int64_t r = a; r < b; ++r) st |= range_status[r];
    if (st) status[i] |= st;
}

size_t class_counts_bytes(int32_t n) { return (((size_t)n + 1) * sizeof(int64_t) + 255) / 256 * 256; }
size_t class_scan_bytes(int32_t n) {
    size_t tmp = 0;
    (void)rocprim::exclusive_scan(nullptr, tmp, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)n + 1,
                                  rocprim::plus<int64_t>());
    return (tmp + 255) / 256 * 256 + 256;
}

}  // namespace

// the workspace of stage 1: {ranges of every pattern, n + 1 int64 | the scan's scratch}
size_t class_ranges_scratch_bytes(int32_t n) {
    if (n < 0) n = 0;
    return class_counts_bytes(n) + class_scan_bytes(n);
}
int64_t *class_ranges_counts(void *scratch) { return static_cast<int64_t *>(scratch); }

int launch_class_range_offsets(void *scratch, size_t scratch_bytes, int32_t n, int64_t *range_off, void *stream) {
    if (n < 0 || scratch_bytes < class_ranges_scratch_bytes(n)) return (int)hipErrorInvalidValue;
    uint8_t *tmp = static_cast<uint8_t *>(scratch) + class_counts_bytes(n);
    size_t tmp_bytes = class_scan_bytes(n);
    return (int)rocprim::exclusive_scan(tmp, tmp_bytes, class_ranges_counts(scratch), range_off, (int64_t)0, (size_t)n + 1,
                                        rocprim::plus<int64_t>(), static_cast<hipStream_t>(stream));
}

int launch_class_hit_offsets(const int32_t *ranges, int32_t m, const int64_t *range_off, int32_t n, int64_t *range_hit_off,
                             int64_t *hit_off, void *scratch, size_t scratch_bytes, void *stream) {
    if (n < 0 || m < 0) return (int)hipErrorInvalidValue;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (int e = launch_hit_offsets(ranges, m, -1, range_hit_off, scratch, scratch_bytes, stream); e) return e;
    hipLaunchKernelGGL(k_class_gather, dim3((unsigned)(((int64_t)n + 1 + 255) / 256)), dim3(256), 0, st, range_off, n, (int64_t)m,
                       range_hit_off, hit_off);
    return (int)hipGetLastError();
}

int launch_class_fold_status(const int64_t *range_off, int32_t n, int32_t m, const int32_t *range_status, int32_t *status, void *stream) {
    if (n <= 0 || m <= 0) return 0;
    hipLaunchKernelGGL(k_class_fold_status, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       range_off, n, (int64_t)m, range_status, status);
    return (int)hipGetLastError();
}

}  // namespace fmx
#endif  // !FMX_COMPACT

namespace FMX_KNS {
using namespace fmx;
#include "fmx_kernel_api.hpp"    // launch_class_search, as fmx_class_api.cpp sees it
#include "fmx_kernel_stage.hpp"  // FMX_FM_INV, grid_for

// what the lanes of ONE wave wrote to LDS is there for its other lanes: a wave's LDS instructions run in order, so only the
// compiler has to be held back (the teams of a wave never wait for another wave)
__device__ __forceinline__ void class_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int32_t class_team_sum(int32_t v) {
    for (int d = 1; d < kClassTeam; d <<= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int32_t class_team_or(int32_t v) {
    for (int d = 1; d < kClassTeam; d <<= 1) v |= __shfl_xor(v, d);
    return v;
}

// LDS of a workgroup: the value-of-offset table of a compact image (static) and, per team, fm_class_team_bytes(max_ranges) of
// dynamic LDS; the launcher keeps both together inside kClassLdsBytes and runs as many teams per workgroup as fit
constexpr size_t kClassLdsBytes = 64 << 10;
#if FMX_COMPACT
constexpr size_t kClassLdsStatic = (size_t)kInvEntries * sizeof(uint16_t);
#else
constexpr size_t kClassLdsStatic = 0;
#endif

// Every loop of the kernel has a WAVE-uniform trip count (the longest of the wave's four patterns, the position with the most
// candidates), so that the ballots and shuffles inside run with all lanes; a team that has nothing to do in a round is
// predicated off.  Whatever is decided per pattern (its positions, the cap) is team-uniform.
template <bool kFill>
__global__ __launch_bounds__(1024) void k_class_search(DevIndex ix, const uint16_t *__restrict__ alt, const int32_t *__restrict__ pos_off,
                                                        const int32_t *__restrict__ pat_off, int32_t n, int32_t max_ranges, int32_t teams,
                                                        int64_t *__restrict__ range_cnt, int32_t *__restrict__ counts,
                                                        int32_t *__restrict__ status_out, const int64_t *__restrict__ range_off,
                                                        int32_t *__restrict__ ranges) {
    extern __shared__ __align__(16) uint8_t s_class[];
    FMX_FM_INV(ix);
    const int team = (int)threadIdx.x / kClassTeam, lane = (int)threadIdx.x % kClassTeam;
    const int pair = lane >> 1, role = lane & 1;
    const int team_shift = (int)threadIdx.x & 63 & ~(kClassTeam - 1);  // the team's first lane in its wave
    const bool team_on = team < teams;
    uint8_t *mine_lds = s_class + (size_t)(team_on ? team : 0) * fm_class_team_bytes(max_ranges);
    int2 *const front0 = reinterpret_cast<int2 *>(mine_lds), *const front1 = front0 + max_ranges;
    int16_t *s_code = reinterpret_cast<int16_t *>(mine_lds + (size_t)max_ranges * 16);  // as mapped, then the kept ones in order
    int16_t *s_kept = s_code + kClassAltsMax;
    if (!kFill && blockIdx.x == 0 && threadIdx.x == 0) range_cnt[n] = 0;  // (the exclusive scan leaves the batch's total there)
    for (int64_t p0 = (int64_t)blockIdx.x * teams; p0 < n; p0 += (int64_t)gridDim.x * teams) {
        const int64_t p = p0 + team;
        const bool live = team_on && p < n;
        int32_t first_pos = 0, m = 0;
        if (live) {
            first_pos = pat_off[p];
            m = pat_off[p + 1] - first_pos;
        }
        int status = ST_OK;
        bool too_many = false;
        bool go = live && m > 0;
        int32_t n_cur = 0;
        int cur = 0;
        // a position of more than kClassAltsMax alternatives ends the pattern wherever it stands
        int32_t wide = 0;
        if (go)
            for (int32_t j = lane; j < m; j += kClassTeam) wide |= pos_off[first_pos + j + 1] - pos_off[first_pos + j] > kClassAltsMax ? 1 : 0;
        if (class_team_or(wide)) {
            too_many = true;
            go = false;
        }
        for (int32_t k = 0; __any(go && k < m); ++k) {  // position m - 1 - k: from the last (FM:456)
            bool step = go && k < m;
            int32_t a0 = 0, n_alt = 0;
            if (step) {
                const int32_t j = first_pos + m - 1 - k;
                a0 = pos_off[j];
                n_alt = pos_off[j + 1] - a0;
                if (n_alt > kClassAltsMax) {
                    too_many = true;
                    go = step = false;
                }
                if (n_alt < 0) n_alt = 0;
            }
            // the position's codes: mapped (FM:457), without code 0 and duplicates, ascending
            if (step)
                for (int32_t t = lane; t < n_alt; t += kClassTeam) s_code[t] = (int16_t)fm_map(ix, alt[a0 + t]);
            class_wave_sync();
            if (step)
                for (int32_t t = lane; t < n_alt; t += kClassTeam) s_kept[t] = fm_class_keep(s_code, n_alt, t) ? s_code[t] : (int16_t)0;
            class_wave_sync();
            int32_t kept = 0;
            if (step)
                for (int32_t t = lane; t < n_alt; t += kClassTeam)
                    if (s_kept[t]) {
                        s_code[fm_class_rank(s_kept, n_alt, t)] = s_kept[t];
                        ++kept;
                    }
            const int32_t n_codes = class_team_sum(kept);
            class_wave_sync();
            // the candidates, code-major and range-minor, a lane pair each, kClassPairs per round
            const int2 *src = cur ? front1 : front0;
            int2 *dst = cur ? front0 : front1;
            const int32_t n_cand = !step ? 0 : (k == 0 ? n_codes : n_codes * n_cur);
            int32_t n_next = 0;
            for (int32_t q0 = 0; __any(q0 < n_cand && !too_many); q0 += kClassPairs) {
                const int32_t q = q0 + pair;
                const bool valid = !too_many && q < n_cand;
                int32_t start = 0, end = 0, rank = 0;
                if (valid) {
                    if (k == 0) {
                        fm_class_first(ix, s_code[q], start, end);
                    } else {
                        int32_t a, r;
                        fm_class_candidate(q, n_cur, a, r);
                        const int2 from = src[r];
                        rank = fm_class_advance(ix, s_inv, from.x, from.y, role, s_code[a], status);
                    }
                }
                const int32_t other = __shfl_xor(rank, 1);
                if (k != 0) {
                    start = role ? other : rank;  // FM:469
                    end = role ? rank : other;    // FM:470
                }
                const bool survivor = valid && role == 0 && fm_class_survives(start, end);
                const uint32_t team_bits = (uint32_t)(__ballot(survivor ? 1 : 0) >> team_shift) & ((1u << kClassTeam) - 1u);
                const int32_t slot = fm_class_slot(n_next, fmx_popc(team_bits & ((1u << lane) - 1u)), fmx_popc(team_bits), max_ranges);
                if (slot < 0) too_many = true;  // (team-uniform: every lane of the team sees the same bits)
                if (survivor && slot >= 0) dst[slot] = make_int2(start, end);
                if (!too_many) n_next += fmx_popc(team_bits);
            }
            if (step) {
                if (too_many) {
                    go = false;
                } else {
                    n_cur = n_next;
                    cur ^= 1;
                    if (n_cur == 0) go = false;  // FM:464: nothing is left to advance
                }
            }
            class_wave_sync();  // (the next position overwrites the codes and the frontier just read)
        }
        // what is left of the pattern: its ranges, their sum, its status
        status = class_team_or(status);
        if (live && m <= 0) status = ST_JAVA_AIOOBE;  // pattern[-1], FM:456-457
        if (too_many) {
            status = ST_TOO_MANY_RANGES;
            n_cur = 0;
        }
        const int2 *fin = cur ? front1 : front0;
        int32_t count = 0;
        if (live)
            for (int32_t i = lane; i < n_cur; i += kClassTeam) count += fin[i].y - fin[i].x;
        count = class_team_sum(count);
        if (!kFill) {
            if (live && lane == 0) {
                range_cnt[p] = n_cur;
                if (counts) counts[p] = count;
                if (status_out) status_out[p] = status;
            }
        } else if (live) {
            const int64_t at = range_off[p], room = range_off[p + 1] - at;  // (stage 1 left exactly n_cur)
            for (int32_t i = lane; i < n_cur && i < room; i += kClassTeam) {
                ranges[2 * (at + i)] = fin[i].x;
                ranges[2 * (at + i) + 1] = fin[i].y;
            }
        }
        class_wave_sync();  // (the next pattern's first position writes the other frontier, and the codes)
    }
}

// teams of a workgroup: as many as `block` lanes hold and as fit the LDS, whole waves of four where more than one wave runs
static int class_teams(int32_t max_ranges, int block) {
    const size_t fit = (kClassLdsBytes - kClassLdsStatic) / fm_class_team_bytes(max_ranges);
    int teams = block / kClassTeam;
    if ((size_t)teams > fit) teams = (int)fit;
    if (teams > 4) teams &= ~3;
    return teams < 1 ? 1 : teams;
}

// stage 1 (ranges == nullptr): range_cnt (n + 1 int64: class_ranges_counts of the call's workspace), counts / status nullable;
// stage 2: ranges at range_off.  max_ranges in [1, kClassRangesMax] (the caller has checked).
int launch_class_search(const DevIndex &ix, int n_cu, const uint16_t *alt, const int32_t *pos_off, const int32_t *pat_off, int32_t n,
                        int32_t max_ranges, int64_t *range_cnt, int32_t *counts, int32_t *status, const int64_t *range_off, int32_t *ranges,
                        hipStream_t st) {
    if (n <= 0) return 0;
    if (max_ranges < 1 || max_ranges > kClassRangesMax) return (int)hipErrorInvalidValue;
    const int teams = class_teams(max_ranges, options().block);
    const int block = (teams * kClassTeam + 63) / 64 * 64;
    const size_t lds = (size_t)teams * fm_class_team_bytes(max_ranges);
    const dim3 grid(grid_for(((int64_t)n + teams - 1) / teams * block, block, n_cu));
    DevIndex launch_ix = ix;
    launch_ix.sb_cache = nullptr;  // (no superblock cache here: its 10 KiB of LDS are frontier)
    if (ranges)
        hipLaunchKernelGGL((k_class_search<true>), grid, dim3(block), lds, st, launch_ix, alt, pos_off, pat_off, n, max_ranges, teams, range_cnt,
                           counts, status, range_off, ranges);
    else
        hipLaunchKernelGGL((k_class_search<false>), grid, dim3(block), lds, st, launch_ix, alt, pos_off, pat_off, n, max_ranges, teams, range_cnt,
                           counts, status, range_off, ranges);
    return (int)hipGetLastError();
}

}  // namespace FMX_KNS
