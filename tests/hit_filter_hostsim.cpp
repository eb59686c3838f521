// hit_filter_hostsim.cpp — TEST-ONLY host build of the device code of "packed hits -> the packed hits that lie in given lines"
// (fmx_hits_in_lines_dev): index4j_amd/csrc/fmx_hit_filter.hpp's fm_filter_line_listed, fm_filter_keep, fm_filter_slot and
// fm_filter_kept_off — with fm_hit_tile / fm_hit_pattern for a hit's pattern and fm_line_of over fences for its line — driven by a
// mirror of the stages of fmx_hit_filter.hip with the lanes run one after the other: k_hit_keep_flags' tile loop, std::exclusive_scan
// for rocPRIM's, k_hit_keep_store's two loops.  The compaction is checked against std::stable_partition over the same flags.  g++
// compiles the header's functions as plain C++, so the CPU suite checks the source of those FUNCTIONS
// (tests/test_field_values_where_cpu.py).  The kernels' own route runs in tests/test_gpu_field_values_where.py only.  Never part of
// libfmx.so.
//
// A stand-alone program:  hit_filter_hostsim IN OUT
//   IN   int64 {n, q, n_hits, count, line_lo, line_hi, max_fences, n_lines_listed}, int32 where_of[n], int64 line_off[q + 1],
//        int32 lines[n_lines_listed], int32 T[count], int64 hit_off[n + 1], int32 locs[n_hits]
//   OUT  int64 kept_off[n + 1], int32 kept_locs[n_hits] (what lies behind kept_off[n] holds kSentinel)
// Exit status 3: the scatter and std::stable_partition disagree.
#include "../index4j_amd/csrc/fmx_hit_filter.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

using namespace fmx;

namespace {

constexpr int32_t kSentinel = -77;

template <class T>
bool get(FILE *f, std::vector<T> &v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}
template <class T>
void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<int64_t> head, line_off, hit_off;
    std::vector<int32_t> where_of, lines, T, locs;
    if (!get(in, head, 8)) return 2;
    const int32_t n = (int32_t)head[0], q = (int32_t)head[1], count = (int32_t)head[3], line_lo = (int32_t)head[4], line_hi = (int32_t)head[5];
    const int64_t n_hits = head[2];
    if (!get(in, where_of, (size_t)n) || !get(in, line_off, (size_t)q + 1) || !get(in, lines, (size_t)head[7]) || !get(in, T, (size_t)count) ||
        !get(in, hit_off, (size_t)n + 1) || !get(in, locs, (size_t)n_hits))
        return 2;
    fclose(in);
    const size_t H = (size_t)n_hits;
    // the fences a workgroup stages in LDS
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, (int32_t)head[6], n_fences);
    std::vector<int32_t> fence((size_t)n_fences);
    for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = T[(size_t)((int64_t)j << shift)];
    // k_hit_keep_flags: tile by tile, lane by lane
    std::vector<int32_t> flag(H + 1, -1), pos(H + 1);
    const int64_t first = fm_filter_slot(hit_off[0], n_hits), total = fm_filter_slot(hit_off[(size_t)n], n_hits);
    flag[H] = 0;
    for (int64_t tile = 0; tile < n_hits; tile += kLocateAllTile) {
        if (tile >= total || tile + kLocateAllTile <= first) {
            for (int64_t t = tile; t < tile + kLocateAllTile && t < n_hits; ++t) flag[(size_t)t] = 0;
            continue;
        }
        const HitTile h = fm_hit_tile(hit_off.data(), n, tile, total);
        const int64_t *slice = hit_off.data() + h.p_lo;
        for (int64_t t = tile; t < tile + kLocateAllTile && t < n_hits; ++t) {
            if (t >= first && t <= h.tile_last) {
                const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
                const int32_t L = fm_line_of(T.data(), count, fence.data(), n_fences, shift, locs[(size_t)t]);
                flag[(size_t)t] = fm_filter_keep(L, line_lo, line_hi, where_of[(size_t)p], line_off.data(), lines.data()) ? 1 : 0;
            } else {
                flag[(size_t)t] = 0;
            }
        }
    }
    std::exclusive_scan(flag.begin(), flag.end(), pos.begin(), (int32_t)0);
    // k_hit_keep_store
    std::vector<int32_t> kept_locs(H, kSentinel);
    std::vector<int64_t> kept_off((size_t)n + 1);
    for (size_t i = 0; i < H; ++i)
        if (flag[i]) kept_locs[(size_t)pos[i]] = locs[i];
    for (int32_t p = 0; p <= n; ++p) kept_off[(size_t)p] = fm_filter_kept_off(hit_off.data(), pos.data(), n_hits, p);
    // the same compaction by the standard library: stable, over the slots' numbers
    std::vector<size_t> slot(H);
    std::iota(slot.begin(), slot.end(), (size_t)0);
    const auto mid = std::stable_partition(slot.begin(), slot.end(), [&](size_t i) { return flag[i] != 0; });
    if ((int64_t)(mid - slot.begin()) != pos[H] || pos[H] != kept_off[(size_t)n]) return 3;
    for (auto it = slot.begin(); it != mid; ++it)
        if (kept_locs[(size_t)(it - slot.begin())] != locs[*it]) return 3;
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    put(out, kept_off);
    put(out, kept_locs);
    return fclose(out) == 0 ? 0 : 2;
}
