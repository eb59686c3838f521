// locate_all_hostsim.cpp — TEST-ONLY host build of the device code of "all occurrences, packed" (fmx_locate_all_*):
// index4j_amd/csrc/fmx_device.hpp's fm_locate_all_hits, fm_hit_pattern, fm_hit_tile, fm_locate_all_resolve and the one-hit functions
// fm_locate_hit / fm_rows_hit, driven by a mirror of k_locate_all's tile loop (fmx_kernels.hip) with the lanes run one after
// the other.  g++ compiles the header's FMX_HD functions as plain C++, so the CPU suite checks the very source the kernel runs
// against the oracle (tests/test_locate_all_cpu.py).  The image's view, the window directory and the row table come from
// tests/rows_hostsim.cpp, included as it stands.  Never part of libfmx.so.
#include "rows_hostsim.cpp"

#include <vector>

namespace {

int32_t all_hit(const DevIndex &ix, int32_t start, int32_t k, int32_t &distance, int &status) {
    if (ix.rows) return fm_rows_hit<kWinAsk>(ix, ix.inv_global, start, k, distance, status);  // k_locate_all_rows
    return ix.win && ix.win_flat ? fm_locate_hit<kWinFlat>(ix, ix.inv_global, start, k, distance, status)  // FMX_DISPATCH_WIN
           : ix.win              ? fm_locate_hit<kWinAlways>(ix, ix.inv_global, start, k, distance, status)
                                 : fm_locate_hit<kWinNever>(ix, ix.inv_global, start, k, distance, status);
}

}  // namespace

extern "C" {

int32_t sim_locate_all_tile() { return kLocateAllTile; }
int32_t sim_locate_all_slice() { return kLocateAllSlice; }

// k_hit_counts + the exclusive scan of fmx_hit_offsets.hip
void sim_hit_offsets(const int32_t *range, int32_t n, int32_t max_matches, int64_t *hit_off) {
    int64_t sum = 0;
    for (int32_t i = 0; i < n; ++i) {
        hit_off[i] = sum;
        sum += fm_locate_all_hits(range[2 * i], range[2 * i + 1], max_matches);
    }
    hit_off[n] = sum;
}

// the search alone: the pattern of every packed hit by fm_hit_pattern over the whole of hit_off
void sim_hit_patterns(const int64_t *hit_off, int32_t n, int32_t *pattern_of) {
    for (int64_t t = 0; t < hit_off[n]; ++t) pattern_of[t] = fm_hit_pattern(hit_off, n, t);
}

// mirrors launch_locate_all + k_locate_all / k_locate_all_rows: `grid` workgroups of `block` lanes (512 / 1024) over the tiles of
// [first_hit, first_hit + n_hits) cut at hit_off[n]; slice_max = kLocateAllSlice, or smaller to send tiles down the route that
// searches hit_off where it lies.  rows (nullable): the row table.  Returns the tiles that took that route.
int64_t sim_locate_all(const uint8_t *blob, const uint32_t *rows, const int32_t *range, const int64_t *hit_off, int32_t n,
                       int64_t first_hit, int64_t n_hits, int32_t *locs, int32_t *lf_steps, int32_t *status_out, int32_t block,
                       int32_t grid, int32_t slice_max) {
    const DevIndex ix = rows_index(blob, rows);
    int64_t global_tiles = 0;
    if (n <= 0 || n_hits <= 0) return 0;
    const int64_t total = hit_off[n];
    if (first_hit >= total) return 0;
    const int64_t last = n_hits < total - first_hit ? first_hit + n_hits : total;
    std::vector<int64_t> s_off((size_t)kLocateAllSlice);
    std::vector<int32_t> lane_p(64), lane_steps(64);
    for (int64_t group = 0; group < grid; ++group) {
        for (int64_t tile = first_hit + group * kLocateAllTile; tile < last; tile += (int64_t)grid * kLocateAllTile) {
            const HitTile h = fm_hit_tile(hit_off, n, tile, last);
            const bool in_lds = h.slice_count <= slice_max;  // (fm_hit_tile_slice, with the caller's bound)
            if (in_lds)
                for (int32_t i = 0; i < h.slice_count; ++i) s_off[(size_t)i] = hit_off[h.p_lo + i];
            else
                ++global_tiles;
            const int64_t *slice = in_lds ? s_off.data() : hit_off + h.p_lo;
            for (int32_t round = 0; round < kLocateAllTile; round += block) {
                for (int32_t wave = 0; wave < block; wave += 64) {
                    for (int32_t lane = 0; lane < 64; ++lane) {
                        const int64_t t = tile + round + wave + lane;
                        int32_t p = -1, steps = 0;
                        if (t <= h.tile_last) {
                            int32_t k, distance = 0;
                            p = fm_locate_all_resolve(slice, h.slice_count, h.p_lo, t, k);
                            int status = ST_OK;
                            locs[t - first_hit] = all_hit(ix, range[2 * (int64_t)p], k, distance, status);
                            steps = distance;
                            if (status && status_out) status_out[p] |= status;
                        }
                        lane_p[(size_t)lane] = p;
                        lane_steps[(size_t)lane] = steps;
                    }
                    if (lf_steps) {  // the wave's fold: a segmented inclusive sum over runs of one pattern, the run's last lane adds
                        for (int o = 1; o < 64; o <<= 1) {
                            const std::vector<int32_t> s_up = lane_steps, p_up = lane_p;
                            for (int32_t lane = o; lane < 64; ++lane)
                                if (p_up[(size_t)(lane - o)] == lane_p[(size_t)lane]) lane_steps[(size_t)lane] += s_up[(size_t)(lane - o)];
                        }
                        for (int32_t lane = 0; lane < 64; ++lane) {
                            const int32_t p = lane_p[(size_t)lane];
                            if (p >= 0 && lane_steps[(size_t)lane] && (lane == 63 || lane_p[(size_t)lane + 1] != p))
                                lf_steps[p] += lane_steps[(size_t)lane];
                        }
                    }
                }
            }
        }
    }
    return global_tiles;
}
}
