// match_lines_hostsim.cpp — TEST-ONLY host build of the device code of "the lines that match" (fmx_line_table_build,
// fmx_lines_of_hits_dev): index4j_amd/csrc/fmx_device.hpp's fm_line_fence_shift, fm_line_of, fm_line_total, fm_line_bounds,
// fm_bits, fm_line_key and its unpacking, fm_line_head — with fm_hit_pattern for a hit's pattern — driven by a mirror of the
// stages of fmx_hit_lines.hip with the lanes run one after the other (the device-wide radix sort = std::sort on the keys, the
// scans = running sums).  g++ compiles the header's functions as plain C++, so the CPU suite checks the source of those FUNCTIONS
// (tests/test_match_lines_cpu.py).  NOT mirrored: k_hit_line_keys' tile loop — the tile's patterns, the LDS slice of hit_off and
// the search of hit_off where it lies for a tile of more than kLocateAllSlice patterns — which is k_locate_all's (fm_hit_tile;
// tests/locate_all_hostsim.cpp mirrors that loop); here a hit's pattern is ONE fm_hit_pattern over the whole of hit_off.  The
// kernel's own route runs in tests/test_gpu_match_lines.py only.  Never part of libfmx.so.
#include "../index4j_amd/csrc/fmx_device.hpp"

#include <algorithm>
#include <cstdint>
#include <vector>

using namespace fmx;

extern "C" {

int32_t sim_line_fences() { return kLineFences; }

// fm_line_of for every p of `ps`, over the fences the key kernel would stage for max_fences (<= 0: none); returns the shift
int32_t sim_line_of(const int32_t *T, int32_t count, int32_t max_fences, const int32_t *ps, int32_t n, int32_t *out, int32_t *n_fences_out) {
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, max_fences, n_fences);
    std::vector<int32_t> fence((size_t)n_fences);
    for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = T[(int64_t)j << shift];
    for (int32_t i = 0; i < n; ++i) out[i] = fm_line_of(T, count, fence.data(), n_fences, shift, ps[i]);
    if (n_fences_out) *n_fences_out = n_fences;
    return shift;
}

int64_t sim_line_total(const int32_t *T, int32_t count, int32_t text_len) { return fm_line_total(T, count, text_len); }

void sim_line_bounds(const int32_t *T, int32_t count, int64_t n_lines, int32_t text_len, const int32_t *ids, int32_t n, int32_t *start,
                     int32_t *stop) {
    for (int32_t i = 0; i < n; ++i) fm_line_bounds(T, count, n_lines, text_len, ids[i], start[i], stop[i]);
}

int32_t sim_bits(uint32_t v) { return fm_bits(v); }

// launch_lines_of_hits: keys for slots [0, n_hits) (a slot behind hit_off[n] gets the pattern n), the sort, heads and their
// exclusive sum, the counts per pattern and theirs, the compaction.  Returns the bits the sort runs over.
int32_t sim_lines_of_hits(const int32_t *T, int32_t count, int32_t max_fences, int32_t n, const int64_t *hit_off, const int32_t *locs,
                          int64_t n_hits, int32_t max_lines, int64_t *line_off, int32_t *lines, int32_t *line_count) {
    if (n <= 0 || n_hits <= 0) {
        for (int32_t i = 0; i <= (n > 0 ? n : 0); ++i) line_off[i] = 0;
        return 0;
    }
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, max_fences, n_fences);
    std::vector<int32_t> fence((size_t)n_fences);
    for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = T[(int64_t)j << shift];
    const int32_t line_bits = fm_bits((uint32_t)count), key_bits = fm_bits((uint32_t)n) + line_bits;
    const int64_t total = hit_off[n] < n_hits ? hit_off[n] : n_hits;
    std::vector<uint64_t> keys((size_t)n_hits);
    for (int64_t t = 0; t < n_hits; ++t)  // k_hit_line_keys
        keys[(size_t)t] = t < total ? fm_line_key(fm_hit_pattern(hit_off, n, t), fm_line_of(T, count, fence.data(), n_fences, shift, locs[t]), line_bits)
                                    : fm_line_key(n, 0, line_bits);
    const uint64_t mask = key_bits >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << key_bits) - 1);
    std::stable_sort(keys.begin(), keys.end(), [&](uint64_t a, uint64_t b) { return (a & mask) < (b & mask); });  // bits [0, key_bits)
    std::vector<int32_t> pos((size_t)n_hits + 1);
    int32_t sum = 0;
    for (int64_t i = 0; i <= n_hits; ++i) {  // k_line_heads + the scan
        pos[(size_t)i] = sum;
        sum += i < n_hits && fm_line_head(keys.data(), i, n, line_bits) ? 1 : 0;
    }
    int64_t stored = 0;
    for (int32_t p = 0; p <= n; ++p) {  // k_line_counts + the scan
        line_off[p] = stored;
        if (p == n) break;
        const int64_t a = hit_off[p] < n_hits ? hit_off[p] : n_hits, b = hit_off[p + 1] < n_hits ? hit_off[p + 1] : n_hits;
        int64_t c = b > a ? pos[(size_t)b] - pos[(size_t)a] : 0;
        if (line_count) line_count[p] = (int32_t)c;
        if (max_lines > 0 && c > max_lines) c = max_lines;
        stored += c;
    }
    for (int64_t i = 0; i < n_hits; ++i) {  // k_line_compact
        if (!fm_line_head(keys.data(), i, n, line_bits)) continue;
        const int32_t p = fm_line_key_pattern(keys[(size_t)i], line_bits);
        const int64_t first = hit_off[p] < n_hits ? hit_off[p] : n_hits;
        const int32_t rank = pos[(size_t)i] - pos[(size_t)first];
        if (max_lines > 0 && rank >= max_lines) continue;
        lines[line_off[p] + rank] = fm_line_key_line(keys[(size_t)i], line_bits);
    }
    return key_bits;
}
}
