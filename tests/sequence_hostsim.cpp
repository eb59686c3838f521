// sequence_hostsim.cpp — TEST-ONLY host build of the device code of "the lines that hold a sequence of terms in order"
// (fmx_sequence_lines_of_hits_dev): index4j_amd/csrc/fmx_device.hpp's fm_seq_key and its unpacking, fm_seq_key_width,
// fm_seq_lower_bound, fm_seq_head, fm_seq_chain, fm_seq_flag — with fm_hit_pattern for a hit's term and fm_line_of for a head's line
// — driven by a mirror of the stages of fmx_sequence_lines.hip with the lanes run one after the other (the device-wide radix sort =
// std::sort over the bits in use, the scans = running sums).  g++ compiles the header's functions as plain C++, so the CPU suite
// checks the source of those FUNCTIONS (tests/test_match_sequence_cpu.py).  NOT mirrored: k_seq_keys' tile loop, which is
// k_hit_line_keys' (tests/locate_all_hostsim.cpp mirrors that loop); here a hit's term is ONE fm_hit_pattern over the whole of
// hit_off.  The kernels' own route runs in tests/test_gpu_match_sequence.py only.  Never part of libfmx.so.
#include "../index4j_amd/csrc/fmx_device.hpp"

#include <algorithm>
#include <cstdint>
#include <vector>

using namespace fmx;

extern "C" {

int32_t sim_seq_key_width(int32_t n) { return fm_seq_key_width(n); }

// pack, then unpack: out = {term, loc}; returns the key
uint64_t sim_seq_key(int32_t term, int32_t loc, int32_t *out) {
    const uint64_t key = fm_seq_key(term, loc);
    out[0] = fm_seq_key_term(key);
    out[1] = fm_seq_key_loc(key);
    return key;
}

int64_t sim_seq_lower_bound(const int32_t *pos, int64_t lo, int64_t hi, int64_t at) { return fm_seq_lower_bound(pos, lo, hi, at); }

// launch_sequence_lines: the tables, keys for slots [0, n_hits) (a slot behind hit_off[n] gets the term n), the sort, the
// positions, the flags of the heads and their exclusive sum, the counts per sequence and theirs, the compaction.  spans: nullable.
// Returns the bits the sort runs over.
int32_t sim_sequence_lines(const int32_t *T, int32_t count, int64_t n_lines, int32_t text_len, int32_t max_fences, int32_t n, int32_t q,
                           const int32_t *query_off, const int32_t *term_len, const int64_t *hit_off, const int32_t *locs, int64_t n_hits,
                           int32_t max_lines, int64_t *line_off, int32_t *lines, int32_t *line_count, int32_t *spans) {
    if (n <= 0 || q <= 0 || n_hits <= 0) {
        for (int32_t i = 0; i <= (q > 0 ? q : 0); ++i) line_off[i] = 0;
        return 0;
    }
    const int32_t key_bits = fm_seq_key_width(n);
    std::vector<int32_t> term_seq((size_t)n);
    for (int32_t i = 0; i < q; ++i)
        for (int32_t t = query_off[i]; t < query_off[i + 1]; ++t) term_seq[(size_t)t] = i;
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, max_fences, n_fences);
    std::vector<int32_t> fence((size_t)n_fences);
    for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = T[(int64_t)j << shift];
    const int64_t total = hit_off[n] < n_hits ? hit_off[n] : n_hits;
    std::vector<uint64_t> keys((size_t)n_hits);
    for (int64_t t = 0; t < n_hits; ++t)  // k_seq_keys
        keys[(size_t)t] = t >= total ? fm_seq_key(n, 0) : fm_seq_key(fm_hit_pattern(hit_off, n, t), locs[t]);
    const uint64_t mask = ((uint64_t)1 << key_bits) - 1;  // (at most 63 bits)
    std::sort(keys.begin(), keys.end(), [&](uint64_t a, uint64_t b) { return (a & mask) < (b & mask); });
    std::vector<int32_t> pos((size_t)n_hits);
    for (int64_t i = 0; i < n_hits; ++i) pos[(size_t)i] = fm_seq_key_loc(keys[(size_t)i]);  // k_seq_positions
    std::vector<int32_t> flag((size_t)n_hits + 1, 0), scan((size_t)n_hits + 1), line_of((size_t)n_hits, -7), end_of((size_t)n_hits, -7);
    for (int64_t i = 0; i < total; ++i) {  // k_seq_chain
        const int32_t t = fm_seq_key_term(keys[(size_t)i]);
        int32_t line = 0, end = 0;
        if (t < n &&
            fm_seq_flag(pos.data(), i, t, hit_off, total, term_seq.data(), query_off, term_len, T, count, n_lines, text_len, fence.data(), n_fences,
                        shift, line, end)) {
            flag[(size_t)i] = 1;
            line_of[(size_t)i] = line;
            end_of[(size_t)i] = end;
        }
    }
    int32_t sum = 0;
    for (int64_t i = 0; i <= n_hits; ++i) {  // the scan
        scan[(size_t)i] = sum;
        sum += flag[(size_t)i];
    }
    std::vector<int32_t> seq_base((size_t)q);
    int64_t stored = 0;
    for (int32_t seq = 0; seq <= q; ++seq) {  // k_seq_counts + the scan
        line_off[seq] = stored;
        if (seq == q) break;
        const int32_t f = query_off[seq];
        int64_t c = 0;
        int32_t base = 0;
        if (f < query_off[seq + 1]) {
            const int64_t a = hit_off[f] < total ? hit_off[f] : total, b = hit_off[f + 1] < total ? hit_off[f + 1] : total;
            base = scan[(size_t)a];
            c = scan[(size_t)b] - base;
        }
        seq_base[(size_t)seq] = base;
        if (line_count) line_count[seq] = (int32_t)c;
        if (max_lines > 0 && c > max_lines) c = max_lines;
        stored += c;
    }
    for (int64_t i = 0; i < n_hits; ++i) {  // k_seq_compact
        if (!flag[(size_t)i]) continue;
        const int32_t seq = term_seq[(size_t)fm_seq_key_term(keys[(size_t)i])];
        const int32_t rank = scan[(size_t)i] - seq_base[(size_t)seq];
        if (max_lines > 0 && rank >= max_lines) continue;
        const int64_t at = line_off[seq] + rank;
        lines[at] = line_of[(size_t)i];
        if (spans) {
            spans[2 * at] = pos[(size_t)i];
            spans[2 * at + 1] = end_of[(size_t)i];
        }
    }
    return key_bits;
}
}
