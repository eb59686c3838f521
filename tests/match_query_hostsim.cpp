// match_query_hostsim.cpp — TEST-ONLY host build of the device code of "the lines that match a query of several terms"
// (fmx_query_lines_of_hits_dev): index4j_amd/csrc/fmx_device.hpp's fm_query_key and its unpacking, fm_query_key_width, fm_query_word,
// fm_query_word_join, fm_query_contribution, fm_query_matches, fm_query_first_group — with fm_hit_pattern for a hit's term and
// fm_line_of for its line — driven by a mirror of the stages of fmx_query_lines.hip with the lanes run one after the other (the
// device-wide radix sort = std::stable_sort over the bits in use, rocPRIM's reduce_by_key = one pass that joins the words of equal
// (query, line) parts, the scans = running sums).  g++ compiles the header's functions as plain C++, so the CPU suite checks the
// source of those FUNCTIONS (tests/test_match_query_cpu.py).  NOT mirrored: k_query_line_keys' tile loop, which is k_hit_line_keys'
// (tests/locate_all_hostsim.cpp mirrors that loop); here a hit's term is ONE fm_hit_pattern over the whole of hit_off.  The kernel's
// own route runs in tests/test_gpu_match_query.py only.  Never part of libfmx.so.
#include "../index4j_amd/csrc/fmx_device.hpp"

#include <algorithm>
#include <cstdint>
#include <vector>

using namespace fmx;

extern "C" {

int32_t sim_query_key_width(int32_t q, int32_t count, int32_t max_terms) { return fm_query_key_width(q, count, max_terms); }

// pack, then unpack: out = {query, line, term}; returns the key
uint64_t sim_query_key(int32_t query, int32_t line, int32_t term, int32_t line_bits, int32_t term_bits, int32_t *out, uint64_t *group) {
    const uint64_t key = fm_query_key(query, line, term, line_bits, term_bits);
    out[0] = fm_query_key_query(key, line_bits, term_bits);
    out[1] = fm_query_key_line(key, line_bits, term_bits);
    out[2] = fm_query_key_term(key, term_bits);
    *group = fm_query_key_group(key, term_bits);
    return key;
}

uint64_t sim_query_word(int32_t kind) { return fm_query_word(kind); }
uint64_t sim_query_word_join(uint64_t a, uint64_t b) { return fm_query_word_join(a, b); }
int32_t sim_query_matches(uint64_t word, int32_t n_all, int32_t n_any) { return fm_query_matches(word, n_all, n_any) ? 1 : 0; }

// launch_query_lines: the tables, keys for slots [0, n_hits) (a slot behind hit_off[n] gets the query q), the sort, the words, the
// reduction by (query, line), the flags and their exclusive sum, the counts per query and theirs, the compaction.  Returns the
// bits the sort runs over; -1 for a key of more than 64 bits (nothing is written).
int32_t sim_query_lines(const int32_t *T, int32_t count, int32_t max_fences, int32_t n, int32_t q, const int32_t *query_off,
                        const uint8_t *term_kind, const int64_t *hit_off, const int32_t *locs, int64_t n_hits, int32_t max_lines,
                        int64_t *line_off, int32_t *lines, int32_t *line_count) {
    int32_t max_terms = 0;
    for (int32_t i = 0; i < q; ++i) max_terms = std::max(max_terms, query_off[i + 1] - query_off[i]);
    const int32_t line_bits = fm_bits((uint32_t)count), term_bits = fm_bits((uint32_t)max_terms);
    const int32_t key_bits = fm_query_key_width(q, count, max_terms);
    if (key_bits > 64) return -1;
    if (n <= 0 || q <= 0 || n_hits <= 0) {
        for (int32_t i = 0; i <= (q > 0 ? q : 0); ++i) line_off[i] = 0;
        return 0;
    }
    std::vector<int32_t> term_query((size_t)n), n_all((size_t)q, 0), n_any((size_t)q, 0);
    for (int32_t i = 0; i < q; ++i)
        for (int32_t t = query_off[i]; t < query_off[i + 1]; ++t) {
            term_query[(size_t)t] = i;
            n_all[(size_t)i] += term_kind[t] == kTermAll;
            n_any[(size_t)i] += term_kind[t] == kTermAny;
        }
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, max_fences, n_fences);
    std::vector<int32_t> fence((size_t)n_fences);
    for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = T[(int64_t)j << shift];
    const int64_t total = hit_off[n] < n_hits ? hit_off[n] : n_hits;
    std::vector<uint64_t> keys((size_t)n_hits);
    for (int64_t t = 0; t < n_hits; ++t) {  // k_query_line_keys
        if (t >= total) {
            keys[(size_t)t] = fm_query_key(q, 0, 0, line_bits, term_bits);
            continue;
        }
        const int32_t p = fm_hit_pattern(hit_off, n, t), query = term_query[(size_t)p];
        keys[(size_t)t] = fm_query_key(query, fm_line_of(T, count, fence.data(), n_fences, shift, locs[t]), p - query_off[query], line_bits, term_bits);
    }
    const uint64_t mask = key_bits >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << key_bits) - 1);
    std::stable_sort(keys.begin(), keys.end(), [&](uint64_t a, uint64_t b) { return (a & mask) < (b & mask); });  // bits [0, key_bits)
    std::vector<uint64_t> word((size_t)n_hits);
    for (int64_t i = 0; i < n_hits; ++i)  // k_query_words
        word[(size_t)i] = fm_query_contribution(keys.data(), i, q, line_bits, term_bits, query_off, term_kind);
    std::vector<uint64_t> group_key, group_word;  // reduce_by_key
    for (int64_t i = 0; i < n_hits; ++i) {
        if (i == 0 || fm_query_key_group(keys[(size_t)i], term_bits) != fm_query_key_group(keys[(size_t)i - 1], term_bits)) {
            group_key.push_back(keys[(size_t)i]);
            group_word.push_back(word[(size_t)i]);
        } else {
            group_word.back() = fm_query_word_join(group_word.back(), word[(size_t)i]);
        }
    }
    const int64_t groups = (int64_t)group_key.size();
    std::vector<int32_t> flag((size_t)n_hits + 1, 0), pos((size_t)n_hits + 1);
    for (int64_t g = 0; g < groups; ++g) {  // k_query_flags
        const int32_t query = fm_query_key_query(group_key[(size_t)g], line_bits, term_bits);
        flag[(size_t)g] = query < q && fm_query_matches(group_word[(size_t)g], n_all[(size_t)query], n_any[(size_t)query]) ? 1 : 0;
    }
    int32_t sum = 0;
    for (int64_t g = 0; g <= n_hits; ++g) {  // the scan
        pos[(size_t)g] = sum;
        sum += flag[(size_t)g];
    }
    std::vector<int32_t> query_base((size_t)q);
    int64_t stored = 0;
    for (int32_t query = 0; query <= q; ++query) {  // k_query_counts + the scan
        line_off[query] = stored;
        if (query == q) break;
        const int64_t a = fm_query_first_group(group_key.data(), groups, query, line_bits, term_bits);
        const int64_t b = fm_query_first_group(group_key.data(), groups, query + 1, line_bits, term_bits);
        int64_t c = pos[(size_t)b] - pos[(size_t)a];
        query_base[(size_t)query] = pos[(size_t)a];
        if (line_count) line_count[query] = (int32_t)c;
        if (max_lines > 0 && c > max_lines) c = max_lines;
        stored += c;
    }
    for (int64_t g = 0; g < groups; ++g) {  // k_query_compact
        if (!flag[(size_t)g]) continue;
        const int32_t query = fm_query_key_query(group_key[(size_t)g], line_bits, term_bits);
        const int32_t rank = pos[(size_t)g] - query_base[(size_t)query];
        if (max_lines > 0 && rank >= max_lines) continue;
        lines[line_off[query] + rank] = fm_query_key_line(group_key[(size_t)g], line_bits, term_bits);
    }
    return key_bits;
}
}
