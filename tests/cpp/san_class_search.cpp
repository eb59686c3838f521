// san_class_search.cpp — sanitizer driver of the class search: tests/class_search_hostsim.cpp (the device header's fm_class_*
// functions and the serial mirror of k_class_search, both stages) as a stand-alone program for -fsanitize=address,undefined.
// Every array has exactly the size the contract gives it — the two frontiers of a team hold max_ranges pairs, the codes
// kClassAltsMax entries, d_ranges 2 * m ints — so a store outside them is a report.  A synthetic log at sample rates 1 and 16,
// each under a roomy cap and under the exact cap S of the batch's largest frontier (and S - 1, which must refuse exactly the
// patterns that reach S); the judge here is the literal search (sim_count) of every string a pattern spells, ascending by
// start (the oracle judges IT in the CPU suite).  Prints one " ok: " line per run; exit code 0 = clean.
#include "../class_search_hostsim.cpp"

#include <algorithm>
#include <cstdio>
#include <string>
#include <utility>

#include "fmx_model.hpp"

extern "C" int fmx_synth_log(uint64_t seed, int32_t n, uint16_t *out);

namespace {

using Pattern = std::vector<std::vector<uint16_t>>;  // positions of alternatives

std::vector<uint16_t> span(uint16_t lo, uint16_t hi) {
    std::vector<uint16_t> v;
    for (uint32_t c = lo; c <= hi; ++c) v.push_back((uint16_t)c);
    return v;
}
std::vector<uint16_t> join(std::vector<uint16_t> a, const std::vector<uint16_t> &b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
Pattern icase(const char *w) {
    Pattern p;
    for (; *w; ++w) {
        const char c = *w;
        std::vector<uint16_t> alts{(uint16_t)c};
        if (c >= 'a' && c <= 'z') alts.push_back((uint16_t)(c - 32));
        if (c >= 'A' && c <= 'Z') alts.push_back((uint16_t)(c + 32));
        p.push_back(alts);
    }
    return p;
}

std::vector<Pattern> batch() {
    const std::vector<uint16_t> digit = span('0', '9'), lower = span('a', 'z'), upper = span('A', 'Z');
    std::vector<Pattern> b;
    b.push_back({{'Q'}, {'z'}, digit});                           // the first pattern: no hits
    b.push_back({digit, digit});                                  // heavy
    b.push_back({join(lower, upper), lower});                     // up to 52 x 26 candidates per round
    b.push_back({{':'}, digit, digit});
    b.push_back(icase("info"));
    b.push_back(icase("error"));
    b.push_back(icase("block"));
    b.push_back({});                                              // no positions
    b.push_back({{'a'}, {}, {'b'}});                              // a position without alternatives
    b.push_back({{'e', 'e', 'e'}, {'r', 0x20AC, 'r'}});           // duplicates, a character the alphabet lacks
    b.push_back({{'e'}, join(span(0x4E00, 0x4E00 + 63), {'r'})});  // 65 alternatives
    b.push_back({join(span(0x4E00, 0x4E00 + 62), {'e'}), {'r'}});  // 64
    b.push_back({digit, digit, digit});
    b.push_back({{'z'}, {'Q'}, {'q', 'Q'}});                      // the last pattern: no hits
    return b;
}

struct Packed {
    std::vector<uint16_t> alt;
    std::vector<int32_t> pos_off{0}, pat_off{0};
};
Packed pack(const std::vector<Pattern> &b) {
    Packed P;
    for (const Pattern &p : b) {
        for (const auto &alts : p) {
            P.alt.insert(P.alt.end(), alts.begin(), alts.end());
            P.pos_off.push_back((int32_t)P.alt.size());
        }
        P.pat_off.push_back((int32_t)P.pos_off.size() - 1);
    }
    return P;
}

// the literal ranges of every string the pattern spells, those with hits, ascending by start; *largest = its largest frontier
std::vector<std::pair<int32_t, int32_t>> judge(const uint8_t *blob, const Pattern &p, int32_t *largest) {
    std::vector<std::vector<uint16_t>> alive{{}};
    std::vector<std::pair<int32_t, int32_t>> ranges;
    *largest = 0;
    for (size_t k = 1; k <= p.size(); ++k) {
        std::vector<uint16_t> units;
        for (uint16_t u : p[p.size() - k])
            if (std::find(units.begin(), units.end(), u) == units.end()) units.push_back(u);
        std::vector<std::vector<uint16_t>> next;
        ranges.clear();
        for (uint16_t u : units)
            for (const auto &s : alive) {
                std::vector<uint16_t> t{u};
                t.insert(t.end(), s.begin(), s.end());
                const int32_t off[2] = {0, (int32_t)t.size()};
                int32_t count = 0, range[2] = {0, 0};
                sim_count(blob, t.data(), off, 1, &count, nullptr, nullptr, range);
                if (range[0] < range[1]) {
                    next.push_back(t);
                    ranges.emplace_back(range[0], range[1]);
                }
            }
        alive.swap(next);
        if ((int32_t)alive.size() > *largest) *largest = (int32_t)alive.size();
        if (alive.empty()) break;
    }
    if (p.empty() || alive.empty()) ranges.clear();
    std::sort(ranges.begin(), ranges.end());
    return ranges;
}

}  // namespace

int main() {
    std::vector<uint16_t> text(50000);
    fmx_synth_log(42, (int32_t)text.size(), text.data());
    const std::vector<Pattern> b = batch();
    const Packed P = pack(b);
    const int32_t n = (int32_t)b.size();
    for (int sr : {1, 16}) {
        fmx::FmModel m;
        std::string err;
        std::vector<uint8_t> blob;
        if (fmx::build_model(text.data(), (int32_t)text.size(), sr, true, m, err) || fmx::flatten_model(m, blob, err)) {
            printf("build failed: %s\n", err.c_str());
            return 1;
        }
        std::vector<std::vector<std::pair<int32_t, int32_t>>> want((size_t)n);
        std::vector<int32_t> largest((size_t)n);
        int32_t S = 0;
        bool wide65 = false;
        for (int32_t i = 0; i < n; ++i) {
            want[(size_t)i] = judge(blob.data(), b[(size_t)i], &largest[(size_t)i]);
            if (largest[(size_t)i] > S) S = largest[(size_t)i];
        }
        if (S < 50 || S > kClassRangesMax) {
            printf("the batch's largest frontier is %d\n", S);
            return 1;
        }
        for (int32_t cap : {S, S - 1}) {
            std::vector<int64_t> range_off((size_t)n + 1);
            std::vector<int32_t> counts((size_t)n), status((size_t)n);
            int64_t info[3];
            sim_class_count(blob.data(), P.alt.data(), P.pos_off.data(), P.pat_off.data(), n, cap, cap == S ? 4 : 3, cap == S ? 2 : 1,
                            range_off.data(), counts.data(), status.data(), info);
            std::vector<int32_t> ranges((size_t)(2 * range_off[(size_t)n]));  // exactly m pairs: one more is a report
            sim_class_fill(blob.data(), P.alt.data(), P.pos_off.data(), P.pat_off.data(), n, cap, cap == S ? 4 : 3, cap == S ? 2 : 1,
                           range_off.data(), ranges.data());
            int32_t refused = 0;
            for (int32_t i = 0; i < n; ++i) {
                const Pattern &p = b[(size_t)i];
                bool wide = false;
                for (const auto &alts : p) wide |= (int32_t)alts.size() > kClassAltsMax;
                wide65 |= wide;
                const int want_status = p.empty() ? ST_JAVA_AIOOBE : (wide || largest[(size_t)i] > cap) ? ST_TOO_MANY_RANGES : ST_OK;
                refused += want_status == ST_TOO_MANY_RANGES;
                const auto none = std::vector<std::pair<int32_t, int32_t>>();
                const auto &w = want_status == ST_OK ? want[(size_t)i] : none;
                int32_t sum = 0;
                bool same = status[(size_t)i] == want_status && range_off[(size_t)i + 1] - range_off[(size_t)i] == (int64_t)w.size();
                for (size_t r = 0; same && r < w.size(); ++r) {
                    const size_t at = (size_t)(2 * (range_off[(size_t)i] + (int64_t)r));
                    same = ranges[at] == w[r].first && ranges[at + 1] == w[r].second;
                    sum += w[r].second - w[r].first;
                }
                if (!same || counts[(size_t)i] != sum) {
                    printf("sr %d cap %d: pattern %d differs (status %d, want %d)\n", sr, cap, i, status[(size_t)i], want_status);
                    return 1;
                }
            }
            if (!wide65 || (cap == S) != (refused == 1)) {
                printf("sr %d cap %d: %d patterns refused\n", sr, cap, refused);
                return 1;
            }
            printf("sr %d cap %d ok: %d patterns, %lld ranges, %lld candidates, largest frontier %lld\n", sr, cap, n,
                   (long long)range_off[(size_t)n], (long long)info[0], (long long)info[2]);
        }
    }
    return 0;
}
