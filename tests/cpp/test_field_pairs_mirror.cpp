// test_field_pairs_mirror.cpp — the C++ host mirror's "statistics by two keys" calls (include/index4j/FmIndex.hpp: fieldValuePairs,
// numberStatsByPair, numberStatsByPairBatch).  `host FIXTURE`: the exception contract of an index that is not resident, no device
// needed.  `gpu FIXTURE`: prints what the calls return on the fixture, one named line each; tests/test_cpp_field_pairs.py compares
// the lines with the judge's answer.  Exit code 0 = the calls and the exception contract held.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "../../include/index4j/FmIndex.hpp"

using index4j::FmIndex;
using index4j::FmIndexBuilder;

static std::u16string utf8_to_u16(const std::string &s) {  // BMP only (the fixture has no astral chars)
    std::u16string out;
    for (size_t i = 0; i < s.size();) {
        unsigned c = (unsigned char)s[i];
        if (c < 0x80) {
            out.push_back((char16_t)c);
            i += 1;
        } else if ((c >> 5) == 6) {
            out.push_back((char16_t)(((c & 0x1f) << 6) | (s[i + 1] & 0x3f)));
            i += 2;
        } else {
            out.push_back((char16_t)(((c & 0x0f) << 12) | ((s[i + 1] & 0x3f) << 6) | (s[i + 2] & 0x3f)));
            i += 3;
        }
    }
    return out;
}

static std::string ascii(const std::u16string &s) {  // (the fixture's keys are ASCII)
    std::string out;
    for (char16_t c : s) out.push_back((char)c);
    return out;
}

template <class V>
static void print(const char *name, const V &v) {
    std::printf("%s", name);
    for (auto x : v) std::printf(" %llu", (unsigned long long)x);
    std::printf("\n");
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "host";
    const char *fixture = argc > 2 ? argv[2] : "tests/golden/HDFS_2k_multichar.log";
    std::ifstream in(fixture, std::ios::binary);
    const std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const std::u16string hdfs = utf8_to_u16(raw);
    const std::u16string stop = u" :.$\n";
    int failures = 0;
    try {
        FmIndex fm = FmIndexBuilder().setSampleRate(16).setDevice(mode == "host" ? -1 : 0).build(hdfs);
        try {  // the shapes the mirror judges itself, before the library is asked
            fm.numberStatsByPairBatch({}, {u"0811"}, {}, {0}, {0, 0}, stop, 32, {}, {-1}, {});
            ++failures;
        } catch (const std::invalid_argument &) {
        }
        try {
            fm.numberStatsByPairBatch({u"size "}, {u"0811"}, {}, {0}, {0}, stop, 32, {}, {-1}, {-1});
            ++failures;
        } catch (const std::invalid_argument &) {
        }
        try {  // an empty key: the reference's exception
            fm.fieldValuePairs(u"0811", u"");
            ++failures;
        } catch (const std::out_of_range &) {
        }
        try {
            fm.numberStatsByPair(u"", u"0811", u"INFO dfs.");
            ++failures;
        } catch (const std::out_of_range &) {
        }
        if (mode == "host") {
            try {  // no CPU fallback: an index that is not resident answers with the library's error
                fm.fieldValuePairs(u"0811", u"INFO dfs.", stop);
                ++failures;
            } catch (const std::out_of_range &) {
                ++failures;
            } catch (const std::exception &) {
            }
            return failures ? 1 : 0;
        }
        try {  // keys are per line: without a line table the library's FMX_E_ARG
            fm.fieldValuePairs(u"0811", u"INFO dfs.", stop);
            ++failures;
        } catch (const std::exception &) {
        }
        fm.buildLineTable();
        const FmIndex::NumberStatsByPair s = fm.numberStatsByPair(u"size ", u"0811", u"INFO dfs.", stop, 32);
        std::printf("pairs");
        for (size_t r = 0; r < s.pairLines.size(); ++r) {
            const auto v = s.pairValues(0, r);
            std::printf(" %s|%s", ascii(v.first).c_str(), ascii(v.second).c_str());
        }
        std::printf("\n");
        print("pair_lines", s.pairLines);
        print("count", s.count);
        print("sum_lo", s.sumLo);
        print("sum_hi", s.sumHi);
        print("min", s.min);
        print("max", s.max);
        print("pct", s.pct);
        print("counters", std::vector<int32_t>{s.noKey[0], s.notNumber[0], s.overflow[0], s.kept[0]});
        if (s.pairOff != std::vector<int64_t>{0, 11} || s.rowOff != std::vector<int64_t>{0, 11} || s.permilles != 2 || s.valOff.size() != 3) ++failures;
        const std::vector<FmIndex::ValuePair> pivot = fm.fieldValuePairs(u"0811", u"INFO dfs.", stop);
        std::vector<int32_t> pivot_lines;
        for (const FmIndex::ValuePair &p : pivot) pivot_lines.push_back(p.lines);
        print("pivot_lines", pivot_lines);
        if (pivot.size() != 11 || pivot[0].a != u"09" || pivot[0].b != u"DataBlockScanner" || pivot[0].lines != 2 || pivot[4].lines != 354) ++failures;
        FmIndex::Query filter;
        filter.all = {u"blk_"};
        filter.none = {u"PacketResponder"};
        const std::vector<FmIndex::ValuePair> filtered = fm.fieldValuePairs(u"0811", u"INFO dfs.", stop, 32, &filter);
        if (filtered.size() != 11 || filtered[4].b != u"DataNode" || filtered[4].lines != 145) ++failures;
        if (!fm.fieldValuePairs(u"0811", u"zzqq#", stop).empty()) ++failures;
        // two pairs in one call, a number pattern on each; a pair of one key
        const FmIndex::NumberStatsByPair two =
            fm.numberStatsByPairBatch({u"size ", u"blk_"}, {u"0811", u"INFO dfs."}, {1, 0}, {0, 1}, {1, 1}, stop, 32, {}, {-1, -1}, {-1, -1});
        if (two.pairOff != std::vector<int64_t>{0, 11, 15} || two.rowOff != std::vector<int64_t>{0, 4, 15} || two.pairGroupA[11] != two.pairGroupB[11]) ++failures;
        try {  // a pair outside the key patterns: FMX_E_ARG surfaces as an exception
            fm.numberStatsByPairBatch({}, {u"0811"}, {}, {0}, {1}, stop, 32, {}, {-1}, {});
            ++failures;
        } catch (const std::exception &) {
        }
        try {  // byOf names pairs
            fm.numberStatsByPairBatch({u"size "}, {u"0811", u"INFO dfs."}, {1}, {0}, {1}, stop, 32, {}, {-1, -1}, {-1});
            ++failures;
        } catch (const std::exception &) {
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
