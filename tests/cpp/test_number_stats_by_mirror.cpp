// test_number_stats_by_mirror.cpp — the C++ host mirror's "statistics by key" calls (include/index4j/FmIndex.hpp:
// numberStatsByBatch, numberStatsBy) on the GPU.  Prints what they return, one named line of integers each;
// tests/test_gpu_number_stats_by.py compares the lines with the judge's answer.  Exit code 0 = the calls and the exception contract
// held.
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

template <class V>
static void print(const char *name, const V &v) {
    std::printf("%s", name);
    for (auto x : v) std::printf(" %llu", (unsigned long long)x);
    std::printf("\n");
}

int main(int argc, char **argv) {
    const char *fixture = argc > 1 ? argv[1] : "tests/golden/HDFS_2k_multichar.log";
    std::ifstream in(fixture, std::ios::binary);
    const std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const std::u16string hdfs = utf8_to_u16(raw);
    int failures = 0;
    try {
        FmIndex fm = FmIndexBuilder().setSampleRate(16).build(hdfs);
        fm.toDevice(0);
        try {  // keys are per line: without a line table the library's FMX_E_ARG
            fm.numberStatsBy(u"size ", u"updated: 10.", u".:");
            ++failures;
        } catch (const std::exception &) {
        }
        fm.buildLineTable();
        FmIndex::Query stored;
        stored.all = {u"addStoredBlock"};
        const FmIndex::NumberStatsBy s =
            fm.numberStatsByBatch({u"size ", u"blk_", u"size "}, {u"INFO ", u"updated: 10."}, {0, 0, 1}, u" :.", 16, {stored}, {-1, -1}, {0, -1, -1}, {0, 500, 1000});
        print("val_off", s.valOff);
        print("row_off", s.rowOff);
        print("lines", s.lines);
        print("count", s.count);
        print("sum_lo", s.sumLo);
        print("sum_hi", s.sumHi);
        print("min", s.min);
        print("max", s.max);
        print("pct", s.pct);
        print("no_key", s.noKey);
        print("not_number", s.notNumber);
        print("overflow", s.overflow);
        print("occurrences", s.occurrences);
        print("kept", s.kept);
        print("key_kept", s.keyKept);
        print("status", s.status);
        std::vector<int32_t> units;
        for (const std::u16string &v : s.values) {
            for (char16_t c : v) units.push_back((int32_t)c);
            units.push_back(0xFFFF);
        }
        print("values", units);
        if (s.values.size() != (size_t)s.valOff[2] || s.permilles != 3) ++failures;
        const FmIndex::NumberStatsBy one = fm.numberStatsBy(u"size ", u"updated: 10.", u".:");
        if (one.values != std::vector<std::u16string>{u"250", u"251"} || one.lines != std::vector<int32_t>{37, 210} || one.count != std::vector<int32_t>{27, 176} ||
            one.sumLo[1] != 11326104278ULL || one.min[0] != 3541872 || one.noKey[0] != 361 || one.notNumber[0] != 44 || one.kept[0] != 608)
            ++failures;
        if (one.mean(0) < 3541872.0 || one.mean(0) > 67108864.0) ++failures;
        const FmIndex::NumberStatsBy w = fm.numberStatsBy(u"size ", u"INFO ", u" :", 32, &stored);
        if (w.values.size() != 60) ++failures;
        try {  // an empty pattern, key or term: the reference's exception
            fm.numberStatsBy(u"", u"INFO ");
            ++failures;
        } catch (const std::out_of_range &) {
        }
        try {
            fm.numberStatsBy(u"size ", u"");
            ++failures;
        } catch (const std::out_of_range &) {
        }
        try {  // byOf outside 0 .. m - 1: FMX_E_ARG surfaces as an exception
            fm.numberStatsByBatch({u"size "}, {u"INFO "}, {1}, u" ", 8, {}, {-1}, {-1});
            ++failures;
        } catch (const std::exception &) {
        }
        try {  // number patterns without a key pattern
            fm.numberStatsByBatch({u"size "}, {}, {0}, u" ", 8, {}, {}, {-1});
            ++failures;
        } catch (const std::exception &) {
        }
        for (int32_t bad : {0, 65}) {
            try {
                fm.numberStatsBy(u"size ", u"INFO ", u" ", bad);
                ++failures;
            } catch (const std::exception &) {
            }
        }
        try {
            fm.numberStatsBy(u"size ", u"INFO ", u" ", 8, nullptr, {1001});
            ++failures;
        } catch (const std::exception &) {
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
