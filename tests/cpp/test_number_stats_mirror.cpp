// test_number_stats_mirror.cpp — the C++ host mirror's "statistics of the number behind a pattern" calls
// (include/index4j/FmIndex.hpp: numberStatsWhereBatch, numberStatsWhere) on the GPU.  Prints what they return, one named line of
// integers each; tests/test_gpu_number_stats.py compares the lines with the judge's answer.  Exit code 0 = the calls and the
// exception contract held.
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
        FmIndex::Query stored;
        stored.all = {u"addStoredBlock"};
        std::vector<int32_t> edges;
        for (int32_t e = 0; e <= 2000; e += 250) edges.push_back(e);
        // without a line table: no edges and no filter need none; edges or a filter are the library's FMX_E_ARG
        const FmIndex::NumberStats one = fm.numberStatsWhereBatch({u"src: /10."}, {}, {-1}, {}, {500, 950}, 3);
        print("one_count", one.count);
        print("one_sum_lo", one.sumLo);
        print("one_sum_hi", one.sumHi);
        print("one_min", one.min);
        print("one_pct", one.pct);
        print("one_tails", std::vector<int32_t>{one.notNumber[0], one.overflow[0]});
        if (one.buckets != 1 || one.permilles != 2 || one.mean(0) < 250100.0 || one.mean(0) > 251910.0) ++failures;
        try {
            fm.numberStatsWhereBatch({u"size "}, {}, {-1}, edges);
            ++failures;
        } catch (const std::exception &) {
        }
        try {
            fm.numberStatsWhere(u"size ", stored, {});
            ++failures;
        } catch (const std::exception &) {
        }
        fm.buildLineTable();
        const FmIndex::NumberStats s = fm.numberStatsWhereBatch({u"size ", u"size ", u"zzqq#", u"blk_"}, {stored}, {-1, 0, 0, -1}, edges);
        print("batch_count", s.count);
        print("batch_sum_lo", s.sumLo);
        print("batch_sum_hi", s.sumHi);
        print("batch_min", s.min);
        print("batch_max", s.max);
        print("batch_pct", s.pct);
        print("batch_not_number", s.notNumber);
        print("batch_overflow", s.overflow);
        print("batch_occurrences", s.occurrences);
        print("batch_kept", s.kept);
        print("batch_status", s.status);
        print("batch_term_status", s.termStatus);
        const FmIndex::NumberStats w = fm.numberStatsWhere(u"size ", stored, {});
        if (w.count != std::vector<int32_t>{254} || w.sumLo[0] != 16264173630ULL || w.min[0] != 2 || w.notNumber[0] != 60 || w.kept[0] != 314) ++failures;
        try {  // an empty pattern or term: the reference's exception
            fm.numberStatsWhere(u"", stored, edges);
            ++failures;
        } catch (const std::out_of_range &) {
        }
        try {
            FmIndex::Query bad;
            bad.none = {u""};
            fm.numberStatsWhere(u"size ", bad, edges);
            ++failures;
        } catch (const std::out_of_range &) {
        }
        for (const std::vector<int32_t> &bad : {std::vector<int32_t>{5}, std::vector<int32_t>{-1, 5}, std::vector<int32_t>{5, 4}}) {
            try {  // edges the library refuses: FMX_E_ARG surfaces as an exception
                fm.numberStatsWhere(u"size ", stored, bad);
                ++failures;
            } catch (const std::exception &) {
            }
        }
        for (const std::vector<int32_t> &bad : {std::vector<int32_t>{1001}, std::vector<int32_t>{-1}, std::vector<int32_t>(17, 5)}) {
            try {  // ... and permilles
                fm.numberStatsWhere(u"size ", stored, edges, bad);
                ++failures;
            } catch (const std::exception &) {
            }
        }
        try {
            fm.numberStatsWhere(u"size ", stored, edges, {500}, 10);
            ++failures;
        } catch (const std::exception &) {
        }
        try {  // whereOf outside -1 .. q - 1
            fm.numberStatsWhereBatch({u"size "}, {stored}, {1}, edges);
            ++failures;
        } catch (const std::exception &) {
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
