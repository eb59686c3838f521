// test_field_values_histogram_mirror.cpp — the C++ host mirror's "top values per bucket" calls (include/index4j/FmIndex.hpp:
// fieldValuesHistogramBatch, fieldValuesHistogram) on the GPU.  Prints what they return, one named line of integers each;
// tests/test_gpu_field_values_histogram.py compares the lines with the judge's answer.  Exit code 0 = the calls and the exception
// contract held.
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
        // no edges and no query: the device-side top-k needs no line table
        const FmIndex::FieldValuesHistogram k = fm.fieldValuesHistogram(u"INFO ", {}, 2, nullptr, u" :");
        if (k.values != std::vector<std::u16string>{u"dfs.FSNamesystem", u"dfs.DataNode$PacketResponder"} || k.rowCount != std::vector<int32_t>{525, 480} ||
            k.counts != k.rowCount || k.other != std::vector<int32_t>{1920 - 525 - 480} || k.nValues[0] != 356 || k.buckets != 1)
            ++failures;
        std::vector<int32_t> edges;
        for (int32_t e = 0; e <= 2000; e += 250) edges.push_back(e);
        try {  // the buckets are lines: without a line table the library's FMX_E_ARG
            fm.fieldValuesHistogram(u"INFO ", edges);
            ++failures;
        } catch (const std::exception &) {
        }
        fm.buildLineTable();
        FmIndex::Query q;
        q.all = {u"blk_"};
        q.none = {u"PacketResponder"};
        const FmIndex::FieldValuesHistogram s = fm.fieldValuesHistogramBatch({u"INFO ", u"zzzq#", u"WARN "}, {q}, {0, -1, -1}, edges, 4, u" :", 64);
        print("row_off", s.rowOff);
        print("row_count", s.rowCount);
        print("row_group", s.rowGroup);
        print("hist", s.counts);
        print("other", s.other);
        print("n_values", s.nValues);
        print("occurrences", s.occurrences);
        print("kept", s.kept);
        print("status", s.status);
        std::vector<int32_t> units;
        for (const std::u16string &v : s.values) {
            for (char16_t c : v) units.push_back((int32_t)c);
            units.push_back(0xFFFF);
        }
        print("values", units);
        if (s.buckets != 8 || s.values.size() != (size_t)s.rowOff[3] || s.row(0).size() != 8 || s.otherOf(2).size() != 8) ++failures;
        const FmIndex::FieldValuesHistogram one = fm.fieldValuesHistogram(u" from /10.", edges, 5, nullptr, u".");
        if (one.values != std::vector<std::u16string>{u"251", u"250"} || one.rowCount != std::vector<int32_t>{181, 41} ||
            one.row(1) != std::vector<int32_t>{7, 1, 6, 4, 6, 8, 5, 4} || one.otherOf(0) != std::vector<int32_t>(8, 0) || one.kept[0] != 222)
            ++failures;
        try {  // an empty pattern: the reference's exception
            fm.fieldValuesHistogram(u"");
            ++failures;
        } catch (const std::out_of_range &) {
        }
        for (int32_t bad : {0, 65537}) {  // top outside [1, 65536]: FMX_E_ARG surfaces as an exception
            try {
                fm.fieldValuesHistogram(u"INFO ", edges, bad);
                ++failures;
            } catch (const std::exception &) {
            }
        }
        try {  // edges that decrease
            fm.fieldValuesHistogram(u"INFO ", {0, 5, 4});
            ++failures;
        } catch (const std::exception &) {
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
