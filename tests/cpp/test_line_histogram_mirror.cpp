// test_line_histogram_mirror.cpp — the C++ host mirror's "matching lines and hits per bucket of lines" calls
// (include/index4j/FmIndex.hpp: lineHistogramBatch, lineHistogram, hitHistogramWhereBatch, hitHistogramWhere) on the GPU.  Prints
// what they return, one named line of integers each; tests/test_gpu_line_histogram.py compares the lines with the judge's answer.
// Exit code 0 = the calls and the exception contract held.
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
    for (auto x : v) std::printf(" %lld", (long long)x);
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
        FmIndex::Query terminating, blocks, nothing;
        terminating.all = {u"terminating"};
        blocks.all = {u"blk_"};
        blocks.none = {u"PacketResponder"};
        nothing.none = {u"INFO"};
        std::vector<int32_t> edges;
        for (int32_t e = 0; e <= 2000; e += 250) edges.push_back(e);
        const std::vector<int32_t> uneven{3, 4, 4, 100, 101, 1024, 1990, 1990, 1999};
        try {  // without a line table: the library's FMX_E_ARG, in both forms, a filter or none
            fm.hitHistogramWhereBatch({u"blk_"}, {}, {-1}, edges);
            ++failures;
        } catch (const std::exception &) {
        }
        try {
            fm.lineHistogram(terminating, edges);
            ++failures;
        } catch (const std::exception &) {
        }
        fm.buildLineTable();
        const FmIndex::LineHistogram l = fm.lineHistogramBatch({terminating, blocks, nothing}, edges);
        print("lines_counts", l.counts);
        print("lines_line_count", l.lineCount);
        print("lines_occurrences", l.occurrences);
        print("lines_status", l.status);
        print("lines_row1", l.row(1));
        print("lines_one", fm.lineHistogram(blocks, uneven));
        const FmIndex::HitHistogram h = fm.hitHistogramWhereBatch({u"blk_", u"blk_", u"zzqq#", u"INFO "}, {terminating, blocks}, {-1, 0, 0, 1}, edges);
        print("hits_counts", h.counts);
        print("hits_occurrences", h.occurrences);
        print("hits_kept", h.kept);
        print("hits_status", h.status);
        print("hits_term_status", h.termStatus);
        print("hits_one", fm.hitHistogramWhere(u"blk_", terminating, uneven));
        print("hits_raw_uneven", fm.hitHistogramWhereBatch({u"blk_"}, {}, {-1}, uneven).counts);
        try {  // an empty term: the reference's exception
            FmIndex::Query bad;
            bad.all = {u""};
            fm.lineHistogram(bad, edges);
            ++failures;
        } catch (const std::out_of_range &) {
        }
        try {
            fm.hitHistogramWhere(u"", terminating, edges);
            ++failures;
        } catch (const std::out_of_range &) {
        }
        for (const std::vector<int32_t> &bad : {std::vector<int32_t>{5}, std::vector<int32_t>{-1, 5}, std::vector<int32_t>{5, 4}, std::vector<int32_t>{}}) {
            try {  // edges the library refuses: FMX_E_ARG surfaces as an exception
                fm.lineHistogram(terminating, bad);
                ++failures;
            } catch (const std::exception &) {
            }
            try {
                fm.hitHistogramWhere(u"blk_", terminating, bad);
                ++failures;
            } catch (const std::exception &) {
            }
        }
        try {  // whereOf outside -1 .. q - 1
            fm.hitHistogramWhereBatch({u"blk_"}, {terminating}, {1}, edges);
            ++failures;
        } catch (const std::exception &) {
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
