// test_extract_packed_mirror.cpp — the C++ host mirror's packed-text calls (include/index4j/FmIndex.hpp: extractPacked,
// lineTextBatch, lineText) on the GPU.  Prints what they return, one named line of integers each (characters as code units);
// tests/test_gpu_extract_packed.py compares the lines with the judge's answer.  Exit code 0 = the calls and the exception
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
    for (auto x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

int main(int argc, char **argv) {
    const char *fixture = argc > 1 ? argv[1] : "tests/golden/HDFS_2k_multichar.log";
    std::ifstream in(fixture, std::ios::binary);
    const std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const std::u16string hdfs = utf8_to_u16(raw);
    const int32_t len = (int32_t)hdfs.size();
    int failures = 0;
    try {
        FmIndex fm = FmIndexBuilder().setSampleRate(16).build(hdfs);
        fm.toDevice(0);
        // ranges: empty, one character, across samples, to the last character, three kinds of status
        const std::vector<int32_t> starts = {5, 0, 15, 1000, len - 40, -1, 10, 70000, 9};
        const std::vector<int32_t> stops = {5, 1, 49, 1300, len, 4, len + 1, 69000, 10};
        const FmIndex::Text t = fm.extractPacked(starts, stops);
        print("offsets", t.offsets);
        print("status", t.status);
        print("chars", t.chars);
        for (size_t i = 0; i < starts.size(); ++i)
            if (t.status[i] == 0 && stops[i] > starts[i] && t[i] != hdfs.substr((size_t)starts[i], (size_t)(stops[i] - starts[i]))) ++failures;
        if (fm.extractPacked({}, {}).offsets != std::vector<int64_t>{0}) ++failures;
        try {
            fm.extractPacked({1, 2}, {3});
            ++failures;
        } catch (const std::invalid_argument &) {
        }
        try {  // no line table yet: the library's FMX_E_ARG surfaces as an exception
            fm.lineText({0});
            ++failures;
        } catch (const std::exception &) {
        }
        print("n_lines", std::vector<int64_t>{fm.buildLineTable()});
        const FmIndex::Text lines = fm.lineTextBatch({0, 1999, -1, 2000, 7});
        print("line_offsets", lines.offsets);
        print("line_status", lines.status);
        print("line_chars", lines.chars);
        const std::vector<std::u16string> two = fm.lineText({3, 4});
        print("line3", two[0]);
        print("line4", two[1]);
        try {  // an id that is no line: the reference's "Requested position less than 0"
            fm.lineText({2000});
            ++failures;
        } catch (const std::exception &) {
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "FAIL: %s\n", e.what());
        return 1;
    }
    if (failures) std::fprintf(stderr, "FAIL: %d checks\n", failures);
    return failures ? 1 : 0;
}
