// test_locate_all_mirror.cpp — the C++ host mirror's "all occurrences" calls (include/index4j/FmIndex.hpp: locateAllBatch,
// locateAll) on the GPU.  Prints what they return, one named line of integers each; tests/test_gpu_locate_all.py compares the
// lines with the oracle's answer.  Exit code 0 = the calls and the exception contract held.
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
        const std::vector<std::u16string> pats = {u"INFO", u"zzzzqq#", u"blk_"};
        const FmIndex::Hits hits = fm.locateAllBatch(pats);
        print("batch_offsets", hits.offsets);
        print("batch_locations", hits.locations);
        const FmIndex::Hits cut = fm.locateAllBatch(pats, 7);
        print("cut_offsets", cut.offsets);
        print("cut_locations", cut.locations);
        print("all", fm.locateAll(u"INFO"));
        if (!fm.locateAll(u"zzzzqq#").empty()) ++failures;
        if (fm.locateAllBatch({}).offsets != std::vector<int64_t>{0}) ++failures;
        try {  // an empty pattern: ArrayIndexOutOfBoundsException (FM:456-457), as locate() raises it
            fm.locateAll(u"");
            ++failures;
        } catch (const std::out_of_range &) {
        }
        try {
            fm.locateAllBatch({u"INFO", u""});
            ++failures;
        } catch (const std::out_of_range &) {
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "FAIL: %s\n", e.what());
        return 1;
    }
    if (failures) std::fprintf(stderr, "FAIL: %d checks\n", failures);
    return failures ? 1 : 0;
}
