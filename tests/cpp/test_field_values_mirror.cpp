// test_field_values_mirror.cpp — the C++ host mirror's "values that follow a pattern, with counts" calls
// (include/index4j/FmIndex.hpp: fieldValuesBatch, fieldValuesClass, fieldValues) on the GPU.  Prints what they return, one named
// line of integers each; tests/test_gpu_field_values.py compares the lines with the judge's answer.  Exit code 0 = the calls and the
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
        const std::u16string stop = u" \n:";
        const FmIndex::FieldValues b = fm.fieldValuesBatch({u"blk_", u"zzqq#", u"INFO ", u"\n"}, stop, 24);
        print("batch_val_off", b.offsets);
        print("batch_counts", b.counts);
        print("batch_text_off", b.textOffsets);
        print("batch_chars", b.chars);
        print("batch_occurrences", b.occurrences);
        print("batch_status", b.status);
        std::vector<int32_t> counts, units;
        for (const auto &vc : fm.fieldValues(u"INFO ", stop, 24)) counts.push_back(vc.second);
        print("one_counts", counts);
        counts.clear();
        for (const auto &vc : fm.fieldValues(u"INFO ", stop, 24, 3)) {
            counts.push_back(vc.second);
            units.insert(units.end(), vc.first.begin(), vc.first.end());
        }
        print("top_counts", counts);
        print("top_chars", units);
        print("icase_values", std::vector<int64_t>{(int64_t)fm.fieldValues(u"BLOCK", stop, 24, 0, true).size()});
        if (!fm.fieldValues(u"bLOCK", stop, 24).empty()) ++failures;  // (no such spelling in the text)
        const FmIndex::FieldValues none = fm.fieldValuesBatch({u"zzqq#", u""}, stop, 24);  // statuses are the patterns' own: nothing is thrown
        if (!none.counts.empty() || none.status[1] != FMX_ST_JAVA_AIOOBE || none.offsets != std::vector<int64_t>{0, 0, 0}) ++failures;
        try {  // an empty pattern: the reference's exception
            fm.fieldValues(u"");
            ++failures;
        } catch (const std::out_of_range &) {
        }
        try {  // max_len outside [1, 64]: the library's FMX_E_ARG surfaces as an exception
            fm.fieldValues(u"blk_", stop, 65);
            ++failures;
        } catch (const std::exception &) {
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
