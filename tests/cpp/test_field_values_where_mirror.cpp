// test_field_values_where_mirror.cpp — the C++ host mirror's "values that follow a pattern, where the line matches a query" calls
// (include/index4j/FmIndex.hpp: fieldValuesWhereBatch, fieldValuesWhere) on the GPU.  Prints what they return, one named line of
// integers each; tests/test_gpu_field_values_where.py compares the lines with the judge's answer.  Exit code 0 = the calls and the
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
        const std::u16string stop = u" \t\r\n:";
        FmIndex::Query terminating, blocks;
        terminating.all = {u"terminating"};
        blocks.all = {u"blk_"};
        blocks.none = {u"PacketResponder"};
        // without a line table: an unfiltered call is fieldValuesBatch's answer, a filtered one the library's FMX_E_ARG
        const FmIndex::FieldValuesWhere plain = fm.fieldValuesWhereBatch({u"blk_", u"INFO "}, {terminating}, {-1, -1}, stop, 32);
        const FmIndex::FieldValues same = fm.fieldValuesBatch({u"blk_", u"INFO "}, stop, 32);
        if (plain.offsets != same.offsets || plain.counts != same.counts || plain.textOffsets != same.textOffsets || plain.chars != same.chars ||
            plain.occurrences != same.occurrences || plain.status != same.status || plain.kept != same.occurrences)
            ++failures;
        try {
            fm.fieldValuesWhere(u"blk_", terminating, stop, 32);
            ++failures;
        } catch (const std::exception &) {
        }
        fm.buildLineTable();
        const FmIndex::FieldValuesWhere b = fm.fieldValuesWhereBatch({u"blk_", u"INFO ", u"zzqq#", u"INFO "}, {terminating, blocks}, {0, 1, 0, -1}, stop, 32);
        print("batch_val_off", b.offsets);
        print("batch_counts", b.counts);
        print("batch_text_off", b.textOffsets);
        print("batch_chars", b.chars);
        print("batch_occurrences", b.occurrences);
        print("batch_kept", b.kept);
        print("batch_status", b.status);
        print("batch_term_status", b.termStatus);
        std::vector<int32_t> counts, units;
        for (const auto &vc : fm.fieldValuesWhere(u"INFO ", blocks, stop, 32)) counts.push_back(vc.second);
        print("one_counts", counts);
        counts.clear();
        for (const auto &vc : fm.fieldValuesWhere(u"INFO ", blocks, stop, 32, 2)) {
            counts.push_back(vc.second);
            units.insert(units.end(), vc.first.begin(), vc.first.end());
        }
        print("top_counts", counts);
        print("top_chars", units);
        const FmIndex::FieldValuesWhere window = fm.fieldValuesWhereBatch({u"blk_"}, {}, {-1}, stop, 32, 100, 200);
        print("window_kept", window.kept);
        try {  // an empty term: the reference's exception
            FmIndex::Query bad;
            bad.all = {u""};
            fm.fieldValuesWhere(u"blk_", bad);
            ++failures;
        } catch (const std::out_of_range &) {
        }
        try {  // whereOf outside -1 .. q - 1: the library's FMX_E_ARG surfaces as an exception
            fm.fieldValuesWhereBatch({u"blk_"}, {terminating}, {1}, stop, 32);
            ++failures;
        } catch (const std::exception &) {
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
