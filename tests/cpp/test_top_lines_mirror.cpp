// test_top_lines_mirror.cpp — the C++ host mirror's "lines ranked by the number behind a pattern" calls
// (include/index4j/FmIndex.hpp: topLinesByNumberBatch, topLinesByNumber) on the GPU.  Prints what they return, one named line of
// integers each; tests/test_gpu_top_lines.py compares the lines with the judge's answer and holds topLinesByNumber to the batch
// form.  Exit code 0 = the calls and the exception contract held.
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
        FmIndex::Query stored;
        stored.all = {u"addStoredBlock"};
        try {  // without a line table: always the library's FMX_E_ARG (the answer is lines)
            fm.topLinesByNumber(u"size ");
            ++failures;
        } catch (const std::exception &) {
        }
        fm.buildLineTable();
        const FmIndex::TopLines s = fm.topLinesByNumberBatch({u"size ", u"size ", u"zzqq#", u"blk_"}, {stored}, {-1, 0, 0, -1}, {1, 0, 1, 0}, 5, 1);
        print("batch_rows", s.rows);
        print("batch_line", s.line);
        print("batch_value", s.value);
        print("batch_loc", s.loc);
        print("batch_lines", s.lines);
        print("batch_numbers", s.numbers);
        print("batch_not_number", s.notNumber);
        print("batch_overflow", s.overflow);
        print("batch_occurrences", s.occurrences);
        print("batch_kept", s.kept);
        print("batch_status", s.status);
        print("batch_term_status", s.termStatus);
        if (s.top != 5 || s.line.size() != 20 || s.value.size() != 20 || s.loc.size() != 20) ++failures;
        // one pattern: the batch form's row, cut to rows[0]
        const FmIndex::TopLines one = fm.topLinesByNumber(u"size ", 5, false, 1, &stored);
        print("one_line", one.line);
        print("one_value", one.value);
        print("one_loc", one.loc);
        print("one_counts", std::vector<int32_t>{one.rows[0], one.lines[0], one.numbers[0], one.notNumber[0], one.overflow[0], one.kept[0]});
        const FmIndex::TopLines src = fm.topLinesByNumber(u"src: /10.", 4, true, 0, nullptr, 3);
        print("src_line", src.line);
        print("src_value", src.value);
        const FmIndex::TopLines win = fm.topLinesByNumber(u"blk_", 2, false, 0, nullptr, 0, 1000, 1100);
        print("win_line", win.line);
        print("win_value", win.value);
        print("win_counts", std::vector<int32_t>{win.rows[0], win.lines[0], win.numbers[0]});
        const FmIndex::TopLines none = fm.topLinesByNumber(u"blk_", 10, false, 1004);
        if (none.rows[0] != 0 || !none.line.empty() || none.lines[0] != 1004) ++failures;
        try {  // an empty pattern or term: the reference's exception
            fm.topLinesByNumber(u"");
            ++failures;
        } catch (const std::out_of_range &) {
        }
        try {
            FmIndex::Query bad;
            bad.none = {u""};
            fm.topLinesByNumber(u"size ", 10, true, 0, &bad);
            ++failures;
        } catch (const std::out_of_range &) {
        }
        struct Bad {
            int32_t top, first, frac, lo, hi;
        };
        for (const Bad b : {Bad{0, 0, 0, 0, INT32_MAX}, Bad{3, -1, 0, 0, INT32_MAX}, Bad{3, 0, 10, 0, INT32_MAX}, Bad{3, 0, -1, 0, INT32_MAX},
                            Bad{3, 0, 0, 5, 4}, Bad{3, 0, 0, -1, 4}}) {
            try {  // arguments the library refuses: FMX_E_ARG surfaces as an exception
                fm.topLinesByNumber(u"size ", b.top, true, b.first, nullptr, b.frac, b.lo, b.hi);
                ++failures;
            } catch (const std::exception &) {
            }
        }
        try {  // whereOf outside -1 .. q - 1
            fm.topLinesByNumberBatch({u"size "}, {stored}, {1}, {1});
            ++failures;
        } catch (const std::exception &) {
        }
        try {  // descending has one entry per pattern
            fm.topLinesByNumberBatch({u"size "}, {stored}, {0}, {1, 0});
            ++failures;
        } catch (const std::invalid_argument &) {
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    return failures ? 1 : 0;
}
