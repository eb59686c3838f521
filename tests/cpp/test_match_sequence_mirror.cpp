// test_match_sequence_mirror.cpp — the C++ host mirror's "lines that hold a sequence of terms in order" calls
// (include/index4j/FmIndex.hpp: matchSequenceBatch, matchSequence) on the GPU.  Prints what they return, one named line of integers
// each; tests/test_gpu_match_sequence.py compares the lines with the judge's answer.  Exit code 0 = the calls and the exception
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
    int failures = 0;
    try {
        FmIndex fm = FmIndexBuilder().setSampleRate(16).build(hdfs);
        fm.toDevice(0);
        const std::vector<std::u16string> two{u"PacketResponder", u"terminating"};
        try {  // no line table yet: the library's FMX_E_ARG surfaces as an exception
            fm.matchSequence(two);
            ++failures;
        } catch (const std::exception &) {
        }
        print("n_lines", std::vector<int64_t>{fm.buildLineTable()});
        const std::vector<std::vector<std::u16string>> sequences = {two,
                                                                    {u"terminating", u"PacketResponder"},
                                                                    {u"blk_", u"blk_", u"blk_"},
                                                                    {},
                                                                    {u"blk_", u"/"},
                                                                    {u":", u":", u":", u":", u":"}};
        const FmIndex::SequenceLines all = fm.matchSequenceBatch(sequences, 0, true);
        print("batch_offsets", all.offsets);
        print("batch_lines", all.lines);
        print("batch_spans", all.spans);
        print("batch_line_count", all.lineCount);
        print("batch_occurrences", all.occurrences);
        const FmIndex::SequenceLines cut = fm.matchSequenceBatch(sequences, 7);
        print("cut_offsets", cut.offsets);
        print("cut_lines", cut.lines);
        print("cut_spans", cut.spans);
        print("cut_line_count", cut.lineCount);
        print("one", fm.matchSequence(two));
        print("one_cut", fm.matchSequence(two, 3));
        if (!fm.matchSequence({u"terminating", u"PacketResponder"}).empty()) ++failures;
        if (!fm.matchSequence({}).empty()) ++failures;
        if (!fm.matchSequence({u"\n"}).empty()) ++failures;  // the boundary itself runs over its line's end
        if (fm.matchSequenceBatch({}).offsets != std::vector<int64_t>{0}) ++failures;
        if (fm.matchSequenceBatch({{}, {}}, 0, true).offsets != std::vector<int64_t>{0, 0, 0}) ++failures;
        try {  // an empty term: ArrayIndexOutOfBoundsException (FM:456-457), as matchLines raises it
            fm.matchSequence({u"INFO", u""});
            ++failures;
        } catch (const std::out_of_range &) {
        }
        try {
            fm.matchSequenceBatch({{u"WARN", u""}});
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
