// index4j/FmIndex.hpp — host-side C++ mirror of com.dynatrace.fm.FmIndex / FmIndexBuilder over the
// C ABI of libfmx.so (include/fmx.h).  Header-only.
//
// The reference's host language is Java; this image has no JDK, so the host layer above the C ABI is
// written in C++ with the reference's method names, argument meaning and error behaviour
// (fm/FmIndex.java:443-941, fm/FmIndexBuilder.java:21-62).  Java exceptions map to:
//   RuntimeException              -> std::runtime_error      (same message)
//   IllegalArgumentException      -> std::invalid_argument   (same message)
//   ArrayIndexOutOfBoundsException-> std::out_of_range
//   IOException                   -> index4j::IoError
// Java `char[]` is std::u16string / char16_t*.  Scalar calls are batches of one on the GPU; the
// *Batch methods are the intended production surface.  bindings/java holds the equivalent JNI shim.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../fmx.h"

namespace index4j {

struct IoError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

namespace detail {
inline void check(int rc, const char *where) {
    if (rc == FMX_OK) return;
    const std::string msg = fmx_last_error() ? fmx_last_error() : "";
    if (rc == FMX_E_ALPHABET) throw std::invalid_argument("Input has more than 32767 different symbols");  // FM:423-426
    if (rc == FMX_E_VERSION) throw IoError(msg);                                                           // SER:46-56
    if (rc == FMX_E_FORMAT) throw IoError(std::string(where) + ": " + msg);
    throw std::runtime_error(std::string(where) + " failed (" + std::to_string(rc) + "): " + msg);
}
// re-throw the reference's exception for a per-query status code
inline void raise_for_status(int status, int aux = 0) {
    if (status == FMX_ST_OK) return;
    char buf[256];
    std::snprintf(buf, sizeof buf, fmx_status_message(status), aux);
    switch (fmx_status_kind(status)) {
        case 1: throw std::invalid_argument(buf);
        case 2: throw std::out_of_range(buf);
        default: throw std::runtime_error(buf);
    }
}
}  // namespace detail

class FmIndex {
public:
    // new FmIndex(char[] input, int sampleRate, boolean enableExtract)  FM:155-174.
    // buildDevice >= 0: the constructor's suffix-array stage (FM:329-394) runs on that GPU — same index, byte for byte
    FmIndex(const std::u16string &input, int sampleRate, bool enableExtract = true, int device = 0,
            int buildDevice = -1) {
        const uint16_t *chars = reinterpret_cast<const uint16_t *>(input.data());
        if (buildDevice >= 0)
            detail::check(fmx_build_on_device(chars, (int32_t)input.size(), sampleRate, enableExtract ? 1 : 0, buildDevice,
                                              &h_, nullptr, nullptr, nullptr),
                          "fmx_build_on_device");
        else
            detail::check(fmx_build(chars, (int32_t)input.size(), sampleRate, enableExtract ? 1 : 0, &h_), "fmx_build");
        if (device >= 0) toDevice(device);
    }
    // FmIndex.read(ObjectInput) FM:983-1025 (raw DataOutput stream or ObjectOutputStream-framed, SER:89-100)
    static FmIndex read(const std::vector<uint8_t> &bytes, int device = 0) {
        fmx_index *h = nullptr;
        detail::check(fmx_load(bytes.data(), bytes.size(), &h), "fmx_load");
        FmIndex f(h);
        if (device >= 0) f.toDevice(device);
        return f;
    }
    FmIndex(FmIndex &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    FmIndex &operator=(FmIndex &&o) noexcept {
        if (this != &o) {
            fmx_free(h_);
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    FmIndex(const FmIndex &) = delete;
    FmIndex &operator=(const FmIndex &) = delete;
    ~FmIndex() { fmx_free(h_); }

    void toDevice(int device) { detail::check(fmx_to_device(h_, device), "fmx_to_device"); }
    fmx_index *handle() const { return h_; }
    // {bytes, replay rows} of the resident index's row table (fmx_locate_rows_info; {0, 0}: none).  An index made resident after
    // fmx_set_option("locate_rows", 1) keeps what locate() returns for every BWT row and gathers its hits instead of walking.
    std::pair<int64_t, int64_t> locateRowsInfo() const {
        int64_t bytes = 0, replay = 0;
        detail::check(fmx_locate_rows_info(h_, &bytes, &replay), "fmx_locate_rows_info");
        return {bytes, replay};
    }

    // FmIndex.write(ObjectOutput) FM:948-975; framed = through Serialization.writeToByteArray SER:67-79
    std::vector<uint8_t> write(bool framed = true) const {
        uint8_t *buf = nullptr;
        size_t len = 0;
        detail::check(fmx_save(h_, framed ? 1 : 0, &buf, &len), "fmx_save");
        std::vector<uint8_t> out(buf, buf + len);
        fmx_free_buffer(buf);
        return out;
    }

    int getInputLength() const { return fmx_input_length(h_); }        // FM:929
    int getAlphabetLength() const { return fmx_alphabet_length(h_); }  // FM:939
    std::string toString() const {                                     // FM:1044-1046
        return "FMIndex-sampleRate:" + std::to_string(fmx_sample_rate(h_)) +
               "-extract:" + (fmx_extract_enabled(h_) ? "true" : "false");
    }

    // ---- batched queries (one GPU launch per call) ----
    std::vector<int32_t> countBatch(const std::vector<std::u16string> &patterns) const {
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        pack(patterns, chars, off);
        std::vector<int32_t> counts(patterns.size()), status(patterns.size());
        detail::check(fmx_count_batch(h_, chars.data(), off.data(), (int32_t)patterns.size(), counts.data(), nullptr,
                                      status.data()),
                      "fmx_count_batch");
        for (int s : status) detail::raise_for_status(s);
        return counts;
    }
    // returns found[i]; locations is patterns.size() rows of maxMatches ints
    std::vector<int32_t> locateBatch(const std::vector<std::u16string> &patterns, int maxMatches,
                                     std::vector<int32_t> &locations) const {
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        pack(patterns, chars, off);
        const int32_t n = (int32_t)patterns.size();
        locations.assign((size_t)n * (size_t)maxMatches, 0);
        std::vector<int32_t> found(patterns.size()), status(patterns.size());
        detail::check(fmx_locate_batch(h_, chars.data(), off.data(), n, maxMatches, locations.data(), maxMatches,
                                       found.data(), nullptr, status.data()),
                      "fmx_locate_batch");
        for (int s : status) detail::raise_for_status(s);
        return found;
    }
    // every hit of every pattern, packed (fmx_locate_all_batch; FM:487-552): the hits of pattern i are
    // locations[offsets[i] .. offsets[i + 1]), in the order locate() stores them; maxMatches > 0 cuts each pattern's hits there
    struct Hits {
        std::vector<int64_t> offsets;
        std::vector<int32_t> locations;
    };
    Hits locateAllBatch(const std::vector<std::u16string> &patterns, int maxMatches = -1) const {
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        pack(patterns, chars, off);
        const int32_t n = (int32_t)patterns.size();
        Hits hits;
        hits.offsets.assign((size_t)n + 1, 0);
        std::vector<int32_t> status(patterns.size());
        int32_t *buf = nullptr;
        detail::check(fmx_locate_all_batch(h_, chars.data(), off.data(), n, maxMatches, hits.offsets.data(), &buf, nullptr,
                                           status.data()),
                      "fmx_locate_all_batch");
        try {
            if (buf) hits.locations.assign(buf, buf + hits.offsets[(size_t)n]);
        } catch (...) {
            fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
            throw;
        }
        fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
        for (int s : status) detail::raise_for_status(s);
        return hits;
    }
    std::vector<int32_t> locateAll(const std::u16string &pattern) const {  // FM:487-489, the array made here
        if (pattern.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        return locateAllBatch({pattern}, -1).locations;
    }
    // the lines that match (fmx.h "THE LINE TABLE"): buildLineTable once per residency, then matchLines / matchLinesBatch —
    // the distinct line ids of pattern i are lines[offsets[i] .. offsets[i + 1]), ascending; maxLines > 0 keeps the first of them,
    // lineCount says how many there are whatever the limit, occurrences is count()
    int64_t buildLineTable(char16_t boundary = u'\n') {
        int64_t lines = 0;
        detail::check(fmx_line_table_build(h_, (uint16_t)boundary, &lines), "fmx_line_table_build");
        return lines;
    }
    struct Lines {
        std::vector<int64_t> offsets;
        std::vector<int32_t> lines, lineCount, occurrences;
    };
    Lines matchLinesBatch(const std::vector<std::u16string> &patterns, int maxLines = 0) const {
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        pack(patterns, chars, off);
        const int32_t n = (int32_t)patterns.size();
        Lines out;
        out.offsets.assign((size_t)n + 1, 0);
        out.lineCount.assign(patterns.size(), 0);
        out.occurrences.assign(patterns.size(), 0);
        std::vector<int32_t> status(patterns.size());
        int32_t *buf = nullptr;
        detail::check(fmx_match_lines_batch(h_, chars.data(), off.data(), n, maxLines, out.offsets.data(), &buf, out.lineCount.data(),
                                            out.occurrences.data(), status.data()),
                      "fmx_match_lines_batch");
        try {
            if (buf) out.lines.assign(buf, buf + out.offsets[(size_t)n]);
        } catch (...) {
            fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
            throw;
        }
        fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
        for (int s : status) detail::raise_for_status(s);
        return out;
    }
    std::vector<int32_t> matchLines(const std::u16string &pattern, int maxLines = 0) const {
        if (pattern.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        return matchLinesBatch({pattern}, maxLines).lines;
    }
    // the lines that match a QUERY of several terms (fmx.h "THE LINES THAT MATCH A QUERY OF SEVERAL TERMS"): a line must hold every
    // term of `all`, at least one of `any` (if there are any) and none of `none`; a query without `all` and `any` has no lines.
    // matchQueryBatch: lines[offsets[Q] .. offsets[Q + 1]) are those of query Q, ascending; lineCount per query, occurrences per
    // term, in the order all, any, none of query 0, then query 1 ...
    struct Query {
        std::vector<std::u16string> all, any, none;
    };
    Lines matchQueryBatch(const std::vector<Query> &queries, int maxLines = 0) const {
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        for (const Query &qu : queries) {
            const std::vector<std::u16string> *groups[3] = {&qu.all, &qu.any, &qu.none};
            for (int k = 0; k < 3; ++k)
                for (const std::u16string &t : *groups[k]) {
                    terms.push_back(t);
                    kind.push_back((uint8_t)k);
                }
            queryOff.push_back((int32_t)terms.size());
        }
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        pack(terms, chars, off);
        const int32_t n = (int32_t)terms.size(), q = (int32_t)queries.size();
        Lines out;
        out.offsets.assign((size_t)q + 1, 0);
        out.lineCount.assign(queries.size(), 0);
        out.occurrences.assign(terms.size(), 0);
        std::vector<int32_t> status(terms.size());
        int32_t *buf = nullptr;
        detail::check(fmx_match_query_batch(h_, chars.data(), off.data(), n, queryOff.data(), kind.data(), q, maxLines, out.offsets.data(), &buf,
                                            out.lineCount.data(), out.occurrences.data(), status.data()),
                      "fmx_match_query_batch");
        try {
            if (buf) out.lines.assign(buf, buf + out.offsets[(size_t)q]);
        } catch (...) {
            fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
            throw;
        }
        fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
        for (int s : status) detail::raise_for_status(s);
        return out;
    }
    std::vector<int32_t> matchQuery(const Query &query, int maxLines = 0) const {
        for (const std::vector<std::u16string> *g : {&query.all, &query.any, &query.none})
            for (const std::u16string &t : *g)
                if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        return matchQueryBatch({query}, maxLines).lines;
    }
    // ... with terms on the NUMBER behind a pattern (fmx.h "THE LINES THAT MATCH A QUERY WITH TERMS ON NUMBERS": latency_ms >= 500).
    // A NumberTerm with lo >= 0 is ranged: it holds on a line iff one of its hits there is followed by a number (numberStatsWhere's
    // value, fracDigits as there) with lo <= value <= hi; kNumberMax is "no upper bound"; the default (lo = -1) is a plain string
    // term.  matchQueryNumberBatch: Lines as matchQueryBatch, and per term kept (the hits that pass), notNumber and overflow (the
    // hits that did not parse, by reason), in the order all, any, none of query 0, then query 1 ...
    static constexpr int64_t kNumberMax = INT64_MAX;
    struct NumberTerm {
        std::u16string pattern;
        int64_t lo = -1, hi = -1;
    };
    struct NumberQuery {
        std::vector<NumberTerm> all, any, none;
    };
    struct NumberLines : Lines {
        std::vector<int32_t> kept, notNumber, overflow;
    };
    NumberLines matchQueryNumberBatch(const std::vector<NumberQuery> &queries, int fracDigits = 0, int maxLines = 0) const {
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int64_t> lo, hi;
        std::vector<int32_t> queryOff{0};
        for (const NumberQuery &qu : queries) {
            const std::vector<NumberTerm> *groups[3] = {&qu.all, &qu.any, &qu.none};
            for (int k = 0; k < 3; ++k)
                for (const NumberTerm &t : *groups[k]) {
                    terms.push_back(t.pattern);
                    kind.push_back((uint8_t)k);
                    lo.push_back(t.lo);
                    hi.push_back(t.hi);
                }
            queryOff.push_back((int32_t)terms.size());
        }
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        pack(terms, chars, off);
        const int32_t n = (int32_t)terms.size(), q = (int32_t)queries.size();
        lo.push_back(0);  // (never an empty array)
        hi.push_back(0);
        NumberLines out;
        out.offsets.assign((size_t)q + 1, 0);
        out.lineCount.assign(queries.size(), 0);
        for (std::vector<int32_t> *a : {&out.occurrences, &out.kept, &out.notNumber, &out.overflow}) a->assign(terms.size(), 0);
        std::vector<int32_t> status(terms.size());
        int32_t *buf = nullptr;
        detail::check(fmx_match_query_number_batch(h_, chars.data(), off.data(), n, lo.data(), hi.data(), fracDigits, queryOff.data(), kind.data(), q,
                                                   maxLines, out.offsets.data(), &buf, out.lineCount.data(), out.occurrences.data(),
                                                   out.kept.data(), out.notNumber.data(), out.overflow.data(), status.data()),
                      "fmx_match_query_number_batch");
        try {
            if (buf) out.lines.assign(buf, buf + out.offsets[(size_t)q]);
        } catch (...) {
            fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
            throw;
        }
        fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
        for (int s : status) detail::raise_for_status(s);
        return out;
    }
    std::vector<int32_t> matchQueryNumber(const NumberQuery &query, int fracDigits = 0, int maxLines = 0) const {
        for (const std::vector<NumberTerm> *g : {&query.all, &query.any, &query.none})
            for (const NumberTerm &t : *g)
                if (t.pattern.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        return matchQueryNumberBatch({query}, fracDigits, maxLines).lines;
    }

    // the lines that hold a SEQUENCE of terms in order, without overlap (fmx.h "THE LINES THAT HOLD A SEQUENCE OF TERMS IN ORDER":
    // grep 'A.*B').  matchSequenceBatch: lines[offsets[Q] .. offsets[Q + 1]) are those of sequence Q, ascending; lineCount per
    // sequence, occurrences per term; wantSpans: spans[2 * i], spans[2 * i + 1] = [start, stop) of the non-greedy match on lines[i]
    // (the leftmost start and from there the earliest end).  A sequence without terms has no lines.
    struct SequenceLines : Lines {
        std::vector<int32_t> spans;
    };
    SequenceLines matchSequenceBatch(const std::vector<std::vector<std::u16string>> &sequences, int maxLines = 0, bool wantSpans = false) const {
        std::vector<std::u16string> terms;
        std::vector<int32_t> queryOff{0};
        for (const std::vector<std::u16string> &sq : sequences) {
            terms.insert(terms.end(), sq.begin(), sq.end());
            queryOff.push_back((int32_t)terms.size());
        }
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        pack(terms, chars, off);
        const int32_t n = (int32_t)terms.size(), q = (int32_t)sequences.size();
        SequenceLines out;
        out.offsets.assign((size_t)q + 1, 0);
        out.lineCount.assign(sequences.size(), 0);
        out.occurrences.assign(terms.size(), 0);
        std::vector<int32_t> status(terms.size());
        int32_t *buf = nullptr, *spans = nullptr;
        detail::check(fmx_match_sequence_batch(h_, chars.data(), off.data(), n, queryOff.data(), q, maxLines, out.offsets.data(), &buf,
                                               wantSpans ? &spans : nullptr, out.lineCount.data(), out.occurrences.data(), status.data()),
                      "fmx_match_sequence_batch");
        try {  // (the spans lie in the lines' buffer, behind them)
            if (buf) out.lines.assign(buf, buf + out.offsets[(size_t)q]);
            if (spans) out.spans.assign(spans, spans + 2 * out.offsets[(size_t)q]);
        } catch (...) {
            fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
            throw;
        }
        fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
        for (int s : status) detail::raise_for_status(s);
        return out;
    }
    std::vector<int32_t> matchSequence(const std::vector<std::u16string> &terms, int maxLines = 0) const {
        for (const std::u16string &t : terms)
            if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        return matchSequenceBatch({terms}, maxLines).lines;
    }

    // patterns of character classes (fmx.h "PATTERNS OF CHARACTER CLASSES"): a ClassPattern is its positions, a position the code
    // units it may hold; the answer is the union over the literal strings the pattern spells.  A pattern that keeps more than
    // maxRanges SA ranges throws std::runtime_error (FMX_ST_TOO_MANY_RANGES).  ignoreCase: per ASCII letter both cases.
    using ClassPattern = std::vector<std::u16string>;
    static ClassPattern ignoreCase(const std::u16string &text) {
        ClassPattern p;
        for (char16_t c : text) {
            std::u16string alts(1, c);
            if (c >= u'a' && c <= u'z') alts.push_back((char16_t)(c - 32));
            if (c >= u'A' && c <= u'Z') alts.push_back((char16_t)(c + 32));
            p.push_back(alts);
        }
        return p;
    }
    std::vector<int32_t> countClass(const std::vector<ClassPattern> &patterns, int maxRanges = 256) const {
        ClassArrays a(patterns);
        std::vector<int32_t> counts(patterns.size()), status(patterns.size());
        detail::check(fmx_count_class_batch(h_, a.alt.data(), a.posOff.data(), a.nPos(), a.patOff.data(), a.n(), maxRanges, counts.data(),
                                            status.data()),
                      "fmx_count_class_batch");
        for (int s : status) detail::raise_for_status(s);
        return counts;
    }
    // locations[offsets[i] .. offsets[i + 1]): the hits of pattern i, one literal string's locate() list after the other
    Hits locateAllClass(const std::vector<ClassPattern> &patterns, int maxRanges = 256) const {
        ClassArrays a(patterns);
        Hits hits;
        hits.offsets.assign(patterns.size() + 1, 0);
        std::vector<int32_t> status(patterns.size());
        int32_t *buf = nullptr;
        detail::check(fmx_locate_all_class_batch(h_, a.alt.data(), a.posOff.data(), a.nPos(), a.patOff.data(), a.n(), maxRanges,
                                                 hits.offsets.data(), &buf, status.data()),
                      "fmx_locate_all_class_batch");
        try {
            if (buf) hits.locations.assign(buf, buf + hits.offsets[patterns.size()]);
        } catch (...) {
            fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
            throw;
        }
        fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
        for (int s : status) detail::raise_for_status(s);
        return hits;
    }
    // matchQueryBatch with class patterns as terms (needs buildLineTable)
    struct ClassQuery {
        std::vector<ClassPattern> all, any, none;
    };
    Lines matchQueryClass(const std::vector<ClassQuery> &queries, int maxLines = 0, int maxRanges = 256) const {
        std::vector<ClassPattern> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        for (const ClassQuery &qu : queries) {
            const std::vector<ClassPattern> *groups[3] = {&qu.all, &qu.any, &qu.none};
            for (int k = 0; k < 3; ++k)
                for (const ClassPattern &t : *groups[k]) {
                    terms.push_back(t);
                    kind.push_back((uint8_t)k);
                }
            queryOff.push_back((int32_t)terms.size());
        }
        ClassArrays a(terms);
        const int32_t q = (int32_t)queries.size();
        Lines out;
        out.offsets.assign((size_t)q + 1, 0);
        out.lineCount.assign(queries.size(), 0);
        out.occurrences.assign(terms.size(), 0);
        std::vector<int32_t> status(terms.size());
        int32_t *buf = nullptr;
        detail::check(fmx_match_query_class_batch(h_, a.alt.data(), a.posOff.data(), a.nPos(), a.patOff.data(), a.n(), maxRanges, queryOff.data(),
                                                  kind.data(), q, maxLines, out.offsets.data(), &buf, out.lineCount.data(),
                                                  out.occurrences.data(), status.data()),
                      "fmx_match_query_class_batch");
        try {
            if (buf) out.lines.assign(buf, buf + out.offsets[(size_t)q]);
        } catch (...) {
            fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
            throw;
        }
        fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
        for (int s : status) detail::raise_for_status(s);
        return out;
    }

    // the distinct VALUES that follow a pattern, with the number of hits that have each (fmx.h "THE VALUES THAT FOLLOW A PATTERN, WITH
    // COUNTS": grep -o 'blk_[^ ]*' | sort | uniq -c).  The value of a hit is the text behind the pattern up to, not including, the
    // first code unit of `stop` (at most 64 units), at most maxLen (1 .. 64) units.  fieldValuesBatch: the values of pattern i are
    // the groups offsets[i] .. offsets[i + 1] - 1, ascending by code unit, a value in front of its extensions; group g is
    // chars[textOffsets[g] .. textOffsets[g + 1]) and counts[g] hits have it; status[i] is the pattern's own (not thrown: one empty
    // pattern does not hide the others).  fieldValues: one pattern as (value, count) pairs; top > 0: the `top` entries with the
    // largest counts, ties by value (sorted on the host over the groups); ignoreCase: the pattern in any case, one answer.
    struct FieldValues {
        std::vector<int64_t> offsets, textOffsets;
        std::vector<int32_t> counts, occurrences, status;
        std::u16string chars;
        std::u16string operator[](size_t g) const { return chars.substr((size_t)textOffsets[g], (size_t)(textOffsets[g + 1] - textOffsets[g])); }
    };
    FieldValues fieldValuesBatch(const std::vector<std::u16string> &patterns, const std::u16string &stop, int maxLen) const {
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        pack(patterns, chars, off);
        const int32_t n = (int32_t)patterns.size();
        FieldValues out = emptyFieldValues(patterns.size());
        int32_t *counts = nullptr;
        int64_t *textOff = nullptr;
        uint16_t *units = nullptr;
        detail::check(fmx_field_values_batch(h_, chars.data(), off.data(), n, reinterpret_cast<const uint16_t *>(stop.data()), (int32_t)stop.size(),
                                             maxLen, out.offsets.data(), &counts, &textOff, &units, out.occurrences.data(), out.status.data()),
                      "fmx_field_values_batch");
        return takeFieldValues(out, counts, textOff, units);
    }
    FieldValues fieldValuesClass(const std::vector<ClassPattern> &patterns, const std::u16string &stop, int maxLen, int maxRanges = 256) const {
        ClassArrays a(patterns);
        FieldValues out = emptyFieldValues(patterns.size());
        int32_t *counts = nullptr;
        int64_t *textOff = nullptr;
        uint16_t *units = nullptr;
        detail::check(fmx_field_values_class_batch(h_, a.alt.data(), a.posOff.data(), a.nPos(), a.patOff.data(), a.n(), maxRanges,
                                                   reinterpret_cast<const uint16_t *>(stop.data()), (int32_t)stop.size(), maxLen, out.offsets.data(),
                                                   &counts, &textOff, &units, out.occurrences.data(), out.status.data()),
                      "fmx_field_values_class_batch");
        return takeFieldValues(out, counts, textOff, units);
    }
    std::vector<std::pair<std::u16string, int32_t>> fieldValues(const std::u16string &pattern, const std::u16string &stop = u" \t\r\n",
                                                                 int maxLen = 32, int top = 0, bool ignoreCaseOfPattern = false) const {
        if (pattern.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const FieldValues v = ignoreCaseOfPattern ? fieldValuesClass({ignoreCase(pattern)}, stop, maxLen) : fieldValuesBatch({pattern}, stop, maxLen);
        detail::raise_for_status(v.status[0]);
        std::vector<std::pair<std::u16string, int32_t>> out;
        for (size_t g = 0; g < v.counts.size(); ++g) out.emplace_back(v[g], v.counts[g]);
        if (top > 0) {  // (a stable sort: equal counts keep the order of the values)
            std::stable_sort(out.begin(), out.end(), [](const auto &a, const auto &b) { return a.second > b.second; });
            if (out.size() > (size_t)top) out.resize((size_t)top);
        }
        return out;
    }
    // ... only within the lines of a query (fmx.h "THE VALUES THAT FOLLOW A PATTERN, WHERE THE LINE MATCHES A QUERY": grep terminating |
    // grep -o 'blk_[^ ]*' | sort | uniq -c; needs buildLineTable unless nothing filters).  A hit of pattern i counts iff its line —
    // the line of its first character — lies in [lineLo, lineHi) and, for whereOf[i] >= 0, matches queries[whereOf[i]] (matchQuery's
    // rule; whereOf[i] = -1: the window alone).  occurrences[i] stays the pattern's count in the whole text, kept[i] is the hits
    // that passed: the counts of the pattern's values add up to it.  termStatus: per term, in the order all, any, none of query 0,
    // then query 1 ... (not thrown).  fieldValuesWhere: one pattern and one query as (value, count) pairs, statuses thrown.
    struct FieldValuesWhere : FieldValues {
        std::vector<int32_t> kept, termStatus;
    };
    FieldValuesWhere fieldValuesWhereBatch(const std::vector<std::u16string> &patterns, const std::vector<Query> &queries,
                                           const std::vector<int32_t> &whereOf, const std::u16string &stop, int maxLen, int32_t lineLo = 0,
                                           int32_t lineHi = INT32_MAX) const {
        if (whereOf.size() != patterns.size()) throw std::invalid_argument("whereOf has one entry per pattern");
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        for (const Query &qu : queries) {
            const std::vector<std::u16string> *groups[3] = {&qu.all, &qu.any, &qu.none};
            for (int k = 0; k < 3; ++k)
                for (const std::u16string &t : *groups[k]) {
                    terms.push_back(t);
                    kind.push_back((uint8_t)k);
                }
            queryOff.push_back((int32_t)terms.size());
        }
        std::vector<uint16_t> chars, termChars;
        std::vector<int32_t> off, termOff;
        pack(patterns, chars, off);
        pack(terms, termChars, termOff);
        FieldValuesWhere out;
        static_cast<FieldValues &>(out) = emptyFieldValues(patterns.size());
        out.kept.assign(patterns.size(), 0);
        out.termStatus.assign(terms.size(), 0);
        kind.push_back(0);  // (never an empty array)
        int32_t *counts = nullptr;
        int64_t *textOff = nullptr;
        uint16_t *units = nullptr;
        detail::check(fmx_field_values_where_batch(h_, chars.data(), off.data(), (int32_t)patterns.size(), termChars.data(), termOff.data(),
                                                   (int32_t)terms.size(), queryOff.data(), kind.data(), (int32_t)queries.size(), whereOf.data(), lineLo,
                                                   lineHi, reinterpret_cast<const uint16_t *>(stop.data()), (int32_t)stop.size(), maxLen,
                                                   out.offsets.data(), &counts, &textOff, &units, out.occurrences.data(), out.kept.data(),
                                                   out.status.data(), out.termStatus.data()),
                      "fmx_field_values_where_batch");
        takeFieldValues(out, counts, textOff, units);
        return out;
    }
    std::vector<std::pair<std::u16string, int32_t>> fieldValuesWhere(const std::u16string &pattern, const Query &where,
                                                                      const std::u16string &stop = u" \t\r\n", int maxLen = 32, int top = 0,
                                                                      int32_t lineLo = 0, int32_t lineHi = INT32_MAX) const {
        if (pattern.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        for (const std::vector<std::u16string> *g : {&where.all, &where.any, &where.none})
            for (const std::u16string &t : *g)
                if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const FieldValuesWhere v = fieldValuesWhereBatch({pattern}, {where}, {0}, stop, maxLen, lineLo, lineHi);
        detail::raise_for_status(v.status[0]);
        for (int s : v.termStatus) detail::raise_for_status(s);
        std::vector<std::pair<std::u16string, int32_t>> out;
        for (size_t g = 0; g < v.counts.size(); ++g) out.emplace_back(v[g], v.counts[g]);
        if (top > 0) {  // (a stable sort: equal counts keep the order of the values)
            std::stable_sort(out.begin(), out.end(), [](const auto &a, const auto &b) { return a.second > b.second; });
            if (out.size() > (size_t)top) out.resize((size_t)top);
        }
        return out;
    }

    // matching lines and hits per bucket of lines, the timeline (fmx.h "LINES AND HITS PER BUCKET OF LINES"; needs buildLineTable).
    // edges: B + 1 line ids that never decrease, bucket b = the lines edges[b] <= L < edges[b + 1]; a line outside edges[0] ..
    // edges[B] is counted nowhere.  lineHistogramBatch: counts[Q * B + b] = the lines of matchQuery(queries[Q]) in bucket b — only
    // the counters come down; lineCount per query, occurrences per term.  hitHistogramWhereBatch: counts[i * B + b] = the hits of
    // patterns[i] that fieldValuesWhereBatch keeps for whereOf[i] (no window) whose line — the line of the hit's first character —
    // lies in bucket b; a hit counts as often as it occurs.  Statuses are not thrown by the batch forms; lineHistogram and
    // hitHistogramWhere answer one row and throw them.
    struct LineHistogram {
        int32_t buckets = 0;
        std::vector<int32_t> counts, lineCount, occurrences, status;
        std::vector<int32_t> row(size_t i) const { return {counts.begin() + i * (size_t)buckets, counts.begin() + (i + 1) * (size_t)buckets}; }
    };
    LineHistogram lineHistogramBatch(const std::vector<Query> &queries, const std::vector<int32_t> &edges) const {
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        flattenQueries(queries, terms, kind, queryOff);
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        pack(terms, chars, off);
        LineHistogram out;
        out.buckets = edges.size() > 1 ? (int32_t)edges.size() - 1 : 0;
        out.counts.assign(queries.size() * (size_t)out.buckets + 1, 0);
        out.lineCount.assign(queries.size(), 0);
        out.occurrences.assign(terms.size(), 0);
        out.status.assign(terms.size(), 0);
        detail::check(fmx_line_histogram_batch(h_, chars.data(), off.data(), (int32_t)terms.size(), queryOff.data(), kind.data(),
                                               (int32_t)queries.size(), edges.data(), (int32_t)edges.size(), out.counts.data(),
                                               out.lineCount.data(), out.occurrences.data(), out.status.data()),
                      "fmx_line_histogram_batch");
        out.counts.pop_back();
        return out;
    }
    std::vector<int32_t> lineHistogram(const Query &query, const std::vector<int32_t> &edges) const {
        for (const std::vector<std::u16string> *g : {&query.all, &query.any, &query.none})
            for (const std::u16string &t : *g)
                if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const LineHistogram h = lineHistogramBatch({query}, edges);
        for (int s : h.status) detail::raise_for_status(s);
        return h.counts;
    }
    struct HitHistogram {
        int32_t buckets = 0;
        std::vector<int32_t> counts, occurrences, kept, status, termStatus;
        std::vector<int32_t> row(size_t i) const { return {counts.begin() + i * (size_t)buckets, counts.begin() + (i + 1) * (size_t)buckets}; }
    };
    HitHistogram hitHistogramWhereBatch(const std::vector<std::u16string> &patterns, const std::vector<Query> &queries,
                                        const std::vector<int32_t> &whereOf, const std::vector<int32_t> &edges) const {
        if (whereOf.size() != patterns.size()) throw std::invalid_argument("whereOf has one entry per pattern");
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        flattenQueries(queries, terms, kind, queryOff);
        std::vector<uint16_t> chars, termChars;
        std::vector<int32_t> off, termOff;
        pack(patterns, chars, off);
        pack(terms, termChars, termOff);
        HitHistogram out;
        out.buckets = edges.size() > 1 ? (int32_t)edges.size() - 1 : 0;
        out.counts.assign(patterns.size() * (size_t)out.buckets + 1, 0);
        out.occurrences.assign(patterns.size(), 0);
        out.kept.assign(patterns.size(), 0);
        out.status.assign(patterns.size(), 0);
        out.termStatus.assign(terms.size(), 0);
        detail::check(fmx_hit_histogram_where_batch(h_, chars.data(), off.data(), (int32_t)patterns.size(), termChars.data(), termOff.data(),
                                                    (int32_t)terms.size(), queryOff.data(), kind.data(), (int32_t)queries.size(), whereOf.data(),
                                                    edges.data(), (int32_t)edges.size(), out.counts.data(), out.occurrences.data(),
                                                    out.kept.data(), out.status.data(), out.termStatus.data()),
                      "fmx_hit_histogram_where_batch");
        out.counts.pop_back();
        return out;
    }
    std::vector<int32_t> hitHistogramWhere(const std::u16string &pattern, const Query &where, const std::vector<int32_t> &edges) const {
        if (pattern.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        for (const std::vector<std::u16string> *g : {&where.all, &where.any, &where.none})
            for (const std::u16string &t : *g)
                if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const HitHistogram h = hitHistogramWhereBatch({pattern}, {where}, {0}, edges);
        detail::raise_for_status(h.status[0]);
        for (int s : h.termStatus) detail::raise_for_status(s);
        return h.counts;
    }

    // statistics of the number behind a pattern, per bucket of lines (fmx.h "THE NUMBER BEHIND A PATTERN"): hitHistogramWhereBatch's
    // patterns, queries, whereOf and edges (no edges at all: one bucket, every line — then a line table is needed only where a
    // pattern asks for a query).  The number is the run of digits behind the pattern; with fracDigits in [0, 9] a '.' and up to
    // that many digits more, scaled by 10^fracDigits ("251.73" at 3 is 251730).  Per row = i * B + b over the kept hits that parse:
    // count, the exact sum = sumHi * 2^64 + sumLo, min, max, and pct[row * P + j] = the nearest-rank percentile permille[j] (up to
    // 16, in thousandths); notNumber / overflow per pattern: the kept hits in some bucket that did not parse.  Statuses are not
    // thrown by the batch form; numberStatsWhere answers one pattern and throws them.
    struct NumberStats {
        int32_t buckets = 0, permilles = 0;
        std::vector<int32_t> count;
        std::vector<uint64_t> sumLo, sumHi;
        std::vector<int64_t> min, max, pct;
        std::vector<int32_t> notNumber, overflow, occurrences, kept, status, termStatus;
        double mean(size_t row) const {  // (a convenience of the host: the sum as a double)
            return count[row] ? ((double)sumHi[row] * 18446744073709551616.0 + (double)sumLo[row]) / count[row] : 0.0;
        }
    };
    NumberStats numberStatsWhereBatch(const std::vector<std::u16string> &patterns, const std::vector<Query> &queries,
                                      const std::vector<int32_t> &whereOf, const std::vector<int32_t> &edges,
                                      const std::vector<int32_t> &permille = {500, 950}, int32_t fracDigits = 0) const {
        if (whereOf.size() != patterns.size()) throw std::invalid_argument("whereOf has one entry per pattern");
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        flattenQueries(queries, terms, kind, queryOff);
        std::vector<uint16_t> chars, termChars;
        std::vector<int32_t> off, termOff;
        pack(patterns, chars, off);
        pack(terms, termChars, termOff);
        NumberStats out;
        out.buckets = edges.empty() ? 1 : edges.size() > 1 ? (int32_t)edges.size() - 1 : 0;
        out.permilles = (int32_t)permille.size();
        const size_t n = patterns.size(), cells = n * (size_t)out.buckets;
        out.count.assign(cells + 1, 0);
        out.sumLo.assign(cells + 1, 0);
        out.sumHi.assign(cells + 1, 0);
        out.min.assign(cells + 1, 0);
        out.max.assign(cells + 1, 0);
        out.pct.assign(cells * permille.size() + 1, 0);
        for (std::vector<int32_t> *v : {&out.notNumber, &out.overflow, &out.occurrences, &out.kept, &out.status}) v->assign(n + 1, 0);
        out.termStatus.assign(terms.size(), 0);
        detail::check(fmx_number_stats_where_batch(h_, chars.data(), off.data(), (int32_t)n, termChars.data(), termOff.data(), (int32_t)terms.size(),
                                                   queryOff.data(), kind.data(), (int32_t)queries.size(), whereOf.data(),
                                                   edges.empty() ? nullptr : edges.data(), (int32_t)edges.size(), fracDigits, permille.data(),
                                                   (int32_t)permille.size(), out.count.data(), out.sumLo.data(), out.sumHi.data(), out.min.data(),
                                                   out.max.data(), out.pct.data(), out.notNumber.data(), out.overflow.data(),
                                                   out.occurrences.data(), out.kept.data(), out.status.data(), out.termStatus.data()),
                      "fmx_number_stats_where_batch");
        for (std::vector<int32_t> *v : {&out.count, &out.notNumber, &out.overflow, &out.occurrences, &out.kept, &out.status}) v->pop_back();
        for (std::vector<uint64_t> *v : {&out.sumLo, &out.sumHi}) v->pop_back();
        for (std::vector<int64_t> *v : {&out.min, &out.max, &out.pct}) v->pop_back();
        return out;
    }
    NumberStats numberStatsWhere(const std::u16string &pattern, const Query &where, const std::vector<int32_t> &edges,
                                 const std::vector<int32_t> &permille = {500, 950}, int32_t fracDigits = 0) const {
        if (pattern.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        for (const std::vector<std::u16string> *g : {&where.all, &where.any, &where.none})
            for (const std::u16string &t : *g)
                if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const NumberStats s = numberStatsWhereBatch({pattern}, {where}, {0}, edges, permille, fracDigits);
        detail::raise_for_status(s.status[0]);
        for (int st : s.termStatus) detail::raise_for_status(st);
        return s;
    }

    // the lines ranked by the number behind a pattern (fmx.h "THE LINES RANKED BY THE NUMBER BEHIND A PATTERN"; ... | sort -k latency
    // -nr | head -10): numberStatsWhereBatch's patterns, queries, whereOf and fracDigits, and a window of lines.  descending[i] != 0:
    // largest first.  A line counts with its best parsing hit (equal values: the smallest position); the candidates are ranked by
    // value, equal values by line id; the ranks first .. first + top - 1 of pattern i are the rows i * top + j, j < rows[i]: line,
    // value, loc (zero behind rows[i]).  lines = the lines that have a candidate, numbers = the kept hits that parse.  Needs
    // buildLineTable().  Statuses are not thrown by the batch form; topLinesByNumber answers one pattern and throws them.
    struct TopLines {
        int32_t top = 0;
        std::vector<int32_t> rows, line, loc;
        std::vector<int64_t> value;
        std::vector<int32_t> lines, numbers, notNumber, overflow, occurrences, kept, status, termStatus;
    };
    TopLines topLinesByNumberBatch(const std::vector<std::u16string> &patterns, const std::vector<Query> &queries,
                                   const std::vector<int32_t> &whereOf, const std::vector<uint8_t> &descending, int32_t top = 10,
                                   int32_t first = 0, int32_t fracDigits = 0, int32_t lineLo = 0, int32_t lineHi = INT32_MAX) const {
        if (whereOf.size() != patterns.size() || descending.size() != patterns.size())
            throw std::invalid_argument("whereOf and descending have one entry per pattern");
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        flattenQueries(queries, terms, kind, queryOff);
        std::vector<uint16_t> chars, termChars;
        std::vector<int32_t> off, termOff;
        pack(patterns, chars, off);
        pack(terms, termChars, termOff);
        TopLines out;
        out.top = top;
        const size_t n = patterns.size(), cells = n * (size_t)(top > 0 ? top : 0);
        out.line.assign(cells + 1, 0);
        out.loc.assign(cells + 1, 0);
        out.value.assign(cells + 1, 0);
        for (std::vector<int32_t> *v : {&out.rows, &out.lines, &out.numbers, &out.notNumber, &out.overflow, &out.occurrences, &out.kept, &out.status})
            v->assign(n + 1, 0);
        out.termStatus.assign(terms.size(), 0);
        detail::check(fmx_top_lines_where_batch(h_, chars.data(), off.data(), (int32_t)n, termChars.data(), termOff.data(), (int32_t)terms.size(),
                                                queryOff.data(), kind.data(), (int32_t)queries.size(), whereOf.data(), lineLo, lineHi,
                                                descending.data(), fracDigits, first, top, out.rows.data(), out.line.data(), out.value.data(),
                                                out.loc.data(), out.lines.data(), out.numbers.data(), out.notNumber.data(), out.overflow.data(),
                                                out.occurrences.data(), out.kept.data(), out.status.data(), out.termStatus.data()),
                      "fmx_top_lines_where_batch");
        for (std::vector<int32_t> *v : {&out.rows, &out.line, &out.loc, &out.lines, &out.numbers, &out.notNumber, &out.overflow, &out.occurrences,
                                        &out.kept, &out.status})
            v->pop_back();
        out.value.pop_back();
        return out;
    }
    // one pattern; the rows behind rows[0] are cut off
    TopLines topLinesByNumber(const std::u16string &pattern, int32_t top = 10, bool largest = true, int32_t first = 0, const Query *where = nullptr,
                              int32_t fracDigits = 0, int32_t lineLo = 0, int32_t lineHi = INT32_MAX) const {
        if (pattern.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        if (where)
            for (const std::vector<std::u16string> *g : {&where->all, &where->any, &where->none})
                for (const std::u16string &t : *g)
                    if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        TopLines s = topLinesByNumberBatch({pattern}, where ? std::vector<Query>{*where} : std::vector<Query>{}, {where ? 0 : -1},
                                           {(uint8_t)(largest ? 1 : 0)}, top, first, fracDigits, lineLo, lineHi);
        detail::raise_for_status(s.status[0]);
        for (int st : s.termStatus) detail::raise_for_status(st);
        s.line.resize((size_t)s.rows[0]);
        s.loc.resize((size_t)s.rows[0]);
        s.value.resize((size_t)s.rows[0]);
        return s;
    }

    // statistics of the number behind a pattern, GROUPED BY THE VALUE OF A FIELD of the same line (fmx.h "STATISTICS BY KEY"; stats
    // count, sum(bytes=), p95(latency_ms=) by status=): byOf[i] names the key pattern number pattern i is grouped by; the key of a
    // line is fieldValues' value (stop, maxLen) of the key pattern's first kept hit on it.  The groups of key pattern k are
    // valOff[k] .. valOff[k + 1]: values[g], lines[g] = the lines that have that key; the rows are packed, row (i, g) at rowOff[i] + g:
    // count, the exact sum = sumHi * 2^64 + sumLo, min, max, pct[row * P + j]; noKey / notNumber / overflow per number pattern.  The
    // same query filters the key patterns' and the number patterns' hits (keyWhereOf, whereOf: -1 = none); needs buildLineTable().
    // Statuses are not thrown by the batch form; numberStatsBy answers one number pattern by one key pattern and throws them.
    struct NumberStatsBy {
        int32_t permilles = 0;
        std::vector<int64_t> valOff, rowOff;
        std::vector<std::u16string> values;
        std::vector<int32_t> lines, count;
        std::vector<uint64_t> sumLo, sumHi;
        std::vector<int64_t> min, max, pct;
        std::vector<int32_t> noKey, notNumber, overflow, occurrences, kept, status, keyOccurrences, keyKept, keyStatus, termStatus;
        double mean(size_t row) const {  // (a convenience of the host: the sum as a double)
            return count[row] ? ((double)sumHi[row] * 18446744073709551616.0 + (double)sumLo[row]) / count[row] : 0.0;
        }
    };
    NumberStatsBy numberStatsByBatch(const std::vector<std::u16string> &patterns, const std::vector<std::u16string> &keys,
                                     const std::vector<int32_t> &byOf, const std::u16string &stop, int32_t maxLen,
                                     const std::vector<Query> &queries, const std::vector<int32_t> &keyWhereOf, const std::vector<int32_t> &whereOf,
                                     const std::vector<int32_t> &permille = {500, 950}, int32_t fracDigits = 0, int32_t lineLo = 0,
                                     int32_t lineHi = INT32_MAX) const {
        if (whereOf.size() != patterns.size() || byOf.size() != patterns.size()) throw std::invalid_argument("whereOf and byOf have one entry per pattern");
        if (keyWhereOf.size() != keys.size()) throw std::invalid_argument("keyWhereOf has one entry per key pattern");
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        flattenQueries(queries, terms, kind, queryOff);
        std::vector<uint16_t> chars, keyChars, termChars;
        std::vector<int32_t> off, keyOff, termOff;
        pack(patterns, chars, off);
        pack(keys, keyChars, keyOff);
        pack(terms, termChars, termOff);
        NumberStatsBy out;
        const size_t n = patterns.size(), m = keys.size(), P = permille.size();
        out.permilles = (int32_t)P;
        out.valOff.assign(m + 1, 0);
        out.rowOff.assign(n + 1, 0);
        for (std::vector<int32_t> *v : {&out.noKey, &out.notNumber, &out.overflow, &out.occurrences, &out.kept, &out.status}) v->assign(n + 1, 0);
        for (std::vector<int32_t> *v : {&out.keyOccurrences, &out.keyKept, &out.keyStatus}) v->assign(m + 1, 0);
        out.termStatus.assign(terms.size(), 0);
        int32_t *lines = nullptr, *count = nullptr;
        int64_t *textOff = nullptr, *vmin = nullptr, *vmax = nullptr, *pct = nullptr;
        uint64_t *sumLo = nullptr, *sumHi = nullptr;
        uint16_t *text = nullptr;
        detail::check(fmx_number_stats_by_batch(h_, keyChars.data(), keyOff.data(), (int32_t)m, chars.data(), off.data(), (int32_t)n, byOf.data(),
                                                termChars.data(), termOff.data(), (int32_t)terms.size(), queryOff.data(), kind.data(),
                                                (int32_t)queries.size(), keyWhereOf.data(), whereOf.data(), lineLo, lineHi,
                                                reinterpret_cast<const uint16_t *>(stop.data()), (int32_t)stop.size(), maxLen, fracDigits,
                                                permille.data(), (int32_t)P, out.valOff.data(), &lines, &textOff, &text, out.rowOff.data(), &count,
                                                &sumLo, &sumHi, &vmin, &vmax, &pct, out.noKey.data(), out.notNumber.data(), out.overflow.data(),
                                                out.occurrences.data(), out.kept.data(), out.status.data(), out.keyOccurrences.data(),
                                                out.keyKept.data(), out.keyStatus.data(), out.termStatus.data()),
                      "fmx_number_stats_by_batch");
        const size_t G = (size_t)out.valOff[m], R = (size_t)out.rowOff[n];
        if (lines) {  // the ONE allocation: copied, then handed back
            out.lines.assign(lines, lines + G);
            for (size_t g = 0; g < G; ++g)
                out.values.emplace_back(reinterpret_cast<const char16_t *>(text) + textOff[g], (size_t)(textOff[g + 1] - textOff[g]));
            out.count.assign(count, count + R);
            out.sumLo.assign(sumLo, sumLo + R);
            out.sumHi.assign(sumHi, sumHi + R);
            out.min.assign(vmin, vmin + R);
            out.max.assign(vmax, vmax + R);
            out.pct.assign(pct, pct + R * P);
            fmx_free_buffer(reinterpret_cast<uint8_t *>(lines));
        }
        for (std::vector<int32_t> *v : {&out.noKey, &out.notNumber, &out.overflow, &out.occurrences, &out.kept, &out.status, &out.keyOccurrences,
                                        &out.keyKept, &out.keyStatus})
            v->pop_back();
        return out;
    }
    NumberStatsBy numberStatsBy(const std::u16string &pattern, const std::u16string &by, const std::u16string &stop = u" \t\r\n", int32_t maxLen = 32,
                                const Query *where = nullptr, const std::vector<int32_t> &permille = {500, 950}, int32_t fracDigits = 0) const {
        if (pattern.empty() || by.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        if (where)
            for (const std::vector<std::u16string> *g : {&where->all, &where->any, &where->none})
                for (const std::u16string &t : *g)
                    if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const int32_t w = where ? 0 : -1;
        const NumberStatsBy s = numberStatsByBatch({pattern}, {by}, {0}, stop, maxLen, where ? std::vector<Query>{*where} : std::vector<Query>{}, {w}, {w},
                                                   permille, fracDigits);
        detail::raise_for_status(s.status[0]);
        detail::raise_for_status(s.keyStatus[0]);
        for (int st : s.termStatus) detail::raise_for_status(st);
        return s;
    }

    // ... GROUPED BY THE VALUES OF TWO FIELDS of the same line (fmx.h "STATISTICS BY TWO KEYS"; stats p95(latency_ms=) by host=,
    // status=): pair j is (pairA[j], pairB[j]), two of the key patterns, and byOf[i] names the PAIR number pattern i is grouped by.  The
    // groups (valOff, values, lines) are the single keys', as numberStatsByBatch returns them; the pairs of j are pairOff[j] ..
    // pairOff[j + 1]: pairGroupA[r] and pairGroupB[r] index the groups of the two key patterns (values[valOff[pairA[j]] +
    // pairGroupA[r]] is a's value), pairLines[r] = the lines that have the pair.  The rows run over the pairs of byOf[i], row (i, r) at
    // rowOff[i] + r.  Without a number pattern the call answers the pairs and their lines: fieldValuePairs is that call.
    struct NumberStatsByPair : NumberStatsBy {
        std::vector<int32_t> pairA, pairB;
        std::vector<int64_t> pairOff;
        std::vector<int32_t> pairGroupA, pairGroupB, pairLines;
        // the two values of packed pair r of pair j
        std::pair<std::u16string, std::u16string> pairValues(size_t j, size_t r) const {
            return {values[(size_t)valOff[(size_t)pairA[j]] + (size_t)pairGroupA[r]], values[(size_t)valOff[(size_t)pairB[j]] + (size_t)pairGroupB[r]]};
        }
    };
    NumberStatsByPair numberStatsByPairBatch(const std::vector<std::u16string> &patterns, const std::vector<std::u16string> &keys,
                                             const std::vector<int32_t> &byOf, const std::vector<int32_t> &pairA, const std::vector<int32_t> &pairB,
                                             const std::u16string &stop, int32_t maxLen, const std::vector<Query> &queries,
                                             const std::vector<int32_t> &keyWhereOf, const std::vector<int32_t> &whereOf,
                                             const std::vector<int32_t> &permille = {500, 950}, int32_t fracDigits = 0, int32_t lineLo = 0,
                                             int32_t lineHi = INT32_MAX) const {
        if (whereOf.size() != patterns.size() || byOf.size() != patterns.size()) throw std::invalid_argument("whereOf and byOf have one entry per pattern");
        if (keyWhereOf.size() != keys.size()) throw std::invalid_argument("keyWhereOf has one entry per key pattern");
        if (pairA.size() != pairB.size()) throw std::invalid_argument("pairA and pairB have one entry per pair");
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        flattenQueries(queries, terms, kind, queryOff);
        std::vector<uint16_t> chars, keyChars, termChars;
        std::vector<int32_t> off, keyOff, termOff;
        pack(patterns, chars, off);
        pack(keys, keyChars, keyOff);
        pack(terms, termChars, termOff);
        NumberStatsByPair out;
        const size_t n = patterns.size(), m = keys.size(), c = pairA.size(), P = permille.size();
        out.permilles = (int32_t)P;
        out.pairA = pairA;
        out.pairB = pairB;
        out.valOff.assign(m + 1, 0);
        out.pairOff.assign(c + 1, 0);
        out.rowOff.assign(n + 1, 0);
        for (std::vector<int32_t> *v : {&out.noKey, &out.notNumber, &out.overflow, &out.occurrences, &out.kept, &out.status}) v->assign(n + 1, 0);
        for (std::vector<int32_t> *v : {&out.keyOccurrences, &out.keyKept, &out.keyStatus}) v->assign(m + 1, 0);
        out.termStatus.assign(terms.size(), 0);
        int32_t *lines = nullptr, *count = nullptr, *groupA = nullptr, *groupB = nullptr, *pairLines = nullptr;
        int64_t *textOff = nullptr, *vmin = nullptr, *vmax = nullptr, *pct = nullptr;
        uint64_t *sumLo = nullptr, *sumHi = nullptr;
        uint16_t *text = nullptr;
        detail::check(fmx_number_stats_by_pair_batch(h_, keyChars.data(), keyOff.data(), (int32_t)m, chars.data(), off.data(), (int32_t)n, byOf.data(),
                                                     (int32_t)c, pairA.data(), pairB.data(), termChars.data(), termOff.data(), (int32_t)terms.size(),
                                                     queryOff.data(), kind.data(), (int32_t)queries.size(), keyWhereOf.data(), whereOf.data(), lineLo,
                                                     lineHi, reinterpret_cast<const uint16_t *>(stop.data()), (int32_t)stop.size(), maxLen, fracDigits,
                                                     permille.data(), (int32_t)P, out.valOff.data(), &lines, &textOff, &text, out.pairOff.data(), &groupA,
                                                     &groupB, &pairLines, out.rowOff.data(), &count, &sumLo, &sumHi, &vmin, &vmax, &pct, out.noKey.data(),
                                                     out.notNumber.data(), out.overflow.data(), out.occurrences.data(), out.kept.data(), out.status.data(),
                                                     out.keyOccurrences.data(), out.keyKept.data(), out.keyStatus.data(), out.termStatus.data()),
                      "fmx_number_stats_by_pair_batch");
        const size_t G = (size_t)out.valOff[m], R = (size_t)out.rowOff[n], pairs = (size_t)out.pairOff[c];
        if (lines) {  // the ONE allocation: copied, then handed back
            out.lines.assign(lines, lines + G);
            for (size_t g = 0; g < G; ++g)
                out.values.emplace_back(reinterpret_cast<const char16_t *>(text) + textOff[g], (size_t)(textOff[g + 1] - textOff[g]));
            out.pairGroupA.assign(groupA, groupA + pairs);
            out.pairGroupB.assign(groupB, groupB + pairs);
            out.pairLines.assign(pairLines, pairLines + pairs);
            out.count.assign(count, count + R);
            out.sumLo.assign(sumLo, sumLo + R);
            out.sumHi.assign(sumHi, sumHi + R);
            out.min.assign(vmin, vmin + R);
            out.max.assign(vmax, vmax + R);
            out.pct.assign(pct, pct + R * P);
            fmx_free_buffer(reinterpret_cast<uint8_t *>(lines));
        }
        for (std::vector<int32_t> *v : {&out.noKey, &out.notNumber, &out.overflow, &out.occurrences, &out.kept, &out.status, &out.keyOccurrences,
                                        &out.keyKept, &out.keyStatus})
            v->pop_back();
        return out;
    }
    // one number pattern by the pair (byA, byB); the rows are in pair order: ascending by a's value, then b's
    NumberStatsByPair numberStatsByPair(const std::u16string &pattern, const std::u16string &byA, const std::u16string &byB,
                                        const std::u16string &stop = u" \t\r\n", int32_t maxLen = 32, const Query *where = nullptr,
                                        const std::vector<int32_t> &permille = {500, 950}, int32_t fracDigits = 0) const {
        if (pattern.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        return byPair({pattern}, byA, byB, stop, maxLen, where, permille, fracDigits);
    }
    // the pivot table count by a, b: (a's value, b's value, the lines that have both) in pair order
    struct ValuePair {
        std::u16string a, b;
        int32_t lines;
    };
    std::vector<ValuePair> fieldValuePairs(const std::u16string &byA, const std::u16string &byB, const std::u16string &stop = u" \t\r\n",
                                           int32_t maxLen = 32, const Query *where = nullptr) const {
        const NumberStatsByPair s = byPair({}, byA, byB, stop, maxLen, where, {}, 0);
        std::vector<ValuePair> out;
        for (size_t r = 0; r < s.pairLines.size(); ++r) {
            const auto v = s.pairValues(0, r);
            out.push_back(ValuePair{v.first, v.second, s.pairLines[r]});
        }
        return out;
    }

    // ... per bucket of lines (fmx.h "STATISTICS BY KEY PER BUCKET"; timechart p95(latency_ms=) by status=): numberStatsByBatch's
    // patterns, keys, byOf, stop, maxLen, queries, keyWhereOf and whereOf, hitHistogramWhereBatch's edges — none at all: one bucket,
    // every line, the device-side top-k of numberStatsBy; with edges only the hits inside edges[0] .. edges[B] count — and top.  The
    // key rows of key pattern k are keyRowOff[k] .. keyRowOff[k + 1]: its min(top, nGroups[k]) groups with the most lines, descending,
    // equal lines in value order; values[r], keyRowLines[r], keyRowGroup[r] (the key's index among the pattern's groups).  Number
    // pattern i has (rows of byOf[i] + 1) * B cells at cellOff[i]: cell(i, r, b), the last row being every other key; count, the
    // exact sum = sumHi * 2^64 + sumLo, min, max, pct[cell * P + j]; noKey / notNumber / overflow per number pattern.  Only the key
    // rows and the cells come down.  Needs buildLineTable().  Statuses are not thrown by the batch form; numberStatsByHistogram
    // answers one number pattern by one key pattern and throws them.
    struct NumberStatsByHistogram {
        int32_t buckets = 1, permilles = 0;
        std::vector<int64_t> keyRowOff, cellOff;
        std::vector<std::u16string> values;
        std::vector<int32_t> keyRowLines, keyRowGroup, nGroups, count;
        std::vector<uint64_t> sumLo, sumHi;
        std::vector<int64_t> min, max, pct;
        std::vector<int32_t> noKey, notNumber, overflow, occurrences, kept, status, keyOccurrences, keyKept, keyStatus, termStatus;
        size_t cell(size_t i, size_t r, size_t b) const { return (size_t)cellOff[i] + r * (size_t)buckets + b; }
    };
    NumberStatsByHistogram numberStatsByHistogramBatch(const std::vector<std::u16string> &patterns, const std::vector<std::u16string> &keys,
                                                       const std::vector<int32_t> &byOf, const std::u16string &stop, int32_t maxLen,
                                                       const std::vector<Query> &queries, const std::vector<int32_t> &keyWhereOf,
                                                       const std::vector<int32_t> &whereOf, const std::vector<int32_t> &edges = {}, int32_t top = 10,
                                                       const std::vector<int32_t> &permille = {500, 950}, int32_t fracDigits = 0) const {
        if (whereOf.size() != patterns.size() || byOf.size() != patterns.size()) throw std::invalid_argument("whereOf and byOf have one entry per pattern");
        if (keyWhereOf.size() != keys.size()) throw std::invalid_argument("keyWhereOf has one entry per key pattern");
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        flattenQueries(queries, terms, kind, queryOff);
        std::vector<uint16_t> chars, keyChars, termChars;
        std::vector<int32_t> off, keyOff, termOff;
        pack(patterns, chars, off);
        pack(keys, keyChars, keyOff);
        pack(terms, termChars, termOff);
        NumberStatsByHistogram out;
        const size_t n = patterns.size(), m = keys.size(), P = permille.size();
        out.buckets = edges.empty() ? 1 : edges.size() > 1 ? (int32_t)edges.size() - 1 : 0;
        out.permilles = (int32_t)P;
        out.keyRowOff.assign(m + 1, 0);
        out.cellOff.assign(n + 1, 0);
        for (std::vector<int32_t> *v : {&out.noKey, &out.notNumber, &out.overflow, &out.occurrences, &out.kept, &out.status}) v->assign(n + 1, 0);
        for (std::vector<int32_t> *v : {&out.nGroups, &out.keyOccurrences, &out.keyKept, &out.keyStatus}) v->assign(m + 1, 0);
        out.termStatus.assign(terms.size(), 0);
        int32_t *rowLines = nullptr, *rowGroup = nullptr, *count = nullptr;
        int64_t *textOff = nullptr, *vmin = nullptr, *vmax = nullptr, *pct = nullptr;
        uint64_t *sumLo = nullptr, *sumHi = nullptr;
        uint16_t *text = nullptr;
        detail::check(fmx_number_stats_by_histogram_batch(h_, keyChars.data(), keyOff.data(), (int32_t)m, chars.data(), off.data(), (int32_t)n,
                                                          byOf.data(), termChars.data(), termOff.data(), (int32_t)terms.size(), queryOff.data(),
                                                          kind.data(), (int32_t)queries.size(), keyWhereOf.data(), whereOf.data(),
                                                          edges.empty() ? nullptr : edges.data(), (int32_t)edges.size(), top,
                                                          reinterpret_cast<const uint16_t *>(stop.data()), (int32_t)stop.size(), maxLen, fracDigits,
                                                          permille.data(), (int32_t)P, out.nGroups.data(), out.keyRowOff.data(), &rowLines, &rowGroup,
                                                          &textOff, &text, out.cellOff.data(), &count, &sumLo, &sumHi, &vmin, &vmax, &pct,
                                                          out.noKey.data(), out.notNumber.data(), out.overflow.data(), out.occurrences.data(),
                                                          out.kept.data(), out.status.data(), out.keyOccurrences.data(), out.keyKept.data(),
                                                          out.keyStatus.data(), out.termStatus.data()),
                      "fmx_number_stats_by_histogram_batch");
        const size_t R = (size_t)out.keyRowOff[m], cells = (size_t)out.cellOff[n];
        if (rowLines) {  // the ONE allocation: copied, then handed back
            out.keyRowLines.assign(rowLines, rowLines + R);
            out.keyRowGroup.assign(rowGroup, rowGroup + R);
            for (size_t r = 0; r < R; ++r)
                out.values.emplace_back(reinterpret_cast<const char16_t *>(text) + textOff[r], (size_t)(textOff[r + 1] - textOff[r]));
            out.count.assign(count, count + cells);
            out.sumLo.assign(sumLo, sumLo + cells);
            out.sumHi.assign(sumHi, sumHi + cells);
            out.min.assign(vmin, vmin + cells);
            out.max.assign(vmax, vmax + cells);
            out.pct.assign(pct, pct + cells * P);
            fmx_free_buffer(reinterpret_cast<uint8_t *>(rowLines));
        }
        for (std::vector<int32_t> *v : {&out.noKey, &out.notNumber, &out.overflow, &out.occurrences, &out.kept, &out.status, &out.nGroups,
                                        &out.keyOccurrences, &out.keyKept, &out.keyStatus})
            v->pop_back();
        return out;
    }
    NumberStatsByHistogram numberStatsByHistogram(const std::u16string &pattern, const std::u16string &by, const std::vector<int32_t> &edges = {},
                                                  int32_t top = 10, const std::u16string &stop = u" \t\r\n", int32_t maxLen = 32,
                                                  const Query *where = nullptr, const std::vector<int32_t> &permille = {500, 950},
                                                  int32_t fracDigits = 0) const {
        if (pattern.empty() || by.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        if (where)
            for (const std::vector<std::u16string> *g : {&where->all, &where->any, &where->none})
                for (const std::u16string &t : *g)
                    if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const int32_t w = where ? 0 : -1;
        const NumberStatsByHistogram s = numberStatsByHistogramBatch({pattern}, {by}, {0}, stop, maxLen,
                                                                     where ? std::vector<Query>{*where} : std::vector<Query>{}, {w}, {w}, edges, top,
                                                                     permille, fracDigits);
        detail::raise_for_status(s.status[0]);
        detail::raise_for_status(s.keyStatus[0]);
        for (int st : s.termStatus) detail::raise_for_status(st);
        return s;
    }

    // the top values of a field per bucket of lines, the stacked timeline (fmx.h "TOP VALUES PER BUCKET"; count by status over time
    // where line has ...): fieldValuesWhereBatch's patterns, queries, whereOf, stop and maxLen, hitHistogramWhereBatch's edges — none
    // at all: one bucket, every line, the device-side top-k of fieldValues (no line table needed unless a pattern asks for a query);
    // with edges only the hits inside edges[0] .. edges[B] count.  The rows of pattern i are rowOff[i] .. rowOff[i + 1]: its min(top,
    // nValues[i]) values with the largest counts, descending, equal counts in value order; values[r], rowCount[r], rowGroup[r] (the
    // value's index among the pattern's distinct values), counts[r * B + b]; other[i * B + b] = the kept hits of no row.  Only the
    // rows come down.  Statuses are not thrown by the batch form; fieldValuesHistogram answers one pattern and throws them.
    struct FieldValuesHistogram {
        int32_t buckets = 1;
        std::vector<int64_t> rowOff;
        std::vector<std::u16string> values;
        std::vector<int32_t> rowCount, rowGroup, counts, other, nValues, occurrences, kept, status, termStatus;
        std::vector<int32_t> row(size_t r) const { return {counts.begin() + r * (size_t)buckets, counts.begin() + (r + 1) * (size_t)buckets}; }
        std::vector<int32_t> otherOf(size_t i) const { return {other.begin() + i * (size_t)buckets, other.begin() + (i + 1) * (size_t)buckets}; }
    };
    FieldValuesHistogram fieldValuesHistogramBatch(const std::vector<std::u16string> &patterns, const std::vector<Query> &queries,
                                                   const std::vector<int32_t> &whereOf, const std::vector<int32_t> &edges = {}, int32_t top = 10,
                                                   const std::u16string &stop = u" ", int32_t maxLen = 64) const {
        if (whereOf.size() != patterns.size()) throw std::invalid_argument("whereOf has one entry per pattern");
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        flattenQueries(queries, terms, kind, queryOff);
        std::vector<uint16_t> chars, termChars;
        std::vector<int32_t> off, termOff;
        pack(patterns, chars, off);
        pack(terms, termChars, termOff);
        FieldValuesHistogram out;
        const size_t n = patterns.size();
        out.buckets = edges.empty() ? 1 : edges.size() > 1 ? (int32_t)edges.size() - 1 : 0;
        out.rowOff.assign(n + 1, 0);
        out.other.assign(n * (size_t)out.buckets + 1, 0);
        for (std::vector<int32_t> *v : {&out.nValues, &out.occurrences, &out.kept, &out.status}) v->assign(n + 1, 0);
        out.termStatus.assign(terms.size(), 0);
        int32_t *rowCount = nullptr, *rowGroup = nullptr, *hist = nullptr;
        int64_t *textOff = nullptr;
        uint16_t *text = nullptr;
        detail::check(fmx_field_values_histogram_where_batch(h_, chars.data(), off.data(), (int32_t)n, termChars.data(), termOff.data(),
                                                             (int32_t)terms.size(), queryOff.data(), kind.data(), (int32_t)queries.size(),
                                                             whereOf.data(), edges.empty() ? nullptr : edges.data(), (int32_t)edges.size(), top,
                                                             reinterpret_cast<const uint16_t *>(stop.data()), (int32_t)stop.size(), maxLen,
                                                             out.nValues.data(), out.rowOff.data(), &rowCount, &rowGroup, &textOff, &text, &hist,
                                                             out.other.data(), out.occurrences.data(), out.kept.data(), out.status.data(),
                                                             out.termStatus.data()),
                      "fmx_field_values_histogram_where_batch");
        const size_t R = (size_t)out.rowOff[n];
        if (rowCount) {  // the ONE allocation: copied, then handed back
            out.rowCount.assign(rowCount, rowCount + R);
            out.rowGroup.assign(rowGroup, rowGroup + R);
            out.counts.assign(hist, hist + R * (size_t)out.buckets);
            for (size_t r = 0; r < R; ++r)
                out.values.emplace_back(reinterpret_cast<const char16_t *>(text) + textOff[r], (size_t)(textOff[r + 1] - textOff[r]));
            fmx_free_buffer(reinterpret_cast<uint8_t *>(rowCount));
        }
        out.other.pop_back();
        for (std::vector<int32_t> *v : {&out.nValues, &out.occurrences, &out.kept, &out.status}) v->pop_back();
        return out;
    }
    FieldValuesHistogram fieldValuesHistogram(const std::u16string &pattern, const std::vector<int32_t> &edges = {}, int32_t top = 10,
                                              const Query *where = nullptr, const std::u16string &stop = u" ", int32_t maxLen = 64) const {
        if (pattern.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        if (where)
            for (const std::vector<std::u16string> *g : {&where->all, &where->any, &where->none})
                for (const std::u16string &t : *g)
                    if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const FieldValuesHistogram h = fieldValuesHistogramBatch({pattern}, where ? std::vector<Query>{*where} : std::vector<Query>{}, {where ? 0 : -1},
                                                                 edges, top, stop, maxLen);
        detail::raise_for_status(h.status[0]);
        for (int st : h.termStatus) detail::raise_for_status(st);
        return h;
    }

    // the distinct values of a field per bucket of lines, dc over time (fmx.h "DISTINCT VALUES PER BUCKET"; timechart dc(user=)
    // where line has ...): fieldValuesHistogramBatch's arguments without top.  distinct[i * B + b] = the different values among the
    // kept hits of pattern i in bucket b; firstSeen[i * B + b] = the values of i whose first kept hit lies in bucket b.  Two ints per
    // bucket come down, however many values there are.  Statuses are not thrown by the batch form; distinctValues answers one pattern
    // and throws them.
    struct DistinctValues {
        int32_t buckets = 1;
        std::vector<int32_t> distinct, firstSeen, nValues, occurrences, kept, status, termStatus;
        std::vector<int32_t> distinctOf(size_t i) const { return {distinct.begin() + i * (size_t)buckets, distinct.begin() + (i + 1) * (size_t)buckets}; }
        std::vector<int32_t> firstSeenOf(size_t i) const { return {firstSeen.begin() + i * (size_t)buckets, firstSeen.begin() + (i + 1) * (size_t)buckets}; }
    };
    DistinctValues distinctValuesBatch(const std::vector<std::u16string> &patterns, const std::vector<Query> &queries,
                                       const std::vector<int32_t> &whereOf, const std::vector<int32_t> &edges = {},
                                       const std::u16string &stop = u" ", int32_t maxLen = 64) const {
        if (whereOf.size() != patterns.size()) throw std::invalid_argument("whereOf has one entry per pattern");
        std::vector<std::u16string> terms;
        std::vector<uint8_t> kind;
        std::vector<int32_t> queryOff{0};
        flattenQueries(queries, terms, kind, queryOff);
        std::vector<uint16_t> chars, termChars;
        std::vector<int32_t> off, termOff;
        pack(patterns, chars, off);
        pack(terms, termChars, termOff);
        DistinctValues out;
        const size_t n = patterns.size();
        out.buckets = edges.empty() ? 1 : edges.size() > 1 ? (int32_t)edges.size() - 1 : 0;
        for (std::vector<int32_t> *v : {&out.distinct, &out.firstSeen}) v->assign(n * (size_t)out.buckets + 1, 0);
        for (std::vector<int32_t> *v : {&out.nValues, &out.occurrences, &out.kept, &out.status}) v->assign(n + 1, 0);
        out.termStatus.assign(terms.size(), 0);
        detail::check(fmx_distinct_values_histogram_where_batch(h_, chars.data(), off.data(), (int32_t)n, termChars.data(), termOff.data(),
                                                                (int32_t)terms.size(), queryOff.data(), kind.data(), (int32_t)queries.size(),
                                                                whereOf.data(), edges.empty() ? nullptr : edges.data(), (int32_t)edges.size(),
                                                                reinterpret_cast<const uint16_t *>(stop.data()), (int32_t)stop.size(), maxLen,
                                                                out.distinct.data(), out.firstSeen.data(), out.nValues.data(),
                                                                out.occurrences.data(), out.kept.data(), out.status.data(), out.termStatus.data()),
                      "fmx_distinct_values_histogram_where_batch");
        for (std::vector<int32_t> *v : {&out.distinct, &out.firstSeen, &out.nValues, &out.occurrences, &out.kept, &out.status}) v->pop_back();
        return out;
    }
    DistinctValues distinctValues(const std::u16string &pattern, const std::vector<int32_t> &edges = {}, const Query *where = nullptr,
                                  const std::u16string &stop = u" ", int32_t maxLen = 64) const {
        if (pattern.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        if (where)
            for (const std::vector<std::u16string> *g : {&where->all, &where->any, &where->none})
                for (const std::u16string &t : *g)
                    if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const DistinctValues d = distinctValuesBatch({pattern}, where ? std::vector<Query>{*where} : std::vector<Query>{}, {where ? 0 : -1}, edges,
                                                     stop, maxLen);
        detail::raise_for_status(d.status[0]);
        for (int st : d.termStatus) detail::raise_for_status(st);
        return d;
    }

    // the text of ranges and of lines in ONE packed array (fmx.h "THE TEXT OF RANGES AND LINES IN ONE PACKED ARRAY"): range / line
    // i is chars[offsets[i] .. offsets[i + 1]) — what extract(start, stop, destination, 0) leaves in destination; memory follows
    // the sum of the lengths.  status[i] is the range's own (not thrown: one range out of the text does not hide the others);
    // a range with a status, or with stop <= start, is empty.  lineText throws for an id that is no line.
    struct Text {
        std::vector<int64_t> offsets;
        std::vector<int32_t> status;
        std::u16string chars;
        std::u16string operator[](size_t i) const { return chars.substr((size_t)offsets[i], (size_t)(offsets[i + 1] - offsets[i])); }
    };
    Text extractPacked(const std::vector<int32_t> &starts, const std::vector<int32_t> &stops) const {
        if (starts.size() != stops.size()) throw std::invalid_argument("extractPacked: starts and stops differ in length");
        const int32_t n = (int32_t)starts.size();
        Text out;
        out.offsets.assign((size_t)n + 1, 0);
        out.status.assign(starts.size(), 0);
        uint16_t *buf = nullptr;
        detail::check(fmx_extract_packed_batch(h_, starts.data(), stops.data(), n, out.offsets.data(), &buf, out.status.data()),
                      "fmx_extract_packed_batch");
        return takeText(out, buf, n);
    }
    Text lineTextBatch(const std::vector<int32_t> &lines) const {
        const int32_t n = (int32_t)lines.size();
        Text out;
        out.offsets.assign((size_t)n + 1, 0);
        out.status.assign(lines.size(), 0);
        uint16_t *buf = nullptr;
        detail::check(fmx_line_text_batch(h_, lines.data(), n, out.offsets.data(), &buf, out.status.data()), "fmx_line_text_batch");
        return takeText(out, buf, n);
    }
    std::vector<std::u16string> lineText(const std::vector<int32_t> &lines) const {
        const Text t = lineTextBatch(lines);
        for (int s : t.status) detail::raise_for_status(s);
        std::vector<std::u16string> out;
        out.reserve(lines.size());
        for (size_t i = 0; i < lines.size(); ++i) out.push_back(t[i]);
        return out;
    }

    // locate, then extract(loc, min(getInputLength(), loc + extractLength), row, 0) per hit, both on the device:
    // the composite the reference times in locateAndExtractBenchmark (FmIndexThroughputBenchmark.java:231-249).
    // Hit k of pattern i: locations[i*maxMatches+k], rows[i*maxMatches+k] (extractLength chars, only the first
    // outLen are the text), hitStatus = status of that extract call (not thrown: one hit near the end of the text
    // fails with "Stop position longer than index string" without hiding the others).
    struct HitRows {
        std::vector<int32_t> found, locations, outLen, hitStatus, hitAux;
        std::vector<std::u16string> rows;
    };
    HitRows locateExtractBatch(const std::vector<std::u16string> &patterns, int maxMatches, int extractLength) const {
        return pipeline(patterns, maxMatches, extractLength, -1, 0);
    }
    // locate, then extractUntilBoundary (mode 0) / ...Left (1) / ...Right (2) per hit, FM:640-922
    HitRows locateLinesBatch(const std::vector<std::u16string> &patterns, int maxMatches, char16_t boundary,
                             int rowLength, int mode = 0) const {
        return pipeline(patterns, maxMatches, rowLength, mode, boundary);
    }

    // ---- scalar API, as in the reference ----
    int count(const std::u16string &pattern) const { return count(pattern, 0, (int)pattern.size()); }  // FM:443-445
    int count(const std::u16string &pattern, int offset, int length) const {                            // FM:455-474
        if (length <= 0 || offset < 0 || (size_t)(offset + length) > pattern.size())
            throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const int32_t off[2] = {0, length};
        int32_t c = 0, st = 0;
        detail::check(fmx_count_batch(h_, reinterpret_cast<const uint16_t *>(pattern.data()) + offset, off, 1, &c,
                                      nullptr, &st),
                      "fmx_count_batch");
        detail::raise_for_status(st);
        return c;
    }
    int locate(const std::u16string &pattern, std::vector<int32_t> &locations) const {  // FM:487-489
        return locate(pattern, 0, (int)pattern.size(), locations, -1);
    }
    int locate(const std::u16string &pattern, int offset, int length, std::vector<int32_t> &locations,
               int maxMatches) const {  // FM:504-552: `locations` is the caller's pre-sized array
        if (length <= 0 || offset < 0 || (size_t)(offset + length) > pattern.size())
            throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const int32_t off[2] = {0, length};
        int32_t found = 0, st = 0;
        detail::check(fmx_locate_batch(h_, reinterpret_cast<const uint16_t *>(pattern.data()) + offset, off, 1,
                                       maxMatches, locations.data(), (int32_t)locations.size(), &found, nullptr, &st),
                      "fmx_locate_batch");
        detail::raise_for_status(st);
        return found;
    }
    int extract(int start, int stop, std::u16string &destination, int offset) const {  // FM:564-608
        int32_t len = 0, st = 0;
        detail::check(fmx_extract_batch(h_, &start, &stop, 1, reinterpret_cast<uint16_t *>(&destination[0]),
                                        (int32_t)destination.size(), offset, &len, nullptr, &st),
                      "fmx_extract_batch");
        detail::raise_for_status(st);
        return len;
    }
    int extractUntilBoundary(int from, std::u16string &destination, int offset, char16_t boundary) const {  // FM:640-759
        return boundaryCall(0, from, destination, offset, boundary);
    }
    int extractUntilBoundaryLeft(int from, std::u16string &destination, int offset, char16_t boundary) const {  // FM:772-831
        return boundaryCall(1, from, destination, offset, boundary);
    }
    int extractUntilBoundaryRight(int from, std::u16string &destination, int offset, char16_t boundary) const {  // FM:844-922
        return boundaryCall(2, from, destination, offset, boundary);
    }

    // FM:239-298
    static int convertBytePatternToCharPattern(const uint8_t *pattern, int offset, int length, char16_t *destination) {
        int32_t bad = 0;
        const int n = fmx_convert_byte_pattern(pattern, offset, length, reinterpret_cast<uint16_t *>(destination), &bad);
        if (n < 0)
            throw std::runtime_error("Found a character that exceeds (32767): it was " + std::to_string(bad));
        return n;
    }

    static void packPatterns(const std::vector<std::u16string> &patterns, std::vector<uint16_t> &chars,
                             std::vector<int32_t> &off) {
        pack(patterns, chars, off);
    }

private:
    explicit FmIndex(fmx_index *h) : h_(h) {}
    // the library's buffer of a packed text, copied into the result and handed back
    static Text takeText(Text &out, uint16_t *buf, int32_t n) {
        try {
            if (buf) out.chars.assign(reinterpret_cast<const char16_t *>(buf), (size_t)out.offsets[(size_t)n]);
        } catch (...) {
            fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
            throw;
        }
        fmx_free_buffer(reinterpret_cast<uint8_t *>(buf));
        return out;
    }

    static void pack(const std::vector<std::u16string> &patterns, std::vector<uint16_t> &chars,
                     std::vector<int32_t> &off) {
        off.assign(1, 0);
        for (const auto &p : patterns) {
            chars.insert(chars.end(), p.begin(), p.end());
            off.push_back((int32_t)chars.size());
        }
        if (chars.empty()) chars.push_back(0);
    }
    // the terms of a batch of queries in the order all, any, none of query 0, then query 1 ..., their kinds (one entry more: never
    // an empty array) and the offsets that cut them into queries (queryOff starts as {0})
    static void flattenQueries(const std::vector<Query> &queries, std::vector<std::u16string> &terms, std::vector<uint8_t> &kind,
                               std::vector<int32_t> &queryOff) {
        for (const Query &qu : queries) {
            const std::vector<std::u16string> *groups[3] = {&qu.all, &qu.any, &qu.none};
            for (int k = 0; k < 3; ++k)
                for (const std::u16string &t : *groups[k]) {
                    terms.push_back(t);
                    kind.push_back((uint8_t)k);
                }
            queryOff.push_back((int32_t)terms.size());
        }
        kind.push_back(0);
    }
    // numberStatsByPairBatch for the one pair (byA, byB) and at most one number pattern, the statuses thrown
    NumberStatsByPair byPair(const std::vector<std::u16string> &patterns, const std::u16string &byA, const std::u16string &byB, const std::u16string &stop,
                             int32_t maxLen, const Query *where, const std::vector<int32_t> &permille, int32_t fracDigits) const {
        if (byA.empty() || byB.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        if (where)
            for (const std::vector<std::u16string> *g : {&where->all, &where->any, &where->none})
                for (const std::u16string &t : *g)
                    if (t.empty()) throw std::out_of_range("ArrayIndexOutOfBoundsException");
        const int32_t w = where ? 0 : -1;
        const NumberStatsByPair s =
            numberStatsByPairBatch(patterns, {byA, byB}, std::vector<int32_t>(patterns.size(), 0), {0}, {1}, stop, maxLen,
                                   where ? std::vector<Query>{*where} : std::vector<Query>{}, {w, w}, std::vector<int32_t>(patterns.size(), w), permille, fracDigits);
        for (int st : s.status) detail::raise_for_status(st);
        for (int st : s.keyStatus) detail::raise_for_status(st);
        for (int st : s.termStatus) detail::raise_for_status(st);
        return s;
    }
    // the three packed arrays of a batch of class patterns (fmx_count_class_batch)
    static FieldValues emptyFieldValues(size_t n) {
        FieldValues out;
        out.offsets.assign(n + 1, 0);
        out.textOffsets.assign(1, 0);
        out.occurrences.assign(n, 0);
        out.status.assign(n, 0);
        return out;
    }
    // the library's ONE buffer {counts | text offsets | code units} into the vectors, then freed (counts owns it)
    static FieldValues takeFieldValues(FieldValues &out, int32_t *counts, const int64_t *textOff, const uint16_t *units) {
        const size_t groups = (size_t)out.offsets.back();
        try {
            if (counts) {
                out.counts.assign(counts, counts + groups);
                out.textOffsets.assign(textOff, textOff + groups + 1);
                out.chars.assign(reinterpret_cast<const char16_t *>(units), (size_t)textOff[groups]);
            }
        } catch (...) {
            fmx_free_buffer(reinterpret_cast<uint8_t *>(counts));
            throw;
        }
        fmx_free_buffer(reinterpret_cast<uint8_t *>(counts));
        return out;
    }
    struct ClassArrays {
        std::vector<uint16_t> alt;
        std::vector<int32_t> posOff{0}, patOff{0};
        explicit ClassArrays(const std::vector<ClassPattern> &patterns) {
            for (const ClassPattern &p : patterns) {
                for (const std::u16string &alts : p) {
                    alt.insert(alt.end(), alts.begin(), alts.end());
                    posOff.push_back((int32_t)alt.size());
                }
                patOff.push_back((int32_t)posOff.size() - 1);
            }
            if (alt.empty()) alt.push_back(0);
        }
        int32_t nPos() const { return (int32_t)posOff.size() - 1; }
        int32_t n() const { return (int32_t)patOff.size() - 1; }
    };
    HitRows pipeline(const std::vector<std::u16string> &patterns, int maxMatches, int rowLength, int mode,
                     char16_t boundary) const {
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        pack(patterns, chars, off);
        const int32_t n = (int32_t)patterns.size();
        const size_t slots = (size_t)n * (size_t)maxMatches;
        HitRows r;
        r.found.assign(patterns.size(), 0);
        r.locations.assign(slots, -1);
        r.outLen.assign(slots, -1);
        r.hitStatus.assign(slots, 0);
        r.hitAux.assign(slots, 0);
        std::vector<uint16_t> dst(slots * (size_t)rowLength, 0);
        std::vector<int32_t> status(patterns.size());
        if (mode < 0)
            detail::check(fmx_locate_extract_batch(h_, chars.data(), off.data(), n, maxMatches, rowLength,
                                                   r.locations.data(), r.found.data(), dst.data(), r.outLen.data(), nullptr,
                                                   status.data(), r.hitStatus.data()),
                          "fmx_locate_extract_batch");
        else
            detail::check(fmx_locate_lines_batch(h_, chars.data(), off.data(), n, maxMatches, (uint16_t)boundary, mode,
                                                 rowLength, r.locations.data(), r.found.data(), dst.data(), r.outLen.data(),
                                                 nullptr, status.data(), r.hitStatus.data(), r.hitAux.data()),
                          "fmx_locate_lines_batch");
        for (int st : status) detail::raise_for_status(st);
        r.rows.resize(slots);
        for (size_t q = 0; q < slots; ++q)
            r.rows[q].assign(reinterpret_cast<const char16_t *>(dst.data()) + q * (size_t)rowLength, (size_t)rowLength);
        return r;
    }
    int boundaryCall(int mode, int from, std::u16string &destination, int offset, char16_t boundary) const {
        int32_t len = 0, st = 0, aux = 0;
        detail::check(fmx_extract_boundary_batch(h_, &from, 1, (uint16_t)boundary, mode,
                                                 reinterpret_cast<uint16_t *>(&destination[0]),
                                                 (int32_t)destination.size(), offset, &len, nullptr, &st, &aux),
                      "fmx_extract_boundary_batch");
        detail::raise_for_status(st, aux);
        return len;
    }
    fmx_index *h_ = nullptr;
};

// fm/FmIndexBuilder.java: defaults sampleRate = 32, enableExtraction = true (FMB:21-22)
class FmIndexBuilder {
public:
    FmIndexBuilder &setSampleRate(int sampleRate) {  // FMB:34-37
        sampleRate_ = sampleRate;
        return *this;
    }
    FmIndexBuilder &setEnableExtraction(bool enable) {  // FMB:46-49
        enableExtraction_ = enable;
        return *this;
    }
    FmIndexBuilder &setDevice(int device) {  // -1 keeps the index on the host (build / save only)
        device_ = device;
        return *this;
    }
    FmIndexBuilder &setBuildDevice(int device) {  // extension: suffix-array stage of the build on this GPU
        buildDevice_ = device;
        return *this;
    }
    FmIndex build(const std::u16string &input) const {  // FMB:59-61
        return FmIndex(input, sampleRate_, enableExtraction_, device_, buildDevice_);
    }

private:
    int sampleRate_ = 32;
    bool enableExtraction_ = true;
    int device_ = 0;
    int buildDevice_ = -1;
};

// One FmIndex on several GPUs of a node (fmx.h "replicas"): FmIndex is immutable and @ThreadSafe (FM:82), index4j's throughput
// benchmark gives every thread an index of its own (FmIndexThroughputState.java:30) — the image is copied to every device named
// (fmx_replicate: peer copies, all destinations at once) and a batch is cut into contiguous shards, one per replica, each stored
// into its own slice of the caller's arrays (fmx_*_multi): no exchange on the query path.  A device may be named more than once.
class FmIndexReplicas {
public:
    FmIndexReplicas(const FmIndex &source, const std::vector<int32_t> &devices) : handles_(devices.size(), nullptr) {
        detail::check(fmx_replicate(source.handle(), devices.data(), (int32_t)devices.size(), handles_.data()), "fmx_replicate");
    }
    FmIndexReplicas(const FmIndexReplicas &) = delete;
    FmIndexReplicas &operator=(const FmIndexReplicas &) = delete;
    ~FmIndexReplicas() {
        for (fmx_index *h : handles_) fmx_free(h);
    }
    size_t size() const { return handles_.size(); }
    int deviceOf(size_t replica) const { return fmx_device_of(handles_[replica]); }
    std::vector<int32_t> countBatch(const std::vector<std::u16string> &patterns) const {
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        FmIndex::packPatterns(patterns, chars, off);
        std::vector<int32_t> counts(patterns.size()), status(patterns.size());
        detail::check(fmx_count_batch_multi(handles_.data(), (int32_t)handles_.size(), chars.data(), off.data(), (int32_t)patterns.size(),
                                            counts.data(), nullptr, status.data()),
                      "fmx_count_batch_multi");
        for (int s : status) detail::raise_for_status(s);
        return counts;
    }
    // returns found[i]; locations is patterns.size() rows of maxMatches ints
    std::vector<int32_t> locateBatch(const std::vector<std::u16string> &patterns, int maxMatches, std::vector<int32_t> &locations) const {
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        FmIndex::packPatterns(patterns, chars, off);
        const int32_t n = (int32_t)patterns.size();
        locations.assign((size_t)n * (size_t)maxMatches, 0);
        std::vector<int32_t> found(patterns.size()), status(patterns.size());
        detail::check(fmx_locate_batch_multi(handles_.data(), (int32_t)handles_.size(), chars.data(), off.data(), n, maxMatches,
                                             locations.data(), maxMatches, found.data(), nullptr, status.data()),
                      "fmx_locate_batch_multi");
        for (int s : status) detail::raise_for_status(s);
        return found;
    }

private:
    std::vector<fmx_index *> handles_;
};

// One long text as K FmIndex objects over consecutive pieces (a Java int cannot address 2^31 chars, FM:131):
// count = sum over the pieces, hits = piece start + local position, in piece order — what a caller's loop over K
// indexes computes, as one device call (fmx_count_segments / fmx_locate_segments).  All pieces on one GPU.
class SegmentedFmIndex {
public:
    void add(FmIndex &&segment, int64_t textOffset) {
        segments_.push_back(std::move(segment));
        bases_.push_back(textOffset);
        handles_.push_back(segments_.back().handle());
    }
    size_t size() const { return segments_.size(); }
    std::vector<int64_t> countBatch(const std::vector<std::u16string> &patterns) const {
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        FmIndex::packPatterns(patterns, chars, off);
        std::vector<int64_t> counts(patterns.size());
        std::vector<int32_t> status(patterns.size());
        detail::check(fmx_count_segments(handles_.data(), (int32_t)handles_.size(), chars.data(), off.data(),
                                         (int32_t)patterns.size(), counts.data(), nullptr, status.data()),
                      "fmx_count_segments");
        for (int st : status) detail::raise_for_status(st);
        return counts;
    }
    // returns found[i]; locations = patterns.size() rows of maxMatches global text positions
    std::vector<int32_t> locateBatch(const std::vector<std::u16string> &patterns, int maxMatches,
                                     std::vector<int64_t> &locations) const {
        std::vector<uint16_t> chars;
        std::vector<int32_t> off;
        FmIndex::packPatterns(patterns, chars, off);
        locations.assign(patterns.size() * (size_t)maxMatches, -1);
        std::vector<int32_t> found(patterns.size()), status(patterns.size());
        detail::check(fmx_locate_segments(handles_.data(), (int32_t)handles_.size(), bases_.data(), chars.data(),
                                          off.data(), (int32_t)patterns.size(), maxMatches, locations.data(), found.data(),
                                          status.data()),
                      "fmx_locate_segments");
        for (int st : status) detail::raise_for_status(st);
        return found;
    }

private:
    std::vector<FmIndex> segments_;
    std::vector<int64_t> bases_;
    std::vector<const fmx_index *> handles_;
};

}  // namespace index4j
