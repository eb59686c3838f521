// san_merged_batch.cpp — sanitizer driver of the merged batch of the where, histogram and stats forms: the checks of a call's HOST
// arrays and the merge of filter terms and value patterns into ONE batch (index4j_amd/csrc/fmx_host_batch.cpp, linked as it is), as a
// stand-alone program for -fsanitize=address,undefined.  Every array lies on the heap with exactly the size the contract gives it
// (an array of no entries is NULL), so a read or a store outside one is a report.  The judge is the merge written out naively
// below: the strings of the terms, then those of the value patterns, laid end to end.  The refusals are checked by their message,
// and by a MergedBatch that is still empty.  The keyed merges (terms | key patterns | number patterns) are judged by two successive
// merges; the checks of the values' and the numbers' shape, the limits of the hits, term_len and the window of lines at their
// edges, by their message.  Prints one " ok: " line per case; exit code 0 = clean.
#include "fmx_host_stage.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

namespace {
int g_code = 0;
std::string g_msg;
int g_cases = 0;
}  // namespace

namespace fmx {
int api_fail(int code, const std::string &msg) {  // the stub: what fmx_last_error would say
    g_code = code;
    g_msg = msg;
    return code;
}
}  // namespace fmx

namespace {

using Str = std::vector<uint16_t>;
using ClassPat = std::vector<Str>;  // positions of alternatives

void require(bool ok, const char *name, const char *what) {
    if (ok) return;
    std::fprintf(stderr, "FAILED %s: %s (last message: \"%s\")\n", name, what, g_msg.c_str());
    std::exit(1);
}
void passed(const char *name) {
    ++g_cases;
    std::printf(" ok: %s\n", name);
}

// exactly v.size() entries on the heap; none at all: NULL
template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {
    if (v.empty()) return nullptr;
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

// a part of a literal call as the ABI takes it: `lead` unused characters in front, so that off[0] == lead
struct Literal {
    std::vector<uint16_t> chars;
    std::vector<int32_t> off;  // count + 1, or none (count == 0 and the array is NULL)
    int32_t count;
    Literal(const std::vector<Str> &strings, int32_t lead, bool null_when_empty) : count((int32_t)strings.size()) {
        chars.assign((size_t)lead, 0xEEEE);
        if (count == 0 && null_when_empty) return;
        off.push_back(lead);
        for (const Str &s : strings) {
            chars.insert(chars.end(), s.begin(), s.end());
            off.push_back((int32_t)chars.size());
        }
    }
};

void literal_case(const char *name, const std::vector<Str> &terms, const std::vector<Str> &pats, int32_t term_lead, int32_t pat_lead) {
    const Literal t(terms, term_lead, true), p(pats, pat_lead, false);
    const auto t_chars = exact(t.chars), p_chars = exact(p.chars);
    const auto t_off = exact(t.off), p_off = exact(p.off);
    require(fmx::check_literal_batches(p_off.get(), p.count, t_off.get(), t.count) == FMX_OK, name, "the checks refuse");
    fmx::MergedBatch m;
    fmx::ValuesBatch b{};
    require(fmx::merge_literal_batch(p_chars.get(), p_off.get(), p.count, t_chars.get(), t_off.get(), t.count, &m, &b) == FMX_OK, name,
            "the merge refuses");
    // the naive merge: the strings end to end
    std::vector<Str> all(terms);
    all.insert(all.end(), pats.begin(), pats.end());
    require(b.n_terms == t.count && b.n == p.count && !b.pos_off && b.n_pos == 0 && b.max_ranges == 0 && b.chars && b.pat_off, name, "the shape");
    require(m.off.size() == all.size() + 1 && b.pat_off == m.off.data() && b.chars == m.chars.data(), name, "the arrays");
    int32_t at = 0;
    for (size_t i = 0; i < all.size(); ++i) {
        require(b.pat_off[i] == at && b.pat_off[i + 1] == at + (int32_t)all[i].size(), name, "an offset");
        for (size_t k = 0; k < all[i].size(); ++k) require(b.chars[(size_t)at + k] == all[i][k], name, "a character");
        at += (int32_t)all[i].size();
    }
    require(b.pat_off[0] == 0 && m.chars.size() == (size_t)at + 1, name, "the ends");
    passed(name);
}

// a part of a class call as the ABI takes it: `lead_alt` unused alternatives and `lead_pos` unused positions in front
struct Class {
    std::vector<uint16_t> alt;
    std::vector<int32_t> pos_off, pat_off;
    int32_t n_pos, count;
    Class(const std::vector<ClassPat> &pats, int32_t lead_alt, int32_t lead_pos) : count((int32_t)pats.size()) {
        alt.assign((size_t)lead_alt, 0xEEEE);
        pos_off.push_back(0);
        for (int32_t j = 0; j < lead_pos; ++j) pos_off.push_back(lead_alt);  // (lead_pos positions over the unused alternatives)
        if (lead_pos == 0) pos_off[0] = lead_alt;
        pat_off.push_back(lead_pos);
        for (const ClassPat &p : pats) {
            for (const Str &s : p) {
                alt.insert(alt.end(), s.begin(), s.end());
                pos_off.push_back((int32_t)alt.size());
            }
            pat_off.push_back((int32_t)pos_off.size() - 1);
        }
        n_pos = (int32_t)pos_off.size() - 1;
    }
};

void class_case(const char *name, const std::vector<ClassPat> &terms, const std::vector<ClassPat> &pats, int32_t lead_alt, int32_t lead_pos) {
    const Class t(terms, lead_alt, lead_pos), p(pats, lead_alt, lead_pos);
    const bool no_terms = terms.empty();  // (no terms: the three arrays of the terms are NULL)
    const auto t_alt = exact(t.alt), p_alt = exact(p.alt);
    const auto t_pos = exact(no_terms ? std::vector<int32_t>() : t.pos_off), p_pos = exact(p.pos_off);
    const auto t_off = exact(no_terms ? std::vector<int32_t>() : t.pat_off), p_off = exact(p.pat_off);
    const int32_t t_n_pos = no_terms ? 0 : t.n_pos;
    require(fmx::check_class_batches(p_alt.get(), p_pos.get(), p.n_pos, p_off.get(), p.count, t_alt.get(), t_pos.get(), t_n_pos, t_off.get(),
                                     t.count) == FMX_OK,
            name, "the checks refuse");
    fmx::MergedBatch m;
    fmx::ValuesBatch b{};
    require(fmx::merge_class_batch(p_alt.get(), p_pos.get(), p.n_pos, p_off.get(), p.count, t_alt.get(), t_pos.get(), t_n_pos, t_off.get(), t.count,
                                   7, &m, &b) == FMX_OK,
            name, "the merge refuses");
    // the naive merge: the patterns' positions one behind the other
    std::vector<ClassPat> all(terms);
    all.insert(all.end(), pats.begin(), pats.end());
    require(b.n_terms == t.count && b.n == p.count && b.max_ranges == 7 && b.chars == m.chars.data() && b.pos_off == m.pos.data() &&
                b.pat_off == m.off.data() && m.off.size() == all.size() + 1,
            name, "the shape");
    int32_t pos = 0, at = 0;
    require(b.pat_off[0] == 0 && b.pos_off[0] == 0, name, "the starts");
    for (size_t i = 0; i < all.size(); ++i) {
        for (const Str &s : all[i]) {
            require(b.pos_off[pos] == at && b.pos_off[pos + 1] == at + (int32_t)s.size(), name, "a position's offsets");
            for (size_t k = 0; k < s.size(); ++k) require(b.chars[(size_t)at + k] == s[k], name, "an alternative");
            at += (int32_t)s.size();
            ++pos;
        }
        require(b.pat_off[i + 1] == pos, name, "a pattern's offset");
    }
    require(b.n_pos == pos && m.pos.size() == (size_t)pos + 1 && m.chars.size() == (size_t)at + 1, name, "the ends");
    passed(name);
}

// the keyed merges: ONE batch terms | keys | numbers.  The judge is what two successive calls of the merges above give — the keys in
// the terms' slot of the first, its answer as the value patterns of the second — and the lengths of the strings themselves.
void same_batch(const char *name, const fmx::MergedBatch &m, const fmx::ValuesBatch &b, const fmx::MergedBatch &ref, const fmx::ValuesBatch &rb) {
    require(m.chars == ref.chars && m.pos == ref.pos && m.off == ref.off, name, "another merged batch than two successive merges give");
    require(b.n_terms == rb.n_terms && b.n == rb.n && b.n_pos == rb.n_pos && b.max_ranges == rb.max_ranges && b.chars == m.chars.data() &&
                b.pat_off == m.off.data() && (rb.pos_off ? b.pos_off == m.pos.data() : !b.pos_off),
            name, "the shape");
}

void keyed_literal_case(const char *name, const std::vector<Str> &terms, const std::vector<Str> &keys, const std::vector<Str> &pats,
                        int32_t term_lead, int32_t key_lead, int32_t pat_lead) {
    const Literal t(terms, term_lead, true), k(keys, key_lead, true), p(pats, pat_lead, false);
    const auto t_chars = exact(t.chars), k_chars = exact(k.chars), p_chars = exact(p.chars);
    const auto t_off = exact(t.off), k_off = exact(k.off), p_off = exact(p.off);
    fmx::MergedBatch both, ref, m;
    fmx::ValuesBatch bb{}, rb{}, b{};
    std::vector<int32_t> len{-7};  // (what was in it goes)
    require(fmx::merge_literal_batch(p_chars.get(), p_off.get(), p.count, k_chars.get(), k_off.get(), k.count, &both, &bb) == FMX_OK &&
                fmx::merge_literal_batch(both.chars.data(), both.off.data(), k.count + p.count, t_chars.get(), t_off.get(), t.count, &ref, &rb) == FMX_OK,
            name, "the two successive merges refuse");
    require(fmx::merge_keyed_literal_batch(k_chars.get(), k_off.get(), k.count, p_chars.get(), p_off.get(), p.count, t_chars.get(), t_off.get(), t.count,
                                           &m, &b, &len) == FMX_OK,
            name, "the keyed merge refuses");
    same_batch(name, m, b, ref, rb);
    require(len.size() == keys.size() + pats.size(), name, "the count of term_len");
    for (size_t i = 0; i < len.size(); ++i)
        require(len[i] == (int32_t)(i < keys.size() ? keys[i] : pats[i - keys.size()]).size(), name, "a term_len");
    passed(name);
}

void keyed_class_case(const char *name, const std::vector<ClassPat> &terms, const std::vector<ClassPat> &keys, const std::vector<ClassPat> &pats,
                      int32_t lead_alt, int32_t lead_pos) {
    const Class t(terms, lead_alt, lead_pos), k(keys, lead_alt, lead_pos), p(pats, lead_alt, lead_pos);
    const bool no_terms = terms.empty();  // (no terms: the three arrays of the terms are NULL; the keys' are always there)
    const auto t_alt = exact(t.alt), k_alt = exact(k.alt), p_alt = exact(p.alt);
    const auto t_pos = exact(no_terms ? std::vector<int32_t>() : t.pos_off), k_pos = exact(k.pos_off), p_pos = exact(p.pos_off);
    const auto t_off = exact(no_terms ? std::vector<int32_t>() : t.pat_off), k_off = exact(k.pat_off), p_off = exact(p.pat_off);
    const int32_t t_n_pos = no_terms ? 0 : t.n_pos;
    fmx::MergedBatch both, ref, m;
    fmx::ValuesBatch bb{}, rb{}, b{};
    std::vector<int32_t> len{-7};
    require(fmx::merge_class_batch(p_alt.get(), p_pos.get(), p.n_pos, p_off.get(), p.count, k_alt.get(), k_pos.get(), k.n_pos, k_off.get(), k.count, 7,
                                   &both, &bb) == FMX_OK &&
                fmx::merge_class_batch(both.chars.data(), both.pos.data(), (int32_t)both.pos.size() - 1, both.off.data(), k.count + p.count, t_alt.get(),
                                       t_pos.get(), t_n_pos, t_off.get(), t.count, 7, &ref, &rb) == FMX_OK,
            name, "the two successive merges refuse");
    require(fmx::merge_keyed_class_batch(k_alt.get(), k_pos.get(), k.n_pos, k_off.get(), k.count, p_alt.get(), p_pos.get(), p.n_pos, p_off.get(), p.count,
                                         t_alt.get(), t_pos.get(), t_n_pos, t_off.get(), t.count, 7, &m, &b, &len) == FMX_OK,
            name, "the keyed merge refuses");
    same_batch(name, m, b, ref, rb);
    require(len.size() == keys.size() + pats.size(), name, "the count of term_len");
    for (size_t i = 0; i < len.size(); ++i)  // (a position is a character)
        require(len[i] == (int32_t)(i < keys.size() ? keys[i] : pats[i - keys.size()]).size(), name, "a term_len");
    passed(name);
}

bool untouched(const fmx::MergedBatch &m) { return m.chars.empty() && m.pos.empty() && m.off.empty(); }

void accepted(const char *name, int rc) {
    require(rc == FMX_OK && g_code == 0, name, "refused");
    passed(name);
}

void refused(const char *name, int rc, const char *message, const fmx::MergedBatch *m = nullptr) {
    require(rc == FMX_E_ARG && g_code == FMX_E_ARG, name, "not refused with FMX_E_ARG");
    require(g_msg == message, name, "another message");
    require(!m || untouched(*m), name, "the merged batch was written");
    g_code = 0;
    g_msg.clear();
    passed(name);
}

Str str(const char *s) {
    Str v;
    for (; *s; ++s) v.push_back((uint16_t)(unsigned char)*s);
    return v;
}

}  // namespace

int main() {
    const std::vector<Str> terms{str("terminating"), str("blk_")}, pats{str("INFO "), str("x"), {0x20AC, 0xFFFF, 0}};
    literal_case("literal, no terms", {}, pats, 0, 0);
    literal_case("literal, no value patterns", terms, {}, 0, 0);
    literal_case("literal, terms and value patterns", terms, pats, 0, 0);
    literal_case("literal, offsets that start above 0", terms, pats, 2, 3);
    literal_case("literal, empty patterns and empty terms", {{}, str("a"), {}}, {{}, {}, str("bc"), {}}, 1, 0);
    literal_case("literal, nothing but empty strings", std::vector<Str>(1), std::vector<Str>(2), 0, 0);

    const ClassPat info{{'i', 'I'}, {'n', 'N'}, {'f', 'F'}, {'o', 'O'}}, digits{{'0', '1', '2', '3'}, {'7'}};
    class_case("class, terms and value patterns", {digits}, {info, digits}, 0, 0);
    class_case("class, a position without alternatives", {{{'a'}, {}, {'b'}}}, {{{}, {'c', 'd'}}, info}, 0, 0);
    class_case("class, terms only", {info, digits}, {}, 0, 0);
    class_case("class, no terms", {}, {digits, info}, 0, 0);
    class_case("class, a pattern with no positions", {{}, digits}, {info, {}, {}}, 0, 0);
    class_case("class, offsets that start above 0", {digits, {}}, {{{}, {'x'}}, info}, 3, 2);
    class_case("class, positions that start above 0", {digits}, {info}, 3, 0);

    // ---- refusals: offsets --------------------------------------------------------------------------------------------------
    {
        const std::vector<int32_t> good{0, 2, 2, 5}, below{-1, 2, 2, 5}, down{0, 3, 2, 5};
        const auto g = exact(good), b = exact(below), d = exact(down);
        refused("pattern offsets start below 0", fmx::check_literal_batches(b.get(), 3, g.get(), 3), "pattern offsets start below 0");
        refused("term offsets start below 0", fmx::check_literal_batches(g.get(), 3, b.get(), 3), "term offsets start below 0");
        refused("pattern offsets decrease", fmx::check_literal_batches(d.get(), 3, nullptr, 0), "pattern offsets decrease");
        refused("term offsets decrease", fmx::check_literal_batches(g.get(), 3, d.get(), 3), "term offsets decrease");
        require(fmx::check_literal_batches(nullptr, 0, nullptr, 0) == FMX_OK && fmx::check_literal_batches(g.get(), 3, g.get(), 3) == FMX_OK,
                "literal offsets", "good offsets are refused");
        passed("literal offsets in order");
    }
    {
        // 2 patterns over 3 positions over 5 alternatives, the same for the terms
        const std::vector<uint16_t> alts{'a', 'b', 'c', 'd', 'e'};
        const std::vector<int32_t> pos{0, 2, 2, 5}, pos_below{-3, 2, 2, 5}, pos_down{0, 2, 1, 5}, off{0, 1, 3}, off_below{-1, 1, 3}, off_down{0, 2, 1},
            off_behind{0, 1, 4};
        const auto a = exact(alts);
        const auto p = exact(pos), pb = exact(pos_below), pd = exact(pos_down), o = exact(off), ob = exact(off_below), od = exact(off_down),
                   oe = exact(off_behind);
        auto check = [&](const int32_t *pos_off, const int32_t *pat_off, const int32_t *term_pos_off, const int32_t *term_off,
                         const uint16_t *alt, const uint16_t *term_alt) {
            return fmx::check_class_batches(alt, pos_off, 3, pat_off, 2, term_alt, term_pos_off, 3, term_off, 2);
        };
        require(check(p.get(), o.get(), p.get(), o.get(), a.get(), a.get()) == FMX_OK, "class offsets", "good offsets are refused");
        require(fmx::check_class_batches(a.get(), p.get(), 3, o.get(), 2, nullptr, nullptr, 0, nullptr, 0) == FMX_OK, "class offsets", "no terms");
        passed("class offsets in order");
        refused("position offsets start below 0", check(pb.get(), o.get(), p.get(), o.get(), a.get(), a.get()), "position offsets start below 0");
        refused("position offsets decrease", check(pd.get(), o.get(), p.get(), o.get(), a.get(), a.get()), "position offsets decrease");
        refused("class pattern offsets start below 0", check(p.get(), ob.get(), p.get(), o.get(), a.get(), a.get()), "pattern offsets start below 0");
        refused("class pattern offsets decrease", check(p.get(), od.get(), p.get(), o.get(), a.get(), a.get()), "pattern offsets decrease");
        refused("term position offsets start below 0", check(p.get(), o.get(), pb.get(), o.get(), a.get(), a.get()),
                "term position offsets start below 0");
        refused("term position offsets decrease", check(p.get(), o.get(), pd.get(), o.get(), a.get(), a.get()), "term position offsets decrease");
        refused("class term offsets start below 0", check(p.get(), o.get(), p.get(), ob.get(), a.get(), a.get()), "term offsets start below 0");
        refused("class term offsets decrease", check(p.get(), o.get(), p.get(), od.get(), a.get(), a.get()), "term offsets decrease");
        refused("pat_off[n] > n_pos", check(p.get(), oe.get(), p.get(), o.get(), a.get(), a.get()), "pattern offsets end behind the positions");
        refused("term_off[n_terms] > term_n_pos", check(p.get(), o.get(), p.get(), oe.get(), a.get(), a.get()),
                "term offsets end behind the positions");
        // ---- a NULL character array with a positive count
        refused("class, no alternatives of the patterns", check(p.get(), o.get(), p.get(), o.get(), nullptr, a.get()), "bad arguments");
        refused("class, no alternatives of the terms", check(p.get(), o.get(), p.get(), o.get(), a.get(), nullptr), "bad arguments");
    }
    {
        const std::vector<uint16_t> chars{'a', 'b', 'c'};
        const std::vector<int32_t> off{0, 1, 3};
        const auto c = exact(chars);
        const auto o = exact(off);
        fmx::MergedBatch m;
        fmx::ValuesBatch b{};
        refused("literal, no characters of the patterns", fmx::merge_literal_batch(nullptr, o.get(), 2, c.get(), o.get(), 2, &m, &b), "bad arguments",
                &m);
        refused("literal, no characters of the terms", fmx::merge_literal_batch(c.get(), o.get(), 2, nullptr, o.get(), 2, &m, &b), "bad arguments",
                &m);
        require(!b.chars && !b.pat_off, "literal refusals", "the batch was written");
    }
    // ---- refusals: more than 2^31 - 1 in one batch.  The offsets alone say so: nothing behind the pointers is read.
    {
        static uint16_t dummy[1];
        const std::vector<int32_t> huge{0, INT32_MAX}, one{0, 1};
        const auto h = exact(huge), o = exact(one);
        fmx::MergedBatch m;
        fmx::ValuesBatch b{};
        require(fmx::check_literal_batches(h.get(), 1, h.get(), 1) == FMX_OK, "characters in one batch", "the checks refuse");
        refused("more than 2^31 - 1 characters in one batch", fmx::merge_literal_batch(dummy, h.get(), 1, dummy, h.get(), 1, &m, &b),
                "more than 2^31 - 1 characters in one batch", &m);
        require(fmx::check_class_batches(dummy, h.get(), 1, o.get(), 1, dummy, h.get(), 1, o.get(), 1) == FMX_OK, "alternatives in one batch",
                "the checks refuse");
        refused("more than 2^31 - 1 alternatives in one batch",
                fmx::merge_class_batch(dummy, h.get(), 1, o.get(), 1, dummy, h.get(), 1, o.get(), 1, 4, &m, &b),
                "more than 2^31 - 1 alternatives in one batch", &m);
        require(!b.chars && !b.pat_off && !b.pos_off, "2^31 - 1 refusals", "the batch was written");
    }
    // ---- the filter's own arrays
    {
        const std::vector<int32_t> where{-1, 0, 1}, low{-1, -2, 1}, high{0, 1, 2}, none{-1, -1, -1};
        const auto w = exact(where), l = exact(low), hi = exact(high), no = exact(none);
        require(fmx::check_where_of(3, w.get(), 2) == FMX_OK && fmx::check_where_of(0, nullptr, 0) == FMX_OK, "where_of", "good entries are refused");
        refused("where_of below -1", fmx::check_where_of(3, l.get(), 2), "where_of[1] is outside -1 .. q - 1");
        refused("where_of at q", fmx::check_where_of(3, hi.get(), 2), "where_of[2] is outside -1 .. q - 1");
        require(fmx::hits_filter_asked(3, w.get()) && !fmx::hits_filter_asked(3, no.get()) && !fmx::hits_filter_asked(0, nullptr) &&
                    fmx::hits_filter_asked(3, no.get(), 1, INT32_MAX) && fmx::hits_filter_asked(0, nullptr, 0, INT32_MAX - 1),
                "hits_filter_asked", "a wrong answer");
        passed("the filter is asked for");
    }
    // ---- the keyed merges: terms | keys | numbers
    {
        const std::vector<Str> keys{str("user="), str("k")}, nums{str("latency_ms="), str(" took "), {0x20AC}};
        keyed_literal_case("keyed literal, m = 0 and n = 0", {}, {}, {}, 0, 0, 0);
        keyed_literal_case("keyed literal, m = 0 and n = 0 behind terms", terms, {}, {}, 0, 0, 0);
        keyed_literal_case("keyed literal, one empty key and one empty number pattern", {}, std::vector<Str>(1), std::vector<Str>(1), 0, 0, 0);
        keyed_literal_case("keyed literal, no terms", {}, keys, nums, 0, 0, 0);
        keyed_literal_case("keyed literal, terms in front", terms, keys, nums, 0, 0, 0);
        keyed_literal_case("keyed literal, key_off[0] > 0 and pat_off[0] > 0", terms, keys, nums, 1, 4, 2);
        keyed_literal_case("keyed literal, empty strings among the others", {{}, str("a")}, {{}, str("bc"), {}}, {str("d"), {}}, 0, 3, 0);
        const ClassPat user{{'u', 'U'}, {'s', 'S'}, {'e', 'E', 0x212F}, {'r'}, {'=', ':', ' '}};
        keyed_class_case("keyed class, m = 0 and n = 0", {}, {}, {}, 0, 0);
        keyed_class_case("keyed class, one empty key and one empty number pattern", {}, std::vector<ClassPat>(1), std::vector<ClassPat>(1), 0, 0);
        keyed_class_case("keyed class, a key with several alternatives per position, no terms", {}, {user}, {digits}, 0, 0);
        keyed_class_case("keyed class, terms in front", {info}, {user, digits}, {digits, {{'m'}, {'s', 'S'}}}, 0, 0);
        keyed_class_case("keyed class, offsets that start above 0", {info, {}}, {user}, {{{}, {'x'}}, digits}, 3, 2);
        // a NULL pattern array with characters in it
        const std::vector<uint16_t> chars{'a', 'b', 'c'};
        const std::vector<int32_t> off{0, 1, 3};
        const auto c = exact(chars);
        const auto o = exact(off);
        fmx::MergedBatch m;
        fmx::ValuesBatch b{};
        std::vector<int32_t> len;
        refused("keyed literal, no characters of the keys",
                fmx::merge_keyed_literal_batch(nullptr, o.get(), 2, c.get(), o.get(), 2, c.get(), o.get(), 2, &m, &b, &len), "bad arguments", &m);
        refused("keyed literal, no characters of the numbers",
                fmx::merge_keyed_literal_batch(c.get(), o.get(), 2, nullptr, o.get(), 2, c.get(), o.get(), 2, &m, &b, &len), "bad arguments", &m);
        refused("keyed literal, no characters of the terms",
                fmx::merge_keyed_literal_batch(c.get(), o.get(), 2, c.get(), o.get(), 2, nullptr, o.get(), 2, &m, &b, &len), "bad arguments", &m);
        require(!b.chars && !b.pat_off && len.empty(), "keyed refusals", "the batch or term_len was written");
    }
    // ---- the shape of the values and of the numbers, the limits of the hits, term_len, the window of lines: at their edges
    {
        const std::vector<uint16_t> stop64(64, ';'), stop65(65, ';');
        const auto s64 = exact(stop64), s65 = exact(stop65);
        const char *const len_msg = "max_len is outside [1, 64]", *const stop_msg = "the stop set is outside [0, 64] code units";
        refused("max_len 0", fmx::check_values_shape(nullptr, 0, 0), len_msg);
        accepted("max_len 1", fmx::check_values_shape(nullptr, 0, 1));
        accepted("max_len 64", fmx::check_values_shape(nullptr, 0, 64));
        refused("max_len 65", fmx::check_values_shape(nullptr, 0, 65), len_msg);
        refused("n_stop -1", fmx::check_values_shape(s64.get(), -1, 8), stop_msg);
        accepted("n_stop 0", fmx::check_values_shape(nullptr, 0, 8));
        accepted("n_stop 64", fmx::check_values_shape(s64.get(), 64, 8));
        refused("n_stop 65", fmx::check_values_shape(s65.get(), 65, 8), stop_msg);
        refused("n_stop 1 without a stop set", fmx::check_values_shape(nullptr, 1, 8), stop_msg);

        const int64_t two31 = (int64_t)1 << 31, two29 = (int64_t)1 << 29;  // (2^29 windows of 64 code units: 2^35)
        accepted("2^31 - 1 hits", fmx::check_values_hits(two31 - 1, 1));
        refused("2^31 hits", fmx::check_values_hits(two31, 1), "more than 2^31 - 1 hits in one call");
        accepted("2^35 code units", fmx::check_values_hits(two29, 64));
        refused("2^35 code units and one window", fmx::check_values_hits(two29 + 1, 64), "the windows of the hits hold more than 2^35 code units");

        const std::vector<int32_t> pm16{0, 1, 10, 50, 100, 250, 500, 750, 900, 950, 990, 995, 999, 1000, 500, 0}, pm_high{500, 1001};
        std::vector<int32_t> pm17(pm16);
        pm17.push_back(7);
        const auto p16 = exact(pm16), p17 = exact(pm17), ph = exact(pm_high);
        refused("frac_digits -1", fmx::check_numbers_shape(-1, nullptr, 0), "frac_digits is outside [0, 9]");
        accepted("frac_digits 0", fmx::check_numbers_shape(0, nullptr, 0));
        accepted("frac_digits 9", fmx::check_numbers_shape(9, nullptr, 0));
        refused("frac_digits 10", fmx::check_numbers_shape(10, nullptr, 0), "frac_digits is outside [0, 9]");
        accepted("n_permille 16", fmx::check_numbers_shape(3, p16.get(), 16));
        refused("n_permille 17", fmx::check_numbers_shape(3, p17.get(), 17), "n_permille is outside [0, 16]");
        refused("a permille of 1001", fmx::check_numbers_shape(3, ph.get(), 2), "a permille is outside [0, 1000]");

        const std::vector<int32_t> lens{3, 0, 64}, neg{3, 0, -1};
        const auto l = exact(lens), ng = exact(neg);
        accepted("term_len, none negative", fmx::check_term_len(3, l.get()));
        accepted("term_len, none at all", fmx::check_term_len(0, nullptr));
        refused("a negative term_len", fmx::check_term_len(3, ng.get()), "term_len[2] is negative");

        const std::vector<int32_t> where{-1, 0, 1}, high{0, 1, 2};
        const auto w = exact(where), hi = exact(high);
        accepted("the window of one line", fmx::check_where(3, w.get(), 2, 5, 5));
        accepted("every line, no patterns", fmx::check_where(0, nullptr, 0, 0, INT32_MAX));
        refused("a window that starts below 0", fmx::check_where(3, w.get(), 2, -1, 5), "bad arguments");
        refused("a window that ends in front of its start", fmx::check_where(3, w.get(), 2, 6, 5), "the window of lines ends in front of its start");
        refused("where_of at q behind a good window", fmx::check_where(3, hi.get(), 2, 0, 9), "where_of[2] is outside -1 .. q - 1");
    }
    std::printf("merged batch: %d cases ok\n", g_cases);
    return 0;
}
