// san_suffix_children.cpp — the suffix table's deepest level as CHILD LISTS (fmx_device.hpp: DevIndex.suffix_child_rows), as a
// stand-alone program for -fsanitize=address,undefined.  Hashed levels 2 .. D are grown and hashed as build_suffix_table does
// (fm_suffix_extend, fm_suffix_home), level D + 1 becomes child lists by the functions the kernels run (fm_suffix_find,
// fm_suffix_child_sort / _entries / _write; the kernels' atomics are plain stores here), every array exactly as large as the library
// makes it.  Texts: a synthetic log of 2^16 characters (D = 2 and 3), 12 random symbols over 2^20 - 1 characters, and over exactly
// 2^20 (D = 4; rank(size) raises there — Q3 — so strings are dropped for a status: their places are gaps).
//
// The judge of every string is the loop itself — the backward search over the index's own rank(), with no table — and a count of
// the string's occurrences in the text:
//   * every string of 2 .. D + 1 characters that occurs and whose search raises no status looks up to the loop's interval, which
//     holds as many rows as the string has occurrences; one whose search raises a status misses (the loop has to run);
//   * 10,000 strings of D + 1 characters that do not occur miss: half of them an occurring string of D characters with a code
//     behind it that never follows it, half random;
//   * holes: lists rebuilt with every third string of a parent removed (as if dropped for a status) flag the gap; the removed
//     strings miss, the kept ones still answer their intervals.
// Prints one " ok: " line per index; exit code 0 = clean.
#include "../hostsim.cpp"

#include <cstdio>
#include <string>
#include <unordered_map>

#include "fmx_model.hpp"

extern "C" int fmx_synth_log(uint64_t seed, int32_t n, uint16_t *out);

namespace {

uint64_t g_rng = 88172645463325252ull;
uint32_t below(uint32_t n) {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng % n);
}

#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                      \
            printf("\n");                             \
            return false;                             \
        }                                             \
    } while (0)

struct Table {
    std::vector<SuffixSlot> slots;
    std::vector<uint32_t> rows;
    std::vector<uint8_t> codes;
    std::vector<SuffixSlot> kids;  // level D + 1 as fm_suffix_extend made it
    uint32_t holes = 0, parents_without_interval = 0;
};

// the hashed levels 2 .. depth, and the strings of depth + 1 codes
void grow_hashed(DevIndex &ix, int depth, Table &t) {
    std::vector<SuffixSlot> level;
    std::vector<std::vector<SuffixSlot>> levels;
    for (int32_t c = 1; c + 1 < ix.n_c && c < ix.wt_sigma; ++c)
        if (ix.C[c] < ix.C[c + 1]) level.push_back(SuffixSlot{(uint64_t)(uint32_t)c, (uint32_t)ix.C[c], (uint32_t)ix.C[c + 1]});
    for (int d = 1; d <= depth; ++d) {
        std::vector<SuffixSlot> next;
        for (const SuffixSlot &parent : level)
            for (int32_t c = 1; c < ix.wt_sigma; ++c) {
                if (c + 1 >= ix.n_c) continue;
                SuffixSlot child;
                if (fm_suffix_extend(ix, parent, d, c, 8, child)) next.push_back(child);
            }
        level.swap(next);
        if (d < depth) levels.push_back(level);
    }
    t.kids = level;
    uint64_t total = 0;
    for (const auto &l : levels) total += l.size();
    uint32_t slots = 1024;
    while (slots < 2 * total) slots <<= 1;
    int log2_slots = 0;
    while ((1u << log2_slots) < slots) ++log2_slots;
    t.slots.assign(slots, SuffixSlot{kSuffixEmpty, 0xffffffffu, 0xffffffffu});  // (the library presets every byte to 0xff)
    ix.suffix_key_bits = 8;
    ix.suffix_chars = depth;
    ix.suffix_shift = (uint32_t)(64 - (log2_slots - kSuffixGroupLog2));
    ix.suffix_mask = slots - 1;
    for (size_t i = 0; i < levels.size(); ++i)
        for (const SuffixSlot &e : levels[i]) {
            uint32_t h = fm_suffix_home(ix, e.key, (int)i + 2);
            while (t.slots[h].key != kSuffixEmpty) h = (h + kSuffixGroup) & ix.suffix_mask;
            t.slots[h] = e;
        }
    ix.suffix_table = t.slots.data();
    ix.suffix_child_rows = nullptr;
    ix.suffix_child_codes = nullptr;
}

// level depth + 1 as child lists (grow_child_lists of fmx_api.cpp with the kernels' steps in line); `keep`: false = the string is left
// out, as if it had been dropped for a status
template <class Keep>
void grow_children(DevIndex &ix, int depth, Table &t, Keep keep) {
    const uint32_t slots = (uint32_t)t.slots.size();
    std::vector<std::vector<SuffixSlot>> runs(slots);
    for (const SuffixSlot &kid : t.kids) {
        if (!keep(kid)) continue;
        Quad q;
        const uint64_t parent = kid.key >> 8;
        uint32_t h = fm_suffix_find(ix, parent, depth, q);
        if (h == kSuffixNoSlot) {  // k_suffix_child_parents: a slot without an interval
            h = fm_suffix_home(ix, parent, depth);
            while (t.slots[h].key != kSuffixEmpty) h = (h + kSuffixGroup) & ix.suffix_mask;
            t.slots[h] = SuffixSlot{parent, 0, 0};
            ++t.parents_without_interval;
        }
        runs[h].push_back(kid);
    }
    std::vector<uint32_t> first(slots, 0);
    uint32_t entries = 0;
    for (uint32_t h = 0; h < slots; ++h) {
        if (runs[h].empty()) continue;
        // (k_suffix_child_place leaves a run in any order)
        for (size_t i = runs[h].size(); i > 1; --i) std::swap(runs[h][i - 1], runs[h][below((uint32_t)i)]);
        fm_suffix_child_sort(runs[h].data(), (uint32_t)runs[h].size());
        first[h] = entries;
        entries += fm_suffix_child_entries(runs[h].data(), (uint32_t)runs[h].size());
    }
    // the rows, and the codes + kSuffixChildPad bytes, of exactly the library's sizes (two vectors here: a step past either is a report)
    t.rows.assign(entries, 0);
    t.codes.assign((size_t)entries + kSuffixChildPad, 0);
    for (uint32_t h = 0; h < slots; ++h) {
        if (runs[h].empty()) continue;
        fm_suffix_child_write(runs[h].data(), (uint32_t)runs[h].size(), first[h], t.rows.data(), t.codes.data());
        t.slots[h].key |= (uint64_t)(first[h] + 1u) << kSuffixChildShift;
    }
    t.holes = 0;
    for (uint32_t r : t.rows) t.holes += (r & kSuffixChildHole) != 0;
    ix.suffix_chars = depth + 1;
    ix.suffix_child_rows = t.rows.data();
    ix.suffix_child_codes = t.codes.data();
}

// the loop over the string's codes (code[j] = j characters before its end): FM:455-474 with no table
void loop_interval(const DevIndex &ix, uint64_t key, int len, int32_t &start, int32_t &end, int &status) {
    status = ST_OK;
    const int32_t c0 = (int32_t)(key & 0xff);
    start = ix.C[c0];
    end = ix.C[c0 + 1];
    for (int j = 1; j < len && start < end; ++j) {
        const int32_t c = (int32_t)((key >> (8 * j)) & 0xff);
        const int32_t s2 = wt_rank_folded(ix, ix.inv_global, (uint32_t)start, c, status);
        const int32_t e2 = wt_rank_folded(ix, ix.inv_global, (uint32_t)end, c, status);
        start = s2;
        end = e2;
    }
}

bool check_index(const char *what, const std::vector<uint16_t> &text, int depth) {
    fmx::FmModel m;
    std::string err;
    std::vector<uint8_t> blob;
    CHECK(!fmx::build_model(text.data(), (int32_t)text.size(), 32, true, m, err) && !fmx::flatten_model(m, blob, err), "build: %s",
          err.c_str());
    DevIndex ix = make_index(blob.data());
    CHECK(ix.wt_sigma <= 256 && depth * 8 <= kSuffixChildShift, "not a text for child lists");
    Table t;
    grow_hashed(ix, depth, t);
    grow_children(ix, depth, t, [](const SuffixSlot &) { return true; });
    CHECK(!t.kids.empty() && t.rows.size() > t.kids.size(), "no level %d", depth + 1);

    // every string of 2 .. depth + 1 characters that occurs, with its occurrences
    std::vector<uint8_t> code(text.size());
    for (size_t i = 0; i < text.size(); ++i) code[i] = (uint8_t)fm_map(ix, text[i]);
    int64_t checked = 0, dropped = 0;
    std::unordered_map<uint64_t, uint32_t> deepest, below_deepest;
    for (int len = 2; len <= depth + 1; ++len) {
        std::unordered_map<uint64_t, uint32_t> occurs;
        for (size_t i = 0; i + len <= text.size(); ++i) {
            uint64_t key = 0;
            for (int j = 0; j < len; ++j) key |= (uint64_t)code[i + len - 1 - j] << (8 * j);
            ++occurs[key];
        }
        for (const auto &kv : occurs) {
            int32_t s = 0, e = 0, ts = -1, te = -1, back = -1;
            int status = ST_OK;
            loop_interval(ix, kv.first, len, s, e, status);
            const bool found = fm_suffix_lookup(ix, kv.first, len, ts, te, back);
            if (status == ST_OK && s < e) {
                CHECK(found && ts == s && te == e && back == len - 1, "%s: string %llx of %d codes: table %d [%d, %d), loop [%d, %d)", what,
                      (unsigned long long)kv.first, len, (int)found, ts, te, s, e);
                CHECK((uint32_t)(e - s) == kv.second, "%s: string %llx: %d rows, %u occurrences", what, (unsigned long long)kv.first, e - s,
                      kv.second);
                ++checked;
            } else {
                CHECK(!found, "%s: string %llx of %d codes raises status %d in the loop and is in the table", what,
                      (unsigned long long)kv.first, len, status);
                ++dropped;
            }
        }
        if (len == depth + 1) deepest.swap(occurs);
        if (len == depth) below_deepest.swap(occurs);
    }
    // every string the level was grown with is one that occurs
    CHECK(t.kids.size() + (size_t)dropped >= deepest.size() && t.kids.size() <= deepest.size(), "%s: %zu strings grown, %zu occur", what,
          t.kids.size(), deepest.size());

    // strings that do not occur
    std::vector<uint64_t> parents;
    for (const auto &kv : below_deepest) parents.push_back(kv.first);
    int absent = 0, absent_with_parent = 0;
    for (int guard = 0; absent < 10000 && guard < 10000000; ++guard) {
        uint64_t key;
        const bool from_parent = absent % 2 == 0;
        if (from_parent) {
            key = (parents[below((uint32_t)parents.size())] << 8) | (1 + below((uint32_t)ix.wt_sigma - 1));
        } else {
            key = 0;
            for (int j = 0; j <= depth; ++j) key |= (uint64_t)(1 + below((uint32_t)ix.wt_sigma - 1)) << (8 * j);
        }
        if (deepest.count(key)) continue;
        int32_t ts = -1, te = -1, back = -1;
        CHECK(!fm_suffix_lookup(ix, key, depth + 1, ts, te, back) && ts == -1 && te == -1 && back == -1,
              "%s: absent string %llx found: [%d, %d)", what, (unsigned long long)key, ts, te);
        ++absent;
        absent_with_parent += from_parent;
    }
    CHECK(absent == 10000 && absent_with_parent == 5000, "%s: only %d absent strings", what, absent);
    const uint32_t natural_holes = t.holes, no_interval = t.parents_without_interval;

    // holes: every third string of the level left out
    Table h;
    grow_hashed(ix, depth, h);
    size_t turn = 0;
    std::unordered_map<uint64_t, int> left_out;
    grow_children(ix, depth, h, [&](const SuffixSlot &kid) {
        const bool out = ++turn % 3 == 0;
        if (out) left_out[kid.key] = 1;
        return !out;
    });
    CHECK(h.holes > 0, "%s: no hole among %zu strings left out", what, left_out.size());
    for (const SuffixSlot &kid : h.kids) {
        int32_t ts = -1, te = -1, back = -1;
        const bool found = fm_suffix_lookup(ix, kid.key, depth + 1, ts, te, back);
        if (left_out.count(kid.key))
            CHECK(!found, "%s: string %llx left out and found", what, (unsigned long long)kid.key);
        else
            CHECK(found && (uint32_t)ts == kid.start && (uint32_t)te == kid.end, "%s: string %llx beside a hole: [%d, %d), grown [%u, %u)",
                  what, (unsigned long long)kid.key, ts, te, kid.start, kid.end);
    }
    // a flagged entry repeats the code of the string in front of it, whose end it is
    for (size_t i = 0; i < h.rows.size(); ++i)
        if (h.rows[i] & kSuffixChildHole)
            CHECK(i > 0 && !(h.rows[i - 1] & kSuffixChildHole) && h.codes[i] == h.codes[i - 1] && h.codes[i] != 0, "%s: hole at %zu", what, i);
    printf(" ok: %s: hashed to %d, %zu strings of %d codes in %zu entries (%u gaps, %u parents without an interval), %lld strings checked, "
           "%lld raise a status; with every third left out: %u gaps\n",
           what, depth, t.kids.size(), depth + 1, t.rows.size(), natural_holes, no_interval, (long long)checked, (long long)dropped, h.holes);
    return true;
}

}  // namespace

int main() {
    std::vector<uint16_t> log_text(1 << 16);
    fmx_synth_log(42, (int32_t)log_text.size(), log_text.data());
    std::vector<uint16_t> random_text((1 << 20) - 1), random_full(1 << 20);
    for (auto &c : random_text) c = (uint16_t)(33 + below(12));
    for (auto &c : random_full) c = (uint16_t)(33 + below(12));
    bool ok = check_index("log, 2^16 characters, D = 2", log_text, 2);
    ok = ok && check_index("log, 2^16 characters, D = 3", log_text, 3);
    ok = ok && check_index("12 symbols, 2^20 - 1 characters, D = 4", random_text, 4);
    ok = ok && check_index("12 symbols, 2^20 characters, D = 4", random_full, 4);
    return ok ? 0 : 1;
}
