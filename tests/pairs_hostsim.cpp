// pairs_hostsim.cpp — TEST-ONLY host build of the device code of "statistics and line counts by the values of two fields of the same
// line" (fmx_pairs_of_first_hits_dev): index4j_amd/csrc/fmx_hit_pairs.hpp's fm_pair_key and its three readers, fm_pair_slot_key,
// fm_pair_head, fm_pair_run_length, fm_pair_first_slot and the host checks fm_pair_args_bad — with fmx_hit_by.hpp's fm_by_find and
// fm_by_row_pattern — driven by a mirror of the kernels of fmx_hit_pairs.hip with the lanes run one after the other: std::stable_sort
// for rocPRIM's sort, running sums for its scans.  Every array has exactly the size the contract gives it, so that the sanitized
// build sees a store behind one.  g++ compiles the header's functions as plain C++, so the CPU suite checks the source of those
// FUNCTIONS (tests/test_field_pairs_cpu.py); the kernels' own route runs in tests/test_gpu_field_pairs.py only.  Never part of
// libfmx.so.
//
// A stand-alone program:
//   pairs_hostsim self          the per-item functions and the host checks at their edges; exit status 4 where one fails
//   pairs_hostsim run IN OUT    IN   int64 {m, c, n_slots, F}, int64 first_off[m + 1] (first_off[0] may be non-zero: entries in front
//                                    of it are no first hits), int32 first_lines[F], int32 group_of_first[F], int64 val_off[m + 1],
//                                    int32 pair_a[c], int32 pair_b[c]
//                               OUT  int64 pair_off[c + 1], int32 pair_group_a[R], int32 pair_group_b[R], int32 pair_lines[R],
//                                    int64 joined_off[c + 1], int32 joined_lines[J], int32 joined_group[J]
//                               exit status 5: fm_pair_args_bad refuses the call
#include "../index4j_amd/csrc/fmx_hit_pairs.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

using namespace fmx;

namespace {

template <class T>
bool get(FILE *f, std::vector<T> &v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}
template <class T>
void put(FILE *f, const T *v, size_t count) {
    if (count) fwrite(v, sizeof(T), count, f);
}

int g_failed = 0;
#define EXPECT(cond)                                           \
    do {                                                       \
        if (!(cond)) {                                         \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
            g_failed = 1;                                      \
        }                                                      \
    } while (0)

void self_checks() {
    // the key: pair above ga above gb, at every width up to 64 bits in all
    for (const int32_t a_bits : {1, 7, 31})
        for (const int32_t b_bits : {1, 12, 31}) {
            const int32_t ga = (int32_t)((((uint64_t)1 << a_bits) - 1) & 0x7fffffff), gb = (int32_t)((((uint64_t)1 << b_bits) - 1) & 0x7fffffff);
            const int32_t pair = a_bits + b_bits == 62 ? 2 : 5;  // (2 bits are left beside 31 + 31: c <= 3, the pair below it)
            const uint64_t k = fm_pair_key(pair, ga, gb, a_bits, b_bits);
            EXPECT(fm_pair_key_pair(k, a_bits, b_bits) == pair && fm_pair_key_a(k, a_bits, b_bits) == ga && fm_pair_key_b(k, b_bits) == gb);
            EXPECT(fm_pair_key(pair, ga, gb, a_bits, b_bits) < fm_pair_key(pair + 1, 0, 0, a_bits, b_bits));
            EXPECT(fm_pair_key(pair, 0, gb, a_bits, b_bits) < fm_pair_key(pair, 1, 0, a_bits, b_bits));
            EXPECT(fm_pair_key(pair, 1, 0, a_bits, b_bits) < fm_pair_key(pair, 1, 1, a_bits, b_bits));
        }
    {  // a slot's key: the partner by one lower bound; no partner, and a group that is no group, give the pair c
        const int32_t lines[] = {2, 5, 9, /* b: */ 1, 5, 9, 12}, group[] = {0, 1, 7, /* b: */ 3, 2, -1, 0};
        const int32_t c = 4, ab = 3, bb = 2;
        const uint64_t none = fm_pair_key(c, 0, 0, ab, bb);
        int32_t line = -1;
        EXPECT(fm_pair_slot_key(lines, group, 0, 3, 7, 1, c, 2, 4, ab, bb, &line) == none && line == 2);                        // line 2: no key of b
        EXPECT(fm_pair_slot_key(lines, group, 1, 3, 7, 1, c, 2, 4, ab, bb, &line) == fm_pair_key(1, 1, 2, ab, bb) && line == 5);  // line 5: (1, 2)
        EXPECT(fm_pair_slot_key(lines, group, 2, 3, 7, 1, c, 8, 4, ab, bb, &line) == none && line == 9);                        // b's group is -1
        EXPECT(fm_pair_slot_key(lines, group, 1, 3, 7, 1, c, 1, 4, ab, bb, &line) == none);                                     // a's group 1 of 1
        EXPECT(fm_pair_slot_key(lines, group, 1, 3, 7, 1, c, 2, 2, ab, bb, &line) == none);                                     // b's group 2 of 2
        EXPECT(fm_pair_slot_key(lines, group, 1, 3, 3, 1, c, 2, 4, ab, bb, &line) == none);                                     // an empty b-side
        EXPECT(fm_pair_slot_key(lines, group, 1, 0, 3, 0, c, 2, 2, ab, bb, &line) == fm_pair_key(0, 1, 1, ab, bb));              // a == b
    }
    {  // heads, run lengths, the first slot of a pair
        const int32_t c = 3, ab = 2, bb = 2;
        const uint64_t keys[] = {fm_pair_key(0, 1, 1, ab, bb), fm_pair_key(0, 1, 1, ab, bb), fm_pair_key(0, 2, 0, ab, bb), fm_pair_key(2, 0, 0, ab, bb),
                                 fm_pair_key(2, 0, 0, ab, bb), fm_pair_key(2, 0, 0, ab, bb), fm_pair_key(3, 0, 0, ab, bb), fm_pair_key(3, 0, 0, ab, bb)};
        const bool head[] = {true, false, true, true, false, false, false, false};
        for (int64_t i = 0; i < 8; ++i) EXPECT(fm_pair_head(keys, i, c, ab, bb) == head[i]);
        EXPECT(fm_pair_run_length(keys, 8, 0) == 2 && fm_pair_run_length(keys, 8, 2) == 1 && fm_pair_run_length(keys, 8, 3) == 3);
        EXPECT(fm_pair_run_length(keys, 6, 3) == 3);  // a run that ends the array
        EXPECT(fm_pair_first_slot(keys, 8, 0, ab, bb) == 0 && fm_pair_first_slot(keys, 8, 1, ab, bb) == 3 && fm_pair_first_slot(keys, 8, 2, ab, bb) == 3);
        EXPECT(fm_pair_first_slot(keys, 8, 3, ab, bb) == 6 && fm_pair_first_slot(keys, 6, 3, ab, bb) == 6);
    }
    {  // the host checks
        const int64_t val_off[] = {0, 3, 3, 10}, down[] = {0, 3, 2, 10}, below[] = {-1, 3, 3, 10};
        const int32_t pa[] = {0, 2, 1}, pb[] = {2, 2, 0}, bad[] = {0, 3, 1}, neg[] = {0, -1, 1};
        int32_t ab = 0, bb = 0;
        EXPECT(fm_pair_args_bad(3, val_off, 3, pa, pb, 100, &ab, &bb) == 0 && ab == 3 && bb == 3);  // fm_bits(7), fm_bits(7)
        EXPECT(fm_pair_args_bad(0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr) == 0);
        EXPECT(fm_pair_args_bad(3, val_off, -1, pa, pb, 0, nullptr, nullptr) == 1 && fm_pair_args_bad(0, val_off, 3, pa, pb, 0, nullptr, nullptr) == 1);
        EXPECT(fm_pair_args_bad(3, val_off, 3, nullptr, pb, 0, nullptr, nullptr) == 1 && fm_pair_args_bad(3, val_off, 3, pa, nullptr, 0, nullptr, nullptr) == 1);
        EXPECT(fm_pair_args_bad(3, val_off, 3, bad, pb, 0, nullptr, nullptr) == 2 && fm_pair_args_bad(3, val_off, 3, pa, neg, 0, nullptr, nullptr) == 2);
        EXPECT(fm_pair_args_bad(3, nullptr, 3, pa, bad, 0, nullptr, nullptr) == 2 && fm_pair_args_bad(3, nullptr, 3, pa, pb, 0, nullptr, nullptr) == 0);
        EXPECT(fm_pair_args_bad(3, down, 3, pa, pb, 0, nullptr, nullptr) == 3 && fm_pair_args_bad(3, below, 3, pa, pb, 0, nullptr, nullptr) == 3);
        EXPECT(fm_pair_args_bad(3, val_off, 3, pa, pb, -1, nullptr, nullptr) == 4);
        EXPECT(fm_pair_args_bad(3, val_off, 3, pa, pb, 0x7fffffff, nullptr, nullptr) == 0 && fm_pair_args_bad(3, val_off, 3, pa, pb, 0x80000000LL, nullptr, nullptr) == 4);
        // 31 + 31 bits of groups: two bits are left for the pair, c <= 3
        const int64_t wide[] = {0, 0x7fffffff, 0xfffffffeLL}, huge[] = {0, 0x80000000LL, 0x80000001LL};
        const int32_t a4[] = {0, 0, 0, 0}, b4[] = {1, 1, 1, 1};
        EXPECT(fm_pair_args_bad(2, wide, 3, a4, b4, 10, &ab, &bb) == 0 && ab == 31 && bb == 31);
        EXPECT(fm_pair_args_bad(2, wide, 4, a4, b4, 10, nullptr, nullptr) == 5);
        EXPECT(fm_pair_args_bad(2, wide, 4, a4, a4, 10, nullptr, nullptr) == 5 && fm_pair_args_bad(2, huge, 1, a4, b4, 10, nullptr, nullptr) == 3);
        const int64_t none[] = {0, 0, 0};
        EXPECT(fm_pair_args_bad(2, none, 4, a4, b4, 10, &ab, &bb) == 0 && ab == 1 && bb == 1);  // no group at all: one bit each
    }
}

int run(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) return 2;
    std::vector<int64_t> head, first_off, val_off;
    std::vector<int32_t> first_lines, group_of_first, pair_a, pair_b;
    if (!get(f, head, 4)) return 2;
    const int32_t m = (int32_t)head[0], c = (int32_t)head[1];
    const int64_t n_slots = head[2], F = head[3];
    if (!get(f, first_off, (size_t)m + 1) || !get(f, first_lines, (size_t)F) || !get(f, group_of_first, (size_t)F) || !get(f, val_off, (size_t)m + 1) ||
        !get(f, pair_a, (size_t)c) || !get(f, pair_b, (size_t)c))
        return 2;
    fclose(f);
    int32_t a_bits = 1, b_bits = 1;
    if (fm_pair_args_bad(m, val_off.data(), c, pair_a.data(), pair_b.data(), n_slots, &a_bits, &b_bits)) return 5;
    const size_t S = (size_t)n_slots, C = (size_t)c;
    // k_pair_lens and its scan
    std::vector<int64_t> slot_off(C + 1, 0);
    for (size_t j = 0; j < C; ++j) slot_off[j + 1] = slot_off[j] + first_off[(size_t)pair_a[j] + 1] - first_off[(size_t)pair_a[j]];
    // k_pair_keys
    std::vector<uint64_t> keys(S);
    std::vector<uint32_t> slots(S);
    std::vector<int32_t> line_of(S);
    const uint64_t no_pair = fm_pair_key(c, 0, 0, a_bits, b_bits);
    for (int64_t s = 0; s < n_slots; ++s) {
        uint64_t key = no_pair;
        int32_t line = 0;
        if (s < slot_off[C]) {
            const int32_t j = fm_by_row_pattern(slot_off.data(), c, s), a = pair_a[(size_t)j], b = pair_b[(size_t)j];
            key = fm_pair_slot_key(first_lines.data(), group_of_first.data(), first_off[(size_t)a] + (s - slot_off[(size_t)j]), first_off[(size_t)b],
                                   first_off[(size_t)b + 1], j, c, val_off[(size_t)a + 1] - val_off[(size_t)a], val_off[(size_t)b + 1] - val_off[(size_t)b],
                                   a_bits, b_bits, &line);
        }
        keys[(size_t)s] = key;
        slots[(size_t)s] = (uint32_t)s;
        line_of[(size_t)s] = line;
    }
    // the stable sort of (key, slot)
    std::vector<size_t> order(S);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return keys[x] < keys[y]; });
    std::vector<uint64_t> skeys(S);
    std::vector<uint32_t> sslots(S);
    for (size_t i = 0; i < S; ++i) skeys[i] = keys[order[i]], sslots[i] = slots[order[i]];
    // k_pair_heads and its scan
    std::vector<int32_t> headf(S + 1, 0), pos(S + 1, 0);
    for (int64_t i = 0; i < n_slots; ++i) headf[(size_t)i] = fm_pair_head(skeys.data(), i, c, a_bits, b_bits) ? 1 : 0;
    for (size_t i = 0; i < S; ++i) pos[i + 1] = pos[i] + headf[i];
    // k_pair_store: the outputs have room for n_slots and not one entry more
    std::vector<int64_t> pair_off(C + 1), joined_off(C + 1);
    std::vector<int32_t> pga(S), pgb(S), plines(S), joined_lines(S), joined_group(S);
    for (int64_t i = 0; i < n_slots; ++i)
        if (headf[(size_t)i]) {
            const size_t r = (size_t)pos[(size_t)i];
            pga.at(r) = fm_pair_key_a(skeys[(size_t)i], a_bits, b_bits);
            pgb.at(r) = fm_pair_key_b(skeys[(size_t)i], b_bits);
            plines.at(r) = (int32_t)fm_pair_run_length(skeys.data(), n_slots, i);
        }
    for (int32_t j = 0; j <= c; ++j) pair_off[(size_t)j] = pos[(size_t)fm_pair_first_slot(skeys.data(), n_slots, j, a_bits, b_bits)];
    // k_pair_back and the scan of the flags in slot order
    std::vector<int32_t> pair_of(S, -7), flag(S + 1, 0), at(S + 1, 0);
    for (int64_t i = 0; i < n_slots; ++i) {
        const int32_t j = fm_pair_key_pair(skeys[(size_t)i], a_bits, b_bits);
        const uint32_t s = sslots[(size_t)i];
        flag[s] = j < c ? 1 : 0;
        if (j < c) pair_of[s] = (int32_t)(pos[(size_t)i] + headf[(size_t)i] - 1 - pair_off[(size_t)j]);
    }
    for (size_t s = 0; s < S; ++s) at[s + 1] = at[s] + flag[s];
    // k_pair_compact
    for (size_t s = 0; s < S; ++s)
        if (flag[s]) {
            joined_lines.at((size_t)at[s]) = line_of[s];
            joined_group.at((size_t)at[s]) = pair_of[s];
        }
    for (size_t j = 0; j <= C; ++j) joined_off[j] = at[(size_t)(slot_off[j] < n_slots ? slot_off[j] : n_slots)];

    FILE *o = fopen(out_path, "wb");
    if (!o) return 2;
    const size_t R = (size_t)pair_off[C], J = (size_t)joined_off[C];
    put(o, pair_off.data(), C + 1);
    put(o, pga.data(), R);
    put(o, pgb.data(), R);
    put(o, plines.data(), R);
    put(o, joined_off.data(), C + 1);
    put(o, joined_lines.data(), J);
    put(o, joined_group.data(), J);
    fclose(o);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "self")) {
        self_checks();
        return g_failed ? 4 : 0;
    }
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    fprintf(stderr, "usage: pairs_hostsim self | run IN OUT\n");
    return 1;
}
