// numbers_hostsim.cpp — TEST-ONLY host build of the device code of "statistics of the number behind a pattern, per bucket of lines"
// (fmx_numbers_of_hits_dev): index4j_amd/csrc/fmx_hit_numbers.hpp's fm_num_parse, fm_num_code, fm_num_segment, fm_num_pct_index,
// fm_num_scan_between, fm_num_sum128 and fm_num_permille_bad — with fm_val_window for a hit's window, fm_hit_tile / fm_hit_pattern
// for its pattern, fm_line_of over fences and fm_hist_bucket for its bucket — driven by a mirror of the stages of
// fmx_hit_numbers.hip with the lanes run one after the other: k_num_ranges' tile loop, k_num_parse over the windows the caller
// hands in (the judge's: the oracle's extract), std::stable_sort twice for rocPRIM's two sorts, running sums for its scans,
// k_num_rows, k_num_tails.  The rows are checked against sums and sorted lists kept hit by hit in 128-bit arithmetic.  g++ compiles
// the header's functions as plain C++, so the CPU suite checks the source of those FUNCTIONS (tests/test_number_stats_cpu.py).  The
// kernels' own route runs in tests/test_gpu_number_stats.py only.  Never part of libfmx.so.
//
// A stand-alone program:
//   numbers_hostsim self            the per-item functions at their edges (below); exit status 4 and a line on stderr where one fails
//   numbers_hostsim parse IN OUT    IN   int64 {windows, frac_digits}, int64 win_off[windows + 1], uint16 win[win_off[windows]]
//                                   OUT  int32 kind[windows], int64 value[windows]
//   numbers_hostsim stats IN OUT    IN   int64 {n, n_hits, count, max_fences, n_edges, P, frac_digits, text_len}, int32 T[count],
//                                        int32 term_len[n], int64 hit_off[n + 1], int32 locs[n_hits], int32 edges[n_edges] (none:
//                                        B = 1), int32 permille[P], int64 win_off[n_hits + 1], uint16 win[win_off[n_hits]]
//                                   OUT  int32 count[n * B], uint64 sum_lo[n * B], uint64 sum_hi[n * B], int64 min[n * B], int64
//                                        max[n * B], int64 pct[n * B * P], int32 not_number[n], int32 overflow[n], int32
//                                        start[n_hits], int32 stop[n_hits]
// Exit status 3: the rows off the sorted order and the rows kept hit by hit disagree.
#include "../index4j_amd/csrc/fmx_hit_filter.hpp"
#include "../index4j_amd/csrc/fmx_hit_numbers.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

using namespace fmx;

namespace {

template <class T>
bool get(FILE *f, std::vector<T> &v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}
template <class T>
void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int g_failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
            g_failed = 1;                                              \
        }                                                              \
    } while (0)

int32_t parse(const std::string &s, int32_t F, int64_t &v) {
    std::vector<uint16_t> w(s.begin(), s.end());
    w.push_back('7');  // (a digit BEHIND the window: never read)
    return fm_num_parse(w.data(), (int32_t)s.size(), F, v);
}
bool is(const std::string &s, int32_t F, int64_t want) {
    int64_t v = -1;
    return parse(s, F, v) == kNumOk && v == want;
}
bool fails(const std::string &s, int32_t F, int32_t kind) {
    int64_t v = -1;
    return parse(s, F, v) == kind && v == 0;
}

void self_checks() {
    const int64_t p10[] = {1, 10, 100, 1000, 10000, 100000, 1000000, 10000000, 100000000, 1000000000};
    for (int32_t k = 0; k <= kNumFracMax; ++k) EXPECT(fm_num_pow10(k) == p10[k]);
    // the parser table, each case at F = 0, 3, 9
    for (const int32_t F : {0, 3, 9}) {
        const int64_t S = fm_num_pow10(F);
        EXPECT(is("0", F, 0) && is("007", F, 7 * S) && is("12", F, 12 * S) && is("12 ", F, 12 * S) && is("12x.5", F, 12 * S));
        EXPECT(is("12.5", F, 12 * S + 5 * S / 10) && is("1.25", F, S + 25 * S / 100) && is("1.", F, S) && is("1..5", F, S) && is("1.x", F, S));
        EXPECT(is("1.2345678901", F, F == 0 ? 1 : F == 3 ? 1234 : 1234567890));  // truncated, not rounded
        EXPECT(is("1.9999999999", F, F == 0 ? 1 : F == 3 ? 1999 : 1999999999));
        EXPECT(fails(".5", F, kNumNotNumber) && fails("x", F, kNumNotNumber) && fails("", F, kNumNotNumber) && fails("-1", F, kNumNotNumber));
        EXPECT(fails(" 1", F, kNumNotNumber) && fails("+1", F, kNumNotNumber));
        if (F == 0) EXPECT(is("9223372036854775807", F, kNumValueMax) && is("9223372036854775807.9", F, kNumValueMax));
        if (F != 0) EXPECT(fails("9223372036854775807", F, kNumOverflow));
        EXPECT(fails("9223372036854775808", F, kNumOverflow) && fails(std::string(20, '9'), F, kNumOverflow));
        EXPECT(fails("18446744073709551616", F, kNumOverflow) && fails("18446744073709551617.5", F, kNumOverflow));  // (past 2^64 too)
        if (F == 9) EXPECT(is("9223372036.854775807", F, kNumValueMax) && fails("9223372036.854775808", F, kNumOverflow));
        if (F == 9) EXPECT(fails("9223372037", F, kNumOverflow) && is("9223372036", F, 9223372036000000000LL));
        if (F == 3) EXPECT(is("9223372036854775.807", F, kNumValueMax) && fails("9223372036854775.808", F, kNumOverflow));
        EXPECT(fails(std::string(31, '0') + "7", F, kNumOverflow));         // D == 32: the run fills the window
        EXPECT(fails(std::string(32, '0'), F, kNumOverflow));
        EXPECT(is(std::string(30, '0') + "7 ", F, 7 * S) && is(std::string(30, '0') + "7", F, 7 * S));  // D == 31, with and without a unit behind
        EXPECT(is(std::string(29, '0') + "7.5", F, 7 * S + 5 * S / 10));  // the fraction's digit is the window's last unit
        EXPECT(is(std::string(30, '0') + "7.", F, 7 * S));                 // the '.' is: no fraction digit can follow
        EXPECT(is("123", F, 123 * S) && is("12", F, 12 * S));             // a run cut by the end of the text: the shorter number
    }
    // units beyond U+007F are no digits, whatever their low byte
    {
        const uint16_t w[] = {'4', 0x0135, '5'}, full[] = {0xFF11, '1'};
        int64_t v;
        EXPECT(fm_num_parse(w, 3, 0, v) == kNumOk && v == 4 && fm_num_parse(full, 2, 0, v) == kNumNotNumber);
        EXPECT(fm_num_parse(w, 0, 0, v) == kNumNotNumber && fm_num_parse(nullptr, 0, 3, v) == kNumNotNumber);  // a window clipped to nothing
    }
    // the window: fm_val_window at max_len = 32, clipped at textLength
    {
        int32_t s, e;
        fm_val_window(10, 5, kNumWindow, 100, s, e);
        EXPECT(s == 15 && e == 47);
        fm_val_window(90, 5, kNumWindow, 100, s, e);
        EXPECT(s == 95 && e == 100);
        fm_val_window(96, 4, kNumWindow, 100, s, e);
        EXPECT(s == 100 && e == 100);
        fm_val_window(96, INT32_MAX, kNumWindow, 100, s, e);
        EXPECT(s == 100 && e == 100);
    }
    // the code of a hit and the key's width: code + 1 never runs into the pattern's bits
    for (const int32_t B : {1, 2, 5, 6, 13, 14, 4096, (1 << 27) - 3, 1 << 27}) {
        const int32_t bits = fm_num_code_bits(B);
        EXPECT(fm_num_code(0, B, kNumOk) == 0 && fm_num_code(B - 1, B, kNumOk) == B - 1 && fm_num_code(B, B, kNumOk) == B);
        EXPECT(fm_num_code(0, B, kNumNotNumber) == B + 1 && fm_num_code(B - 1, B, kNumOverflow) == B + 2);
        EXPECT(fm_num_code(B, B, kNumNotNumber) == B && fm_num_code(B, B, kNumOverflow) == B);  // outside the buckets: not counted
        EXPECT(((uint64_t)(B + 3) >> bits) == 0 && bits <= 28);
        for (const int32_t p : {0, 1, 2, 3, 1000})
            for (const int32_t c : {0, B, B + 1, B + 2}) {
                const uint64_t k = fm_hist_key(p, c, bits);
                EXPECT(fm_hist_key_pattern(k, bits) == p && fm_hist_key_bucket(k, bits) == c && fm_hist_key(p, c + 1, bits) == k + 1);
                EXPECT(fm_hist_key(p + 1, 0, bits) > fm_hist_key(p, B + 3, bits));  // (what fm_hist_count's second search relies on)
            }
    }
    EXPECT(fm_num_key_width(1, 1) == 1 + 3 && fm_num_key_width(0x7fffffff, 1 << 27) == 31 + 28);
    // nearest rank
    {
        struct Case {
            int32_t pm;
            int64_t c, want;
        };
        for (const Case k : {Case{0, 1, 0}, Case{1, 1, 0}, Case{500, 1, 0}, Case{999, 1, 0}, Case{1000, 1, 0}, Case{0, 2, 0}, Case{1, 2, 0},
                             Case{500, 2, 0}, Case{501, 2, 1}, Case{999, 2, 1}, Case{1000, 2, 1}, Case{500, 3, 1}, Case{333, 3, 0}, Case{334, 3, 1},
                             Case{666, 3, 1}, Case{667, 3, 2}, Case{999, 3, 2}, Case{0, 1000, 0}, Case{1, 1000, 0}, Case{2, 1000, 1},
                             Case{500, 1000, 499}, Case{999, 1000, 998}, Case{1000, 1000, 999}, Case{1, 1001, 1}, Case{500, 1001, 500},
                             Case{999, 1001, 999}, Case{1000, 1001, 1000}, Case{950, 0x7fffffff, 2040109464}, Case{1000, 0x7fffffff, 0x7ffffffe}})
            EXPECT(fm_num_pct_index(k.pm, k.c) == k.want);
    }
    // the 128-bit sum from the two running sums
    {
        uint64_t lo, hi;
        fm_num_sum128(0, 0, lo, hi);
        EXPECT(lo == 0 && hi == 0);
        fm_num_sum128(0xffffffffu, 0x7fffffffu, lo, hi);  // one value 2^63 - 1
        EXPECT(lo == (uint64_t)kNumValueMax && hi == 0);
        fm_num_sum128(3 * 0xffffffffULL, 3 * 0x7fffffffULL, lo, hi);  // three of them: past 2^64
        const unsigned __int128 three = (unsigned __int128)kNumValueMax * 3;
        EXPECT(lo == (uint64_t)three && hi == (uint64_t)(three >> 64) && hi == 1);
        const uint64_t many = 0x7fffffff;  // 2^31 - 1 values of 2^63 - 1: the largest sums a call can meet
        fm_num_sum128(many * 0xffffffffULL, many * 0x7fffffffULL, lo, hi);
        const unsigned __int128 all = (unsigned __int128)kNumValueMax * many;
        EXPECT(lo == (uint64_t)all && hi == (uint64_t)(all >> 64));
        const uint64_t scan[] = {5, 5, 12, 12, 40};
        EXPECT(fm_num_scan_between(scan, 0, 0) == 0 && fm_num_scan_between(scan, 0, 1) == 5 && fm_num_scan_between(scan, 0, 5) == 40);
        EXPECT(fm_num_scan_between(scan, 2, 1) == 7 && fm_num_scan_between(scan, 1, 3) == 7 && fm_num_scan_between(scan, 4, 1) == 28);
        EXPECT(fm_num_scan_between(scan, 5, 0) == 0 && fm_num_low(0x123456789abcdef0ULL) == 0x9abcdef0u && fm_num_high(0x123456789abcdef0ULL) == 0x12345678u);
    }
    // the permilles the C ABI refuses
    const int32_t ok[] = {0, 1, 500, 1000}, neg[] = {5, -1}, big[] = {1001};
    int32_t many[17] = {0};
    EXPECT(fm_num_permille_bad(ok, 4) == 0 && fm_num_permille_bad(nullptr, 0) == 0 && fm_num_permille_bad(many, 16) == 0);
    EXPECT(fm_num_permille_bad(many, 17) == 1 && fm_num_permille_bad(ok, -1) == 1 && fm_num_permille_bad(nullptr, 1) == 1);
    EXPECT(fm_num_permille_bad(neg, 2) == 2 && fm_num_permille_bad(big, 1) == 2);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "self")) {
        self_checks();
        return g_failed ? 4 : 0;
    }
    if (argc < 4) return 2;
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 2;
    FILE *out = nullptr;
    std::vector<int64_t> head, win_off;
    std::vector<uint16_t> win;
    if (!strcmp(argv[1], "parse")) {
        if (!get(in, head, 2) || !get(in, win_off, (size_t)head[0] + 1) || !get(in, win, (size_t)win_off.back())) return 2;
        std::vector<int32_t> kind((size_t)head[0]);
        std::vector<int64_t> value((size_t)head[0]);
        for (int64_t t = 0; t < head[0]; ++t)
            kind[(size_t)t] = fm_num_parse(win.data() + win_off[(size_t)t], (int32_t)(win_off[(size_t)t + 1] - win_off[(size_t)t]), (int32_t)head[1],
                                           value[(size_t)t]);
        fclose(in);
        if (!(out = fopen(argv[3], "wb"))) return 2;
        put(out, kind);
        put(out, value);
        return fclose(out) == 0 ? 0 : 2;
    }
    std::vector<int64_t> hit_off;
    std::vector<int32_t> T, term_len, locs, edges, permille;
    if (!get(in, head, 8)) return 2;
    const int32_t n = (int32_t)head[0], count = (int32_t)head[2], n_edges = (int32_t)head[4], P = (int32_t)head[5], F = (int32_t)head[6];
    const int32_t text_len = (int32_t)head[7], B = n_edges > 0 ? n_edges - 1 : 1;
    const int64_t n_hits = head[1];
    if (!get(in, T, (size_t)count) || !get(in, term_len, (size_t)n) || !get(in, hit_off, (size_t)n + 1) || !get(in, locs, (size_t)n_hits) ||
        !get(in, edges, (size_t)n_edges) || !get(in, permille, (size_t)P) || !get(in, win_off, (size_t)n_hits + 1) ||
        !get(in, win, (size_t)win_off.back()))
        return 2;
    fclose(in);
    if ((n_edges > 0 && fm_hist_edges_bad(edges.data(), n_edges)) || fm_num_permille_bad(permille.data(), P) || F < 0 || F > kNumFracMax) return 2;
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, (int32_t)head[3], n_fences);
    std::vector<int32_t> fence((size_t)n_fences);
    for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = T[(size_t)((int64_t)j << shift)];
    // k_num_ranges: tile by tile, lane by lane
    const int32_t code_bits = fm_num_code_bits(B);
    const uint64_t no_hit = fm_hist_key(n, 0, code_bits);
    std::vector<uint64_t> keys((size_t)n_hits, ~(uint64_t)0), values((size_t)n_hits, ~(uint64_t)0);
    std::vector<int32_t> start((size_t)n_hits, -1), stop((size_t)n_hits, -1);
    const int64_t first = fm_filter_slot(hit_off[0], n_hits), total = fm_filter_slot(hit_off[(size_t)n], n_hits);
    for (int64_t tile = 0; tile < n_hits; tile += kLocateAllTile) {
        if (tile >= total || tile + kLocateAllTile <= first) {
            for (int64_t t = tile; t < tile + kLocateAllTile && t < n_hits; ++t) {
                keys[(size_t)t] = no_hit;
                start[(size_t)t] = stop[(size_t)t] = 0;
            }
            continue;
        }
        const HitTile h = fm_hit_tile(hit_off.data(), n, tile, total);
        const int64_t *slice = hit_off.data() + h.p_lo;
        for (int64_t t = tile; t < tile + kLocateAllTile && t < n_hits; ++t) {
            if (t >= first && t <= h.tile_last) {
                const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
                fm_val_window(locs[(size_t)t], term_len[(size_t)p], kNumWindow, text_len, start[(size_t)t], stop[(size_t)t]);
                const int32_t b = n_edges > 0 ? fm_hist_bucket(edges.data(), n_edges, fm_line_of(T.data(), count, fence.data(), n_fences, shift, locs[(size_t)t])) : 0;
                keys[(size_t)t] = fm_hist_key(p, b, code_bits);
            } else {
                keys[(size_t)t] = no_hit;
                start[(size_t)t] = stop[(size_t)t] = 0;
            }
        }
    }
    // k_num_parse, and the rows kept hit by hit
    std::vector<std::vector<int64_t>> direct((size_t)n * B);
    std::vector<int32_t> direct_nn((size_t)n, 0), direct_ov((size_t)n, 0);
    for (int64_t t = 0; t < n_hits; ++t) {
        const int32_t p = fm_hist_key_pattern(keys[(size_t)t], code_bits);
        if (p >= n) {
            values[(size_t)t] = 0;
            continue;
        }
        const int64_t at = win_off[(size_t)t];
        const int32_t len = (int32_t)(win_off[(size_t)t + 1] - at);
        if (len != stop[(size_t)t] - start[(size_t)t]) return 5;  // (the caller's windows are not the stage's)
        int64_t v;
        const int32_t kind = fm_num_parse(win.data() + at, len, F, v), b = fm_hist_key_bucket(keys[(size_t)t], code_bits);
        keys[(size_t)t] = fm_hist_key(p, fm_num_code(b, B, kind), code_bits);
        values[(size_t)t] = (uint64_t)v;
        if (b < B) {
            if (kind == kNumOk) direct[(size_t)p * B + b].push_back(v);
            direct_nn[(size_t)p] += kind == kNumNotNumber;
            direct_ov[(size_t)p] += kind == kNumOverflow;
        }
    }
    // rocPRIM's two stable sorts: by value, then by key
    std::vector<int64_t> order((size_t)n_hits);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return values[(size_t)a] < values[(size_t)b]; });
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return keys[(size_t)a] < keys[(size_t)b]; });
    std::vector<uint64_t> skeys((size_t)n_hits), svals((size_t)n_hits), scan_lo((size_t)n_hits), scan_hi((size_t)n_hits);
    for (int64_t j = 0; j < n_hits; ++j) {
        skeys[(size_t)j] = keys[(size_t)order[(size_t)j]];
        svals[(size_t)j] = values[(size_t)order[(size_t)j]];
        if ((svals[(size_t)j] >> 63) != 0) return 3;  // (the value sort looks at 63 bits)
        scan_lo[(size_t)j] = (j ? scan_lo[(size_t)j - 1] : 0) + fm_num_low(svals[(size_t)j]);
        scan_hi[(size_t)j] = (j ? scan_hi[(size_t)j - 1] : 0) + fm_num_high(svals[(size_t)j]);
    }
    if (n_hits > 0 && fm_num_key_width(n, B) < 64 && (skeys.back() >> fm_num_key_width(n, B)) != 0) return 3;
    // k_num_rows, k_num_tails
    const size_t cells = (size_t)n * B;
    std::vector<int32_t> cnt(cells), nn((size_t)n), ov((size_t)n);
    std::vector<uint64_t> sum_lo(cells), sum_hi(cells);
    std::vector<int64_t> mn(cells), mx(cells), pct(cells * (size_t)P);
    for (int64_t i = 0; i < (int64_t)cells; ++i) {
        const int64_t p = i / B;
        int64_t lo;
        const int64_t c = fm_num_segment(skeys.data(), hit_off.data(), n_hits, first, (int32_t)p, (int32_t)(i - p * B), code_bits, lo);
        cnt[(size_t)i] = (int32_t)c;
        mn[(size_t)i] = c > 0 ? (int64_t)svals[(size_t)lo] : 0;
        mx[(size_t)i] = c > 0 ? (int64_t)svals[(size_t)(lo + c - 1)] : 0;
        fm_num_sum128(fm_num_scan_between(scan_lo.data(), lo, c), fm_num_scan_between(scan_hi.data(), lo, c), sum_lo[(size_t)i], sum_hi[(size_t)i]);
        for (int32_t j = 0; j < P; ++j)
            pct[(size_t)i * P + j] = c > 0 ? (int64_t)svals[(size_t)(lo + fm_num_pct_index(permille[(size_t)j], c))] : 0;
        std::vector<int64_t> &d = direct[(size_t)i];
        std::sort(d.begin(), d.end());
        unsigned __int128 sum = 0;
        for (const int64_t v : d) sum += (unsigned __int128)v;
        if ((int64_t)d.size() != c || sum_lo[(size_t)i] != (uint64_t)sum || sum_hi[(size_t)i] != (uint64_t)(sum >> 64)) return 3;
        if (c > 0 && (mn[(size_t)i] != d.front() || mx[(size_t)i] != d.back())) return 3;
        for (int32_t j = 0; j < P && c > 0; ++j) {
            const __int128 rank = ((__int128)permille[(size_t)j] * c + 999) / 1000;  // ceil, in arithmetic that cannot wrap
            if (pct[(size_t)i * P + j] != d[(size_t)((rank < 1 ? 1 : rank) - 1)]) return 3;
        }
    }
    for (int32_t p = 0; p < n; ++p) {
        nn[(size_t)p] = fm_hist_count(skeys.data(), hit_off.data(), n_hits, first, p, B + kNumNotNumber, code_bits);
        ov[(size_t)p] = fm_hist_count(skeys.data(), hit_off.data(), n_hits, first, p, B + kNumOverflow, code_bits);
        if (nn[(size_t)p] != direct_nn[(size_t)p] || ov[(size_t)p] != direct_ov[(size_t)p]) return 3;
    }
    if (!(out = fopen(argv[3], "wb"))) return 2;
    put(out, cnt);
    put(out, sum_lo);
    put(out, sum_hi);
    put(out, mn);
    put(out, mx);
    put(out, pct);
    put(out, nn);
    put(out, ov);
    put(out, start);
    put(out, stop);
    return fclose(out) == 0 ? 0 : 2;
}
