// range_hostsim.cpp — TEST-ONLY host build of the device code of "the packed hits whose number lies in a range"
// (fmx_hits_in_number_range_dev): index4j_amd/csrc/fmx_hit_range.hpp's fm_range_ranged, fm_range_code, fm_range_tail,
// fm_range_not_number, fm_range_overflow and fm_range_args_bad — with fm_val_window for a hit's window, fm_hit_tile / fm_hit_pattern
// for its pattern, fm_filter_slot / fm_filter_kept_off for the packed output — driven by a mirror of the stages of fmx_hit_range.hip
// with the lanes run one after the other: k_range_windows' tile loop, k_range_flags over the windows the caller hands in (the
// judge's: the oracle's extract), running sums for rocPRIM's two exclusive scans, k_hit_keep_store's stable store, k_range_tails.
// The counters off the scans are checked against counters kept hit by hit.  g++ compiles the header's functions as plain C++, so the
// CPU suite checks the source of those FUNCTIONS (tests/test_number_range_cpu.py).  The kernels' own route runs in
// tests/test_gpu_number_range.py only.  Never part of libfmx.so.
//
// A stand-alone program:
//   range_hostsim self            the per-item functions at their edges (below); exit status 4 and a line on stderr where one fails
//   range_hostsim range IN OUT    IN   int64 {n, n_hits, frac_digits, text_len, extract}, int32 term_len[n], int64 num_lo[n], int64
//                                      num_hi[n], int64 hit_off[n + 1], int32 locs[n_hits], int64 win_off[n_hits + 1], uint16
//                                      win[win_off[n_hits]] (a slot of an unranged pattern and a slot that is no hit: no units)
//                                 OUT  int64 kept_off[n + 1], int32 kept_locs[n_hits] (kSentinel behind kept_off[n]), int32 kept[n],
//                                      int32 not_number[n], int32 overflow[n], int32 start[n_hits], int32 stop[n_hits], int32
//                                      pattern[n_hits], int32 not_enabled[n] (1: extract == 0 and the pattern is ranged)
// Exit status 3: the counters off the scans and those kept hit by hit disagree; 5: the caller's windows are not the stage's.
#include "../index4j_amd/csrc/fmx_hit_range.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace fmx;

namespace {

constexpr int32_t kSentinel = -77;

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
#define EXPECT(cond)                                           \
    do {                                                       \
        if (!(cond)) {                                         \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
            g_failed = 1;                                      \
        }                                                      \
    } while (0)

int32_t code(const std::string &s, int32_t F, int64_t lo, int64_t hi) {
    std::vector<uint16_t> w(s.begin(), s.end());
    w.push_back('7');  // (a digit BEHIND the window: never read)
    return fm_range_code(w.data(), (int32_t)s.size(), F, lo, hi);
}

void self_checks() {
    const int64_t M = kNumValueMax;
    EXPECT(fm_range_ranged(0) && fm_range_ranged(M) && !fm_range_ranged(-1) && !fm_range_ranged(INT64_MIN));
    // a value v against [v, v], [v + 1, max], [0, v - 1], [0, max] and [3, 2]
    for (const int32_t F : {0, 3, 9}) {
        const int64_t S = fm_num_pow10(F);
        struct Case {
            const char *text;
            int64_t v;
        };
        for (const Case c : {Case{"0", 0}, Case{"007", 7 * S}, Case{"12 ", 12 * S}, Case{"12.5", 12 * S + 5 * S / 10}, Case{"1.", S}}) {
            EXPECT(code(c.text, F, c.v, c.v) == kRangeKeep && code(c.text, F, c.v + 1, M) == kRangeOutside);
            EXPECT(code(c.text, F, 0, M) == kRangeKeep && code(c.text, F, 3, 2) == kRangeOutside);
            if (c.v > 0) EXPECT(code(c.text, F, 0, c.v - 1) == kRangeOutside && code(c.text, F, c.v - 1, c.v) == kRangeKeep);
            EXPECT(code(c.text, F, c.v, c.v + 1) == kRangeKeep && code(c.text, F, c.v, 0) == (c.v == 0 ? kRangeKeep : kRangeOutside));
        }
        // what does not parse never passes, whatever the range
        for (const char *t : {".5", "x", "", "-1", " 1"})
            EXPECT(code(t, F, 0, M) == kRangeNotNumber && code(t, F, 0, 0) == kRangeNotNumber && code(t, F, 3, 2) == kRangeNotNumber);
        for (const std::string &t : {std::string("9223372036854775808"), std::string(20, '9'), std::string(31, '0') + "7", std::string(32, '0')})
            EXPECT(code(t, F, 0, M) == kRangeOverflow && code(t, F, M, M) == kRangeOverflow && code(t, F, 3, 2) == kRangeOverflow);
    }
    EXPECT(code("9223372036854775807", 0, M, M) == kRangeKeep && code("9223372036854775807", 0, 0, M - 1) == kRangeOutside);
    EXPECT(code("9223372036854775807", 3, 0, M) == kRangeOverflow && code("9223372036.854775807", 9, M, M) == kRangeKeep);
    EXPECT(code("9223372036.854775808", 9, 0, M) == kRangeOverflow && code(std::string(30, '0') + "7", 0, 7, 7) == kRangeKeep);
    // the word of the two reasons and the counters of [a, b) off its exclusive scan: neither half runs into the other
    EXPECT(fm_range_tail(kRangeOutside) == 0 && fm_range_tail(kRangeKeep) == 0 && fm_range_tail(kRangeNotNumber) == 1 &&
           fm_range_tail(kRangeOverflow) == (1ull << 32));
    {
        const int32_t codes[] = {kRangeNotNumber, kRangeKeep, kRangeOverflow, kRangeOverflow, kRangeOutside, kRangeNotNumber, kRangeNotNumber};
        uint64_t scan[8] = {0};
        for (int i = 0; i < 7; ++i) scan[i + 1] = scan[i] + fm_range_tail(codes[i]);
        EXPECT(fm_range_not_number(scan, 0, 7) == 3 && fm_range_overflow(scan, 0, 7) == 2 && fm_range_not_number(scan, 1, 5) == 0);
        EXPECT(fm_range_overflow(scan, 1, 5) == 2 && fm_range_not_number(scan, 5, 7) == 2 && fm_range_overflow(scan, 4, 4) == 0);
        const uint64_t most[2] = {0, 0x7fffffffull | (0x7fffffffull << 32)};  // 2^31 - 1 of each: the largest a call can meet
        EXPECT(fm_range_not_number(most, 0, 1) == 0x7fffffff && fm_range_overflow(most, 0, 1) == 0x7fffffff);
    }
    // the arguments the C ABI refuses
    const int32_t ok[] = {0, 5, INT32_MAX}, neg[] = {5, -1};
    EXPECT(fm_range_args_bad(3, ok, 0) == 0 && fm_range_args_bad(3, ok, 9) == 0 && fm_range_args_bad(0, nullptr, 0) == 0);
    EXPECT(fm_range_args_bad(3, ok, -1) == 1 && fm_range_args_bad(3, ok, 10) == 1 && fm_range_args_bad(2, neg, 0) == 2);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "self")) {
        self_checks();
        return g_failed ? 4 : 0;
    }
    if (argc < 4 || strcmp(argv[1], "range")) return 2;
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 2;
    std::vector<int64_t> head, num_lo, num_hi, hit_off, win_off;
    std::vector<int32_t> term_len, locs;
    std::vector<uint16_t> win;
    if (!get(in, head, 5)) return 2;
    const int32_t n = (int32_t)head[0], F = (int32_t)head[2], text_len = (int32_t)head[3];
    const int64_t n_hits = head[1];
    const bool extract = head[4] != 0;
    if (!get(in, term_len, (size_t)n) || !get(in, num_lo, (size_t)n) || !get(in, num_hi, (size_t)n) || !get(in, hit_off, (size_t)n + 1) ||
        !get(in, locs, (size_t)n_hits) || !get(in, win_off, (size_t)n_hits + 1) || !get(in, win, (size_t)win_off.back()))
        return 2;
    fclose(in);
    if (n <= 0 || n_hits <= 0 || fm_range_args_bad(n, term_len.data(), F)) return 2;
    const size_t H = (size_t)n_hits;
    // k_range_windows: tile by tile, lane by lane
    std::vector<int32_t> pattern(H, -1), start(H, -1), stop(H, -1);
    const int64_t first = fm_filter_slot(hit_off[0], n_hits), total = fm_filter_slot(hit_off[(size_t)n], n_hits);
    for (int64_t tile = 0; tile < n_hits; tile += kLocateAllTile) {
        if (tile >= total || tile + kLocateAllTile <= first) {
            for (int64_t t = tile; t < tile + kLocateAllTile && t < n_hits; ++t) {
                pattern[(size_t)t] = n;
                start[(size_t)t] = stop[(size_t)t] = 0;
            }
            continue;
        }
        const HitTile h = fm_hit_tile(hit_off.data(), n, tile, total);
        const int64_t *slice = hit_off.data() + h.p_lo;
        for (int64_t t = tile; t < tile + kLocateAllTile && t < n_hits; ++t) {
            if (t >= first && t <= h.tile_last) {
                const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
                int32_t s = 0, e = 0;
                if (fm_range_ranged(num_lo[(size_t)p])) fm_val_window(locs[(size_t)t], term_len[(size_t)p], kNumWindow, text_len, s, e);
                pattern[(size_t)t] = p;
                start[(size_t)t] = s;
                stop[(size_t)t] = e;
            } else {
                pattern[(size_t)t] = n;
                start[(size_t)t] = stop[(size_t)t] = 0;
            }
        }
    }
    // k_range_flags, and the counters kept hit by hit
    std::vector<int32_t> flag(H + 1, -1), direct_kept((size_t)n, 0), direct_nn((size_t)n, 0), direct_ov((size_t)n, 0);
    std::vector<uint64_t> tail(H + 1, ~0ull);
    flag[H] = 0;
    tail[H] = 0;
    for (int64_t t = 0; t < n_hits; ++t) {
        const int32_t p = pattern[(size_t)t];
        int32_t c = kRangeOutside;
        if (p < n) {
            const int64_t lo = num_lo[(size_t)p];
            if (!fm_range_ranged(lo)) {
                c = kRangeKeep;
            } else if (extract) {
                const int64_t at = win_off[(size_t)t];
                const int32_t len = (int32_t)(win_off[(size_t)t + 1] - at);
                if (len != stop[(size_t)t] - start[(size_t)t]) return 5;
                c = fm_range_code(win.data() + at, len, F, lo, num_hi[(size_t)p]);
            }
            direct_kept[(size_t)p] += c == kRangeKeep;
            direct_nn[(size_t)p] += c == kRangeNotNumber;
            direct_ov[(size_t)p] += c == kRangeOverflow;
        } else if (win_off[(size_t)t + 1] != win_off[(size_t)t]) {
            return 5;
        }
        flag[(size_t)t] = c == kRangeKeep ? 1 : 0;
        tail[(size_t)t] = fm_range_tail(c);
    }
    // rocPRIM's two exclusive scans over n_hits + 1 entries
    std::vector<int32_t> pos(H + 1);
    std::vector<uint64_t> tail_pos(H + 1);
    int32_t run = 0;
    uint64_t run64 = 0;
    for (size_t t = 0; t <= H; ++t) {
        pos[t] = run;
        tail_pos[t] = run64;
        run += flag[t];
        run64 += tail[t];
    }
    // k_hit_keep_store
    std::vector<int64_t> kept_off((size_t)n + 1);
    std::vector<int32_t> kept_locs(H, kSentinel);
    for (int64_t t = 0; t < n_hits; ++t)
        if (flag[(size_t)t]) kept_locs[(size_t)pos[(size_t)t]] = locs[(size_t)t];
    for (int32_t p = 0; p <= n; ++p) kept_off[(size_t)p] = fm_filter_kept_off(hit_off.data(), pos.data(), n_hits, p);
    // k_range_tails
    std::vector<int32_t> kept((size_t)n), nn((size_t)n), ov((size_t)n), not_enabled((size_t)n, 0);
    for (int32_t p = 0; p < n; ++p) {
        int64_t a = fm_filter_slot(hit_off[(size_t)p], n_hits), b = fm_filter_slot(hit_off[(size_t)p + 1], n_hits);
        a = a < first ? first : a;
        b = b < a ? a : b;
        kept[(size_t)p] = pos[(size_t)b] - pos[(size_t)a];
        nn[(size_t)p] = fm_range_not_number(tail_pos.data(), a, b);
        ov[(size_t)p] = fm_range_overflow(tail_pos.data(), a, b);
        not_enabled[(size_t)p] = !extract && fm_range_ranged(num_lo[(size_t)p]);
        if (kept[(size_t)p] != direct_kept[(size_t)p] || nn[(size_t)p] != direct_nn[(size_t)p] || ov[(size_t)p] != direct_ov[(size_t)p]) return 3;
        if (kept[(size_t)p] != kept_off[(size_t)p + 1] - kept_off[(size_t)p]) return 3;
    }
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    put(out, kept_off);
    put(out, kept_locs);
    put(out, kept);
    put(out, nn);
    put(out, ov);
    put(out, start);
    put(out, stop);
    put(out, pattern);
    put(out, not_enabled);
    return fclose(out) == 0 ? 0 : 2;
}
