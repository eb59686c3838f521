// by_key_hostsim.cpp — TEST-ONLY host build of the device code of "statistics of the number behind a pattern, grouped by the value of
// a field of the same line" (fmx_first_hits_of_lines_dev, fmx_values_of_hits_groups_dev, fmx_numbers_by_key_dev):
// index4j_amd/csrc/fmx_hit_by.hpp's fm_first_key, fm_first_head, fm_by_find, fm_by_code, fm_by_row_pattern and fm_by_rows_bad — with
// fmx_hit_values.hpp's window, length, run and chunk-key functions and fmx_hit_numbers.hpp's parser, segments and sums — driven by a
// mirror of the three stages with the lanes run one after the other: std::sort / std::stable_sort for rocPRIM's sorts, running sums
// for its scans.  The windows' text is cut from the TEXT the caller hands in (the judge takes the oracle's extract).  The mirror of
// stage b runs over stage a's hits, which stand in LINE order, not in SA-row order: the judge then confirms that the grouping is
// exact for hits in any order.  g++ compiles the headers' functions as plain C++, so the CPU suite checks the source of those
// FUNCTIONS (tests/test_number_stats_by_cpu.py); the kernels' own route runs in tests/test_gpu_number_stats_by.py only.  Never part
// of libfmx.so.
//
// A stand-alone program:
//   by_key_hostsim self          the per-item functions and the host checks at their edges; exit status 4 where one fails
//   by_key_hostsim run IN OUT    IN   int64 {m, n, n_hits, count, max_fences, n_stop, max_len, P, frac_digits, text_len}, int32 T[count],
//                                     int32 term_len[m + n], int32 by_of[n], int64 hit_off[m + n + 1] (hit_off[0] may be non-zero),
//                                     int32 locs[n_hits], uint16 stop[n_stop], int32 permille[P], uint16 text[text_len]
//                                OUT  int64 first_off[m + 1], int64 F, int32 first_lines[F], int32 first_locs[F], int32 group[F],
//                                     int64 val_off[m + 1], int32 lines[G], int64 text_off[G + 1], uint16 chars[text_off[G]],
//                                     int64 row_off[n + 1], int32 count[R], uint64 sum_lo[R], uint64 sum_hi[R], int64 min[R],
//                                     int64 max[R], int64 pct[R * P], int32 no_key[n], int32 not_number[n], int32 overflow[n]
#include "../index4j_amd/csrc/fmx_hit_by.hpp"
#include "../index4j_amd/csrc/fmx_hit_filter.hpp"

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

void self_checks() {
    // the key of stage a: pattern above the position's bits, positions up to text_len
    for (const int32_t text_len : {0, 1, 1023, 1024, 0x7ffffffe}) {
        const int32_t bits = fm_bits((uint32_t)text_len);
        const uint64_t k = fm_first_key(5, text_len, bits);
        EXPECT(fm_first_key_pattern(k, bits) == 5 && fm_first_key_loc(k, bits) == text_len);
        EXPECT(fm_first_key(5, text_len, bits) < fm_first_key(6, 0, bits) && fm_first_key(4, text_len, bits) < fm_first_key(5, 0, bits));
    }
    {  // heads: another pattern, another line, a slot that is no hit
        const int32_t bits = 8, m = 2;
        const uint64_t keys[] = {fm_first_key(0, 3, bits), fm_first_key(0, 9, bits), fm_first_key(0, 12, bits), fm_first_key(1, 12, bits),
                                 fm_first_key(2, 0, bits)};
        const int32_t line_of[] = {0, 0, 1, 1, 0};
        EXPECT(fm_first_head(keys, line_of, 0, m, bits) && !fm_first_head(keys, line_of, 1, m, bits) && fm_first_head(keys, line_of, 2, m, bits));
        EXPECT(fm_first_head(keys, line_of, 3, m, bits) && !fm_first_head(keys, line_of, 4, m, bits));
    }
    {  // the line of a number hit among the first lines of its key pattern
        const int32_t lines[] = {7, 2, 5, 9, 1};
        EXPECT(fm_by_find(lines, 1, 4, 2) == 1 && fm_by_find(lines, 1, 4, 9) == 3 && fm_by_find(lines, 1, 4, 5) == 2);
        EXPECT(fm_by_find(lines, 1, 4, 1) == -1 && fm_by_find(lines, 1, 4, 7) == -1 && fm_by_find(lines, 1, 4, 3) == -1 && fm_by_find(lines, 1, 4, 10) == -1);
        EXPECT(fm_by_find(lines, 2, 2, 5) == -1);  // a key pattern without a first hit
        const int32_t group[] = {0, 2, 1, -1, 3};
        EXPECT(fm_by_code(group, 1, 3) == 2 && fm_by_code(group, -1, 3) == 3 && fm_by_code(group, 3, 3) == 3 && fm_by_code(group, 4, 3) == 3);
    }
    {  // the pattern of a packed row: runs of equal offsets end in the pattern that holds the row
        const int64_t row_off[] = {0, 0, 3, 3, 3, 5};
        EXPECT(fm_by_row_pattern(row_off, 5, 0) == 1 && fm_by_row_pattern(row_off, 5, 2) == 1 && fm_by_row_pattern(row_off, 5, 3) == 4);
        EXPECT(fm_by_row_pattern(row_off, 5, 4) == 4);
        const int64_t one[] = {0, 4};
        EXPECT(fm_by_row_pattern(one, 1, 0) == 0 && fm_by_row_pattern(one, 1, 3) == 0);
    }
    {  // the host checks
        const int32_t by_of[] = {1, 0, 1}, bad[] = {0, 2, 0}, neg[] = {-1, 0, 0};
        const int64_t val_off[] = {0, 2, 7}, down[] = {0, 3, 2}, below[] = {-1, 0, 0};
        int64_t row_off[4];
        int32_t B = 0;
        EXPECT(fm_by_rows_bad(3, by_of, 2, val_off, 2, row_off, &B) == 0 && row_off[0] == 0 && row_off[1] == 5 && row_off[2] == 7 && row_off[3] == 12 && B == 5);
        EXPECT(fm_by_rows_bad(0, nullptr, 0, nullptr, 0, nullptr, nullptr) == 0);
        EXPECT(fm_by_rows_bad(3, by_of, 0, val_off, 0, nullptr, nullptr) == 1 && fm_by_rows_bad(3, nullptr, 2, val_off, 0, nullptr, nullptr) == 1);
        EXPECT(fm_by_rows_bad(3, bad, 2, val_off, 0, nullptr, nullptr) == 2 && fm_by_rows_bad(3, neg, 2, val_off, 0, nullptr, nullptr) == 2);
        EXPECT(fm_by_rows_bad(3, bad, 2, nullptr, 0, nullptr, nullptr) == 2 && fm_by_rows_bad(3, by_of, 2, nullptr, 0, nullptr, nullptr) == 0);
        EXPECT(fm_by_rows_bad(3, by_of, 2, down, 0, nullptr, nullptr) == 3 && fm_by_rows_bad(3, by_of, 2, below, 0, nullptr, nullptr) == 3);
        const int64_t wide[] = {0, kHistCellsMax, kHistCellsMax + 1}, half[] = {0, kHistCellsMax / 2, kHistCellsMax / 2};
        const int32_t first[] = {0}, both[] = {0, 1}, twice[] = {0, 0}, thrice[] = {0, 0, 0};
        EXPECT(fm_by_rows_bad(1, first, 2, wide, 0, nullptr, &B) == 0 && B == kHistCellsMax);  // exactly 2^27 rows
        EXPECT(fm_by_rows_bad(2, both, 2, wide, 0, nullptr, nullptr) == 4 && fm_by_rows_bad(1, first, 2, wide, 2, nullptr, nullptr) == 5);
        EXPECT(fm_by_rows_bad(2, twice, 2, half, 1, nullptr, nullptr) == 0 && fm_by_rows_bad(3, thrice, 2, half, 1, nullptr, nullptr) == 4);
        B = 0;
        const int64_t none[] = {0, 0, 0};
        EXPECT(fm_by_rows_bad(3, by_of, 2, none, 16, row_off, &B) == 0 && row_off[3] == 0 && B == 1);  // no group at all: B stays 1
    }
}

struct In {
    int64_t m, n, n_hits, count, max_fences, n_stop, max_len, P, frac_digits, text_len;
    std::vector<int32_t> T, term_len, by_of, locs, permille;
    std::vector<int64_t> hit_off;
    std::vector<uint16_t> stop, text;
};

// the pattern of slot t of a packed block, by the tile functions the key kernels use; -1 for a slot that is no hit
int32_t pattern_of(const int64_t *hit_off, int32_t n, int64_t n_hits, int64_t t) {
    const int64_t first = fm_filter_slot(hit_off[0], n_hits), total = fm_filter_slot(hit_off[n], n_hits);
    if (t < first || t >= total) return -1;
    const int64_t tile = t / kLocateAllTile * kLocateAllTile;
    const HitTile h = fm_hit_tile(hit_off, n, tile, total);
    return h.p_lo + fm_hit_pattern(hit_off + h.p_lo, h.slice_count, t);
}

int run(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) return 2;
    In a;
    std::vector<int64_t> head;
    if (!get(f, head, 10)) return 2;
    a.m = head[0], a.n = head[1], a.n_hits = head[2], a.count = head[3], a.max_fences = head[4], a.n_stop = head[5], a.max_len = head[6];
    a.P = head[7], a.frac_digits = head[8], a.text_len = head[9];
    if (!get(f, a.T, (size_t)a.count) || !get(f, a.term_len, (size_t)(a.m + a.n)) || !get(f, a.by_of, (size_t)a.n) ||
        !get(f, a.hit_off, (size_t)(a.m + a.n + 1)) || !get(f, a.locs, (size_t)a.n_hits) || !get(f, a.stop, (size_t)a.n_stop) ||
        !get(f, a.permille, (size_t)a.P) || !get(f, a.text, (size_t)a.text_len))
        return 2;
    fclose(f);
    const int32_t m = (int32_t)a.m, n = (int32_t)a.n, count = (int32_t)a.count, text_len = (int32_t)a.text_len, max_len = (int32_t)a.max_len;
    const int32_t P = (int32_t)a.P;
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, (int32_t)a.max_fences, n_fences);
    std::vector<int32_t> fence((size_t)n_fences);
    for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = a.T[(size_t)((int64_t)j << shift)];
    auto line_of_pos = [&](int32_t p) { return fm_line_of(a.T.data(), count, fence.data(), n_fences, shift, p); };
    std::sort(a.stop.begin(), a.stop.end());

    // ---- stage a over the key patterns' part: the slots [0, hit_off[m]) and some behind them ----
    const int64_t *key_off = a.hit_off.data();
    // (up to 70 slots behind hit_off[m] — number hits, or slots that hold nothing — are handed in too: to this stage they are no hits)
    const int64_t a_slots = fm_filter_slot(key_off[m] + 70, a.n_hits);
    const int32_t pos_bits = fm_bits((uint32_t)text_len);
    std::vector<uint64_t> keys((size_t)a_slots);
    for (int64_t t = 0; t < a_slots; ++t) {
        const int32_t p = pattern_of(key_off, m, a_slots, t);
        keys[(size_t)t] = p < 0 ? fm_first_key(m, 0, pos_bits) : fm_first_key(p, a.locs[(size_t)t], pos_bits);
    }
    std::sort(keys.begin(), keys.end());
    std::vector<int32_t> line_of((size_t)a_slots), head_a((size_t)a_slots + 1, 0), pos_a((size_t)a_slots + 1, 0);
    for (int64_t i = 0; i < a_slots; ++i)
        line_of[(size_t)i] = fm_first_key_pattern(keys[(size_t)i], pos_bits) < m ? line_of_pos(fm_first_key_loc(keys[(size_t)i], pos_bits)) : 0;
    for (int64_t i = 0; i < a_slots; ++i) head_a[(size_t)i] = fm_first_head(keys.data(), line_of.data(), i, m, pos_bits) ? 1 : 0;
    for (int64_t i = 0; i < a_slots; ++i) pos_a[(size_t)i + 1] = pos_a[(size_t)i] + head_a[(size_t)i];
    const int64_t F = pos_a[(size_t)a_slots];
    std::vector<int64_t> first_off((size_t)m + 1);
    std::vector<int32_t> first_lines((size_t)F), first_locs((size_t)F);
    for (int64_t i = 0; i < a_slots; ++i)
        if (head_a[(size_t)i]) {
            first_lines[(size_t)pos_a[(size_t)i]] = line_of[(size_t)i];
            first_locs[(size_t)pos_a[(size_t)i]] = fm_first_key_loc(keys[(size_t)i], pos_bits);
        }
    const int64_t a_first = fm_filter_slot(key_off[0], a_slots);
    for (int32_t p = 0; p <= m; ++p) {
        const int64_t at = fm_filter_slot(key_off[p], a_slots);
        first_off[(size_t)p] = pos_a[(size_t)((at < a_first ? a_first : at) - a_first)];
    }

    // ---- stage b over the first hits: k_val_ranges .. k_val_offsets, then the two kernels of the twin ----
    const size_t H = (size_t)F;
    std::vector<int32_t> pat(H), vlen(H), flag(H + 1, 0), scan(H + 1, 0);
    std::vector<const uint16_t *> win(H);
    for (size_t t = 0; t < H; ++t) {
        pat[t] = pattern_of(first_off.data(), m, F, (int64_t)t);
        int32_t s, e;
        fm_val_window(first_locs[t], a.term_len[(size_t)pat[t]], max_len, text_len, s, e);
        win[t] = a.text.data() + s;
        vlen[t] = fm_val_length<false>(win[t], e - s, a.stop.data(), (int32_t)a.n_stop);
    }
    for (size_t i = 0; i < H; ++i) flag[i] = i == 0 || pat[i - 1] != pat[i] || !fm_val_same(win[i - 1], vlen[i - 1], win[i], vlen[i]);
    for (size_t i = 0; i < H; ++i) scan[i + 1] = scan[i] + flag[i];
    const int32_t R = scan[H];
    std::vector<int32_t> run_start((size_t)R + 1);
    for (size_t i = 0; i < H; ++i)
        if (flag[i]) run_start[(size_t)scan[i]] = (int32_t)i;
    run_start[(size_t)R] = (int32_t)H;
    std::vector<uint32_t> perm((size_t)R);
    std::iota(perm.begin(), perm.end(), 0u);
    auto pass = [&](auto key) { std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return key(x) < key(y); }); };
    pass([&](uint32_t r) { return (uint64_t)vlen[(size_t)run_start[r]]; });
    for (int32_t c = fm_val_chunks(max_len) - 1; c >= 0; --c)
        pass([&](uint32_t r) { return fm_val_chunk_key(win[(size_t)run_start[r]], vlen[(size_t)run_start[r]], c); });
    pass([&](uint32_t r) { return (uint64_t)pat[(size_t)run_start[r]]; });
    std::vector<int32_t> head_b((size_t)R + 1, 0), hscan((size_t)R + 1, 0), run_group((size_t)R);
    for (int32_t j = 0; j < R; ++j) {
        const int32_t h = run_start[perm[(size_t)j]];
        int32_t fl = 1;
        if (j > 0 && pat[(size_t)run_start[perm[(size_t)j - 1]]] == pat[(size_t)h]) {
            const int32_t g = run_start[perm[(size_t)j - 1]];
            fl = !fm_val_same(win[(size_t)g], vlen[(size_t)g], win[(size_t)h], vlen[(size_t)h]);
        }
        head_b[(size_t)j] = fl;
    }
    for (int32_t j = 0; j < R; ++j) hscan[(size_t)j + 1] = hscan[(size_t)j] + head_b[(size_t)j];
    const int32_t G = hscan[(size_t)R];
    std::vector<int64_t> val_off((size_t)m + 1, G), text_off((size_t)G + 1, 0);
    std::vector<int32_t> lines((size_t)G, 0), group_of_first(H);
    std::vector<uint16_t> chars;
    for (int32_t j = 0; j < R; ++j) {
        const uint32_t r = perm[(size_t)j];
        const int32_t g = hscan[(size_t)j] + head_b[(size_t)j] - 1, h = run_start[r];
        run_group[r] = g;
        lines[(size_t)g] += run_start[r + 1] - h;
        if (head_b[(size_t)j]) {
            chars.insert(chars.end(), win[(size_t)h], win[(size_t)h] + vlen[(size_t)h]);
            text_off[(size_t)g + 1] = (int64_t)chars.size();
        }
    }
    for (int32_t p = m; p >= 0; --p) {  // val_off[p] = the group at the first sorted run whose pattern is not below p
        int32_t j = 0;
        while (j < R && pat[(size_t)run_start[perm[(size_t)j]]] < p) ++j;
        val_off[(size_t)p] = hscan[(size_t)j];
    }
    for (size_t i = 0; i < H; ++i) group_of_first[i] = (int32_t)(run_group[(size_t)scan[i + 1] - 1] - val_off[(size_t)pat[i]]);

    // ---- stage c over the number patterns' part: hit_off + m, the slots [0, hit_off[m + n]) ----
    const int64_t *num_off = a.hit_off.data() + m;
    const int64_t c_slots = fm_filter_slot(num_off[n], a.n_hits), c_first = fm_filter_slot(num_off[0], c_slots);
    std::vector<int64_t> row_off((size_t)n + 1, 0);
    int32_t B = 1;
    if (fm_by_rows_bad(n, a.by_of.data(), m, val_off.data(), P, row_off.data(), &B)) return 5;
    const int32_t code_bits = fm_num_code_bits(B);
    std::vector<uint64_t> ckey((size_t)c_slots), cval((size_t)c_slots, 0);
    for (int64_t t = 0; t < c_slots; ++t) {
        const int32_t p = pattern_of(num_off, n, c_slots, t);
        if (p < 0) {
            ckey[(size_t)t] = fm_hist_key(n, 0, code_bits);
            continue;
        }
        const int32_t loc = a.locs[(size_t)t], k = a.by_of[(size_t)p];
        int32_t s, e;
        fm_val_window(loc, a.term_len[(size_t)m + p], kNumWindow, text_len, s, e);
        const int64_t found = fm_by_find(first_lines.data(), first_off[(size_t)k], first_off[(size_t)k + 1], line_of_pos(loc));
        const int32_t code = fm_by_code(group_of_first.data(), found, B);
        int64_t v;
        const int32_t kind = fm_num_parse(a.text.data() + s, e - s, (int32_t)a.frac_digits, v);
        ckey[(size_t)t] = fm_hist_key(p, fm_num_code(code, B, kind), code_bits);
        cval[(size_t)t] = (uint64_t)v;
    }
    std::vector<size_t> order((size_t)c_slots);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return cval[x] < cval[y]; });
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return ckey[x] < ckey[y]; });
    std::vector<uint64_t> skey((size_t)c_slots), sval((size_t)c_slots), scan_lo((size_t)c_slots), scan_hi((size_t)c_slots);
    for (size_t i = 0; i < order.size(); ++i) {
        skey[i] = ckey[order[i]];
        sval[i] = cval[order[i]];
        scan_lo[i] = (i ? scan_lo[i - 1] : 0) + fm_num_low(sval[i]);
        scan_hi[i] = (i ? scan_hi[i - 1] : 0) + fm_num_high(sval[i]);
    }
    const int64_t rows = row_off[(size_t)n];
    std::vector<int32_t> cnt((size_t)rows), no_key((size_t)n), nn((size_t)n), ov((size_t)n);
    std::vector<uint64_t> sum_lo((size_t)rows), sum_hi((size_t)rows);
    std::vector<int64_t> vmin((size_t)rows), vmax((size_t)rows), pct((size_t)(rows * P));
    for (int64_t i = 0; i < rows; ++i) {
        const int32_t p = fm_by_row_pattern(row_off.data(), n, i);
        int64_t lo;
        const int64_t c = fm_num_segment(skey.data(), num_off, c_slots, c_first, p, (int32_t)(i - row_off[(size_t)p]), code_bits, lo);
        cnt[(size_t)i] = (int32_t)c;
        vmin[(size_t)i] = c > 0 ? (int64_t)sval[(size_t)lo] : 0;
        vmax[(size_t)i] = c > 0 ? (int64_t)sval[(size_t)(lo + c - 1)] : 0;
        fm_num_sum128(fm_num_scan_between(scan_lo.data(), lo, c), fm_num_scan_between(scan_hi.data(), lo, c), sum_lo[(size_t)i], sum_hi[(size_t)i]);
        for (int32_t j = 0; j < P; ++j)
            pct[(size_t)(i * P + j)] = c > 0 ? (int64_t)sval[(size_t)(lo + fm_num_pct_index(a.permille[(size_t)j], c))] : 0;
    }
    for (int32_t p = 0; p < n; ++p) {
        no_key[(size_t)p] = fm_hist_count(skey.data(), num_off, c_slots, c_first, p, B, code_bits);
        nn[(size_t)p] = fm_hist_count(skey.data(), num_off, c_slots, c_first, p, B + kNumNotNumber, code_bits);
        ov[(size_t)p] = fm_hist_count(skey.data(), num_off, c_slots, c_first, p, B + kNumOverflow, code_bits);
    }

    FILE *o = fopen(out_path, "wb");
    if (!o) return 2;
    put(o, first_off);
    put(o, std::vector<int64_t>{F});
    put(o, first_lines);
    put(o, first_locs);
    put(o, group_of_first);
    put(o, val_off);
    put(o, lines);
    put(o, text_off);
    put(o, chars);
    put(o, row_off);
    put(o, cnt);
    put(o, sum_lo);
    put(o, sum_hi);
    put(o, vmin);
    put(o, vmax);
    put(o, pct);
    put(o, no_key);
    put(o, nn);
    put(o, ov);
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
    fprintf(stderr, "usage: by_key_hostsim self | run IN OUT\n");
    return 1;
}
