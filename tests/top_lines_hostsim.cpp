// top_lines_hostsim.cpp — TEST-ONLY host build of the device code of "the lines ranked by the number behind a pattern"
// (fmx_top_lines_of_hits_dev): index4j_amd/csrc/fmx_hit_top.hpp's fm_top_ordered, fm_top_value, fm_top_better, fm_top_line_key,
// fm_top_tail_code, fm_top_segment, fm_top_rows and fm_top_args_bad — with fm_val_window for a hit's window, fm_hit_tile /
// fm_hit_pattern for its pattern, fm_num_parse for its value, fm_line_of over fences for its line and fm_range_tail's word for the
// reasons — driven by a mirror of the stages of fmx_hit_top.hip with the lanes run one after the other: k_top_keys' tile loop,
// k_top_parse over the windows the caller hands in (the judge's: the oracle's extract), a running sum for rocPRIM's scan,
// std::stable_sort for its radix sorts, a fold per run for its reduce_by_key (from the left AND from the right: the operator is
// associative and commutative, the two must agree), k_top_cands, k_top_patterns, k_top_tails, k_top_rows.  The rows are checked
// against a ranking kept line by line in a map.  g++ compiles the header's functions as plain C++, so the CPU suite checks the source
// of those FUNCTIONS (tests/test_top_lines_cpu.py).  The kernels' own route runs in tests/test_gpu_top_lines.py only.  Never part
// of libfmx.so.
//
// A stand-alone program:
//   top_lines_hostsim self          the per-item functions at their edges (below); exit status 4 and a line on stderr where one fails
//   top_lines_hostsim top IN OUT    IN   int64 {n, n_hits, count, max_fences, frac_digits, text_len, first, top}, int32 T[count],
//                                        int32 term_len[n], uint8 descending[n], int64 hit_off[n + 1], int32 locs[n_hits], int64
//                                        win_off[n_hits + 1], uint16 win[win_off[n_hits]]
//                                   OUT  int32 rows[n], int32 row_line[n * top], int64 row_value[n * top], int32 row_loc[n * top],
//                                        int32 lines[n], int32 numbers[n], int32 not_number[n], int32 overflow[n], int32
//                                        start[n_hits], int32 stop[n_hits]
// Exit status 3: the rows off the sorted order and the ranking kept line by line disagree; 5: the caller's windows are not the stage's.
#include "../index4j_amd/csrc/fmx_hit_top.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <utility>
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

bool same(const TopCand &a, const TopCand &b) { return a.u == b.u && a.loc == b.loc; }

void self_checks() {
    // the ordered value: 0 and INT64_MAX sit at both ends in both orders, and the order of u is the order asked for
    EXPECT(fm_top_ordered(0, false) == 0 && fm_top_ordered(kNumValueMax, false) == (uint64_t)kNumValueMax);
    EXPECT(fm_top_ordered(0, true) == (uint64_t)kNumValueMax && fm_top_ordered(kNumValueMax, true) == 0);
    for (const int64_t v : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)67108864, kNumValueMax - 1, kNumValueMax})
        for (const bool d : {false, true}) {
            const uint64_t u = fm_top_ordered(v, d);
            EXPECT((u >> 63) == 0 && fm_top_value(u, d) == v);  // (the sort by u looks at 63 bits)
            if (v > 0) EXPECT(d ? u < fm_top_ordered(v - 1, d) : u > fm_top_ordered(v - 1, d));
        }
    // the minimum of (u, position): associative, commutative, idempotent
    {
        const TopCand c[] = {{5, 10}, {5, 3}, {4, 99}, {4, 99}, {0, 0}, {(uint64_t)kNumValueMax, 0x7fffffff}, {5, 11}};
        const TopBetter op;
        for (const TopCand &a : c)
            for (const TopCand &b : c) {
                EXPECT(same(op(a, b), op(b, a)) && same(op(a, b), fm_top_better(a, b)) && same(op(a, a), a));
                for (const TopCand &d : c) EXPECT(same(op(op(a, b), d), op(a, op(b, d))));
            }
        EXPECT(same(op(c[0], c[1]), c[1]) && same(op(c[0], c[2]), c[2]) && same(op(c[0], c[6]), c[0]) && same(op(c[4], c[5]), c[4]));
    }
    // the run key
    for (const int32_t p : {0, 1, 1000, 0x7fffffff})
        for (const int32_t l : {0, 1, 2000, 0x7fffffff}) {
            const uint64_t k = fm_top_line_key(p, l);
            EXPECT(fm_top_line_key_pattern(k) == p && fm_top_line_key_line(k) == l);
            if (p < 0x7fffffff) EXPECT(fm_top_line_key(p + 1, 0) > k);
        }
    // the reasons' word
    EXPECT(fm_range_tail(fm_top_tail_code(kNumOk)) == 0 && fm_range_tail(fm_top_tail_code(kNumNotNumber)) == 1 &&
           fm_range_tail(fm_top_tail_code(kNumOverflow)) == (1ull << 32));
    // the segment of a pattern among the ranked slots
    {
        const uint32_t pat[] = {0, 0, 2, 2, 2, 5, 7, 7};  // 7 = n: no candidate
        EXPECT(fm_top_segment(pat, 8, 0) == 0 && fm_top_segment(pat, 8, 1) == 2 && fm_top_segment(pat, 8, 2) == 2 && fm_top_segment(pat, 8, 3) == 5);
        EXPECT(fm_top_segment(pat, 8, 5) == 5 && fm_top_segment(pat, 8, 6) == 6 && fm_top_segment(pat, 8, 7) == 6 && fm_top_segment(pat, 8, 8) == 8);
        EXPECT(fm_top_segment(pat, 0, 0) == 0 && fm_top_segment(nullptr, 0, 3) == 0);
    }
    // the rows of a pattern
    EXPECT(fm_top_rows(0, 0, 10) == 0 && fm_top_rows(3, 0, 10) == 3 && fm_top_rows(10, 0, 10) == 10 && fm_top_rows(11, 0, 10) == 10);
    EXPECT(fm_top_rows(1004, 1000, 10) == 4 && fm_top_rows(1004, 1004, 10) == 0 && fm_top_rows(1004, 0x7fffffff, 10) == 0);
    EXPECT(fm_top_rows(0x7fffffff, 0, 1 << 27) == (1 << 27) && fm_top_rows(5, 4, 1) == 1 && fm_top_rows(5, 5, 1) == 0);
    // the arguments the C ABI refuses
    {
        const int32_t len[] = {5, 0, 3}, neg[] = {5, -1, 3};
        const uint8_t desc[] = {1, 0, 7};
        EXPECT(fm_top_args_bad(3, len, desc, 0, 0, 1) == 0 && fm_top_args_bad(3, len, desc, 9, 0x7fffffff, 1 << 20) == 0);
        EXPECT(fm_top_args_bad(0, nullptr, nullptr, 0, 0, 1) == 0 && fm_top_args_bad(1, len, desc, 0, 0, 1 << 27) == 0);
        EXPECT(fm_top_args_bad(3, len, desc, -1, 0, 1) == 1 && fm_top_args_bad(3, len, desc, 10, 0, 1) == 1);
        EXPECT(fm_top_args_bad(3, neg, desc, 0, 0, 1) == 2 && fm_top_args_bad(3, len, desc, 0, -1, 1) == 3);
        EXPECT(fm_top_args_bad(3, len, desc, 0, 0, 0) == 4 && fm_top_args_bad(3, len, desc, 0, 0, -5) == 4);
        EXPECT(fm_top_args_bad(3, len, desc, 0, 0, (1 << 27) / 3 + 1) == 5 && fm_top_args_bad(2, len, desc, 0, 0, (1 << 26) + 1) == 5);
        EXPECT(fm_top_args_bad(3, nullptr, desc, 0, 0, 1) == 6 && fm_top_args_bad(3, len, nullptr, 0, 0, 1) == 6);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "self")) {
        self_checks();
        return g_failed ? 4 : 0;
    }
    if (argc < 4 || strcmp(argv[1], "top")) return 2;
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 2;
    std::vector<int64_t> head, win_off, hit_off;
    std::vector<uint16_t> win;
    std::vector<int32_t> T, term_len, locs;
    std::vector<uint8_t> descending;
    if (!get(in, head, 8)) return 2;
    const int32_t n = (int32_t)head[0], count = (int32_t)head[2], F = (int32_t)head[4], text_len = (int32_t)head[5];
    const int32_t first_rank = (int32_t)head[6], top = (int32_t)head[7];
    const int64_t n_hits = head[1];
    if (!get(in, T, (size_t)count) || !get(in, term_len, (size_t)n) || !get(in, descending, (size_t)n) || !get(in, hit_off, (size_t)n + 1) ||
        !get(in, locs, (size_t)n_hits) || !get(in, win_off, (size_t)n_hits + 1) || !get(in, win, (size_t)win_off.back()))
        return 2;
    fclose(in);
    if (fm_top_args_bad(n, term_len.data(), descending.data(), F, first_rank, top)) return 2;
    int32_t n_fences = 0;
    const int32_t shift = fm_line_fence_shift(count, (int32_t)head[3], n_fences);
    std::vector<int32_t> fence((size_t)n_fences);
    for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = T[(size_t)((int64_t)j << shift)];
    const size_t H = (size_t)n_hits;
    // k_top_keys: tile by tile, lane by lane
    const int32_t pos_bits = fm_bits((uint32_t)text_len);
    const uint64_t no_hit = fm_first_key(n, 0, pos_bits);
    std::vector<uint64_t> keys(H, ~(uint64_t)0), u(H, ~(uint64_t)0), tail(H + 1, ~(uint64_t)0), tail_pos(H + 1, 0);
    std::vector<int32_t> start(H, -1), stop(H, -1);
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
                keys[(size_t)t] = fm_first_key(p, locs[(size_t)t], pos_bits);
            } else {
                keys[(size_t)t] = no_hit;
                start[(size_t)t] = stop[(size_t)t] = 0;
            }
        }
    }
    // k_top_parse, and the ranking kept line by line: (pattern, line) -> the best (u, position)
    std::map<std::pair<int32_t, int32_t>, TopCand> direct;
    std::vector<int32_t> direct_num((size_t)n, 0), direct_nn((size_t)n, 0), direct_ov((size_t)n, 0);
    for (int64_t t = 0; t <= n_hits; ++t) {
        if (t == n_hits) {
            tail[(size_t)t] = 0;
            continue;
        }
        const int32_t p = fm_first_key_pattern(keys[(size_t)t], pos_bits);
        if (p >= n) {
            u[(size_t)t] = 0;
            tail[(size_t)t] = 0;
            continue;
        }
        const int64_t at = win_off[(size_t)t];
        const int32_t len = (int32_t)(win_off[(size_t)t + 1] - at);
        if (len != stop[(size_t)t] - start[(size_t)t]) return 5;
        int64_t v;
        const int32_t kind = fm_num_parse(win.data() + at, len, F, v);
        if (kind != kNumOk) keys[(size_t)t] = no_hit;
        u[(size_t)t] = kind == kNumOk ? fm_top_ordered(v, descending[(size_t)p] != 0) : 0;
        tail[(size_t)t] = fm_range_tail(fm_top_tail_code(kind));
        direct_num[(size_t)p] += kind == kNumOk;
        direct_nn[(size_t)p] += kind == kNumNotNumber;
        direct_ov[(size_t)p] += kind == kNumOverflow;
        if (kind == kNumOk) {
            const int32_t line = fm_line_of(T.data(), count, nullptr, 0, 0, locs[(size_t)t]);
            const TopCand c{u[(size_t)t], (int64_t)locs[(size_t)t]};
            auto it = direct.find({p, line});
            if (it == direct.end())
                direct[{p, line}] = c;
            else if (c.u < it->second.u || (c.u == it->second.u && c.loc < it->second.loc))
                it->second = c;
        }
    }
    // rocPRIM: the exclusive scan of the reasons' words, the sort by pattern | position
    for (size_t t = 1; t <= H; ++t) tail_pos[t] = tail_pos[t - 1] + tail[t - 1];
    std::vector<int64_t> order(H);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return keys[(size_t)a] < keys[(size_t)b]; });
    const int32_t key_bits = fm_bits((uint32_t)n) + pos_bits;
    // k_top_lines
    std::vector<uint64_t> run_key(H);
    std::vector<TopCand> run_cand(H);
    for (size_t i = 0; i < H; ++i) {
        const uint64_t key = keys[(size_t)order[i]];
        if (key_bits < 64 && (key >> key_bits) != 0) return 3;  // (the sort looks at key_bits bits)
        const int32_t p = fm_first_key_pattern(key, pos_bits);
        if (p < n) {
            const int32_t loc = fm_first_key_loc(key, pos_bits);
            run_key[i] = fm_top_line_key(p, fm_line_of(T.data(), count, fence.data(), n_fences, shift, loc));
            run_cand[i] = TopCand{u[(size_t)order[i]], (int64_t)loc};
        } else {
            run_key[i] = fm_top_line_key(n, 0);
            run_cand[i] = TopCand{0, 0};
        }
        if (i > 0 && run_key[i] < run_key[i - 1]) return 3;  // (lines never decrease within a pattern)
    }
    // k_top_fill, reduce_by_key: a fold per run, from the left and from the right
    std::vector<uint64_t> cand_key(H, fm_top_line_key(n, 0));
    std::vector<TopCand> cand(H, TopCand{~(uint64_t)0, -1});
    size_t runs = 0;
    const TopBetter better;
    for (size_t i = 0; i < H;) {
        size_t j = i + 1;
        while (j < H && run_key[j] == run_key[i]) ++j;
        TopCand left = run_cand[i], right = run_cand[j - 1];
        for (size_t k = i + 1; k < j; ++k) left = better(left, run_cand[k]);
        for (size_t k = j - 1; k-- > i;) right = better(run_cand[k], right);
        if (!same(left, right)) return 3;
        cand_key[runs] = run_key[i];
        cand[runs] = left;
        ++runs;
        i = j;
    }
    // k_top_cands, the stable sort by u; k_top_patterns, the stable sort by pattern
    std::vector<uint64_t> cand_u(H);
    std::vector<uint32_t> idx(H), pat(H);
    for (size_t i = 0; i < H; ++i) {
        cand_u[i] = fm_top_line_key_pattern(cand_key[i]) < n ? cand[i].u : 0;
        if ((cand_u[i] >> 63) != 0) return 3;  // (the sort by u looks at 63 bits)
        idx[i] = (uint32_t)i;
    }
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return cand_u[a] < cand_u[b]; });
    std::stable_sort(idx.begin(), idx.end(),
                     [&](uint32_t a, uint32_t b) { return fm_top_line_key_pattern(cand_key[a]) < fm_top_line_key_pattern(cand_key[b]); });
    for (size_t i = 0; i < H; ++i) pat[i] = (uint32_t)fm_top_line_key_pattern(cand_key[idx[i]]);
    // k_top_tails, k_top_rows
    const size_t cells = (size_t)n * (size_t)top;
    std::vector<int64_t> seg((size_t)n + 1);
    std::vector<int32_t> rows((size_t)n), lines((size_t)n), numbers((size_t)n), nn((size_t)n), ov((size_t)n), row_line(cells), row_loc(cells);
    std::vector<int64_t> row_value(cells);
    for (int32_t p = 0; p <= n; ++p) {
        const int64_t lo = fm_top_segment(pat.data(), n_hits, p);
        seg[(size_t)p] = lo;
        if (p == n) continue;
        const int64_t c = fm_top_segment(pat.data(), n_hits, p + 1) - lo;
        const int64_t a = fm_filter_slot(hit_off[(size_t)p], n_hits), b = fm_filter_slot(hit_off[(size_t)p + 1], n_hits);
        nn[(size_t)p] = fm_range_not_number(tail_pos.data(), a, b);
        ov[(size_t)p] = fm_range_overflow(tail_pos.data(), a, b);
        rows[(size_t)p] = fm_top_rows(c, first_rank, top);
        lines[(size_t)p] = (int32_t)c;
        numbers[(size_t)p] = (int32_t)(b - a) - nn[(size_t)p] - ov[(size_t)p];
        if (nn[(size_t)p] != direct_nn[(size_t)p] || ov[(size_t)p] != direct_ov[(size_t)p] || numbers[(size_t)p] != direct_num[(size_t)p]) return 3;
    }
    for (size_t r = 0; r < cells; ++r) {
        const int64_t p = (int64_t)(r / (size_t)top), rank = (int64_t)first_rank + (int64_t)(r - (size_t)p * (size_t)top), lo = seg[(size_t)p];
        if (rank < seg[(size_t)p + 1] - lo) {
            const uint32_t c = idx[(size_t)(lo + rank)];
            row_line[r] = fm_top_line_key_line(cand_key[c]);
            row_loc[r] = (int32_t)cand[c].loc;
            row_value[r] = fm_top_value(cand[c].u, descending[(size_t)p] != 0);
        }
    }
    // the ranking kept line by line: per pattern the candidates by (u, line)
    for (int32_t p = 0; p < n; ++p) {
        std::vector<std::pair<uint64_t, int32_t>> ranked;
        std::map<int32_t, TopCand> mine;
        for (const auto &kv : direct)
            if (kv.first.first == p) {
                ranked.push_back({kv.second.u, kv.first.second});
                mine[kv.first.second] = kv.second;
            }
        std::sort(ranked.begin(), ranked.end());
        if ((int64_t)ranked.size() != lines[(size_t)p]) return 3;
        for (int32_t j = 0; j < top; ++j) {
            const size_t r = (size_t)p * (size_t)top + (size_t)j;
            const int64_t rank = (int64_t)first_rank + j;
            if (rank < (int64_t)ranked.size()) {
                const TopCand &c = mine[ranked[(size_t)rank].second];
                if (j >= rows[(size_t)p] || row_line[r] != ranked[(size_t)rank].second || row_loc[r] != (int32_t)c.loc ||
                    row_value[r] != fm_top_value(c.u, descending[(size_t)p] != 0))
                    return 3;
            } else if (j < rows[(size_t)p] || row_line[r] != 0 || row_loc[r] != 0 || row_value[r] != 0) {
                return 3;
            }
        }
    }
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    put(out, rows);
    put(out, row_line);
    put(out, row_value);
    put(out, row_loc);
    put(out, lines);
    put(out, numbers);
    put(out, nn);
    put(out, ov);
    put(out, start);
    put(out, stop);
    return fclose(out) == 0 ? 0 : 2;
}
