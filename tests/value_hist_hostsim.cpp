// value_hist_hostsim.cpp — TEST-ONLY host build of the device code of "the top values of a field per bucket of lines"
// (fmx_values_top_histogram_dev, fmx_values_gather_rows_dev): index4j_amd/csrc/fmx_value_hist.hpp's fm_vh_rank_key*, fm_vh_rank,
// fm_vh_rows, fm_vh_shape_bad, fm_vh_key*, fm_vh_code, fm_vh_count, fm_vh_counter and fm_vh_unit_row — with fm_hit_tile /
// fm_hit_pattern for a slot's pattern, fm_line_of over fences for its line and fm_hist_bucket for its bucket — driven by a mirror of
// the four stages of fmx_value_hist.hip with the lanes run one after the other: k_vh_rank_keys, std::stable_sort for rocPRIM's
// stable sort of the rank keys, k_vh_ranks; k_vh_keys' tile loop; std::sort for rocPRIM's; k_vh_counts.  The counters are checked
// against counters incremented hit by hit.  g++ compiles the header's functions as plain C++, so the CPU suite checks the source of
// those FUNCTIONS (tests/test_field_values_histogram_cpu.py).  The kernels' own route runs in
// tests/test_gpu_field_values_histogram.py only.  Never part of libfmx.so.
//
// A stand-alone program:
//   value_hist_hostsim self          the per-item functions at their edges (below); exit status 4 and a line on stderr where one fails
//   value_hist_hostsim run IN OUT    IN   int64 {n, n_hits, count, max_fences, n_edges, top, G}, int32 T[count], int64 hit_off[n + 1],
//                                         int32 locs[n_hits], int32 edges[n_edges] (n_edges == 0: one bucket, every line, T unused),
//                                         int64 val_off[n + 1], int32 group_count[G], int32 group_of_hit[n_hits]
//                                    OUT  int64 row_off[n + 1]; int32 row_group[R], row_count[R], hist[R * B], other[n * B], each with
//                                         kPad sentinels behind it; int64 row_text_off[R + 1] for a text of g + 1 units per group g
// Exit status 3: the sorted-key counters and the hit-by-hit counters disagree, or a key is wider than the bits in use.
#include "../index4j_amd/csrc/fmx_hit_filter.hpp"
#include "../index4j_amd/csrc/fmx_value_hist.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace fmx;

namespace {

constexpr int32_t kSentinel = -77;
constexpr size_t kPad = 8;

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

struct Call {
    int32_t n = 0, count = 0, max_fences = 0, n_edges = 0, top = 0;
    int64_t n_hits = 0, G = 0;
    std::vector<int32_t> T, locs, edges, group_count, group_of_hit;
    std::vector<int64_t> hit_off, val_off;
};
struct Answer {
    std::vector<int64_t> row_off, row_text_off;
    std::vector<int32_t> row_group, row_count, hist, other;
};

// the four stages, lane by lane; 0, or the exit status
int run(const Call &c, Answer &out) {
    const int32_t n = c.n, top = c.top, B = c.n_edges > 0 ? c.n_edges - 1 : 1;
    const int64_t n_hits = c.n_hits, G = c.G;
    out.row_off.assign((size_t)n + 1, 0);
    if (fm_vh_shape_bad(n, c.val_off.data(), top, B, out.row_off.data()) || c.val_off[(size_t)n] != G) return 2;
    const int64_t R = out.row_off[(size_t)n];
    // 1. rank: k_vh_rank_keys, the stable sort, k_vh_ranks
    std::vector<uint64_t> rank_keys((size_t)G);
    std::vector<uint32_t> order((size_t)G);
    for (int64_t g = 0; g < G; ++g) {
        const int32_t cnt = c.group_count[(size_t)g];
        rank_keys[(size_t)g] = fm_vh_rank_key(fm_hit_pattern(c.val_off.data(), n, g), cnt < 0 ? 0 : cnt);
        order[(size_t)g] = (uint32_t)g;
        if ((rank_keys[(size_t)g] >> fm_vh_rank_key_width(n)) != 0) return 3;
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rank_keys[a] < rank_keys[b]; });
    std::vector<int32_t> rank_of_group((size_t)G, kSentinel);
    out.row_group.assign((size_t)R + kPad, kSentinel);
    out.row_count.assign((size_t)R + kPad, kSentinel);
    for (int64_t j = 0; j < G; ++j) {
        const uint64_t key = rank_keys[order[(size_t)j]];
        const int32_t p = fm_vh_rank_key_pattern(key);
        const int64_t g = order[(size_t)j], first = c.val_off[(size_t)p];
        const int32_t rank = fm_vh_rank(j, first, top);
        rank_of_group[(size_t)g] = rank;
        if (rank < top) {
            const int64_t row = out.row_off[(size_t)p] + rank;
            if (row >= out.row_off[(size_t)p + 1]) return 3;
            out.row_group[(size_t)row] = (int32_t)(g - first);
            out.row_count[(size_t)row] = fm_vh_rank_key_count(key);
        }
    }
    // 2. keys: k_vh_keys, tile by tile, lane by lane
    int32_t n_fences = 0;
    const int32_t shift = c.n_edges > 0 ? fm_line_fence_shift(c.count, c.max_fences, n_fences) : 0;
    std::vector<int32_t> fence((size_t)n_fences);
    for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = c.T[(size_t)((int64_t)j << shift)];
    const int32_t code_bits = fm_bits((uint32_t)top), bucket_bits = fm_bits((uint32_t)B), width = fm_vh_key_width(n, top, B);
    const uint64_t no_hit = fm_vh_key(n, 0, 0, code_bits, bucket_bits);
    std::vector<uint64_t> keys((size_t)n_hits, ~(uint64_t)0);
    std::vector<int32_t> direct((size_t)(R + n) * B, 0);
    const int64_t first = fm_filter_slot(c.hit_off[0], n_hits), total = fm_filter_slot(c.hit_off[(size_t)n], n_hits);
    for (int64_t tile = 0; tile < n_hits; tile += kLocateAllTile) {
        if (tile >= total || tile + kLocateAllTile <= first) {
            for (int64_t t = tile; t < tile + kLocateAllTile && t < n_hits; ++t) keys[(size_t)t] = no_hit;
            continue;
        }
        const HitTile h = fm_hit_tile(c.hit_off.data(), n, tile, total);
        const int64_t *slice = c.hit_off.data() + h.p_lo;
        for (int64_t t = tile; t < tile + kLocateAllTile && t < n_hits; ++t) {
            if (t >= first && t <= h.tile_last) {
                const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
                int32_t b = 0;
                if (c.n_edges > 0)
                    b = fm_hist_bucket(c.edges.data(), c.n_edges, fm_line_of(c.T.data(), c.count, fence.data(), n_fences, shift, c.locs[(size_t)t]));
                const int64_t g0 = c.val_off[(size_t)p];
                const int32_t code = fm_vh_code(rank_of_group.data(), g0, c.val_off[(size_t)p + 1] - g0, c.group_of_hit[(size_t)t], top);
                keys[(size_t)t] = fm_vh_key(p, code, b, code_bits, bucket_bits);
                if (fm_vh_key_pattern(keys[(size_t)t], code_bits, bucket_bits) != p || fm_vh_key_code(keys[(size_t)t], code_bits, bucket_bits) != code ||
                    fm_vh_key_bucket(keys[(size_t)t], bucket_bits) != b)
                    return 3;
                if (b < B) ++direct[(size_t)((code < top ? out.row_off[(size_t)p] + code : R + p) * B + b)];
            } else {
                keys[(size_t)t] = no_hit;
            }
        }
    }
    // 3. the sort (rocPRIM's radix sort over `width` bits)
    std::sort(keys.begin(), keys.end());
    if (width < 64 && !keys.empty() && (keys.back() >> width) != 0) return 3;
    // 4. k_vh_counts
    out.hist.assign((size_t)(R * B) + kPad, kSentinel);
    out.other.assign((size_t)n * B + kPad, kSentinel);
    for (int64_t i = 0; i < (R + n) * B; ++i) {
        int32_t p, code, b;
        fm_vh_counter(out.row_off.data(), n, R, B, top, i, p, code, b);
        const int32_t cnt = fm_vh_count(keys.data(), c.hit_off.data(), n_hits, first, p, code, b, code_bits, bucket_bits);
        if (cnt != direct[(size_t)i]) return 3;
        if (i < R * B)
            out.hist[(size_t)i] = cnt;
        else
            out.other[(size_t)(i - R * B)] = cnt;
    }
    // the gather's offsets and rows over a text of g + 1 units per group g (k_vh_row_sources, k_vh_row_lengths, the scan, k_vh_gather's search)
    out.row_text_off.assign((size_t)R + 1, 0);
    for (int64_t r = 0; r < R; ++r) {
        const int64_t src = c.val_off[(size_t)fm_hit_pattern(out.row_off.data(), n, r)] + out.row_group[(size_t)r];
        out.row_text_off[(size_t)r + 1] = out.row_text_off[(size_t)r] + (src % 3 == 2 ? 0 : src + 1);  // (every third group's text is empty)
    }
    for (int64_t u = 0; u < out.row_text_off[(size_t)R]; ++u) {
        const int64_t r = fm_vh_unit_row(out.row_text_off.data(), R, u);
        if (u < out.row_text_off[(size_t)r] || u >= out.row_text_off[(size_t)r + 1]) return 3;
    }
    return 0;
}

void self_checks() {
    // the rank key: the larger count sorts first, the pattern above the count; pack and unpack at both ends
    EXPECT(fm_vh_rank_key(0, INT32_MAX) == 0 && fm_vh_rank_key(0, 0) == 0x7fffffffu && fm_vh_rank_key(1, INT32_MAX) == ((uint64_t)1 << 31));
    EXPECT(fm_vh_rank_key(3, 10) < fm_vh_rank_key(3, 9) && fm_vh_rank_key(3, 0) < fm_vh_rank_key(4, INT32_MAX));
    for (const int32_t p : {0, 1, 0x7ffffffe})
        for (const int32_t c : {0, 1, 12345, INT32_MAX}) {
            const uint64_t k = fm_vh_rank_key(p, c);
            EXPECT(fm_vh_rank_key_pattern(k) == p && fm_vh_rank_key_count(k) == c && (k >> fm_vh_rank_key_width(p + 1)) == 0);
        }
    EXPECT(fm_vh_rank_key_width(1) == 32 && fm_vh_rank_key_width(0x7fffffff) == 62);
    // rank = top - 1 is the last row, rank = top and everything behind it is "other"
    EXPECT(fm_vh_rank(10, 10, 4) == 0 && fm_vh_rank(13, 10, 4) == 3 && fm_vh_rank(14, 10, 4) == 4 && fm_vh_rank(0x7fffffff, 10, 4) == 4);
    EXPECT(fm_vh_rank(65535, 0, 65536) == 65535 && fm_vh_rank(65536, 0, 65536) == 65536);
    EXPECT(fm_vh_rows(0, 5) == 0 && fm_vh_rows(4, 5) == 4 && fm_vh_rows(5, 5) == 5 && fm_vh_rows(6, 5) == 5);
    // the shape: top's interval, val_off's rules, the limit on the counters, the rows
    {
        const int64_t v[] = {0, 0, 3, 4, 9}, neg[] = {1, 2}, down[] = {0, 3, 2}, huge[] = {0, (int64_t)1 << 31};
        int64_t r[5];
        EXPECT(fm_vh_shape_bad(4, v, 4, 8, r) == 0 && r[0] == 0 && r[1] == 0 && r[2] == 3 && r[3] == 4 && r[4] == 8);
        EXPECT(fm_vh_shape_bad(4, v, 1, 1, r) == 0 && r[4] == 3 && fm_vh_shape_bad(4, v, 65536, 1, r) == 0 && r[4] == 9);
        EXPECT(fm_vh_shape_bad(4, v, 0, 8, nullptr) == 1 && fm_vh_shape_bad(4, v, 65537, 8, nullptr) == 1);
        EXPECT(fm_vh_shape_bad(1, neg, 4, 8, nullptr) == 2 && fm_vh_shape_bad(2, down, 4, 8, nullptr) == 2 && fm_vh_shape_bad(1, huge, 4, 8, nullptr) == 2);
        EXPECT(fm_vh_shape_bad(1, v, 1, 1 << 26, nullptr) == 0 && fm_vh_shape_bad(1, v, 1, (1 << 26) + 1, nullptr) == 3);
        EXPECT(fm_vh_shape_bad(4, v, 65536, 512, nullptr) == 3 && fm_vh_shape_bad(0, v, 4, 8, r) == 0 && r[0] == 0);
    }
    // the key's packing and unpacking at the narrowest and the widest widths (76 bits are stated, 64 are the limit: the widest shapes
    // here fill 64 exactly)
    EXPECT(fm_vh_key_width(1, 1, 1) == 3 && fm_vh_key_width(0x7fffffff, 65536, 1 << 27) == 31 + 17 + 28);
    {
        struct Shape {
            int32_t n, top, B;
        };
        for (const Shape s : {Shape{1, 1, 1}, Shape{3, 10, 60}, Shape{0xffff, 65536, 0x7fff}, Shape{0x7fffffff, 65536, 0xffff}, Shape{0x7ffff, 65536, 1 << 27},
                              Shape{0x7fffffff, 31, 1 << 27}}) {
            const int32_t cb = fm_bits((uint32_t)s.top), bb = fm_bits((uint32_t)s.B), width = fm_vh_key_width(s.n, s.top, s.B);
            EXPECT(width <= 64);
            if (s.n == 0x7fffffff || s.n == 0x7ffff) EXPECT(width == 64);
            for (const int32_t p : {0, 1, s.n / 2, s.n - 1, s.n})
                for (const int32_t c : {0, 1, s.top / 2, s.top - 1, s.top})
                    for (const int32_t b : {0, 1, s.B / 2, s.B - 1, s.B}) {
                        const uint64_t k = fm_vh_key(p, c, b, cb, bb);
                        EXPECT(fm_vh_key_pattern(k, cb, bb) == p && fm_vh_key_code(k, cb, bb) == c && fm_vh_key_bucket(k, bb) == b);
                        EXPECT(width == 64 || (k >> width) == 0);
                        if (b < s.B) EXPECT(fm_vh_key(p, c, b + 1, cb, bb) == k + 1);  // what fm_vh_count's second search relies on
                        if (c < s.top) EXPECT(fm_vh_key(p, c + 1, 0, cb, bb) > fm_vh_key(p, c, s.B, cb, bb));
                        if (p < s.n) EXPECT(fm_vh_key(p + 1, 0, 0, cb, bb) > fm_vh_key(p, s.top, s.B, cb, bb));
                    }
        }
    }
    // the code of a hit: its group's rank; a group outside the pattern's groups is "other"
    {
        const int32_t rank[] = {9, 9, 2, 0, 1, 4};  // the groups 2 .. 5 are the pattern's
        EXPECT(fm_vh_code(rank, 2, 4, 0, 4) == 2 && fm_vh_code(rank, 2, 4, 3, 4) == 4 && fm_vh_code(rank, 2, 4, -1, 4) == 4 && fm_vh_code(rank, 2, 4, 4, 4) == 4);
        EXPECT(fm_vh_code(rank, 2, 0, 0, 4) == 4);
    }
    // the counters: an empty pattern range, a pattern in front of the call's slots, the counter's decoding
    {
        const int32_t cb = fm_bits(2), bb = fm_bits(2);
        std::vector<uint64_t> keys{fm_vh_key(0, 0, 0, cb, bb), fm_vh_key(0, 0, 1, cb, bb), fm_vh_key(0, 2, 1, cb, bb), fm_vh_key(2, 1, 0, cb, bb),
                                   fm_vh_key(2, 1, 0, cb, bb), fm_vh_key(2, 1, 2, cb, bb)};
        const int64_t off[] = {0, 3, 3, 6};
        EXPECT(fm_vh_count(keys.data(), off, 6, 0, 0, 0, 0, cb, bb) == 1 && fm_vh_count(keys.data(), off, 6, 0, 0, 0, 1, cb, bb) == 1);
        EXPECT(fm_vh_count(keys.data(), off, 6, 0, 0, 2, 1, cb, bb) == 1 && fm_vh_count(keys.data(), off, 6, 0, 0, 1, 0, cb, bb) == 0);
        EXPECT(fm_vh_count(keys.data(), off, 6, 0, 1, 0, 0, cb, bb) == 0 && fm_vh_count(keys.data(), off, 6, 0, 1, 2, 1, cb, bb) == 0);  // the empty range
        EXPECT(fm_vh_count(keys.data(), off, 6, 0, 2, 1, 0, cb, bb) == 2 && fm_vh_count(keys.data(), off, 6, 0, 2, 1, 1, cb, bb) == 0);
        EXPECT(fm_vh_count(keys.data(), off, 6, 0, 2, 1, 2, cb, bb) == 1);  // (the bucket B itself: no counter asks, the search still ends inside)
        EXPECT(fm_vh_count(keys.data(), off, 3, 0, 2, 1, 0, cb, bb) == 0);  // fewer slots than hits: pattern 2 lies behind them
        const int64_t row_off[] = {0, 2, 2, 3};
        int32_t p, c, b;
        fm_vh_counter(row_off, 3, 3, 2, 2, 0, p, c, b);
        EXPECT(p == 0 && c == 0 && b == 0);
        fm_vh_counter(row_off, 3, 3, 2, 2, 3, p, c, b);
        EXPECT(p == 0 && c == 1 && b == 1);
        fm_vh_counter(row_off, 3, 3, 2, 2, 4, p, c, b);
        EXPECT(p == 2 && c == 0 && b == 0);  // (pattern 1 has no row)
        fm_vh_counter(row_off, 3, 3, 2, 2, 6, p, c, b);
        EXPECT(p == 0 && c == 2 && b == 0);  // the first "other"
        fm_vh_counter(row_off, 3, 3, 2, 2, 11, p, c, b);
        EXPECT(p == 2 && c == 2 && b == 1);
    }
    // the row of a code unit: empty rows are skipped
    {
        const int64_t off[] = {0, 0, 3, 3, 3, 5};
        EXPECT(fm_vh_unit_row(off, 5, 0) == 1 && fm_vh_unit_row(off, 5, 2) == 1 && fm_vh_unit_row(off, 5, 3) == 4 && fm_vh_unit_row(off, 5, 4) == 4);
        const int64_t one[] = {0, 7};
        EXPECT(fm_vh_unit_row(one, 1, 0) == 0 && fm_vh_unit_row(one, 1, 6) == 0);
    }
    // a whole call: two patterns, ties across the cut, a pattern without groups between them
    {
        Call c;
        c.n = 3;
        c.top = 2;
        c.n_edges = 3;
        c.edges = {0, 2, 3};
        c.T = {10, 20, 30};  // the lines: [0, 10], [11, 20], [21, 30], [31, ..)
        c.count = 3;
        c.max_fences = 2;
        c.hit_off = {1, 6, 6, 8};
        c.n_hits = 9;
        c.locs = {-5, 5, 15, 25, 35, 12, 1, 22, -5};
        c.val_off = {0, 3, 3, 4};
        c.G = 4;
        c.group_count = {1, 2, 2, 2};  // pattern 0: the groups 1 and 2 tie in front of group 0; pattern 2: one group
        c.group_of_hit = {-1, 1, 1, 2, 2, 0, 0, 0, -1};
        Answer a;
        EXPECT(run(c, a) == 0);
        EXPECT(a.row_off == (std::vector<int64_t>{0, 2, 2, 3}));
        EXPECT(a.row_group[0] == 1 && a.row_group[1] == 2 && a.row_group[2] == 0 && a.row_group[3] == kSentinel);
        EXPECT(a.row_count[0] == 2 && a.row_count[1] == 2 && a.row_count[2] == 2);
        const int32_t hist[] = {2, 0, 0, 1, 1, 1}, other[] = {1, 0, 0, 0, 0, 0};  // (the hit at 35 lies in line 3, in no bucket: it is in its row's count only)
        for (int i = 0; i < 6; ++i) EXPECT(a.hist[(size_t)i] == hist[i] && a.other[(size_t)i] == other[i]);
        EXPECT(a.hist[6] == kSentinel && a.other[6] == kSentinel);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "self")) {
        self_checks();
        return g_failed ? 4 : 0;
    }
    if (argc < 4 || strcmp(argv[1], "run")) return 2;
    FILE *in = fopen(argv[2], "rb");
    if (!in) return 2;
    std::vector<int64_t> head;
    Call c;
    if (!get(in, head, 7)) return 2;
    c.n = (int32_t)head[0];
    c.n_hits = head[1];
    c.count = (int32_t)head[2];
    c.max_fences = (int32_t)head[3];
    c.n_edges = (int32_t)head[4];
    c.top = (int32_t)head[5];
    c.G = head[6];
    if (!get(in, c.T, (size_t)c.count) || !get(in, c.hit_off, (size_t)c.n + 1) || !get(in, c.locs, (size_t)c.n_hits) ||
        !get(in, c.edges, (size_t)c.n_edges) || !get(in, c.val_off, (size_t)c.n + 1) || !get(in, c.group_count, (size_t)c.G) ||
        !get(in, c.group_of_hit, (size_t)c.n_hits))
        return 2;
    fclose(in);
    if (c.n_edges > 0 && fm_hist_edges_bad(c.edges.data(), c.n_edges)) return 2;
    Answer a;
    if (const int rc = run(c, a)) return rc;
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    put(out, a.row_off);
    put(out, a.row_group);
    put(out, a.row_count);
    put(out, a.hist);
    put(out, a.other);
    put(out, a.row_text_off);
    return fclose(out) == 0 ? 0 : 2;
}
