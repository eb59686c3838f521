// distinct_hostsim.cpp — TEST-ONLY host build of the device code of "the distinct values of a field per bucket of lines"
// (fmx_values_distinct_histogram_dev): index4j_amd/csrc/fmx_distinct.hpp's fm_dv_shape_bad, fm_dv_key*, fm_dv_hit_key,
// fm_dv_head_key, fm_dv_is_head, fm_dv_is_first, fm_dv_head_of and fm_dv_counts — with fm_hit_tile / fm_hit_pattern for a slot's
// pattern, fm_line_of over fences for its line and fm_hist_bucket for its bucket — driven by a mirror of the five steps of
// fmx_distinct.hip with the lanes run one after the other: k_dv_keys' tile loop; std::stable_sort for rocPRIM's; k_dv_heads;
// std::stable_sort again; k_dv_counts.  The counters are checked against a std::set of (pattern, group, bucket) filled hit by hit.
// g++ compiles the header's functions as plain C++, so the CPU suite checks the source of those FUNCTIONS
// (tests/test_distinct_values_cpu.py).  The kernels' own route runs in tests/test_gpu_distinct_values.py only.  Never part of
// libfmx.so.
//
// A stand-alone program:
//   distinct_hostsim self          the per-item functions at their edges (below); exit status 4 and a line on stderr where one fails
//   distinct_hostsim run IN OUT    IN   int64 {n, n_hits, count, max_fences, n_edges, G}, int32 T[count], int64 hit_off[n + 1],
//                                       int32 locs[n_hits], int32 edges[n_edges] (n_edges == 0: one bucket, every line, T unused),
//                                       int64 val_off[n + 1], int32 group_of_hit[n_hits]
//                                  OUT  int32 distinct[n * B], first_seen[n * B], each with kPad sentinels behind it
// Exit status 3: the sorted-key counters and the set's disagree, or a key is wider than the bits in use.
#include "../index4j_amd/csrc/fmx_distinct.hpp"
#include "../index4j_amd/csrc/fmx_hit_filter.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <tuple>
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
    int32_t n = 0, count = 0, max_fences = 0, n_edges = 0;
    int64_t n_hits = 0, G = 0;
    std::vector<int32_t> T, locs, edges, group_of_hit;
    std::vector<int64_t> hit_off, val_off;
};
struct Answer {
    std::vector<int32_t> distinct, first_seen;
};

// the five steps, lane by lane; 0, or the exit status
int run(const Call &c, Answer &out) {
    const int32_t n = c.n, B = c.n_edges > 0 ? c.n_edges - 1 : 1;
    const int64_t n_hits = c.n_hits;
    int64_t max_groups = 0;
    if (fm_dv_shape_bad(n, c.val_off.data(), B, &max_groups) || c.val_off[(size_t)n] != c.G) return 2;
    // 1. keys: k_dv_keys, tile by tile, lane by lane
    int32_t n_fences = 0;
    const int32_t shift = c.n_edges > 0 ? fm_line_fence_shift(c.count, c.max_fences, n_fences) : 0;
    std::vector<int32_t> fence((size_t)n_fences);
    for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = c.T[(size_t)((int64_t)j << shift)];
    const int32_t group_bits = fm_bits((uint32_t)max_groups), bucket_bits = fm_bits((uint32_t)B), width = fm_dv_key_width(n, max_groups, B);
    if (width > 60) return 3;
    const uint64_t no_hit = fm_dv_key(n, 0, 0, group_bits, bucket_bits);
    std::vector<uint64_t> keys((size_t)n_hits, ~(uint64_t)0);
    std::set<std::tuple<int32_t, int32_t, int32_t>> direct;  // (pattern, group, bucket) of every hit that counts
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
                const int64_t groups = c.val_off[(size_t)p + 1] - c.val_off[(size_t)p];
                const int32_t g = c.group_of_hit[(size_t)t];
                const uint64_t key = fm_dv_hit_key(n, p, groups, g, b, B, group_bits, bucket_bits);
                keys[(size_t)t] = key;
                if (b < B && g >= 0 && g < groups) {
                    if (fm_dv_key_pattern(key, group_bits, bucket_bits) != p || fm_dv_key_group(key, group_bits, bucket_bits) != g ||
                        fm_dv_key_bucket(key, bucket_bits) != b)
                        return 3;
                    direct.insert({p, g, b});
                } else if (key != no_hit) {
                    return 3;
                }
            } else {
                keys[(size_t)t] = no_hit;
            }
        }
    }
    // 2. the sort (rocPRIM's radix sort over `width` bits)
    std::stable_sort(keys.begin(), keys.end());
    if (!keys.empty() && (keys.back() >> width) != 0) return 3;
    // 3. k_dv_heads
    std::vector<uint64_t> heads((size_t)n_hits);
    for (int64_t j = 0; j < n_hits; ++j) heads[(size_t)j] = fm_dv_head_of(keys.data(), j, n, group_bits, bucket_bits);
    // 4. the second sort, over fm_dv_head_key_width bits
    std::stable_sort(heads.begin(), heads.end());
    if (!heads.empty() && (heads.back() >> fm_dv_head_key_width(n, B)) != 0) return 3;
    // 5. k_dv_counts, against the set: its (pattern, group) runs are in order of the bucket, so a run's first entry is the first
    std::vector<int32_t> want_distinct((size_t)n * B, 0), want_first((size_t)n * B, 0);
    {
        int32_t last_p = -1, last_g = -1;
        for (const auto &e : direct) {
            const int32_t p = std::get<0>(e), g = std::get<1>(e), b = std::get<2>(e);
            ++want_distinct[(size_t)p * B + b];
            if (p != last_p || g != last_g) ++want_first[(size_t)p * B + b];
            last_p = p;
            last_g = g;
        }
    }
    out.distinct.assign((size_t)n * B + kPad, kSentinel);
    out.first_seen.assign((size_t)n * B + kPad, kSentinel);
    for (int64_t i = 0; i < (int64_t)n * B; ++i) {
        const int32_t p = (int32_t)(i / B);
        int32_t d, f;
        fm_dv_counts(heads.data(), n_hits, p, (int32_t)(i - (int64_t)p * B), bucket_bits, d, f);
        if (d != want_distinct[(size_t)i] || f != want_first[(size_t)i]) return 3;
        out.distinct[(size_t)i] = d;
        out.first_seen[(size_t)i] = f;
    }
    return 0;
}

void self_checks() {
    // the shape: val_off's rules, the limit on the counters, the largest pattern
    {
        const int64_t v[] = {0, 0, 3, 4, 9}, neg[] = {1, 2}, down[] = {0, 3, 2}, huge[] = {0, (int64_t)1 << 31}, most[] = {0, 0x7fffffff};
        int64_t m = -1;
        EXPECT(fm_dv_shape_bad(4, v, 8, &m) == 0 && m == 5 && fm_dv_shape_bad(0, v, 8, &m) == 0 && m == 0);
        EXPECT(fm_dv_shape_bad(1, neg, 8, nullptr) == 2 && fm_dv_shape_bad(2, down, 8, nullptr) == 2 && fm_dv_shape_bad(1, huge, 8, nullptr) == 2);
        EXPECT(fm_dv_shape_bad(1, most, 1 << 27, &m) == 0 && m == 0x7fffffff && fm_dv_shape_bad(1, most, (1 << 27) + 1, nullptr) == 3);
        EXPECT(fm_dv_shape_bad(4, v, 1 << 25, nullptr) == 0 && fm_dv_shape_bad(4, v, (1 << 25) + 1, nullptr) == 3);
    }
    // the key's packing and unpacking at the narrowest and the widest widths: n * B = 2^27 and G = 2^31 - 1 stay at 60 bits or below
    EXPECT(fm_dv_key_width(1, 0, 1) == 3 && fm_dv_key_width(1, 1, 1) == 3 && fm_dv_head_key_width(1, 1) == 3);
    {
        struct Shape {
            int32_t n, B;
            int64_t G;
        };
        for (const Shape s : {Shape{1, 1, 0}, Shape{1, 1, 1}, Shape{3, 60, 10}, Shape{1, 1 << 27, 0x7fffffff}, Shape{1 << 27, 1, 0x7fffffff},
                              Shape{1 << 13, 1 << 14, 0x7fffffff}, Shape{(1 << 14) - 1, 1 << 13, 0x7fffffff}, Shape{5, 8, 0x7fffffff}}) {
            const int32_t gb = fm_bits((uint32_t)s.G), bb = fm_bits((uint32_t)s.B), width = fm_dv_key_width(s.n, s.G, s.B);
            EXPECT((int64_t)s.n * s.B <= kHistCellsMax && width <= 60 && fm_dv_head_key_width(s.n, s.B) <= 30);
            if (s.n == 1 << 13) EXPECT(width == 60 && fm_dv_head_key_width(s.n, s.B) == 30);
            const int32_t G = (int32_t)s.G;
            for (const int32_t p : {0, 1, s.n / 2, s.n - 1, s.n})
                for (const int32_t g : {0, 1, G / 2, G > 0 ? G - 1 : 0})
                    for (const int32_t b : {0, 1, s.B / 2, s.B - 1, s.B}) {
                        const uint64_t k = fm_dv_key(p, g, b, gb, bb);
                        EXPECT(fm_dv_key_pattern(k, gb, bb) == p && fm_dv_key_group(k, gb, bb) == g && fm_dv_key_bucket(k, bb) == b);
                        EXPECT((k >> width) == 0);
                        if (p < s.n) EXPECT(fm_dv_key(p + 1, 0, 0, gb, bb) > fm_dv_key(p, G, s.B, gb, bb));
                        if (p < s.n && b < s.B) {  // the head key: the first in front, key + 2 the next bucket, the last bucket stays in its pattern
                            const uint64_t hk = fm_dv_head_key(p, b, true, bb);
                            EXPECT(fm_dv_head_key(p, b, false, bb) == hk + 1 && fm_dv_head_key(p, b + 1, true, bb) == hk + 2);
                            EXPECT((hk >> (bb + 1)) == (uint64_t)p && ((hk + 2) >> (bb + 1)) == (uint64_t)p);
                            EXPECT(((hk + 2) >> fm_dv_head_key_width(s.n, s.B)) == 0 && hk + 2 <= fm_dv_head_key(s.n, 0, true, bb));
                        }
                    }
            // what counts nowhere gets the key of pattern n
            const uint64_t none = fm_dv_key(s.n, 0, 0, gb, bb);
            EXPECT(fm_dv_hit_key(s.n, 0, s.G, -1, 0, s.B, gb, bb) == none && fm_dv_hit_key(s.n, 0, s.G, G, 0, s.B, gb, bb) == none);
            EXPECT(fm_dv_hit_key(s.n, 0, s.G, 0, s.B, s.B, gb, bb) == none);
            if (G > 0) EXPECT(fm_dv_hit_key(s.n, s.n - 1, s.G, G - 1, s.B - 1, s.B, gb, bb) == fm_dv_key(s.n - 1, G - 1, s.B - 1, gb, bb));
        }
    }
    // heads and firsts: j = 0, a run of equal keys, a new bucket of the same group, a new group, a new pattern whose first group and
    // bucket equal the last ones of the pattern in front, the slots of pattern n
    {
        const int32_t n = 3, gb = fm_bits(2), bb = fm_bits(4);
        const std::vector<uint64_t> k{fm_dv_key(0, 0, 1, gb, bb), fm_dv_key(0, 0, 1, gb, bb), fm_dv_key(0, 0, 3, gb, bb), fm_dv_key(0, 1, 3, gb, bb),
                                      fm_dv_key(1, 1, 3, gb, bb), fm_dv_key(1, 1, 3, gb, bb), fm_dv_key(2, 0, 0, gb, bb), fm_dv_key(3, 0, 0, gb, bb),
                                      fm_dv_key(3, 0, 0, gb, bb)};
        const bool head[] = {true, false, true, true, true, false, true, false, false}, first[] = {true, false, false, true, true, false, true, false, false};
        const uint64_t none = fm_dv_head_key(n, 0, true, bb);
        for (int64_t j = 0; j < (int64_t)k.size(); ++j) {
            EXPECT(fm_dv_is_head(k.data(), j, n, gb, bb) == head[j]);
            if (head[j]) EXPECT(fm_dv_is_first(k.data(), j, bb) == first[j]);
            const uint64_t want = head[j] ? fm_dv_head_key(fm_dv_key_pattern(k[(size_t)j], gb, bb), fm_dv_key_bucket(k[(size_t)j], bb), first[j], bb) : none;
            EXPECT(fm_dv_head_of(k.data(), j, n, gb, bb) == want);
        }
        const std::vector<uint64_t> lone{fm_dv_key(3, 0, 0, gb, bb)};  // j = 0 of a block without a hit
        EXPECT(!fm_dv_is_head(lone.data(), 0, n, gb, bb) && fm_dv_head_of(lone.data(), 0, n, gb, bb) == none);
    }
    // the three bounds: an empty bucket, a bucket whose keys are all firsts, one with none, one with both, the last bucket of the last
    // pattern in front of the slots of pattern n, no slot at all
    {
        const int32_t n = 2, B = 4, bb = fm_bits(4);
        const std::vector<uint64_t> h{fm_dv_head_key(0, 0, true, bb),  fm_dv_head_key(0, 0, true, bb),  fm_dv_head_key(0, 2, false, bb),
                                      fm_dv_head_key(0, 2, false, bb), fm_dv_head_key(0, 2, false, bb), fm_dv_head_key(0, 3, true, bb),
                                      fm_dv_head_key(0, 3, false, bb), fm_dv_head_key(1, 3, true, bb),  fm_dv_head_key(1, 3, false, bb),
                                      fm_dv_head_key(1, 3, false, bb), fm_dv_head_key(n, 0, true, bb),  fm_dv_head_key(n, 0, true, bb)};
        const int32_t want_d[] = {2, 0, 3, 2, 0, 0, 0, 3}, want_f[] = {2, 0, 0, 1, 0, 0, 0, 1};
        for (int32_t i = 0; i < n * B; ++i) {
            int32_t d = -1, f = -1;
            fm_dv_counts(h.data(), (int64_t)h.size(), i / B, i % B, bb, d, f);
            EXPECT(d == want_d[i] && f == want_f[i]);
            fm_dv_counts(h.data(), 0, i / B, i % B, bb, d, f);
            EXPECT(d == 0 && f == 0);
        }
        int32_t d = -1, f = -1;  // without the slots of pattern n behind: the searches end at the array's end
        fm_dv_counts(h.data(), 10, 1, 3, bb, d, f);
        EXPECT(d == 3 && f == 1);
    }
    // a whole call: three patterns, the one in the middle without hits, hits in no bucket, a slot without a group, slots in front and behind
    {
        Call c;
        c.n = 3;
        c.n_edges = 3;
        c.edges = {0, 2, 3};
        c.T = {10, 20, 30};  // the lines: [0, 10], [11, 20], [21, 30], [31, ..)
        c.count = 3;
        c.max_fences = 2;
        c.hit_off = {1, 7, 7, 9};
        c.n_hits = 10;
        c.locs = {-5, 5, 15, 25, 35, 12, 1, 22, 3, -5};
        c.val_off = {0, 3, 3, 4};
        c.G = 4;
        c.group_of_hit = {-1, 1, 1, 2, 0, 0, -1, 0, 0, -1};
        Answer a;
        EXPECT(run(c, a) == 0);
        // pattern 0: group 1 in bucket 0 twice, group 2 in bucket 1, group 0 at 35 in no bucket and at 12 in bucket 0, a slot without a
        // group; pattern 2: group 0 in bucket 1 (line 2) and in bucket 0 (line 0): its first is bucket 0
        const int32_t distinct[] = {2, 1, 0, 0, 1, 1}, first[] = {2, 1, 0, 0, 1, 0};
        for (int i = 0; i < 6; ++i) EXPECT(a.distinct[(size_t)i] == distinct[i] && a.first_seen[(size_t)i] == first[i]);
        EXPECT(a.distinct[6] == kSentinel && a.first_seen[6] == kSentinel);
        c.n_edges = 0;  // no edges: one bucket, no line is looked up, the hit at 35 counts
        c.edges.clear();
        EXPECT(run(c, a) == 0);
        EXPECT(a.distinct[0] == 3 && a.distinct[1] == 0 && a.distinct[2] == 1 && a.first_seen[0] == 3 && a.first_seen[2] == 1 && a.distinct[3] == kSentinel);
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
    if (!get(in, head, 6)) return 2;
    c.n = (int32_t)head[0];
    c.n_hits = head[1];
    c.count = (int32_t)head[2];
    c.max_fences = (int32_t)head[3];
    c.n_edges = (int32_t)head[4];
    c.G = head[5];
    if (!get(in, c.T, (size_t)c.count) || !get(in, c.hit_off, (size_t)c.n + 1) || !get(in, c.locs, (size_t)c.n_hits) ||
        !get(in, c.edges, (size_t)c.n_edges) || !get(in, c.val_off, (size_t)c.n + 1) || !get(in, c.group_of_hit, (size_t)c.n_hits))
        return 2;
    fclose(in);
    if (c.n_edges > 0 && fm_hist_edges_bad(c.edges.data(), c.n_edges)) return 2;
    Answer a;
    if (const int rc = run(c, a)) return rc;
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    put(out, a.distinct);
    put(out, a.first_seen);
    return fclose(out) == 0 ? 0 : 2;
}
