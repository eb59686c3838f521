// line_hist_hostsim.cpp — TEST-ONLY host build of the device code of "matching lines and hits per bucket of lines"
// (fmx_lines_histogram_dev, fmx_hits_histogram_dev): index4j_amd/csrc/fmx_line_hist.hpp's fm_hist_rank, fm_hist_between,
// fm_hist_bucket, fm_hist_key*, fm_hist_key_rank, fm_hist_count and fm_hist_edges_bad — with fm_hit_tile / fm_hit_pattern for a
// hit's pattern and fm_line_of over fences for its line — driven by a mirror of the stages of fmx_line_hist.hip with the lanes run
// one after the other: k_hist_ranks and k_hist_diffs; k_hist_keys' tile loop, std::sort for rocPRIM's, k_hist_counts.  The hits
// form is checked against counters incremented hit by hit.  g++ compiles the header's functions as plain C++, so the CPU suite
// checks the source of those FUNCTIONS (tests/test_line_histogram_cpu.py).  The kernels' own route runs in
// tests/test_gpu_line_histogram.py only.  Never part of libfmx.so.
//
// A stand-alone program:
//   line_hist_hostsim self            the per-item functions at their edges (below); exit status 4 and a line on stderr where one fails
//   line_hist_hostsim lines IN OUT    IN   int64 {q, n_edges, n_listed}, int64 line_off[q + 1], int32 lines[n_listed], int32 edges[n_edges]
//                                     OUT  int32 hist[q * B] and kPad sentinels
//   line_hist_hostsim hits IN OUT     IN   int64 {n, n_hits, count, max_fences, n_edges}, int32 T[count], int64 hit_off[n + 1],
//                                          int32 locs[n_hits], int32 edges[n_edges]
//                                     OUT  int32 hist[n * B] and kPad sentinels
// Exit status 3: the sorted-key counters and the hit-by-hit counters disagree.
#include "../index4j_amd/csrc/fmx_hit_filter.hpp"
#include "../index4j_amd/csrc/fmx_line_hist.hpp"

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

// k_hist_ranks and k_hist_diffs, lane by lane
std::vector<int32_t> lines_form(int32_t q, const std::vector<int64_t> &line_off, const std::vector<int32_t> &lines,
                                const std::vector<int32_t> &edges) {
    const int32_t n_edges = (int32_t)edges.size(), B = n_edges - 1;
    std::vector<int64_t> rank((size_t)q * n_edges);
    for (int64_t i = 0; i < (int64_t)q * n_edges; ++i) {
        const int64_t Q = i / n_edges, lo = line_off[(size_t)Q], hi = line_off[(size_t)Q + 1];
        rank[(size_t)i] = hi > lo ? fm_hist_rank(lines.data(), lo, hi, edges[(size_t)(i - Q * n_edges)]) : lo;
    }
    std::vector<int32_t> hist((size_t)q * B + kPad, kSentinel);
    for (int64_t i = 0; i < (int64_t)q * B; ++i) {
        const int64_t Q = i / B, at = Q * n_edges + (i - Q * B);
        hist[(size_t)i] = fm_hist_between(rank[(size_t)at], rank[(size_t)at + 1]);
    }
    return hist;
}

void self_checks() {
    // the bucket of a line at every edge relation: below the first edge, on an edge, between two, on the last, above the last,
    // equal neighbouring edges, an edge beyond the line count (the lines here end at 9)
    const int32_t e[] = {2, 5, 5, 8, 1000};
    const int32_t B = 4;
    EXPECT(fm_hist_bucket(e, 5, 0) == B && fm_hist_bucket(e, 5, 1) == B);  // below the first: no bucket
    EXPECT(fm_hist_bucket(e, 5, 2) == 0);                                   // on the first edge
    EXPECT(fm_hist_bucket(e, 5, 3) == 0 && fm_hist_bucket(e, 5, 4) == 0);  // between
    EXPECT(fm_hist_bucket(e, 5, 5) == 2);                                   // on equal edges: the empty bucket 1 stays empty
    EXPECT(fm_hist_bucket(e, 5, 7) == 2 && fm_hist_bucket(e, 5, 8) == 3 && fm_hist_bucket(e, 5, 9) == 3);
    EXPECT(fm_hist_bucket(e, 5, 999) == 3);                                 // an edge beyond the line count still closes its bucket
    EXPECT(fm_hist_bucket(e, 5, 1000) == B && fm_hist_bucket(e, 5, INT32_MAX) == B);  // on the last edge, above it: no bucket
    const int32_t two[] = {0, 1}, same[] = {3, 3}, zero[] = {0, 0, 0};
    EXPECT(fm_hist_bucket(two, 2, 0) == 0 && fm_hist_bucket(two, 2, 1) == 1 && fm_hist_bucket(two, 2, -1) == 1);
    EXPECT(fm_hist_bucket(same, 2, 2) == 1 && fm_hist_bucket(same, 2, 3) == 1 && fm_hist_bucket(same, 2, 4) == 1);
    EXPECT(fm_hist_bucket(zero, 3, 0) == 2 && fm_hist_bucket(zero, 3, 5) == 2);
    // the rank difference over lists that are empty, that have one entry, that have duplicates
    const std::vector<int32_t> edges(e, e + 5);
    {
        const std::vector<int32_t> lines{4, 1, 2, 2, 5, 5, 5, 7, 999, 1000};  // list 0: nothing; 1: {4}; 2: the rest, with duplicates
        const std::vector<int64_t> off{0, 0, 1, 10};
        const std::vector<int32_t> h = lines_form(3, off, lines, edges);
        const int32_t want[] = {0, 0, 0, 0, 1, 0, 0, 0, 2, 0, 4, 1};
        for (int i = 0; i < 12; ++i) EXPECT(h[(size_t)i] == want[i]);
        for (size_t i = 12; i < h.size(); ++i) EXPECT(h[i] == kSentinel);
        EXPECT(fm_hist_rank(lines.data(), 0, 0, 5) == 0 && fm_hist_rank(lines.data(), 0, 1, 4) == 0 && fm_hist_rank(lines.data(), 0, 1, 5) == 1);
        EXPECT(fm_hist_rank(lines.data(), 1, 10, 5) == 4 && fm_hist_rank(lines.data(), 1, 10, 6) == 7 && fm_hist_rank(lines.data(), 1, 10, 2) == 2);
    }
    // the key's packing and unpacking at 1, 32 and 33 bits in use (the pattern 0 takes no bit; fm_bits never answers 0, so a CALL's
    // narrowest key, n = B = 1, takes 2)
    EXPECT(fm_hist_key_width(1, 1) == 2 && fm_hist_key_width(0x7fffffff, 1 << 27) == 31 + 28);
    {
        EXPECT(fm_hist_key(0, 0, 1) == 0 && fm_hist_key(0, 1, 1) == 1);  // 1 bit
        EXPECT(fm_hist_key_pattern(1, 1) == 0 && fm_hist_key_bucket(1, 1) == 1);
        struct Shape {
            int32_t n, B;
        };
        for (const Shape s : {Shape{1, 1}, Shape{0xffff, 0xffff}, Shape{0x1ffff, 0xffff}, Shape{0xffff, 0x1ffff}, Shape{0x7fffffff, 1 << 27},
                              Shape{15, (1 << 27) - 1}, Shape{(1 << 28) - 1, 15}}) {
            const int32_t bb = fm_bits((uint32_t)s.B), width = fm_hist_key_width(s.n, s.B);
            if (s.n == 0xffff && s.B == 0xffff) EXPECT(width == 32);
            if (s.n == 0x1ffff || s.B == 0x1ffff) EXPECT(width == 33);
            for (const int32_t p : {0, 1, s.n / 2, s.n - 1, s.n})
                for (const int32_t b : {0, 1, s.B / 2, s.B - 1, s.B}) {
                    const uint64_t k = fm_hist_key(p, b, bb);
                    EXPECT(fm_hist_key_pattern(k, bb) == p && fm_hist_key_bucket(k, bb) == b);
                    EXPECT(width == 64 || (k >> width) == 0);
                    if (b < s.B) EXPECT(fm_hist_key(p, b + 1, bb) == k + 1);  // what fm_hist_count's second search relies on
                    if (p < s.n) EXPECT(fm_hist_key(p + 1, 0, bb) > fm_hist_key(p, s.B, bb));
                }
        }
    }
    // the edges the C ABI refuses
    const int32_t neg[] = {-1, 3}, down[] = {0, 4, 3};
    EXPECT(fm_hist_edges_bad(nullptr, 2) == 1 && fm_hist_edges_bad(two, 1) == 1 && fm_hist_edges_bad(neg, 2) == 2);
    EXPECT(fm_hist_edges_bad(down, 3) == 3 && fm_hist_edges_bad(two, 2) == 0 && fm_hist_edges_bad(zero, 3) == 0 && fm_hist_edges_bad(e, 5) == 0);
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
    std::vector<int64_t> head;
    std::vector<int32_t> hist;
    if (!strcmp(argv[1], "lines")) {
        std::vector<int64_t> line_off;
        std::vector<int32_t> lines, edges;
        if (!get(in, head, 3)) return 2;
        const int32_t q = (int32_t)head[0];
        if (!get(in, line_off, (size_t)q + 1) || !get(in, lines, (size_t)head[2]) || !get(in, edges, (size_t)head[1])) return 2;
        if (fm_hist_edges_bad(edges.data(), (int32_t)edges.size())) return 2;
        hist = lines_form(q, line_off, lines, edges);
    } else {
        std::vector<int64_t> hit_off;
        std::vector<int32_t> T, locs, edges;
        if (!get(in, head, 5)) return 2;
        const int32_t n = (int32_t)head[0], count = (int32_t)head[2], n_edges = (int32_t)head[4], B = n_edges - 1;
        const int64_t n_hits = head[1];
        if (!get(in, T, (size_t)count) || !get(in, hit_off, (size_t)n + 1) || !get(in, locs, (size_t)n_hits) || !get(in, edges, (size_t)n_edges))
            return 2;
        if (fm_hist_edges_bad(edges.data(), n_edges)) return 2;
        int32_t n_fences = 0;
        const int32_t shift = fm_line_fence_shift(count, (int32_t)head[3], n_fences);
        std::vector<int32_t> fence((size_t)n_fences);
        for (int32_t j = 0; j < n_fences; ++j) fence[(size_t)j] = T[(size_t)((int64_t)j << shift)];
        // k_hist_keys: tile by tile, lane by lane
        const int32_t bucket_bits = fm_bits((uint32_t)B);
        const uint64_t no_hit = fm_hist_key(n, 0, bucket_bits);
        std::vector<uint64_t> keys((size_t)n_hits, ~(uint64_t)0);
        std::vector<int32_t> direct((size_t)n * B, 0);
        const int64_t first = fm_filter_slot(hit_off[0], n_hits), total = fm_filter_slot(hit_off[(size_t)n], n_hits);
        for (int64_t tile = 0; tile < n_hits; tile += kLocateAllTile) {
            if (tile >= total || tile + kLocateAllTile <= first) {
                for (int64_t t = tile; t < tile + kLocateAllTile && t < n_hits; ++t) keys[(size_t)t] = no_hit;
                continue;
            }
            const HitTile h = fm_hit_tile(hit_off.data(), n, tile, total);
            const int64_t *slice = hit_off.data() + h.p_lo;
            for (int64_t t = tile; t < tile + kLocateAllTile && t < n_hits; ++t) {
                if (t >= first && t <= h.tile_last) {
                    const int32_t p = h.p_lo + fm_hit_pattern(slice, h.slice_count, t);
                    const int32_t L = fm_line_of(T.data(), count, fence.data(), n_fences, shift, locs[(size_t)t]);
                    const int32_t b = fm_hist_bucket(edges.data(), n_edges, L);
                    keys[(size_t)t] = fm_hist_key(p, b, bucket_bits);
                    if (b < B) ++direct[(size_t)p * B + b];
                } else {
                    keys[(size_t)t] = no_hit;
                }
            }
        }
        std::sort(keys.begin(), keys.end());  // (rocPRIM's radix sort over fm_hist_key_width(n, B) bits)
        if (!keys.empty() && (keys.back() >> fm_hist_key_width(n, B)) != 0) return 3;
        // k_hist_counts
        hist.assign((size_t)n * B + kPad, kSentinel);
        for (int64_t i = 0; i < (int64_t)n * B; ++i) {
            const int64_t p = i / B;
            hist[(size_t)i] = fm_hist_count(keys.data(), hit_off.data(), n_hits, first, (int32_t)p, (int32_t)(i - p * B), bucket_bits);
            if (hist[(size_t)i] != direct[(size_t)i]) return 3;
        }
    }
    fclose(in);
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    put(out, hist);
    return fclose(out) == 0 ? 0 : 2;
}
