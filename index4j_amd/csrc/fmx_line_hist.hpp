// fmx_line_hist.hpp — MATCHING LINES AND HITS PER BUCKET OF LINES, the timeline of a log search (fmx_lines_histogram_dev,
// fmx_hits_histogram_dev, fmx_line_histogram_batch, fmx_hit_histogram_where_batch): the per-item functions of fmx_line_hist.hip,
// host and device alike, so that the CPU suite compiles them as plain C++ (tests/line_hist_hostsim.cpp).
//
// EDGES: n_edges >= 2 line ids, edges[0] >= 0, never decreasing; B = n_edges - 1 buckets.  Bucket b holds the lines L with
// edges[b] <= L < edges[b + 1]; equal neighbours make an empty bucket; a line below edges[0] or at or above edges[B] lies in no
// bucket.  Edges may exceed the number of lines.
//   lines form   hist[Q * B + b] = the entries of the ascending list Q inside bucket b = rank(edges[b + 1]) - rank(edges[b]), where
//                rank(e) is the number of entries below e: ONE lower bound per (list, edge), whatever the list's length.  An entry
//                that occurs twice counts twice.
//   hits form    a hit belongs to the line of its first character (fm_line_of) and to the bucket of that line; the key
//                (pattern << bucket_bits) | bucket, with the bucket B for "no bucket" and the pattern n for a slot that is no hit,
//                lets ONE device-wide sort put the hits of (pattern, bucket) side by side: hist[i * B + b] = lb(key(i, b + 1)) -
//                lb(key(i, b)) in the sorted keys.
#pragma once

#include "fmx_device.hpp"

namespace fmx {

constexpr int32_t kHistEdgesLds = 4096;                // edges a workgroup of the key kernel stages in LDS (16 KiB)
constexpr int64_t kHistCellsMax = (int64_t)1 << 27;    // rows * B of one call

// the number of entries of a[lo, hi) (ascending) below v
FMX_HD int64_t fm_hist_rank(const int32_t *a, int64_t lo, int64_t hi, int32_t v) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// the entries of an ascending list between two neighbouring edges, from their ranks
FMX_HD int32_t fm_hist_between(int64_t rank_lo, int64_t rank_hi) { return (int32_t)(rank_hi - rank_lo); }

// the bucket of line L: the last b with edges[b] <= L (an upper bound: of equal edges the last one, so that an empty bucket stays
// empty), or B = n_edges - 1 where L lies in no bucket
FMX_HD int32_t fm_hist_bucket(const int32_t *edges, int32_t n_edges, int32_t L) {
    int32_t lo = 0, hi = n_edges;  // the number of edges <= L
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (edges[mid] <= L)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo == 0 || lo == n_edges ? n_edges - 1 : lo - 1;
}

// the sort key of one slot: bucket in [0, B] takes bucket_bits = fm_bits(B), the pattern in [0, n] fm_bits(n): at most 31 + 28 bits
FMX_HD uint64_t fm_hist_key(int32_t pattern, int32_t bucket, int32_t bucket_bits) {
    return ((uint64_t)(uint32_t)pattern << bucket_bits) | (uint32_t)bucket;
}
FMX_HD int32_t fm_hist_key_pattern(uint64_t key, int32_t bucket_bits) { return (int32_t)(key >> bucket_bits); }
FMX_HD int32_t fm_hist_key_bucket(uint64_t key, int32_t bucket_bits) { return (int32_t)(key & (((uint64_t)1 << bucket_bits) - 1)); }
FMX_HHD int32_t fm_hist_key_width(int32_t n, int32_t B) { return fm_bits((uint32_t)n) + fm_bits((uint32_t)B); }

// the number of keys[lo, hi) (ascending) below key
FMX_HD int64_t fm_hist_key_rank(const uint64_t *keys, int64_t lo, int64_t hi, uint64_t key) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// counter (pattern, bucket) off the sorted keys.  The slots of the call are [first, total) of n_hits (fm_filter_slot's clamp of
// hit_off[0] and hit_off[n]); the slots in front of `first` carry the pattern n and sort last, so the keys of pattern p lie at
// [slot(hit_off[p]) - first, slot(hit_off[p + 1]) - first) and the two searches stay inside them.
FMX_HD int32_t fm_hist_count(const uint64_t *keys, const int64_t *hit_off, int64_t n_hits, int64_t first, int32_t pattern, int32_t bucket,
                             int32_t bucket_bits) {
    int64_t a = hit_off[pattern], b = hit_off[pattern + 1];
    a = (a < first ? first : a < n_hits ? a : n_hits) - first;
    b = (b < first ? first : b < n_hits ? b : n_hits) - first;
    if (b <= a) return 0;
    const int64_t lo = fm_hist_key_rank(keys, a, b, fm_hist_key(pattern, bucket, bucket_bits));
    return (int32_t)(fm_hist_key_rank(keys, lo, b, fm_hist_key(pattern, bucket + 1, bucket_bits)) - lo);
}

// the HOST check of an edge array (the C-ABI layer and the launchers): 0, or which rule it breaks
FMX_HHD int32_t fm_hist_edges_bad(const int32_t *edges, int32_t n_edges) {
    if (!edges || n_edges < 2) return 1;
    if (edges[0] < 0) return 2;
    for (int32_t i = 1; i < n_edges; ++i)
        if (edges[i] < edges[i - 1]) return 3;
    return 0;
}

}  // namespace fmx
