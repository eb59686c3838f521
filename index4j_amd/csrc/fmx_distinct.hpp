// fmx_distinct.hpp — THE DISTINCT VALUES OF A FIELD PER BUCKET OF LINES ("timechart dc(user=)", countDistinct, cardinality — and
// its sibling, the values seen for the first time in a bucket: fmx_values_distinct_histogram_dev,
// fmx_distinct_values_histogram_where_batch): the per-item functions of fmx_distinct.hip, host and device alike, so that the CPU
// suite compiles them as plain C++ (tests/distinct_hostsim.cpp).
//
// IN: the packed kept hits of n patterns, the group offsets of the values stage over them (val_off) and the group of every hit
// (fmx_values_of_hits_groups_dev).  OUT, per pattern i with B buckets:
//   distinct[i * B + b]    the number of different groups among the hits of i whose line lies in bucket b
//   first_seen[i * B + b]  the number of groups of i whose first hit — the hit with the smallest line, and therefore with the
//                          smallest bucket — lies in bucket b
// KEYS: the sort key of one slot is pattern | group | bucket with the group in [0, G_i) (group_bits = fm_bits(max_i G_i), at most
// 31: val_off holds at most 2^31 - 1 groups), the bucket in [0, B) (bucket_bits = fm_bits(B)) and the pattern in [0, n].  The key
// of pattern n, group 0, bucket 0 sorts behind every hit's; it is the key of a slot that is no hit, of a hit whose line lies in no
// bucket and of a hit whose group is outside its pattern's groups (-1: the values stage gave the slot no group).  WIDTH: fm_bits(v)
// <= log2(v) + 1, so n * B <= 2^27 (kHistCellsMax) gives fm_bits(n) + fm_bits(B) <= 27 + 2 = 29, and with the group 29 + 31 = 60
// bits: every call that passes the limit on the counters has a key below 64 bits, there is no refusal of its own for the width.
// HEADS: after ONE sort, slot j opens a run of equal keys — a (pattern, group, bucket) of its own — iff its key is a hit's and
// differs from slot j - 1's; the bucket is the key's low field, so the head is the FIRST of its (pattern, group) iff j == 0 or the
// key above the bucket differs from slot j - 1's.  A head becomes the key (pattern | bucket) << 1 | (first ? 0 : 1), fm_bits(n) +
// fm_bits(B) + 1 <= 30 bits; every other slot the key of pattern n.
// COUNTERS: after the second sort the heads of (i, b) lie side by side, the firsts in front.  With a = lb(i, b, 0), m = lb(i, b, 1)
// and z = lb((i, b, 1) + 1): first_seen = m - a, distinct = z - a.  (i, b, 1) + 1 = (i, b + 1, 0), and b + 1 <= B fits the
// bucket's bits: it never carries into the pattern.  The searches run over ALL slots: hits without a bucket have moved behind the
// hits, so a pattern's keys no longer lie in its hit_off range.
#pragma once

#include "fmx_line_hist.hpp"

namespace fmx {

// the HOST check of a call's shape; *max_groups (nullable) gets max_i G_i: 0, or which rule it breaks —
// 2 val_off does not start at 0 or decreases, or holds more than 2^31 - 1 groups; 3 n * B above 2^27
FMX_HHD int32_t fm_dv_shape_bad(int32_t n, const int64_t *val_off, int32_t B, int64_t *max_groups) {
    if (n > 0 && val_off[0] != 0) return 2;
    int64_t most = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (val_off[i + 1] < val_off[i] || val_off[i + 1] > 0x7fffffff) return 2;
        if (val_off[i + 1] - val_off[i] > most) most = val_off[i + 1] - val_off[i];
    }
    if (max_groups) *max_groups = most;
    if ((int64_t)n * B > kHistCellsMax) return 3;
    return 0;
}

// ---- keys --------------------------------------------------------------------------------------------------------------------
FMX_HHD int32_t fm_dv_key_width(int32_t n, int64_t max_groups, int32_t B) {
    return fm_bits((uint32_t)n) + fm_bits((uint32_t)max_groups) + fm_bits((uint32_t)B);
}
FMX_HD uint64_t fm_dv_key(int32_t pattern, int32_t group, int32_t bucket, int32_t group_bits, int32_t bucket_bits) {
    return ((((uint64_t)(uint32_t)pattern << group_bits) | (uint32_t)group) << bucket_bits) | (uint32_t)bucket;
}
FMX_HD int32_t fm_dv_key_pattern(uint64_t key, int32_t group_bits, int32_t bucket_bits) { return (int32_t)(key >> (group_bits + bucket_bits)); }
FMX_HD int32_t fm_dv_key_group(uint64_t key, int32_t group_bits, int32_t bucket_bits) {
    return (int32_t)((key >> bucket_bits) & (((uint64_t)1 << group_bits) - 1));
}
FMX_HD int32_t fm_dv_key_bucket(uint64_t key, int32_t bucket_bits) { return (int32_t)(key & (((uint64_t)1 << bucket_bits) - 1)); }
// the key of a hit of `pattern`, which has `groups` groups, in `bucket` (B: its line lies in no bucket): the key of pattern n for a
// hit without a bucket or with a group outside [0, groups)
FMX_HD uint64_t fm_dv_hit_key(int32_t n, int32_t pattern, int64_t groups, int32_t group_of_hit, int32_t bucket, int32_t B, int32_t group_bits,
                              int32_t bucket_bits) {
    const bool counts = bucket < B && group_of_hit >= 0 && group_of_hit < groups;
    return counts ? fm_dv_key(pattern, group_of_hit, bucket, group_bits, bucket_bits) : fm_dv_key(n, 0, 0, group_bits, bucket_bits);
}

// ---- heads -------------------------------------------------------------------------------------------------------------------
FMX_HHD int32_t fm_dv_head_key_width(int32_t n, int32_t B) { return fm_bits((uint32_t)n) + fm_bits((uint32_t)B) + 1; }
FMX_HD uint64_t fm_dv_head_key(int32_t pattern, int32_t bucket, bool first, int32_t bucket_bits) {
    return (fm_hist_key(pattern, bucket, bucket_bits) << 1) | (first ? 0u : 1u);
}
// sorted slot j opens a (pattern, group, bucket) of its own
FMX_HD bool fm_dv_is_head(const uint64_t *keys, int64_t j, int32_t n, int32_t group_bits, int32_t bucket_bits) {
    return fm_dv_key_pattern(keys[j], group_bits, bucket_bits) < n && (j == 0 || keys[j] != keys[j - 1]);
}
// ... and, being a head, the smallest bucket of its (pattern, group)
FMX_HD bool fm_dv_is_first(const uint64_t *keys, int64_t j, int32_t bucket_bits) {
    return j == 0 || (keys[j] >> bucket_bits) != (keys[j - 1] >> bucket_bits);
}
// what sorted slot j hands the second sort
FMX_HD uint64_t fm_dv_head_of(const uint64_t *keys, int64_t j, int32_t n, int32_t group_bits, int32_t bucket_bits) {
    if (!fm_dv_is_head(keys, j, n, group_bits, bucket_bits)) return fm_dv_head_key(n, 0, true, bucket_bits);
    return fm_dv_head_key(fm_dv_key_pattern(keys[j], group_bits, bucket_bits), fm_dv_key_bucket(keys[j], bucket_bits),
                          fm_dv_is_first(keys, j, bucket_bits), bucket_bits);
}

// ---- counters ----------------------------------------------------------------------------------------------------------------
// counter (pattern, bucket) off the sorted head keys of all n_hits slots: three lower bounds, each inside what the one before left
FMX_HD void fm_dv_counts(const uint64_t *heads, int64_t n_hits, int32_t pattern, int32_t bucket, int32_t bucket_bits, int32_t &distinct,
                         int32_t &first_seen) {
    const uint64_t key = fm_dv_head_key(pattern, bucket, true, bucket_bits);
    const int64_t a = fm_hist_key_rank(heads, 0, n_hits, key);
    const int64_t m = fm_hist_key_rank(heads, a, n_hits, key + 1);
    const int64_t z = fm_hist_key_rank(heads, m, n_hits, key + 2);  // (bucket + 1 <= B fits the bucket's bits)
    first_seen = (int32_t)(m - a);
    distinct = (int32_t)(z - a);
}

}  // namespace fmx
