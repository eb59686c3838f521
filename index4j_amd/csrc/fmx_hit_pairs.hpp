// fmx_hit_pairs.hpp — STATISTICS AND LINE COUNTS BY THE VALUES OF TWO FIELDS OF THE SAME LINE (fmx_pairs_of_first_hits_dev,
// fmx_number_stats_by_pair_batch; stats p95(latency_ms=) by host=, status= and the pivot table count by host=, status=): the
// per-item functions of fmx_hit_pairs.hip, host and device alike, so that the CPU suite compiles them as plain C++
// (tests/pairs_hostsim.cpp).
//
// A call has m key patterns and c PAIRS (pair_a[j], pair_b[j]), each a key pattern of the call; the two may be equal.  The key
// of a line for a key pattern and its group are fmx_hit_by.hpp's.  Line L has a PAIR KEY for pair j iff it has a key for
// pair_a[j] and one for pair_b[j]: (ga, gb), the two groups.  The PAIRS of j are the distinct (ga, gb) of its lines, ascending by
// ga, then gb — the value order of a, then of b — each with pair_lines >= 1, the lines that have it.
//
// THE JOIN runs over stage a's and b's answers (first_off, first_lines, group_of_first) and leaves lists of the same form, so
// that stage c (fmx_numbers_by_key_dev) runs over them unchanged with m := c and val_off := pair_off:
//   SLOTS: the first hits of pair_a[j], pair after pair: slot_off[j] = the sum of |first hits of pair_a[j']| over j' < j (c + 1
//   entries).  The offsets can hold runs of equal entries — a pair whose a-side is empty between two that are not — so the pair
//   of a slot is the LAST j with slot_off[j] <= slot (fm_by_row_pattern).  The caller hands in n_slots >= slot_off[c]; the slots
//   behind slot_off[c] are no slots.
//   KEYS: a slot finds its line's b-side hit by ONE lower bound (fm_by_find) and makes the key pair | ga | gb; a slot without a
//   partner and every slot behind the real ones gets the key of pair c, which sorts behind every pair.  pair in [0, c] takes
//   fm_bits(c) bits, ga fm_bits(the most groups of an a-side), gb fm_bits(the most groups of a b-side): a call whose key is wider
//   than 64 bits is refused (fm_pair_args_bad).
//   ONE stable sort of (key, slot); a sorted slot whose key differs from its predecessor's is the HEAD of a pair; a scan numbers
//   the heads; a head stores ga, gb and the length of its run (an upper bound by binary search: no lane walks a run); every sorted
//   slot writes the index of its pair within pair j back to the slot it came from; a scan and a stable compaction over the slots
//   in their original order leave the joined lists — the a-side arrives ascending by line, so nothing more is sorted.
// Integers only, no atomics: the result does not depend on the order the lanes run in.
#pragma once

#include "fmx_hit_by.hpp"

namespace fmx {

// the sort key of one slot
FMX_HD uint64_t fm_pair_key(int32_t pair, int32_t ga, int32_t gb, int32_t a_bits, int32_t b_bits) {
    return ((((uint64_t)(uint32_t)pair << a_bits) | (uint32_t)ga) << b_bits) | (uint32_t)gb;
}
FMX_HD int32_t fm_pair_key_pair(uint64_t key, int32_t a_bits, int32_t b_bits) { return (int32_t)(key >> (a_bits + b_bits)); }
FMX_HD int32_t fm_pair_key_a(uint64_t key, int32_t a_bits, int32_t b_bits) { return (int32_t)((key >> b_bits) & (((uint64_t)1 << a_bits) - 1)); }
FMX_HD int32_t fm_pair_key_b(uint64_t key, int32_t b_bits) { return (int32_t)(key & (((uint64_t)1 << b_bits) - 1)); }

// the key of slot t of pair j, whose a-side hit is entry `at` of the first hits: the groups of its line for pair_a[j] and — by one
// lower bound in the first lines [b_lo, b_hi) of pair_b[j] — for pair_b[j].  A line without a key of b, and a group that is no
// group of its key pattern (nothing is read through a key), give the key of pair c.  *line: the slot's line.
FMX_HD uint64_t fm_pair_slot_key(const int32_t *first_lines, const int32_t *group_of_first, int64_t at, int64_t b_lo, int64_t b_hi, int32_t j, int32_t c,
                                 int64_t groups_a, int64_t groups_b, int32_t a_bits, int32_t b_bits, int32_t *line) {
    const int32_t L = first_lines[at];
    *line = L;
    const int64_t found = fm_by_find(first_lines, b_lo, b_hi, L);
    if (found < 0) return fm_pair_key(c, 0, 0, a_bits, b_bits);
    const int32_t ga = group_of_first[at], gb = group_of_first[found];
    if (ga < 0 || ga >= groups_a || gb < 0 || gb >= groups_b) return fm_pair_key(c, 0, 0, a_bits, b_bits);
    return fm_pair_key(j, ga, gb, a_bits, b_bits);
}

// sorted slot i opens a pair: a slot with a partner (pair < c) whose key differs from its predecessor's
FMX_HD bool fm_pair_head(const uint64_t *keys, int64_t i, int32_t c, int32_t a_bits, int32_t b_bits) {
    return fm_pair_key_pair(keys[i], a_bits, b_bits) < c && (i == 0 || keys[i] != keys[i - 1]);
}

// the slots of the run of equal keys that sorted slot i opens, among keys[0, n): an upper bound, no walk over the run
FMX_HD int64_t fm_pair_run_length(const uint64_t *keys, int64_t n, int64_t i) { return fm_hist_key_rank(keys, i + 1, n, keys[i] + 1) - i; }

// the first sorted slot of pair j in [0, c] among keys[0, n) (n where there is none at or behind it): pos[] there is pair_off[j]
FMX_HD int64_t fm_pair_first_slot(const uint64_t *keys, int64_t n, int32_t j, int32_t a_bits, int32_t b_bits) {
    return fm_hist_key_rank(keys, 0, n, fm_pair_key(j, 0, 0, a_bits, b_bits));
}

// the HOST checks of a call's small arrays and the widths of its key: 0, or which rule is broken.  val_off: m + 1 offsets of the
// key patterns' groups (stage b's answer, read by the caller; nullptr: rules 1 and 2 alone, the host form judges its pairs before
// anything is searched); *a_bits, *b_bits (out; nullable): the bits of ga and gb
//   1  m <= 0 with c > 0, c < 0 or a missing array      2  pair_a[j] or pair_b[j] outside [0, m)
//   3  val_off starts below 0, decreases or holds more than 2^31 - 1 groups      4  n_slots below 0 or above 2^31 - 1
//   5  the key pair | ga | gb is wider than 64 bits
FMX_HHD int32_t fm_pair_args_bad(int32_t m, const int64_t *val_off, int32_t c, const int32_t *pair_a, const int32_t *pair_b, int64_t n_slots,
                                 int32_t *a_bits, int32_t *b_bits) {
    if (c < 0) return 1;
    if (c > 0 && (m <= 0 || !pair_a || !pair_b)) return 1;
    for (int32_t j = 0; j < c; ++j)
        if (pair_a[j] < 0 || pair_a[j] >= m || pair_b[j] < 0 || pair_b[j] >= m) return 2;
    if (n_slots < 0 || n_slots > 0x7fffffff) return 4;
    if (!val_off || c == 0) return 0;
    if (val_off[0] < 0) return 3;
    for (int32_t k = 0; k < m; ++k)
        if (val_off[k + 1] < val_off[k] || val_off[k + 1] - val_off[k] > 0x7fffffff) return 3;
    int64_t widest_a = 0, widest_b = 0;
    for (int32_t j = 0; j < c; ++j) {
        const int64_t ga = val_off[pair_a[j] + 1] - val_off[pair_a[j]], gb = val_off[pair_b[j] + 1] - val_off[pair_b[j]];
        if (ga > widest_a) widest_a = ga;
        if (gb > widest_b) widest_b = gb;
    }
    const int32_t wa = fm_bits((uint32_t)widest_a), wb = fm_bits((uint32_t)widest_b);
    if (fm_bits((uint32_t)c) + wa + wb > 64) return 5;
    if (a_bits) *a_bits = wa;
    if (b_bits) *b_bits = wb;
    return 0;
}

}  // namespace fmx
