// fmx_hit_range.hpp — PACKED HITS -> THE PACKED HITS WHOSE NUMBER LIES IN A RANGE (fmx_hits_in_number_range_dev,
// fmx_match_query_number_batch; latency_ms >= 500): the per-item functions of fmx_hit_range.hip, host and device alike, so that the
// CPU suite compiles them as plain C++ (tests/range_hostsim.cpp).
//
// A call carries per batch of n patterns num_lo and num_hi (n int64 each) and ONE frac_digits F in [0, 9].
//   Pattern i is RANGED iff num_lo[i] >= 0 (a value is never negative: a negative num_lo[i] is a plain string term — every hit
//   passes, nothing is read).
//   A hit h of a ranged pattern of length len has fmx_hit_numbers.hpp's value, exactly: the window fm_val_window(h, len, kNumWindow,
//   textLength), its text what extract(s, e, destination, 0) stores, parsed by fm_num_parse(win, e - s, F, value).
//   The hit PASSES iff the parse is kNumOk and num_lo[i] <= value <= num_hi[i].  "Not a number" and "overflow" never pass, whatever
//   num_hi is — a run of 32 digits and a value above 2^63 - 1 included.  num_hi[i] = INT64_MAX is "no upper bound";
//   num_lo[i] > num_hi[i] is legal and keeps nothing.
// Per pattern the stage reports kept, not_number and overflow (an unranged pattern: every hit, 0, 0), so
//     kept + not_number + overflow <= hits,   the rest are numbers outside the range;
// with num_lo = 0 and num_hi = INT64_MAX the three are count, not_number and overflow of fmx_number_stats_where_batch for the same
// pattern without edges and without a filter.  The kept hits keep the order they had (fmx_hit_filter.hpp's stable compaction: flag,
// exclusive scan, store), and the output is the packed format of the input.
//
// THE CODE of a slot is one of four; the flag of the compaction is code == kRangeKeep, and the two reasons travel side by side in
// ONE 64-bit word per slot (fm_range_tail: not a number in the low half, overflow in the high half), so that one exclusive scan
// gives both counters of every pattern as a difference — at most 2^31 - 1 slots, neither half runs into the other.
#pragma once

#include "fmx_hit_filter.hpp"
#include "fmx_hit_numbers.hpp"

namespace fmx {

constexpr int32_t kRangeOutside = 0, kRangeKeep = 1, kRangeNotNumber = 2, kRangeOverflow = 3;

FMX_HD bool fm_range_ranged(int64_t num_lo) { return num_lo >= 0; }

// the code of a hit of a RANGED pattern from its window of `len` <= kNumWindow code units
FMX_HD int32_t fm_range_code(const uint16_t *win, int32_t len, int32_t frac_digits, int64_t num_lo, int64_t num_hi) {
    int64_t v;
    const int32_t kind = fm_num_parse(win, len, frac_digits, v);
    if (kind == kNumNotNumber) return kRangeNotNumber;
    if (kind != kNumOk) return kRangeOverflow;
    return num_lo <= v && v <= num_hi ? kRangeKeep : kRangeOutside;
}

// what a slot of code `code` adds to the running word of the reasons, and the two counters of the slots [a, b) from the EXCLUSIVE
// scan of those words
FMX_HD uint64_t fm_range_tail(int32_t code) { return code == kRangeNotNumber ? 1ull : code == kRangeOverflow ? 1ull << 32 : 0ull; }
FMX_HD int32_t fm_range_not_number(const uint64_t *tail_pos, int64_t a, int64_t b) {
    return (int32_t)((tail_pos[b] - tail_pos[a]) & 0xffffffffu);
}
FMX_HD int32_t fm_range_overflow(const uint64_t *tail_pos, int64_t a, int64_t b) { return (int32_t)((tail_pos[b] - tail_pos[a]) >> 32); }

// the HOST checks of the call's small arrays: 0, or which rule is broken (1: frac_digits, 2: a negative term_len)
FMX_HHD int32_t fm_range_args_bad(int32_t n, const int32_t *term_len, int32_t frac_digits) {
    if (frac_digits < 0 || frac_digits > kNumFracMax) return 1;
    for (int32_t i = 0; i < n; ++i)
        if (term_len[i] < 0) return 2;
    return 0;
}

}  // namespace fmx
