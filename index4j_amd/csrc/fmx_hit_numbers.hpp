// fmx_hit_numbers.hpp — STATISTICS OF THE NUMBER BEHIND A PATTERN, PER BUCKET OF LINES (fmx_numbers_of_hits_dev,
// fmx_number_stats_where_batch; stats sum(size) p95(size) by minute where line has addStoredBlock): the per-item functions of
// fmx_hit_numbers.hip, host and device alike, so that the CPU suite compiles them as plain C++ (tests/numbers_hostsim.cpp).
//
// THE VALUE OF A HIT.  With len the length of the hit's pattern, the hit's window is fm_val_window(loc, len, kNumWindow,
// textLength) (fmx_hit_values.hpp's rule at max_len = 32), its text what extract(s, e, destination, 0) stores.  Over the window's
// code units, with F = frac_digits in [0, 9]:
//   D = the maximal run of units '0' .. '9' at the window's start; D == 0: NOT A NUMBER; D == 32: OVERFLOW (the run fills the
//       window and may go on);
//   with F > 0 and the unit behind the run '.', up to F digit units behind it are the fraction, k of them; further digits are
//       ignored (truncation).  Without a '.', or with F == 0, k = 0: "12.5" at F == 0 is 12, "1." at F == 3 is 1000;
//   value = int(run) * 10^F + int(fraction) * 10^(F - k); value > 2^63 - 1: OVERFLOW.
// No sign, no exponent, no thousands separator.
//
// WHAT COMES BACK: rows of n x B, row = i * B + b, over the hits of pattern i whose line lies in bucket b (fmx_line_hist.hpp's
// edges and buckets; no edges at all: B = 1, every line) and that parse: count, the exact sum as 128 bits, min, max, and the
// nearest-rank percentiles; per pattern the hits IN SOME BUCKET that did not parse, by reason.  For every i,
//     sum over b of count[i, b] + not_number[i] + overflow[i] = the total of row i of the hits histogram over the same hits.
//
// THE KEY of a slot is fm_hist_key(pattern, code, code_bits) with the code in [0, B + 2]: a bucket, B = no bucket, B + 1 = not a
// number, B + 2 = overflow; the pattern n for a slot that is no hit.  code_bits = fm_bits(B + 3): fm_hist_count looks for
// code + 1, which must not run into the pattern's bits.  Ordered by (key, value) — a stable sort by value, then one by key — the
// values of (pattern, bucket) lie side by side, ascending: min is the first, max the last, a percentile an index, and the sum the
// difference of two running sums.
#pragma once

#include "fmx_hit_values.hpp"
#include "fmx_line_hist.hpp"

namespace fmx {

constexpr int32_t kNumWindow = 32;        // code units of a hit's window
constexpr int32_t kNumFracMax = 9;        // frac_digits is in [0, 9]
constexpr int32_t kNumPermilleMax = 16;   // n_permille is in [0, 16]
constexpr int64_t kNumValueMax = 0x7fffffffffffffffLL;

constexpr int32_t kNumOk = 0, kNumNotNumber = 1, kNumOverflow = 2;

FMX_HHD int64_t fm_num_pow10(int32_t k) {  // k in [0, 9]
    int64_t p = 1;
    for (int32_t i = 0; i < k; ++i) p *= 10;
    return p;
}

FMX_HD bool fm_num_digit(uint16_t u) { return u >= '0' && u <= '9'; }

// the value of a window of `len` <= kNumWindow code units: kNumOk and value, or why there is none (value = 0 then).  Saturating:
// once the number has passed 2^63 - 1 it stays "too large", whatever follows.
FMX_HD int32_t fm_num_parse(const uint16_t *win, int32_t len, int32_t frac_digits, int64_t &value) {
    value = 0;
    int32_t d = 0;
    uint64_t v = 0;
    bool over = false;
    for (; d < len && fm_num_digit(win[d]); ++d) {
        const uint64_t digit = (uint64_t)(win[d] - '0');
        if (v > ((uint64_t)kNumValueMax - digit) / 10) over = true;
        if (!over) v = v * 10 + digit;
    }
    if (d == 0) return kNumNotNumber;
    if (d >= kNumWindow || over) return kNumOverflow;
    const uint64_t scale = (uint64_t)fm_num_pow10(frac_digits);
    uint64_t frac = 0;
    if (frac_digits > 0 && d < len && win[d] == '.') {
        int32_t k = 0;
        for (; k < frac_digits && d + 1 + k < len && fm_num_digit(win[d + 1 + k]); ++k) frac = frac * 10 + (uint64_t)(win[d + 1 + k] - '0');
        frac *= (uint64_t)fm_num_pow10(frac_digits - k);
    }
    if (v > (uint64_t)kNumValueMax / scale) return kNumOverflow;
    v *= scale;
    if (v > (uint64_t)kNumValueMax - frac) return kNumOverflow;
    value = (int64_t)(v + frac);
    return kNumOk;
}

// the code of a hit of bucket `bucket` in [0, B] (B: no bucket) whose window parsed as `kind`: a hit outside the buckets keeps B
FMX_HD int32_t fm_num_code(int32_t bucket, int32_t B, int32_t kind) { return bucket >= B ? B : kind == kNumOk ? bucket : B + kind; }
FMX_HHD int32_t fm_num_code_bits(int32_t B) { return fm_bits((uint32_t)B + 3u); }
FMX_HHD int32_t fm_num_key_width(int32_t n, int32_t B) { return fm_bits((uint32_t)n) + fm_num_code_bits(B); }

// the slots [lo, lo + count) of (pattern, code) in the sorted keys: fm_hist_count's two searches, confined to the pattern's slots
FMX_HD int64_t fm_num_segment(const uint64_t *keys, const int64_t *hit_off, int64_t n_hits, int64_t first, int32_t pattern, int32_t code,
                              int32_t code_bits, int64_t &lo) {
    int64_t a = hit_off[pattern], b = hit_off[pattern + 1];
    a = (a < first ? first : a < n_hits ? a : n_hits) - first;
    b = (b < first ? first : b < n_hits ? b : n_hits) - first;
    lo = a;
    if (b <= a) return 0;
    lo = fm_hist_key_rank(keys, a, b, fm_hist_key(pattern, code, code_bits));
    return fm_hist_key_rank(keys, lo, b, fm_hist_key(pattern, code + 1, code_bits)) - lo;
}

// nearest rank: the index into c >= 1 ascending values of the permille-th thousandth, permille in [0, 1000]
FMX_HD int64_t fm_num_pct_index(int32_t permille, int64_t c) {
    const int64_t rank = ((int64_t)permille * c + 999) / 1000;
    return (rank < 1 ? 1 : rank) - 1;
}

// the two halves of a value as the running sums take them, and the 128-bit sum of a segment from the differences of the two
// INCLUSIVE running sums over the sorted values (scan[i] = the sum of the halves of values 0 .. i); at most 2^31 - 1 values of
// 32 bits each: neither running sum wraps
FMX_HD uint64_t fm_num_low(uint64_t v) { return v & 0xffffffffu; }
FMX_HD uint64_t fm_num_high(uint64_t v) { return v >> 32; }
FMX_HD uint64_t fm_num_scan_between(const uint64_t *scan, int64_t lo, int64_t count) {
    return count <= 0 ? 0 : scan[lo + count - 1] - (lo > 0 ? scan[lo - 1] : 0);
}
FMX_HD void fm_num_sum128(uint64_t low_sum, uint64_t high_sum, uint64_t &sum_lo, uint64_t &sum_hi) {
    const uint64_t shifted = high_sum << 32;
    sum_lo = shifted + low_sum;
    sum_hi = (high_sum >> 32) + (sum_lo < shifted ? 1u : 0u);
}

// the HOST checks of the call's small arrays: 0, or which rule is broken
FMX_HHD int32_t fm_num_permille_bad(const int32_t *permille, int32_t n_permille) {
    if (n_permille < 0 || n_permille > kNumPermilleMax || (n_permille > 0 && !permille)) return 1;
    for (int32_t j = 0; j < n_permille; ++j)
        if (permille[j] < 0 || permille[j] > 1000) return 2;
    return 0;
}

}  // namespace fmx
