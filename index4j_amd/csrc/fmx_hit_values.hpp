// fmx_hit_values.hpp — THE VALUES THAT FOLLOW A PATTERN, WITH COUNTS (fmx_values_of_hits_dev, fmx_field_values_batch; grep -o |
// sort | uniq -c): the per-item functions of fmx_hit_values.hip, host and device alike, so that the CPU suite compiles them as
// plain C++ (tests/values_hostsim.cpp).
//
// With textLength = getInputLength() - 1 and len the length of the hit's pattern, a hit h has the WINDOW [s, e):
//     s = min(max(h + len, 0), textLength),   e = min(s + max_len, textLength)
// what extract(s, e, destination, 0) stores is the window's text, and the hit's VALUE is that text up to, not including, its first
// code unit of the stop set (all of it where there is none).  The empty string is a value.  The answer of a pattern is its
// distinct values, ascending by UTF-16 code unit, a value in front of its extensions, each with the number of hits that have it.
//
// The hits of one pattern stand in SA-row order — ordered by the text that follows the pattern — so equal values are neighbours
// nearly always: a RUN is a maximal stretch of neighbouring hits of one pattern with one value.  Runs alone are not the answer (a
// value V met with two terminators x < y has every V + z, x < z < y, between its two runs), so the runs are grouped exactly: by
// stable least-significant-first sorting passes over (length; the chunks of four code units, last to first, padded with 0;
// pattern).  The length pass tells a value from the same value followed by U+0000, which the padded chunks do not.
#pragma once

#include "fmx_device.hpp"

namespace fmx {

constexpr int32_t kValuesMaxLen = 64;   // max_len is in [1, 64]
constexpr int32_t kValuesMaxStop = 64;  // n_stop is in [0, 64]
constexpr int32_t kValuesChunk = 4;     // code units per 64-bit sort key
constexpr int64_t kValuesMaxUnits = (int64_t)1 << 35;  // n_hits * max_len: the code units of all windows of one call
constexpr int32_t kStopBitmapWords = 65536 / 32;  // the stop set as a bitmap over the code units: 8 KiB

// the window of hit `loc` of a pattern of `len` characters (the sums in 64 bits: loc + len may pass 2^31)
FMX_HHD void fm_val_window(int32_t loc, int32_t len, int32_t max_len, int32_t text_len, int32_t &s, int32_t &e) {
    int64_t a = (int64_t)loc + len;
    if (a < 0) a = 0;
    if (a > text_len) a = text_len;
    const int64_t b = a + max_len < text_len ? a + max_len : text_len;
    s = (int32_t)a;
    e = (int32_t)b;
}

// the stop set: a bitmap (word u >> 5, bit u & 31), or its units sorted ascending (duplicates stay: they are found like the rest)
FMX_HD bool fm_val_stop_in_bitmap(const uint32_t *bitmap, uint16_t u) { return (bitmap[u >> 5] >> (u & 31)) & 1u; }
FMX_HD bool fm_val_stop_in_list(const uint16_t *sorted, int32_t n_stop, uint16_t u) {
    int32_t lo = 0, hi = n_stop;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < u)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n_stop && sorted[lo] == u;
}
// the length of the value of a window of `len` units
template <bool kBitmap>
FMX_HD int32_t fm_val_length(const uint16_t *win, int32_t len, const void *stop_set, int32_t n_stop) {
    int32_t k = 0;
    for (; k < len; ++k) {
        const bool stop = kBitmap ? fm_val_stop_in_bitmap(static_cast<const uint32_t *>(stop_set), win[k])
                                  : fm_val_stop_in_list(static_cast<const uint16_t *>(stop_set), n_stop, win[k]);
        if (stop) break;
    }
    return k;
}

// two values, unit by unit
FMX_HD bool fm_val_same(const uint16_t *a, int32_t a_len, const uint16_t *b, int32_t b_len) {
    if (a_len != b_len) return false;
    for (int32_t k = 0; k < a_len; ++k)
        if (a[k] != b[k]) return false;
    return true;
}

// chunk c of a value: units [4c, 4c + 4), the first one most significant, 0 behind the value's end
FMX_HHD int32_t fm_val_chunks(int32_t max_len) { return (max_len + kValuesChunk - 1) / kValuesChunk; }
FMX_HD uint64_t fm_val_chunk_key(const uint16_t *val, int32_t len, int32_t c) {
    uint64_t key = 0;
    for (int32_t j = 0; j < kValuesChunk; ++j) {
        const int32_t k = kValuesChunk * c + j;
        key = (key << 16) | (k < len ? val[k] : 0);
    }
    return key;
}

// the number of entries of keys[0, count) (ascending) below p: where pattern p's groups begin among the sorted runs
FMX_HD int64_t fm_val_lower_bound(const uint32_t *keys, int64_t count, uint32_t p) {
    int64_t lo = 0, hi = count;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

}  // namespace fmx
