// fmx_sa_device.hpp — the search routines of index4j's SuffixArray (suffixarray/SuffixArray.java, "SA" below) over
// its resident form, as FMX_HD functions: the kernels of fmx_sa_query.hip run them on the device, and a test-only host
// build (tests/sa_hostsim.cpp) runs the very same source on the CPU.
//
// Resident form: the text as uint16, the array as int32 (n + 1 rows; row 0 is the empty suffix n), and a FENCE TABLE:
// the first K chars of the suffix at every 2^shift-th row (rows 0, 2^shift, ... < n), 0-padded, with min(K, suffix
// length) per fence kept apart (read only when a compare meets a 0 char: a real '\0' or the end of a short suffix).
//
// count (SA:100-104) runs two binary searches with r = n, so row n is never read:
//   left  = the first row in [0, n) whose suffix is >= p (compareTo, SA:56-68), or n;
//   right = the first row in [left, n) whose suffix does not start with p (SA:70-87), or n;
//   count = right - left (one fewer than the occurrences when the largest suffix starts with p: DESIGN.md §2).
// Both predicates are monotone over the rows they search, so any search that finds these two boundaries is parity-exact.
// Here: the left search first runs over the fences (in LDS on the device), then over the rows between two fences in
// HBM, each compare starting at the smaller of the lcps with the two bounds (Manber-Myers); the right search starts at
// left and is bounded by the smallest row the first search saw above p that does not start with p.
#pragma once

#include <cstdint>

#ifndef FMX_HD
#if defined(__HIPCC__)
#define FMX_HD __device__ inline __attribute__((always_inline))
#else
#define FMX_HD inline
#endif
#endif

namespace fmx {

struct SaView {
    const uint16_t *text;      // n chars
    const int32_t *sa;         // n + 1 rows
    int32_t n;
    const uint8_t *fence_len;  // per fence: min(K, length of its suffix)
    int32_t n_fences;          // 0 = no fence table
    int32_t fence_shift;       // fence j = row j << fence_shift
    int32_t fence_chars;       // K
};

// how p compares with a suffix
constexpr int kSaGreater = 1;  // p > suffix (compareTo > 0)
constexpr int kSaPrefix = 0;   // the suffix starts with p (compareTo <= 0)
constexpr int kSaLess = -1;    // p < suffix and the suffix does not start with p

FMX_HD int32_t sa_min(int32_t a, int32_t b) { return a < b ? a : b; }
FMX_HD int32_t sa_max(int32_t a, int32_t b) { return a > b ? a : b; }
FMX_HD int32_t sa_mid(int32_t lo, int32_t hi) { return (int32_t)(((uint32_t)lo + (uint32_t)hi) >> 1); }

// p (plen chars) against the suffix at text position pos, from char `lcp` on (the caller knows the first lcp chars agree);
// lcp becomes the common prefix of the two.  Four chars are loaded per step, so that their requests are in flight together.
FMX_HD int sa_compare_text(const uint16_t *text, int32_t n, int32_t pos, const uint16_t *p, int32_t plen, int32_t &lcp) {
    const int32_t lim = sa_min(plen, n - pos);
    int32_t k = lcp;
    while (k < lim) {
        const int32_t m = sa_min(lim - k, 4);
        uint16_t t[4], q[4];
        for (int u = 0; u < 4; ++u) {
            t[u] = u < m ? text[pos + k + u] : (uint16_t)0;
            q[u] = u < m ? p[k + u] : (uint16_t)0;
        }
        for (int u = 0; u < 4; ++u)
            if (u < m && t[u] != q[u]) {
                lcp = k + u;
                return q[u] > t[u] ? kSaGreater : kSaLess;
            }
        k += m;
    }
    lcp = lim;
    return lim == plen ? kSaPrefix : kSaGreater;  // (else the suffix is a proper prefix of p)
}

// p against fence j (keys: the fence table's chars, in LDS on the device), from char `lcp` on.  Settled from the key alone
// unless p is longer than K and agrees with all K chars of a suffix that has at least K: then against the text.
FMX_HD int sa_compare_fence(const SaView &v, const uint16_t *keys, int32_t j, const uint16_t *p, int32_t plen,
                            int32_t &lcp) {
    const int32_t K = v.fence_chars;
    const uint16_t *key = keys + (int64_t)j * K;
    int32_t flen = K;  // the suffix has at least this many chars (exact once fence_len was read)
    bool exact = false;
    const int32_t lim = sa_min(plen, K);
    int32_t k = lcp;
    for (; k < lim; ++k) {
        const uint16_t c = key[k];
        if (c == 0 && !exact) {
            flen = v.fence_len[j];
            exact = true;
        }
        if (k >= flen) break;  // the suffix ended: it is a proper prefix of p
        if (c != p[k]) {
            lcp = k;
            return p[k] > c ? kSaGreater : kSaLess;
        }
    }
    lcp = k;
    if (k < lim) return kSaGreater;
    if (plen <= K) return kSaPrefix;
    return sa_compare_text(v.text, v.n, v.sa[(int64_t)j << v.fence_shift], p, plen, lcp);
}

struct SaRange {
    int32_t left, right;
};

// SA:131-157 for one pattern
FMX_HD SaRange sa_search(const SaView &v, const uint16_t *keys, const uint16_t *p, int32_t plen) {
    int32_t lo = 0, hi = v.n;            // left lies in [lo, hi]
    int32_t lcp_lo = 0, lcp_hi = 0;      // lcps of p with rows lo - 1 (p is greater) and hi (p is not)
    int32_t bound = v.n, lcp_bound = 0;  // the smallest row seen above p whose suffix does not start with p
    int32_t prefix_max = -1;             // the largest row seen whose suffix starts with p
    auto seen = [&](int r, int32_t row, int32_t l) {
        if (r == kSaGreater) {
            lo = row + 1;
            lcp_lo = l;
        } else {
            hi = row;
            lcp_hi = l;
            if (r == kSaLess) {
                if (row < bound) {
                    bound = row;
                    lcp_bound = l;
                }
            } else {
                prefix_max = sa_max(prefix_max, row);
            }
        }
    };
    // the first levels over the fences
    int32_t a = 0, b = v.n_fences;
    while (a < b) {
        const int32_t j = sa_mid(a, b);
        int32_t l = sa_min(lcp_lo, lcp_hi);
        const int r = sa_compare_fence(v, keys, j, p, plen, l);
        seen(r, j << v.fence_shift, l);
        if (r == kSaGreater)
            a = j + 1;
        else
            b = j;
    }
    // the rest in HBM
    while (lo < hi) {
        const int32_t mid = sa_mid(lo, hi);
        int32_t l = sa_min(lcp_lo, lcp_hi);
        seen(sa_compare_text(v.text, v.n, v.sa[mid], p, plen, l), mid, l);
    }
    SaRange out;
    out.left = lo;
    // rows [left, prefix_max] start with p, rows from `bound` on do not
    int32_t l2 = sa_max(lo, prefix_max + 1), r2 = bound;
    int32_t lcp_l2 = l2 > lo ? plen : lcp_lo, lcp_r2 = lcp_bound;
    while (l2 < r2) {
        const int32_t mid = sa_mid(l2, r2);
        int32_t l = sa_min(lcp_l2, lcp_r2);
        if (sa_compare_text(v.text, v.n, v.sa[mid], p, plen, l) == kSaPrefix) {
            l2 = mid + 1;
            lcp_l2 = plen;
        } else {
            r2 = mid;
            lcp_r2 = l;
        }
    }
    out.right = r2;
    return out;
}

}  // namespace fmx
