// fmx_hit_filter.hpp — PACKED HITS -> THE PACKED HITS THAT LIE IN GIVEN LINES (fmx_hits_in_lines_dev, fmx_field_values_where_batch;
// grep terminating | grep -o 'blk_[^ ]*'): the per-item functions of fmx_hit_filter.hip, host and device alike, so that the CPU
// suite compiles them as plain C++ (tests/hit_filter_hostsim.cpp).
//
// A hit h of pattern i is KEPT iff, with L = fm_line_of(h) (a hit belongs to the line of its first character),
//     line_lo <= L < line_hi,   and   where_of[i] < 0  or  L is one of lines[line_off[w] .. line_off[w + 1]), w = where_of[i]
// (the lines of a query: ascending and distinct, what the line stages leave without a limit).  The kept hits keep the order they
// had: flag, exclusive scan, scatter — a stable compaction, so the hits of a pattern stay in SA-row order for the values stage.
// The hits of the call are the slots [hit_off[0], min(hit_off[n], n_hits)) of locs: hit_off[0] may be non-zero (filter terms and
// value patterns side by side in one packed block), slots in front and behind are ignored.
#pragma once

#include "fmx_device.hpp"

namespace fmx {

// L occurs in lines[lo, hi), ascending and distinct: one lower bound
FMX_HD bool fm_filter_line_listed(const int32_t *lines, int64_t lo, int64_t hi, int32_t L) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (lines[mid] < L)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < end && lines[lo] == L;
}

// the keep rule for a hit of line L whose pattern asks for query w (w < 0: no query, the window alone)
FMX_HD bool fm_filter_keep(int32_t L, int32_t line_lo, int32_t line_hi, int32_t w, const int64_t *line_off, const int32_t *lines) {
    if (L < line_lo || L >= line_hi) return false;
    return w < 0 || fm_filter_line_listed(lines, line_off[w], line_off[w + 1], L);
}

// slot v of hit_off inside the slots the call looks at: [0, n_hits]
FMX_HHD int64_t fm_filter_slot(int64_t v, int64_t n_hits) { return v < 0 ? 0 : v < n_hits ? v : n_hits; }

// kept_off[p], p in [0, n]: pos = the exclusive scan of the flags (n_hits + 1 entries; the flags in front of hit_off[0] are 0, so
// kept_off[0] = 0)
FMX_HD int64_t fm_filter_kept_off(const int64_t *hit_off, const int32_t *pos, int64_t n_hits, int32_t p) {
    return pos[fm_filter_slot(hit_off[p], n_hits)];
}

}  // namespace fmx
