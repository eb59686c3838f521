// rows_hostsim.cpp — TEST-ONLY host build of the row table's device code (index4j_amd/csrc/fmx_device.hpp: fm_row_word,
// fm_ticket_record / fm_ticket_publish (fm_locate_share), fm_rows_hit, fm_rows_gather — what k_rows_fill and k_locate_rows of
// fmx_kernels.hip run).
//
// g++ compiles the header's FMX_HD functions as plain C++, so the CPU suite checks the very source the kernels run against the
// oracle (tests/test_locate_rows_cpu.py).  Everything else a resident index has — the image's view, the window directory in its
// three forms — comes from tests/hostsim.cpp, included as it stands (as tests/cpp/fuzz_load.cpp does).  Never part of libfmx.so.
#if !defined(ROWS_HOSTSIM_NO_BASE)  // (tests/cpp/fuzz_rows.cpp has it already)
#include "hostsim.cpp"
#endif

namespace {

// the index as a kernel sees it: hostsim's view of the image (+ the directory attached to it), and the table
DevIndex rows_index(const uint8_t *blob, const uint32_t *rows) {
    DevIndex ix = make_index(blob);
    ix.rows = rows;
    return ix;
}
// (the instantiation launch_rows_fill picks for the directory the index has)
uint32_t row_word(const DevIndex &ix, uint32_t r) {
    return ix.win && ix.win_flat ? fm_row_word<kWinFlat>(ix, ix.inv_global, r)
           : ix.win              ? fm_row_word<kWinAlways>(ix, ix.inv_global, r)
                                 : fm_row_word<kWinNever>(ix, ix.inv_global, r);
}

}  // namespace

extern "C" {

// rows of the table of this image (wt_size)
int64_t sim_rows_size(const uint8_t *blob) { return (int64_t)rows_index(blob, nullptr).wt_size; }

// k_rows_fill: a word per BWT row, over the directory attached to the blob (sim_win_attach) or the tree; returns the replay rows
int64_t sim_rows_fill(const uint8_t *blob, uint32_t *rows) {
    const DevIndex ix = rows_index(blob, nullptr);
    int64_t replay = 0;
    for (uint32_t r = 0; r < ix.wt_size; ++r) {
        rows[r] = row_word(ix, r);
        replay += rows[r] >> 31;
    }
    return replay;
}

// the walk of a hit at every row as k_locate_walk runs it (position, distance, status): three arrays of wt_size entries
void sim_row_walk_all(const uint8_t *blob, int32_t *at, int32_t *distance, int32_t *status_out) {
    const DevIndex ix = rows_index(blob, nullptr);
    for (uint32_t r = 0; r < ix.wt_size; ++r) {
        int status = ST_OK;
        at[r] = fm_locate_hit<kWinAsk>(ix, ix.inv_global, (int32_t)r, 0, distance[r], status);
        status_out[r] = status;
    }
}

// mirrors launch_locate_walk's row-table branch + k_locate_rows: a group of 2^lanes_log2 lanes per pattern, lane g takes hits
// g, g + lanes, ...; the lanes of a group run one after the other here, each through the header's record, share and publish
// (fm_ticket_*).  order (nullable): 4 ints per record {start, end, pattern, -}.
// set_locs (nullable) / set_base / taken (nullable): a segment of a set.  Returns the group's width.
int32_t sim_locate_rows(const uint8_t *blob, const uint32_t *rows, const int32_t *range, int32_t n, int32_t max_matches, int32_t *locs,
                        int32_t loc_cap, int32_t *found, int32_t *lf, int32_t *status_out, const int32_t *taken, const int32_t *order,
                        int64_t *set_locs, int64_t set_base) {
    const DevIndex ix = rows_index(blob, rows);
    const int32_t lanes_log2 = fm_rows_lanes_log2(fm_locate_slots(max_matches, loc_cap));
    const int32_t lanes = 1 << lanes_log2;
    const int64_t total = (int64_t)n << lanes_log2;
    for (int64_t t = 0; t < total; ++t) {
        const int32_t g = (int32_t)(t & (lanes - 1));
        LocateTicket tk;
        const int32_t wanted = fm_ticket_record(tk, t >> lanes_log2, range, order, max_matches, loc_cap, taken);
        fm_ticket_publish(tk.p, g, tk.located, wanted, loc_cap, found, status_out);
        int status = ST_OK;
        const int32_t steps = fm_rows_gather<kWinAsk>(ix, ix.inv_global, tk.start, tk.located, g, lanes, locs + (int64_t)tk.p * loc_cap,
                                                      set_locs ? set_locs + fm_ticket_dest(tk.p, tk.before, 0, loc_cap, set_locs) : nullptr,
                                                      set_base, status);
        if (lf) lf[tk.p] += steps;
        if (status && status_out) status_out[tk.p] |= status;
    }
    return lanes;
}
}
