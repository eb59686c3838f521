// extract_packed_hostsim.cpp — TEST-ONLY host build of the device code of "extract, packed" (fmx_extract_packed_*):
// index4j_amd/csrc/fmx_device.hpp's fm_extract_packed_status / _length, fm_piece_len / _count / _bounds, fm_seek_at_or_after,
// fm_extract_piece, fm_redo_once and the literal fm_extract, driven by mirrors of the three kernels of fmx_extract_packed.hip —
// the sizes pass with its two scans, the fill kernel's tile loop (fm_hit_tile, fm_locate_all_resolve over piece_off) and the
// redo pass — with the lanes run one after the other.  g++ compiles the header's FMX_HD functions as plain C++, so the CPU suite
// checks the very source the kernels run against the oracle (tests/test_extract_packed_cpu.py).  The image's view and the
// window directory come from tests/hostsim.cpp, included as it stands.  Never part of libfmx.so.
#include "hostsim.cpp"

#include <vector>

namespace {

// (the instantiation FMX_DISPATCH_WIN picks for the directory the index has)
bool packed_piece(const DevIndex &ix, int32_t a, int32_t b, bool last, uint16_t *dest, int32_t &steps) {
    return ix.win && ix.win_flat ? fm_extract_piece<kWinFlat>(ix, ix.inv_global, a, b, last, dest, steps)
           : ix.win              ? fm_extract_piece<kWinAlways>(ix, ix.inv_global, a, b, last, dest, steps)
                                 : fm_extract_piece<kWinNever>(ix, ix.inv_global, a, b, last, dest, steps);
}
void packed_literal(const DevIndex &ix, int32_t start, int32_t stop, uint16_t *dest, int32_t &steps, int &status) {
    if (ix.win && ix.win_flat)
        (void)fm_extract<kWinFlat>(ix, ix.inv_global, start, stop, dest, stop - start, 0, steps, status);
    else if (ix.win)
        (void)fm_extract<kWinAlways>(ix, ix.inv_global, start, stop, dest, stop - start, 0, steps, status);
    else
        (void)fm_extract<kWinNever>(ix, ix.inv_global, start, stop, dest, stop - start, 0, steps, status);
}

}  // namespace

extern "C" {

int32_t sim_piece_len(const uint8_t *blob) { return fm_piece_len(make_index(blob)); }

// out = {row, skip} of fm_seek_at_or_after(x), {row, skip} of fm_seek_after(x), then the rows both walks stand on once their skip
// is dropped (-1: a step of that walk was not clean)
void sim_packed_seek(const uint8_t *blob, int32_t x, int32_t *out) {
    const DevIndex ix = make_index(blob);
    fm_seek_at_or_after(ix, x, out[0], out[1]);
    fm_seek_after(ix, x, out[2], out[3]);
    for (int w = 0; w < 2; ++w) {
        int32_t row = out[2 * w];
        for (int32_t d = 0; d < out[2 * w + 1] && row >= 0; ++d) {
            int32_t c;
            int status = ST_OK;
            bool suspect = false;
            row = fm_lf_step<false, kWinAsk>(ix, ix.inv_global, row, c, status, suspect);
            if (status != ST_OK || suspect) row = -1;
        }
        out[4 + w] = row;
    }
}

// k_extract_packed_sizes + the two exclusive scans
void sim_packed_offsets(const uint8_t *blob, const int32_t *starts, const int32_t *stops, int32_t n, int64_t *text_off, int64_t *piece_off,
                        int32_t *status_out) {
    const DevIndex ix = make_index(blob);
    int64_t chars = 0, pieces = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int status = fm_extract_packed_status(ix, starts[i], stops[i]);
        status_out[i] = status;
        text_off[i] = chars;
        piece_off[i] = pieces;
        chars += fm_extract_packed_length(status, starts[i], stops[i]);
        pieces += status == ST_OK ? fm_piece_count(ix, starts[i], stops[i]) : 0;
    }
    text_off[n] = chars;
    piece_off[n] = pieces;
}

// [a, b) of every piece of the packed order, 2 ints each, and the range it belongs to (fm_hit_pattern over the whole of piece_off)
void sim_packed_pieces(const uint8_t *blob, const int32_t *starts, const int32_t *stops, int32_t n, const int64_t *piece_off, int32_t *ab,
                       int32_t *range_of) {
    const DevIndex ix = make_index(blob);
    for (int64_t t = 0; t < piece_off[n]; ++t) {
        const int32_t r = fm_hit_pattern(piece_off, n, t);
        range_of[t] = r;
        fm_piece_bounds(ix, starts[r], stops[r], (int32_t)(t - piece_off[r]), ab[2 * t], ab[2 * t + 1]);
    }
}

// mirrors launch_extract_packed_fill: k_extract_packed_fill with `grid` workgroups of `block` lanes over the tiles of piece_off
// (slice_max = kLocateAllSlice, or smaller to send tiles down the route that searches piece_off where it lies), then
// k_extract_packed_redo over the list.  redo: kPackedRedoHead + n ints, flags: n ints (both zeroed here, as the launcher does).
// info (6 slots) = {ranges redone, tiles that searched piece_off where it lies, LF-steps of the fill, the longest chain of one
// piece, LF-steps of the redo pass, tiles}.
void sim_packed_fill(const uint8_t *blob, const int32_t *starts, const int32_t *stops, int32_t n, const int64_t *text_off,
                     const int64_t *piece_off, uint16_t *chars, int32_t *status_out, int32_t *redo, int32_t *flags, int32_t block,
                     int32_t grid, int32_t slice_max, int64_t *info) {
    const DevIndex ix = make_index(blob);
    for (int i = 0; i < 6; ++i) info[i] = 0;
    for (int i = 0; i < kPackedRedoHead; ++i) redo[i] = 0;
    if (n <= 0) return;
    for (int32_t i = 0; i < n; ++i) flags[i] = 0;
    const int64_t total = piece_off[n];
    std::vector<int64_t> s_off((size_t)kLocateAllSlice);
    for (int64_t group = 0; group < grid; ++group) {
        if (group * kLocateAllTile >= total) continue;
        for (int64_t tile = group * kLocateAllTile; tile < total; tile += (int64_t)grid * kLocateAllTile) {
            const HitTile h = fm_hit_tile(piece_off, n, tile, total);
            const bool in_lds = h.slice_count <= slice_max;  // (fm_hit_tile_slice, with the caller's bound)
            if (in_lds)
                for (int32_t i = 0; i < h.slice_count; ++i) s_off[(size_t)i] = piece_off[h.p_lo + i];
            else
                ++info[1];
            ++info[5];
            const int64_t *slice = in_lds ? s_off.data() : piece_off + h.p_lo;
            for (int32_t round = 0; round < kLocateAllTile; round += block) {
                for (int32_t lane = 0; lane < block; ++lane) {
                    const int64_t t = tile + round + lane;
                    if (t > h.tile_last) continue;
                    int32_t k, a, b, steps;
                    const int32_t r = fm_locate_all_resolve(slice, h.slice_count, h.p_lo, t, k);
                    const int32_t start = starts[r], stop = stops[r];
                    fm_piece_bounds(ix, start, stop, k, a, b);
                    if (!packed_piece(ix, a, b, b == stop, chars + text_off[r] + (a - start), steps)) fm_redo_once(flags, redo, r);
                    info[2] += steps;
                    if (steps > info[3]) info[3] = steps;
                }
            }
        }
    }
    info[0] = redo[0];
    for (int32_t t = 0; t < redo[0]; ++t) {
        const int32_t r = redo[kPackedRedoHead + t];
        int status = ST_OK;
        int32_t steps;
        packed_literal(ix, starts[r], stops[r], chars + text_off[r], steps, status);
        status_out[r] = status;
        info[4] += steps;
    }
}
}
