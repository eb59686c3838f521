// fmx_extract_packed.hip — the text of n ranges in ONE packed array, lanes per PIECE (fmx_extract_packed_*, fmx_line_text_batch;
// FM:564-608).  fmx_device.hpp ("EXTRACT, PACKED") has the contract and the per-item functions; here:
//
//   k_extract_packed_sizes   a lane per range: status, length, pieces; two exclusive scans (rocPRIM) give text_off and piece_off
//   k_extract_packed_fill    lanes per piece: tiles of kLocateAllTile pieces in a grid-stride loop, the tile's ranges decoded as
//                            k_locate_all decodes its patterns (fm_hit_tile, fm_hit_tile_slice), one fm_extract_piece per lane
//   k_extract_packed_redo    a lane per range on the redo list: the literal fm_extract into the range's slice, its status taken
//
// Compiled twice, like fmx_kernels.hip: as it stands (namespace fmx: the sizes pass, which looks at no image, and the walks over
// expanded images) and with -DFMX_COMPACT=1 -DFMX_KNS=fmxc (the walks over compact images).
#include <hip/hip_runtime.h>

#include "fmx_device.hpp"
#include "fmx_options.hpp"
#include "fmx_plan.hpp"

#if !defined(FMX_KNS)
#define FMX_KNS fmx
#endif

#if !FMX_COMPACT
#include <rocprim/device/device_scan.hpp>

namespace fmx {
namespace {

// lengths[i], pieces[i] of range i for i < n, 0 for i == n (the exclusive scans then leave the totals there)
__global__ __launch_bounds__(256) void k_extract_packed_sizes(int32_t enable_extract, int32_t length, int32_t sample_rate,
                                                               const int32_t *__restrict__ starts, const int32_t *__restrict__ stops,
                                                               int32_t n, int64_t *__restrict__ lengths, int64_t *__restrict__ pieces,
                                                               int32_t *__restrict__ status_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        lengths[i] = pieces[i] = 0;
        return;
    }
    DevIndex ix;  // (the three fields the geometry reads)
    ix.enable_extract = enable_extract;
    ix.length = length;
    ix.sample_rate = sample_rate;
    const int32_t start = starts[i], stop = stops[i];
    const int status = fm_extract_packed_status(ix, start, stop);
    status_out[i] = status;
    lengths[i] = fm_extract_packed_length(status, start, stop);
    pieces[i] = status == ST_OK ? fm_piece_count(ix, start, stop) : 0;
}

size_t sizes_bytes(int32_t n) { return (((size_t)n + 1) * sizeof(int64_t) + 255) / 256 * 256; }
size_t scan_bytes(int32_t n) {
    size_t tmp = 0;
    (void)rocprim::exclusive_scan(nullptr, tmp, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)n + 1,
                                  rocprim::plus<int64_t>());
    return (tmp + 255) / 256 * 256 + 256;
}
size_t redo_bytes(int32_t n) { return (((size_t)kPackedRedoHead + (size_t)n) * sizeof(int32_t) + 255) / 256 * 256; }
size_t flag_bytes(int32_t n) { return ((size_t)n * sizeof(int32_t) + 255) / 256 * 256 + 256; }

}  // namespace

// the workspace of both stages: {redo list | flags} for the fill, {lengths | pieces | the scan's scratch} for the offsets
size_t extract_packed_scratch_bytes(int32_t n) {
    if (n < 0) n = 0;
    return redo_bytes(n) + flag_bytes(n) + 2 * sizes_bytes(n) + scan_bytes(n);
}
int32_t *extract_packed_redo(void *scratch) { return static_cast<int32_t *>(scratch); }
int32_t *extract_packed_flags(void *scratch, int32_t n) {
    return reinterpret_cast<int32_t *>(static_cast<uint8_t *>(scratch) + redo_bytes(n));
}

int launch_extract_packed_offsets(const DevIndex &ix, const int32_t *start, const int32_t *stop, int32_t n, int64_t *text_off,
                                  int64_t *piece_off, int32_t *status, void *scratch, size_t scratch_bytes, void *stream) {
    if (n < 0) return 0;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (scratch_bytes < extract_packed_scratch_bytes(n)) return (int)hipErrorInvalidValue;
    uint8_t *at = static_cast<uint8_t *>(scratch) + redo_bytes(n) + flag_bytes(n);
    int64_t *lengths = reinterpret_cast<int64_t *>(at);
    int64_t *pieces = reinterpret_cast<int64_t *>(at + sizes_bytes(n));
    uint8_t *tmp = at + 2 * sizes_bytes(n);
    size_t tmp_bytes = scan_bytes(n);
    hipLaunchKernelGGL(k_extract_packed_sizes, dim3((unsigned)(((int64_t)n + 1 + 255) / 256)), dim3(256), 0, st, ix.enable_extract,
                       ix.length, ix.sample_rate, start, stop, n, lengths, pieces, status);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, lengths, text_off, (int64_t)0, (size_t)n + 1,
                                               rocprim::plus<int64_t>(), st);
        e != hipSuccess)
        return (int)e;
    return (int)rocprim::exclusive_scan(tmp, tmp_bytes, pieces, piece_off, (int64_t)0, (size_t)n + 1,
                                        rocprim::plus<int64_t>(), st);
}

}  // namespace fmx
#endif  // !FMX_COMPACT

namespace FMX_KNS {
using namespace fmx;
#include "fmx_kernel_api.hpp"    // launch_extract_packed_fill, as fmx_api.cpp sees it
#include "fmx_kernel_stage.hpp"  // the LDS stages, FMX_EXTRACT_KERNEL, grid_for, FMX_DISPATCH_WIN

// Lanes per PIECE.  A workgroup takes tiles of kLocateAllTile consecutive pieces of the packed order piece_off describes (n + 1
// entries: piece t belongs to the LAST range r with piece_off[r] <= t, exactly k_locate_all's layout of hits), in a grid-stride
// loop; lane i of a tile takes piece i (+ kBlock): adjacent lanes, adjacent pieces of the text — and adjacent slices of `chars`.
// A piece is a chain of at most P + sampleRate LF-steps whatever the range's length; a range of a megabyte is 32 tiles.
// A workgroup without a tile leaves before it stages anything (the grid is sized without knowing piece_off[n]).
// (over a compact image the value-of-offset table and the slice of piece_off make 67 KiB of LDS: two workgroups of 512 lanes per
// CU, four waves per SIMD — no occupancy target is asked for there, as for FMX_WALK_KERNEL)
#if FMX_COMPACT
#define FMX_PACKED_FILL_KERNEL(BLOCK) __global__ __launch_bounds__(BLOCK)
#else
#define FMX_PACKED_FILL_KERNEL(BLOCK) FMX_EXTRACT_KERNEL(BLOCK)
#endif
template <int kBlock, int kWin>
FMX_PACKED_FILL_KERNEL(kBlock) void k_extract_packed_fill(DevIndex ix_global, const int32_t *__restrict__ starts,
                                                      const int32_t *__restrict__ stops, int32_t n,
                                                      const int64_t *__restrict__ text_off, const int64_t *__restrict__ piece_off,
                                                      uint16_t *__restrict__ chars, int32_t *__restrict__ redo,
                                                      int32_t *__restrict__ flags) {
    static_assert(kLocateAllTile % kBlock == 0, "every lane of a workgroup runs the same number of rounds per tile");
    const int64_t total = piece_off[n];
    if ((int64_t)blockIdx.x * kLocateAllTile >= total) return;  // (workgroup-uniform)
    __shared__ int64_t s_off[kLocateAllSlice];
    FMX_FM_INV(ix_global);
    FMX_WITH_SB_CACHE(ix_global, ix);
    FMX_WITH_C_LDS(ix, kWin);
    for (int64_t tile = (int64_t)blockIdx.x * kLocateAllTile; tile < total; tile += (int64_t)gridDim.x * kLocateAllTile) {
        const HitTile h = fm_hit_tile(piece_off, n, tile, total);
        bool in_lds;
        const int64_t *slice = fm_hit_tile_slice<kBlock>(s_off, piece_off, h, in_lds);
        for (int32_t i = threadIdx.x; i < kLocateAllTile; i += kBlock) {
            const int64_t t = tile + i;
            if (t > h.tile_last) continue;
            int32_t k, a, b, steps;
            const int32_t r = fm_locate_all_resolve(slice, h.slice_count, h.p_lo, t, k);
            const int32_t start = starts[r], stop = stops[r];
            fm_piece_bounds(ix, start, stop, k, a, b);
            if (!fm_extract_piece<kWin>(ix, s_inv, a, b, b == stop, chars + text_off[r] + (a - start), steps)) fm_redo_once(flags, redo, r);
        }
        if (in_lds) __syncthreads();  // (the next tile's slice overwrites this one)
    }
}

// The ranges on the redo list, literally: fm_extract with dst_len = the range's length and offset 0 into the range's slice (its
// ragged ends leave character by character: the neighbours' characters stay), and the status it ends with.  The list's count is
// read here, on the device; nearly every launch finds 0 and stages nothing.
template <int kBlock, int kWin>
FMX_EXTRACT_KERNEL(kBlock) void k_extract_packed_redo(DevIndex ix_global, const int32_t *__restrict__ starts,
                                                      const int32_t *__restrict__ stops, const int64_t *__restrict__ text_off,
                                                      uint16_t *__restrict__ chars, int32_t *__restrict__ status_out,
                                                      const int32_t *__restrict__ redo) {
    const int32_t m = redo[0];
    if (m <= 0) return;
    FMX_FM_INV(ix_global);
    FMX_WITH_SB_CACHE(ix_global, ix);
    FMX_WITH_C_LDS(ix, kWin);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < m; t += stride) {
        const int32_t r = redo[kPackedRedoHead + t];
        const int32_t start = starts[r], stop = stops[r];
        int status = ST_OK;
        int32_t steps;
        (void)fm_extract<kWin>(ix, s_inv, start, stop, chars + text_off[r], stop - start, 0, steps, status);
        status_out[r] = status;
    }
}

// redo / flags: extract_packed_redo / extract_packed_flags of the call's workspace.  pieces: piece_off[n] where the host knows it
// (the grid is then a workgroup per tile up to the grid cap), -1 where it does not (the grid cap; a workgroup without a tile
// leaves at once).
int launch_extract_packed_fill(const DevIndex &ix, int n_cu, const int32_t *start, const int32_t *stop, int32_t n, const int64_t *text_off,
                               const int64_t *piece_off, int64_t pieces, uint16_t *chars, int32_t *status, int32_t *redo, int32_t *flags,
                               hipStream_t st) {
    if (hipError_t e = hipMemsetAsync(redo, 0, kPackedRedoHead * sizeof(int32_t), st); e != hipSuccess) return (int)e;
    if (n <= 0 || pieces == 0) return 0;
    if (hipError_t e = hipMemsetAsync(flags, 0, (size_t)n * sizeof(int32_t), st); e != hipSuccess) return (int)e;
    const int64_t most = (int64_t)1 << 48;  // (tiles x lanes stays inside an int64)
    const int64_t tiles = pieces < 0 ? most : ((pieces < most ? pieces : most) + kLocateAllTile - 1) / kLocateAllTile;
    const int64_t lanes = tiles * options().block;  // grid_for: a workgroup per `block` lanes
    FMX_DISPATCH_WIN(k_extract_packed_fill, ix, lanes, ix, start, stop, n, text_off, piece_off, chars, redo, flags);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    FMX_DISPATCH_WIN(k_extract_packed_redo, ix, (int64_t)n, ix, start, stop, text_off, chars, status, redo);
    return (int)hipGetLastError();
}

}  // namespace FMX_KNS
