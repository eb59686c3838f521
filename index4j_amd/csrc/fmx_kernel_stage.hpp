// fmx_kernel_stage.hpp — what the FM kernels of fmx_kernels.hip and fmx_extract_packed.hip share: the tables a workgroup stages
// in LDS before it walks (the value-of-offset table of a compact image, the superblock headers, cumulativeCounts), the register
// budget of the extract kernels, the grid rule and the dispatch of a walk kernel by directory form.
//
// NO include guard and no namespace of its own: like fmx_kernel_api.hpp it is included INSIDE the namespace a translation unit
// defines its kernels in (fmx for expanded images, fmxc — with -DFMX_COMPACT=1 — for compact ones), behind `using namespace fmx`,
// fmx_device.hpp, fmx_options.hpp and <hip/hip_runtime.h>.

// the value-of-offset table of an FM kernel: none in an expanded image, 32 KiB of LDS in a compact one
#if FMX_COMPACT
#define FMX_FM_INV(IX)                                \
    __shared__ uint16_t s_inv_lds[kInvEntries];       \
    stage_inverse_table(s_inv_lds, (IX).inv_global);  \
    const uint16_t *s_inv = s_inv_lds
#else
#define FMX_FM_INV(IX) const uint16_t *s_inv = nullptr /* no RRR vector on an expanded image's path */
#endif

// k_extract: 49.8 ms at a budget for 8 waves, 47.7 ms at 6 (locate -> extract pipeline, tools/bench_pipeline.py)
#ifndef FMX_EXTRACT_WAVES
#define FMX_EXTRACT_WAVES 6
#endif
#define FMX_EXTRACT_KERNEL(BLOCK) \
    __global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(FMX_EXTRACT_WAVES, 8)))

__device__ __forceinline__ void stage_inverse_table(uint16_t *s_inv, const uint16_t *g_inv) {
    const uint4 *src = reinterpret_cast<const uint4 *>(g_inv);
    uint4 *dst = reinterpret_cast<uint4 *>(s_inv);
    for (int i = threadIdx.x; i < kInvEntries * 2 / 16; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// The header quad and the bit-vector view quad of every superblock (32 bytes each) are staged in LDS when the
// index has at most kSbCacheMax superblocks (335 M symbols): the first stage of every rank / inverseSelect then
// reads LDS instead of HBM, and what depends only on the header is requested one round trip earlier.
constexpr int kSbCacheMax = 320;
__device__ __forceinline__ const Quad *stage_sb_cache(Quad *s_sb, const DevIndex &ix) {
    if (ix.n_sb > kSbCacheMax || ix.n_sb > ix.sb_cache_limit) return nullptr;
    const Quad *src = reinterpret_cast<const Quad *>(ix.sbd);
    for (int i = threadIdx.x; i < 2 * ix.n_sb; i += blockDim.x) s_sb[i] = src[(i >> 1) * 4 + (i & 1) * 2];
    __syncthreads();
    return s_sb;
}
#define FMX_WITH_SB_CACHE(GLOBAL_IX, LOCAL_IX)      \
    __shared__ Quad s_sb[2 * kSbCacheMax];          \
    DevIndex LOCAL_IX = GLOBAL_IX;                  \
    LOCAL_IX.sb_cache = stage_sb_cache(s_sb, GLOBAL_IX)

// cumulativeCounts in LDS for the kernels that read SYMBOLS out of a window directory with four-byte entries (win_symbol_of_row:
// an entry is the row a step arrives at, its symbol the largest c with C[c] < row) — extract and extractUntilBoundary; locate
// never asks.  Alphabets beyond kWinSymbolSearchMax entries keep six-byte entries (or, forced to four, search C where it lies).
__device__ __forceinline__ void stage_c_lds(int32_t *s_c, uint16_t *s_lut, DevIndex &ix) {
    ix.c_lds = nullptr;
    ix.c_lut = nullptr;
    ix.c_lut_shift = 0;
    if (!ix.win || !ix.win_entry4 || ix.n_c > kWinSymbolSearchMax) return;
    for (int i = threadIdx.x; i < ix.n_c; i += blockDim.x) s_c[i] = ix.C[i];
    __syncthreads();
    ix.c_lds = s_c;
    // where a row's search starts: entry b = the largest c with C[c] < b << shift (win_symbol_of_row)
    const int32_t shift = win_lut_shift(ix.length);
    for (int b = threadIdx.x; b <= kWinLutBuckets; b += blockDim.x) {
        const int64_t row = (int64_t)b << shift;
        s_lut[b] = (uint16_t)win_symbol_of_row(ix, row > 0x7fffffff ? 0x7fffffff : (int32_t)row);
    }
    __syncthreads();
    ix.c_lut = s_lut;
    ix.c_lut_shift = shift;
}
#define FMX_WITH_C_LDS(IX, KWIN)                                                  \
    __shared__ int32_t s_c_lds[(KWIN) == kWinNever ? 1 : kWinSymbolSearchMax];    \
    __shared__ uint16_t s_c_lut[(KWIN) == kWinNever ? 1 : kWinLutBuckets + 2];    \
    if ((KWIN) != kWinNever) stage_c_lds(s_c_lds, s_c_lut, IX)

// tunables: fmx_options.hpp (one reading of an option per decision)
static int grid_for(int64_t lanes, int block, int n_cu) {
    int64_t blocks = (lanes + block - 1) / block;
    const int64_t cap = (int64_t)n_cu * options().groups_per_cu;  // a few rounds of workgroups per CU, grid-stride the rest
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

// ... of a walk kernel instantiated for indexes with a window directory (in either form) and without one (fmx_device.hpp: kWinAlways /
// kWinFlat / kWinNever)
#define FMX_DISPATCH_WIN(KERNEL, IX, LANES, ...)                                                                       \
    do {                                                                                                               \
        const int blk__ = options().block;                                                                             \
        const dim3 grid__(grid_for((LANES), blk__, n_cu));                                                             \
        const size_t lds__ = (size_t)options().lds_pad_kb * 1024;                                                      \
        if ((IX).win && (IX).win_flat) {                                                                               \
            if (blk__ == 1024)                                                                                         \
                hipLaunchKernelGGL((KERNEL<1024, kWinFlat>), grid__, dim3(1024), lds__, st, __VA_ARGS__);             \
            else                                                                                                       \
                hipLaunchKernelGGL((KERNEL<512, kWinFlat>), grid__, dim3(512), lds__, st, __VA_ARGS__);               \
        } else if ((IX).win) {                                                                                         \
            if (blk__ == 1024)                                                                                         \
                hipLaunchKernelGGL((KERNEL<1024, kWinAlways>), grid__, dim3(1024), lds__, st, __VA_ARGS__);           \
            else                                                                                                       \
                hipLaunchKernelGGL((KERNEL<512, kWinAlways>), grid__, dim3(512), lds__, st, __VA_ARGS__);             \
        } else {                                                                                                       \
            if (blk__ == 1024)                                                                                         \
                hipLaunchKernelGGL((KERNEL<1024, kWinNever>), grid__, dim3(1024), lds__, st, __VA_ARGS__);            \
            else                                                                                                       \
                hipLaunchKernelGGL((KERNEL<512, kWinNever>), grid__, dim3(512), lds__, st, __VA_ARGS__);              \
        }                                                                                                              \
    } while (0)
