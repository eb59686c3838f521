// fmx_sa_query.hip — the kernels of index4j's SuffixArray (SA:100-157) over its resident form (fmx_sa_device.hpp), and the
// gather of BurrowsWheelerTransform (BWT:100-108).
//
// k_sa_search: one lane per pattern, grid-stride.  Each workgroup first stages the fence table in LDS (64 KiB at the
// default 4,096 fences x 8 chars); the left search then runs its first levels there — a pattern of at most K chars reads
// no text until it leaves the fences — and the rest in HBM.  A level in HBM is two dependent random requests (the array
// entry, then the text), so the kernel is bound by requests in flight, not by instructions: the LDS table caps it at two
// workgroups per CU, i.e. 16 waves per CU at 512 lanes and 32 at 1024 (option "block").
// k_sa_locate_copy: SA[left .. left + found) of every pattern into its row of `locs`, flattened over an inclusive scan of
// `found`, so that neighbouring lanes read neighbouring entries.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "fmx_options.hpp"
#include "fmx_sa_index.hpp"

namespace fmx {
namespace {

constexpr size_t kFenceLdsMax = 64 * 1024;  // fence keys staged per workgroup

int grid_for(int64_t lanes, int block, int n_cu) {
    int64_t blocks = (lanes + block - 1) / block;
    const int64_t cap = (int64_t)n_cu * options().groups_per_cu;  // a few rounds of workgroups per CU, grid-stride the rest
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

__global__ void k_sa_fences(SaView v, uint16_t *__restrict__ keys, uint8_t *__restrict__ lens) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= v.n_fences) return;
    const int32_t pos = v.sa[j << v.fence_shift];
    const int32_t len = sa_min(v.fence_chars, v.n - pos);
    for (int32_t u = 0; u < v.fence_chars; ++u) keys[j * v.fence_chars + u] = u < len ? v.text[pos + u] : (uint16_t)0;
    lens[j] = (uint8_t)len;
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_sa_search(SaView v, const uint16_t *__restrict__ g_keys,
                                                     const uint16_t *__restrict__ pat, const int32_t *__restrict__ pat_off,
                                                     int32_t n, int32_t max_matches, int32_t *__restrict__ counts,
                                                     int32_t *__restrict__ left, int32_t *__restrict__ found) {
    extern __shared__ uint4 s_keys[];
    const int32_t words = (int32_t)(((int64_t)v.n_fences * v.fence_chars * 2 + 15) / 16);
    const uint4 *src = reinterpret_cast<const uint4 *>(g_keys);
    for (int32_t w = threadIdx.x; w < words; w += BLOCK) s_keys[w] = src[w];
    __syncthreads();
    const uint16_t *keys = reinterpret_cast<const uint16_t *>(s_keys);
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const int32_t o = pat_off[i];
        const SaRange r = sa_search(v, keys, pat + o, pat_off[i + 1] - o);
        const int32_t c = r.right - r.left;
        if (counts) counts[i] = c;
        if (left) left[i] = r.left;
        if (found) found[i] = sa_min(c, max_matches);
    }
}

// lane t of the flattened hits: pattern i = the first with incl[i] > t, hit k = t - (incl[i] - found[i])
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_sa_locate_copy(const int32_t *__restrict__ sa, const int32_t *__restrict__ left,
                                                          const int32_t *__restrict__ found,
                                                          const int32_t *__restrict__ incl, int32_t n, int32_t max_matches,
                                                          int32_t *__restrict__ locs) {
    const int64_t total = n > 0 ? incl[n - 1] : 0;
    for (int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * BLOCK) {
        int32_t a = 0, b = n - 1;
        while (a < b) {
            const int32_t m = sa_mid(a, b);
            if (incl[m] > t)
                b = m;
            else
                a = m + 1;
        }
        const int32_t k = (int32_t)(t - (incl[a] - found[a]));
        locs[(int64_t)a * max_matches + k] = sa[left[a] + k];
    }
}

__global__ void k_bwt_gather(const int32_t *__restrict__ sa, const uint16_t *__restrict__ text1, int32_t n1,
                             uint16_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    const int32_t s = sa[i + 1];
    out[i] = s == 0 ? (uint16_t)0 : text1[s - 1];
}

}  // namespace

int sa_fence_settings(int32_t n, int32_t *n_fences, int32_t *shift, int32_t *chars) {
    const int32_t most = options().sa_fences, k = options().sa_fence_chars;
    int32_t s = 0;
    while (most > 0 && (((int64_t)n + (1ll << s) - 1) >> s) > most) ++s;
    *n_fences = most > 0 ? (int32_t)(((int64_t)n + (1ll << s) - 1) >> s) : 0;
    *shift = s;
    *chars = k;
    return (size_t)*n_fences * (size_t)k * 2 <= kFenceLdsMax ? 0 : -1;
}

int launch_sa_fences(const SaView &v, uint16_t *keys, uint8_t *lens, void *stream) {
    if (v.n_fences > 0)
        hipLaunchKernelGGL(k_sa_fences, dim3((unsigned)((v.n_fences + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), v, keys, lens);
    return (int)hipGetLastError();
}

int launch_sa_search(const SaView &v, const uint16_t *keys, int n_cu, const uint16_t *pat, const int32_t *pat_off,
                     int32_t n, int32_t max_matches, int32_t *counts, int32_t *left, int32_t *found, void *stream) {
    if (n <= 0) return 0;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int blk = options().block;
    const dim3 grid(grid_for(n, blk, n_cu));
    const size_t lds = ((size_t)v.n_fences * v.fence_chars * 2 + 15) / 16 * 16;
    if (blk == 1024)
        hipLaunchKernelGGL(k_sa_search<1024>, grid, dim3(1024), lds, st, v, keys, pat, pat_off, n, max_matches, counts,
                           left, found);
    else
        hipLaunchKernelGGL(k_sa_search<512>, grid, dim3(512), lds, st, v, keys, pat, pat_off, n, max_matches, counts, left,
                           found);
    return (int)hipGetLastError();
}

size_t sa_locate_scratch_bytes(int32_t n) {
    size_t tmp = 0;
    (void)rocprim::inclusive_scan(nullptr, tmp, (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)(n > 0 ? n : 1),
                                  rocprim::plus<int32_t>());
    return (size_t)(n > 0 ? n : 1) * 4 + (tmp + 255) / 256 * 256 + 256;
}

int launch_sa_locate_copy(const SaView &v, int n_cu, const int32_t *left, const int32_t *found, int32_t n,
                          int32_t max_matches, int32_t *locs, void *scratch, size_t scratch_bytes, void *stream) {
    if (n <= 0 || max_matches <= 0) return 0;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t *incl = static_cast<int32_t *>(scratch);
    uint8_t *tmp = static_cast<uint8_t *>(scratch) + ((size_t)n * 4 + 255) / 256 * 256;
    size_t tmp_bytes = scratch_bytes - ((size_t)n * 4 + 255) / 256 * 256;
    hipError_t e = rocprim::inclusive_scan(tmp, tmp_bytes, found, incl, (size_t)n, rocprim::plus<int32_t>(), st);
    if (e != hipSuccess) return (int)e;
    const int blk = options().block;
    const dim3 grid(grid_for((int64_t)n * max_matches, blk, n_cu));
    if (blk == 1024)
        hipLaunchKernelGGL(k_sa_locate_copy<1024>, grid, dim3(1024), 0, st, v.sa, left, found, incl, n, max_matches, locs);
    else
        hipLaunchKernelGGL(k_sa_locate_copy<512>, grid, dim3(512), 0, st, v.sa, left, found, incl, n, max_matches, locs);
    return (int)hipGetLastError();
}

int launch_bwt_gather(const int32_t *d_sa, const uint16_t *d_text1, int32_t n1, uint16_t *d_out, void *stream) {
    if (n1 > 0)
        hipLaunchKernelGGL(k_bwt_gather, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           d_sa, d_text1, n1, d_out);
    return (int)hipGetLastError();
}

}  // namespace fmx
