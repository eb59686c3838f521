// fmx_hit_offsets.hip — the packed layout of "all occurrences" (fmx_locate_all_*; FM:487-552): from the {start, end} ranges the
// range search of a batch left (FM:506-523), hit_off[i] = number of hits of patterns 0 .. i - 1, n + 1 int64 entries.
// k_hit_counts clamps each range to what locate() stores for it (fm_locate_all_hits: min(count, maxMatches) for maxMatches > 0,
// FM:544-546), rocPRIM's exclusive scan sums them.  Nothing here looks at the image, so this file is compiled once — not per
// image form like fmx_kernels.hip.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "fmx_device.hpp"
#include "fmx_plan.hpp"

namespace fmx {
namespace {

// counts[i] = hits of pattern i for i < n, and 0 for i == n (the exclusive scan then leaves the batch's total there)
__global__ __launch_bounds__(256) void k_hit_counts(const int32_t *__restrict__ range, int32_t n, int32_t max_matches,
                                                    int64_t *__restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    counts[i] = i < n ? fm_locate_all_hits(range[2 * i], range[2 * i + 1], max_matches) : 0;
}

size_t counts_bytes(int32_t n) { return ((size_t)n + 1) * sizeof(int64_t) / 256 * 256 + 256; }

}  // namespace

size_t hit_offsets_scratch_bytes(int32_t n) {
    size_t tmp = 0;
    (void)rocprim::exclusive_scan(nullptr, tmp, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)n + 1,
                                  rocprim::plus<int64_t>());
    return counts_bytes(n) + (tmp + 255) / 256 * 256 + 256;
}

int launch_hit_offsets(const int32_t *range, int32_t n, int32_t max_matches, int64_t *hit_off, void *scratch, size_t scratch_bytes,
                       void *stream) {
    if (n < 0) return 0;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (scratch_bytes < hit_offsets_scratch_bytes(n)) return (int)hipErrorInvalidValue;
    int64_t *counts = static_cast<int64_t *>(scratch);
    uint8_t *tmp = static_cast<uint8_t *>(scratch) + counts_bytes(n);
    size_t tmp_bytes = scratch_bytes - counts_bytes(n);
    hipLaunchKernelGGL(k_hit_counts, dim3((unsigned)(((int64_t)n + 1 + 255) / 256)), dim3(256), 0, st, range, n, max_matches, counts);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    return (int)rocprim::exclusive_scan(tmp, tmp_bytes, counts, hit_off, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st);
}

}  // namespace fmx
