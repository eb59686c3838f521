// fmx_class_api.cpp — the device stages of the class search (include/fmx.h "CLASS PATTERNS over device pointers") over
// fmx_class_search.hip's launchers: argument checks, the image form, the launch.  Of a handle this file sees what fmx::class_view
// hands out.  The host forms (fmx_count_class_batch, fmx_locate_all_class_batch, fmx_match_query_class_batch) run these stages from
// fmx_api.cpp, in the one sequence of the packed host forms.
#include "fmx_device.hpp"
#include "fmx_host_stage.hpp"

#include <hip/hip_runtime.h>

namespace fmx {
#include "fmx_kernel_api.hpp"
}  // namespace fmx
namespace fmxc {
#include "fmx_kernel_api.hpp"
}

namespace {

using fmx::api_fail;
using fmx::guarded;

int launch_search(const fmx::ClassView &v, const uint16_t *alt, const int32_t *pos_off, const int32_t *pat_off, int32_t n, int32_t max_ranges,
                  int64_t *range_cnt, int32_t *counts, int32_t *status, const int64_t *range_off, int32_t *ranges, hipStream_t st) {
    const int e = v.compact ? fmxc::launch_class_search(*v.dev, v.n_cu, alt, pos_off, pat_off, n, max_ranges, range_cnt, counts, status,
                                                        range_off, ranges, st)
                            : fmx::launch_class_search(*v.dev, v.n_cu, alt, pos_off, pat_off, n, max_ranges, range_cnt, counts, status,
                                                       range_off, ranges, st);
    if (e) return api_fail(FMX_E_HIP, std::string("k_class_search launch: ") + hipGetErrorString((hipError_t)e));
    return FMX_OK;
}

bool max_ranges_ok(int32_t max_ranges) { return max_ranges >= 1 && max_ranges <= FMX_CLASS_RANGES_MAX; }

}  // namespace

extern "C" {

size_t fmx_class_ranges_scratch_bytes(int32_t n) { return fmx::class_ranges_scratch_bytes(n); }

int fmx_class_ranges_count_dev(const fmx_index *idx, const uint16_t *d_alt, const int32_t *d_pos_off, const int32_t *d_pat_off, int32_t n,
                               int32_t max_ranges, int64_t *d_range_off, int32_t *d_counts, int32_t *d_status, void *scratch,
                               size_t scratch_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || !d_range_off || !max_ranges_ok(max_ranges) || (n > 0 && (!d_pos_off || !d_pat_off || !scratch)))
        return api_fail(FMX_E_ARG, "bad arguments");
    fmx::ClassView view;
    if (const int rc = fmx::class_view(idx, &view)) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) {
        FMX_HIP_TRY(hipMemsetAsync(d_range_off, 0, sizeof(int64_t), st));
        return FMX_OK;
    }
    if (scratch_bytes < fmx::class_ranges_scratch_bytes(n)) return api_fail(FMX_E_ARG, "scratch smaller than fmx_class_ranges_scratch_bytes");
    if (const int rc = launch_search(view, d_alt, d_pos_off, d_pat_off, n, max_ranges, fmx::class_ranges_counts(scratch), d_counts, d_status,
                                     nullptr, nullptr, st))
        return rc;
    const int e = fmx::launch_class_range_offsets(scratch, scratch_bytes, n, d_range_off, stream);
    if (e) return api_fail(FMX_E_HIP, std::string("class range offsets: ") + hipGetErrorString((hipError_t)e));
    return FMX_OK;
    });
}

int fmx_class_ranges_fill_dev(const fmx_index *idx, const uint16_t *d_alt, const int32_t *d_pos_off, const int32_t *d_pat_off, int32_t n,
                              int32_t max_ranges, const int64_t *d_range_off, int32_t *d_ranges, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || !d_range_off || !max_ranges_ok(max_ranges) || (n > 0 && (!d_pos_off || !d_pat_off || !d_ranges)))
        return api_fail(FMX_E_ARG, "bad arguments");
    fmx::ClassView view;
    if (const int rc = fmx::class_view(idx, &view)) return rc;
    if (n == 0) return FMX_OK;
    return launch_search(view, d_alt, d_pos_off, d_pat_off, n, max_ranges, nullptr, nullptr, nullptr, d_range_off, d_ranges,
                         static_cast<hipStream_t>(stream));
    });
}

size_t fmx_class_hit_offsets_scratch_bytes(int64_t m) { return m < 0 || m > INT32_MAX ? 0 : fmx::hit_offsets_scratch_bytes((int32_t)m); }

int fmx_class_hit_offsets_dev(const fmx_index *idx, int32_t n, const int64_t *d_range_off, const int32_t *d_ranges, int64_t m,
                              int64_t *d_range_hit_off, int64_t *d_hit_off, void *scratch, size_t scratch_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || m < 0 || m > INT32_MAX || !d_range_hit_off || !d_hit_off || (n > 0 && !d_range_off) || (m > 0 && !d_ranges) || !scratch)
        return api_fail(FMX_E_ARG, "bad arguments");
    fmx::ClassView view;
    if (const int rc = fmx::class_view(idx, &view)) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) {
        FMX_HIP_TRY(hipMemsetAsync(d_hit_off, 0, sizeof(int64_t), st));
        FMX_HIP_TRY(hipMemsetAsync(d_range_hit_off, 0, sizeof(int64_t), st));
        return FMX_OK;
    }
    if (scratch_bytes < fmx::hit_offsets_scratch_bytes((int32_t)m)) return api_fail(FMX_E_ARG, "scratch smaller than fmx_class_hit_offsets_scratch_bytes");
    const int e = fmx::launch_class_hit_offsets(d_ranges, (int32_t)m, d_range_off, n, d_range_hit_off, d_hit_off, scratch, scratch_bytes, stream);
    if (e) return api_fail(FMX_E_HIP, std::string("class hit offsets: ") + hipGetErrorString((hipError_t)e));
    return FMX_OK;
    });
}

int fmx_class_fold_status_dev(const fmx_index *idx, int32_t n, const int64_t *d_range_off, int64_t m, const int32_t *d_range_status,
                              int32_t *d_status, void *stream) {
    return guarded([&]() -> int {
    if (!idx || n < 0 || m < 0 || m > INT32_MAX || (n > 0 && (!d_range_off || !d_status)) || (m > 0 && !d_range_status))
        return api_fail(FMX_E_ARG, "bad arguments");
    fmx::ClassView view;
    if (const int rc = fmx::class_view(idx, &view)) return rc;
    const int e = fmx::launch_class_fold_status(d_range_off, n, (int32_t)m, d_range_status, d_status, stream);
    if (e) return api_fail(FMX_E_HIP, std::string("class fold status: ") + hipGetErrorString((hipError_t)e));
    return FMX_OK;
    });
}

}  // extern "C"
