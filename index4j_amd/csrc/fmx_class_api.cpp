// fmx_class_api.cpp — the C ABI of the class search (include/fmx.h "PATTERNS OF CHARACTER CLASSES", "CLASS PATTERNS over device
// pointers"): the device stages over fmx_class_search.hip's launchers, and the three host forms, which run those stages and then
// the EXISTING packed calls (fmx_locate_all_fill_dev, fmx_query_lines_of_hits_dev) through the public ABI — the ranges of a class
// batch are made so that everything downstream runs unchanged.  Of a handle this file sees what fmx::class_view hands out; device
// blocks come from the recycling cache of the other host forms and the kernels run on the calling thread's stream (fmx_plan.hpp).
#include "../../include/fmx.h"
#include "fmx_device.hpp"
#include "fmx_plan.hpp"

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>
#include <exception>
#include <new>
#include <string>

namespace fmx {
#include "fmx_kernel_api.hpp"
int api_fail(int code, const std::string &msg);  // fmx_api.cpp: the calling thread's fmx_last_error
}  // namespace fmx
namespace fmxc {
#include "fmx_kernel_api.hpp"
}

namespace {

using fmx::api_fail;

template <class F>
int guarded(F &&body) {  // (the ABI never throws)
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return api_fail(FMX_E_UNSUPPORTED, "out of host memory");
    } catch (const std::exception &e) {
        return api_fail(FMX_E_UNSUPPORTED, std::string("internal error: ") + e.what());
    }
}

#define CLASS_HIP_TRY(expr)                                                                  \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            (void)hipGetLastError();                                                         \
            return api_fail(FMX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
        }                                                                                    \
    } while (0)

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

// ---- what the host forms own for the length of a call ----------------------------------------------------------------------
struct DevBlock {  // a block of the recycling cache the other host forms use (hipMalloc / hipFree cost more than a small batch's kernels)
    void *p = nullptr;
    size_t bytes = 0;
    int device = 0;
    ~DevBlock() { fmx::class_scratch_give(device, bytes, p); }
    int alloc(size_t want) {
        bytes = want ? want : 8;
        const hipError_t e = (hipError_t)fmx::class_scratch_take(&bytes, &device, &p);
        if (e == hipSuccess) return FMX_OK;
        (void)hipGetLastError();
        p = nullptr;
        if (e == hipErrorOutOfMemory) return api_fail(FMX_E_NOMEM, "out of device memory for " + std::to_string(want) + " bytes of scratch");
        return api_fail(FMX_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
};
struct CallStream {  // the calling thread's stream; declared BEHIND the call's blocks: it is waited for before they return to the cache
    hipStream_t s = nullptr;
    int init(int device) {
        void *st = nullptr;
        const int rc = fmx::class_call_stream(device, &st);
        s = static_cast<hipStream_t>(st);
        return rc;
    }
    ~CallStream() {
        if (s) (void)hipStreamSynchronize(s);
    }
};
struct HostResult {  // a result that was not handed over is freed
    int32_t *p = nullptr;
    ~HostResult() { free(p); }
};

int check_class_offsets(const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n) {
    if (pos_off[0] < 0 || pat_off[0] < 0) return api_fail(FMX_E_ARG, "offsets start below 0");
    for (int32_t j = 0; j < n_pos; ++j)
        if (pos_off[j + 1] < pos_off[j]) return api_fail(FMX_E_ARG, "position offsets decrease");
    for (int32_t i = 0; i < n; ++i)
        if (pat_off[i + 1] < pat_off[i]) return api_fail(FMX_E_ARG, "pattern offsets decrease");
    if (pat_off[n] > n_pos) return api_fail(FMX_E_ARG, "pattern offsets end behind the positions");
    return FMX_OK;
}

// the batch on the device and both stages of its search
struct ClassCall {
    fmx::ClassView view{};
    DevBlock alt, pos, pat, range_off, counts, status, scratch, ranges;
    int64_t m = 0;
};

int class_args(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n,
               int32_t max_ranges, fmx::ClassView *view) {
    if (!idx || n < 0 || n_pos < 0 || !pos_off || !pat_off || !max_ranges_ok(max_ranges)) return api_fail(FMX_E_ARG, "bad arguments");
    if (const int rc = check_class_offsets(pos_off, n_pos, pat_off, n)) return rc;  // (the arrays first: they are judged on any handle)
    if (pos_off[n_pos] > 0 && !alt) return api_fail(FMX_E_ARG, "bad arguments");
    return fmx::class_view(idx, view);
}

// n > 0, the arguments checked: the arrays go up, stage 1 runs, m comes down, stage 2 (want_ranges) fills call.ranges
int class_search_host(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n,
                      int32_t max_ranges, bool want_ranges, ClassCall &call, hipStream_t st) {
    const size_t alts = (size_t)pos_off[n_pos];
    int rc;
    if ((rc = call.alt.alloc(alts * 2 + 8)) || (rc = call.pos.alloc(((size_t)n_pos + 1) * 4)) || (rc = call.pat.alloc(((size_t)n + 1) * 4)) ||
        (rc = call.range_off.alloc(((size_t)n + 1) * 8)) || (rc = call.counts.alloc((size_t)n * 4)) || (rc = call.status.alloc((size_t)n * 4)))
        return rc;
    const size_t ws_bytes = fmx::class_ranges_scratch_bytes(n);
    if ((rc = call.scratch.alloc(ws_bytes))) return rc;
    if (alts) CLASS_HIP_TRY(hipMemcpyAsync(call.alt.p, alt, alts * 2, hipMemcpyHostToDevice, st));
    CLASS_HIP_TRY(hipMemcpyAsync(call.pos.p, pos_off, ((size_t)n_pos + 1) * 4, hipMemcpyHostToDevice, st));
    CLASS_HIP_TRY(hipMemcpyAsync(call.pat.p, pat_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, st));
    rc = fmx_class_ranges_count_dev(idx, call.alt.as<uint16_t>(), call.pos.as<int32_t>(), call.pat.as<int32_t>(), n, max_ranges,
                                    call.range_off.as<int64_t>(), call.counts.as<int32_t>(), call.status.as<int32_t>(), call.scratch.p, ws_bytes, st);
    if (rc) return rc;
    if (!want_ranges) return FMX_OK;
    CLASS_HIP_TRY(hipMemcpyAsync(&call.m, call.range_off.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    CLASS_HIP_TRY(hipStreamSynchronize(st));
    if (call.m > INT32_MAX) return api_fail(FMX_E_ARG, "more than 2^31 - 1 ranges in one batch");
    if ((rc = call.ranges.alloc((size_t)call.m * 8))) return rc;
    return fmx_class_ranges_fill_dev(idx, call.alt.as<uint16_t>(), call.pos.as<int32_t>(), call.pat.as<int32_t>(), n, max_ranges,
                                     call.range_off.as<int64_t>(), call.ranges.as<int32_t>(), st);
}

// the packed hit layout of a searched batch: range_hit_off (m + 1), hit_off (n + 1), *total = hit_off[n]
int class_hit_layout(const fmx_index *idx, int32_t n, ClassCall &call, DevBlock &range_hit_off, DevBlock &hit_off, DevBlock &ws, int64_t *total,
                     hipStream_t st) {
    int rc;
    const size_t ws_bytes = fmx_class_hit_offsets_scratch_bytes(call.m);
    if ((rc = range_hit_off.alloc(((size_t)call.m + 1) * 8)) || (rc = hit_off.alloc(((size_t)n + 1) * 8)) || (rc = ws.alloc(ws_bytes))) return rc;
    rc = fmx_class_hit_offsets_dev(idx, n, call.range_off.as<int64_t>(), call.ranges.as<int32_t>(), call.m, range_hit_off.as<int64_t>(),
                                   hit_off.as<int64_t>(), ws.p, ws_bytes, st);
    if (rc) return rc;
    CLASS_HIP_TRY(hipMemcpyAsync(total, hit_off.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    CLASS_HIP_TRY(hipStreamSynchronize(st));
    return FMX_OK;
}

int check_class_queries(int32_t n, int32_t q, const int32_t *query_off, const uint8_t *term_kind) {
    if (query_off[0] != 0 || query_off[q] != n) return api_fail(FMX_E_ARG, "query offsets must run from 0 to the number of terms");
    for (int32_t i = 0; i < q; ++i)
        if (query_off[i + 1] < query_off[i]) return api_fail(FMX_E_ARG, "query offsets decrease");
    for (int32_t t = 0; t < n; ++t)
        if (term_kind[t] > FMX_TERM_NONE) return api_fail(FMX_E_ARG, "a term's kind is none of FMX_TERM_ALL, FMX_TERM_ANY, FMX_TERM_NONE");
    return FMX_OK;
}

constexpr int64_t kClassHitWindow = (int64_t)1 << 24;  // (fmx_locate_all_batch's: 64 MiB of positions)

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
        CLASS_HIP_TRY(hipMemsetAsync(d_range_off, 0, sizeof(int64_t), st));
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
        CLASS_HIP_TRY(hipMemsetAsync(d_hit_off, 0, sizeof(int64_t), st));
        CLASS_HIP_TRY(hipMemsetAsync(d_range_hit_off, 0, sizeof(int64_t), st));
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

// stage 1 alone: the counts and the statuses come down, no range is stored
int fmx_count_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n,
                          int32_t max_ranges, int32_t *counts, int32_t *status) {
    return guarded([&]() -> int {
    if (n > 0 && !counts) return api_fail(FMX_E_ARG, "bad arguments");
    ClassCall call;
    if (const int rc = class_args(idx, alt, pos_off, n_pos, pat_off, n, max_ranges, &call.view)) return rc;
    if (n == 0) return FMX_OK;
    CLASS_HIP_TRY(hipSetDevice(call.view.device));
    CallStream stream;
    if (const int rc_stream = stream.init(call.view.device)) return rc_stream;
    if (const int rc = class_search_host(idx, alt, pos_off, n_pos, pat_off, n, max_ranges, false, call, stream.s)) return rc;
    CLASS_HIP_TRY(hipMemcpyAsync(counts, call.counts.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream.s));
    if (status) CLASS_HIP_TRY(hipMemcpyAsync(status, call.status.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream.s));
    CLASS_HIP_TRY(hipStreamSynchronize(stream.s));
    return FMX_OK;
    });
}

// both stages, the hit layout, ONE 8-byte read of the hit total, the result malloc'ed to that size, then fmx_locate_all_fill_dev over
// the m ranges in windows of device scratch, each copied into its place (fmx_locate_all_batch's sequence)
int fmx_locate_all_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                               int32_t n, int32_t max_ranges, int64_t *hit_off, int32_t **locs, int32_t *status) {
    return guarded([&]() -> int {
    if (locs) *locs = nullptr;
    if (!hit_off || !locs) return api_fail(FMX_E_ARG, "bad arguments");
    ClassCall call;
    if (const int rc = class_args(idx, alt, pos_off, n_pos, pat_off, n, max_ranges, &call.view)) return rc;
    if (n == 0) {
        hit_off[0] = 0;
        return FMX_OK;
    }
    CLASS_HIP_TRY(hipSetDevice(call.view.device));
    DevBlock d_range_hit, d_hit, d_ws, d_win, d_range_status;
    HostResult result;
    CallStream stream;
    if (const int rc_stream = stream.init(call.view.device)) return rc_stream;
    const hipStream_t st = stream.s;
    int rc;
    if ((rc = class_search_host(idx, alt, pos_off, n_pos, pat_off, n, max_ranges, true, call, st))) return rc;
    int64_t total = 0;
    if ((rc = class_hit_layout(idx, n, call, d_range_hit, d_hit, d_ws, &total, st))) return rc;
    if (total > 0) {
        if ((uint64_t)total > SIZE_MAX / 4) return api_fail(FMX_E_NOMEM, "the batch's hits do not fit this host's address space");
        result.p = static_cast<int32_t *>(malloc((size_t)total * 4));
        if (!result.p) return api_fail(FMX_E_NOMEM, "out of host memory for " + std::to_string(total) + " hits");
        const int64_t window = total < kClassHitWindow ? total : kClassHitWindow;
        if ((rc = d_win.alloc((size_t)window * 4))) return rc;
        if (status) {
            if ((rc = d_range_status.alloc((size_t)call.m * 4))) return rc;
            CLASS_HIP_TRY(hipMemsetAsync(d_range_status.p, 0, (size_t)call.m * 4, st));
        }
        for (int64_t at = 0; at < total; at += window) {
            const int64_t hits = total - at < window ? total - at : window;
            rc = fmx_locate_all_fill_dev(idx, (int32_t)call.m, d_range_hit.as<int64_t>(), call.ranges.as<int32_t>(), at, hits, d_win.as<int32_t>(),
                                         nullptr, status ? d_range_status.as<int32_t>() : nullptr, st);
            if (rc) return rc;
            CLASS_HIP_TRY(hipMemcpyAsync(result.p + at, d_win.p, (size_t)hits * 4, hipMemcpyDeviceToHost, st));
        }
        if (status &&
            (rc = fmx_class_fold_status_dev(idx, n, call.range_off.as<int64_t>(), call.m, d_range_status.as<int32_t>(), call.status.as<int32_t>(), st)))
            return rc;
    }
    CLASS_HIP_TRY(hipMemcpyAsync(hit_off, d_hit.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (status) CLASS_HIP_TRY(hipMemcpyAsync(status, call.status.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    CLASS_HIP_TRY(hipStreamSynchronize(st));
    *locs = result.p;
    result.p = nullptr;
    return FMX_OK;
    });
}

// fmx_match_query_batch's sequence with the class search in place of the literal range search: both stages, the hit layout, the
// fill of every hit at once (the sort wants them all), fmx_query_lines_of_hits_dev, ONE 8-byte read of the line total
int fmx_match_query_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                int32_t n, int32_t max_ranges, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                int32_t max_lines, int64_t *line_off, int32_t **lines, int32_t *line_count, int32_t *occurrences,
                                int32_t *status) {
    return guarded([&]() -> int {
    if (lines) *lines = nullptr;
    if (q < 0 || !line_off || !lines || !query_off || (n > 0 && !term_kind)) return api_fail(FMX_E_ARG, "bad arguments");
    ClassCall call;
    int rc;
    if ((rc = class_args(idx, alt, pos_off, n_pos, pat_off, n, max_ranges, &call.view))) return rc;
    if ((rc = check_class_queries(n, q, query_off, term_kind))) return rc;
    int32_t boundary = -1;
    if ((rc = fmx_line_table_info(idx, &boundary, nullptr, nullptr))) return rc;
    if (boundary < 0) return api_fail(FMX_E_ARG, "the index has no line table (call fmx_line_table_build)");
    CLASS_HIP_TRY(hipSetDevice(call.view.device));
    DevBlock d_range_hit, d_hit, d_ws, d_locs, d_lines, d_loff, d_lcnt, d_qws, d_range_status;
    HostResult result;
    CallStream stream;
    if (const int rc_stream = stream.init(call.view.device)) return rc_stream;
    const hipStream_t st = stream.s;
    int64_t total = 0, n_out = 0;
    if (n > 0) {
        if ((rc = class_search_host(idx, alt, pos_off, n_pos, pat_off, n, max_ranges, true, call, st))) return rc;
        if ((rc = class_hit_layout(idx, n, call, d_range_hit, d_hit, d_ws, &total, st))) return rc;
        if (total > INT32_MAX) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one batch");
    }
    if ((rc = d_loff.alloc(((size_t)q + 1) * 8)) || (rc = d_lcnt.alloc((size_t)q * 4 + 4))) return rc;
    CLASS_HIP_TRY(hipMemsetAsync(d_loff.p, 0, ((size_t)q + 1) * 8, st));
    CLASS_HIP_TRY(hipMemsetAsync(d_lcnt.p, 0, (size_t)q * 4 + 4, st));
    // (a query set whose key does not fit is turned away by fmx_query_lines_of_hits_dev; a batch without hits asks it all the same)
    const size_t qws_bytes = fmx_query_lines_scratch_bytes(n, q, total);
    if ((rc = d_locs.alloc((size_t)total * 4)) || (rc = d_lines.alloc((size_t)total * 4)) || (rc = d_qws.alloc(qws_bytes))) return rc;
    if (total > 0) {
        if (status) {
            if ((rc = d_range_status.alloc((size_t)call.m * 4))) return rc;
            CLASS_HIP_TRY(hipMemsetAsync(d_range_status.p, 0, (size_t)call.m * 4, st));
        }
        rc = fmx_locate_all_fill_dev(idx, (int32_t)call.m, d_range_hit.as<int64_t>(), call.ranges.as<int32_t>(), 0, total, d_locs.as<int32_t>(), nullptr,
                                     status ? d_range_status.as<int32_t>() : nullptr, st);
        if (rc) return rc;
        if (status &&
            (rc = fmx_class_fold_status_dev(idx, n, call.range_off.as<int64_t>(), call.m, d_range_status.as<int32_t>(), call.status.as<int32_t>(), st)))
            return rc;
    }
    if (n > 0) {
        rc = fmx_query_lines_of_hits_dev(idx, n, q, query_off, term_kind, d_hit.as<int64_t>(), d_locs.as<int32_t>(), total, max_lines,
                                         d_loff.as<int64_t>(), d_lines.as<int32_t>(), d_lcnt.as<int32_t>(), d_qws.p, qws_bytes, st);
        if (rc) return rc;
    }
    CLASS_HIP_TRY(hipMemcpyAsync(&n_out, d_loff.as<int64_t>() + q, 8, hipMemcpyDeviceToHost, st));
    CLASS_HIP_TRY(hipStreamSynchronize(st));
    if (n_out > 0) {
        result.p = static_cast<int32_t *>(malloc((size_t)n_out * 4));
        if (!result.p) return api_fail(FMX_E_NOMEM, "out of host memory for " + std::to_string(n_out) + " lines");
        CLASS_HIP_TRY(hipMemcpyAsync(result.p, d_lines.p, (size_t)n_out * 4, hipMemcpyDeviceToHost, st));
    }
    CLASS_HIP_TRY(hipMemcpyAsync(line_off, d_loff.p, ((size_t)q + 1) * 8, hipMemcpyDeviceToHost, st));
    if (line_count && q > 0) CLASS_HIP_TRY(hipMemcpyAsync(line_count, d_lcnt.p, (size_t)q * 4, hipMemcpyDeviceToHost, st));
    if (occurrences && n > 0) CLASS_HIP_TRY(hipMemcpyAsync(occurrences, call.counts.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (status && n > 0) CLASS_HIP_TRY(hipMemcpyAsync(status, call.status.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    CLASS_HIP_TRY(hipStreamSynchronize(st));
    *lines = result.p;
    result.p = nullptr;
    return FMX_OK;
    });
}

}  // extern "C"
