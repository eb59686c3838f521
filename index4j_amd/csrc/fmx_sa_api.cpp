// fmx_sa_api.cpp — the C ABI of index4j's SuffixArray (suffixarray/SuffixArray.java, "SA") and BurrowsWheelerTransform
// (encoding/BurrowsWheelerTransform.java, "BWT"): construction on the device or the host, the resident form, and the batch
// entry points that launch the kernels of fmx_sa_query.hip.
//
// Construction (SA:89-91): the reference calls jsuffixarrays' SuffixArrays.create (QSufSort), whose array has n + 1 entries,
// the empty suffix n first.  That is the suffix array of text -> 1 + rank(char) with a unique 0 appended, which is unique:
// the device's prefix doubling (fmx_sa_gpu.hip) and the host's SA-IS (fmx_sais.hpp) both give it.
#include "fmx_abi.hpp"
#include "fmx_build_stage.hpp"
#include "fmx_sa_index.hpp"
#include "fmx_sais.hpp"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>

namespace fmx {
namespace {

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
};

int stage_code(int rc) { return rc == -5 ? FMX_E_NO_DEVICE : rc == -1 ? FMX_E_ARG : FMX_E_HIP; }

size_t fence_key_bytes(int32_t n_fences, int32_t chars) { return ((size_t)n_fences * chars * 2 + 15) / 16 * 16; }

// the resident SuffixArray of a handle (FMX_E_ARG: another kind of handle; FMX_E_NO_DEVICE: not resident)
int resident(const fmx_index *idx, SaIndex **out) {
    SaIndex *s = sa_of(idx);
    if (!s) return api_fail(FMX_E_ARG, "not a SuffixArray handle");
    if (!s->d_sa) return api_fail(FMX_E_NO_DEVICE, "suffix array is not resident on a HIP device (call fmx_to_device)");
    *out = s;
    return FMX_OK;
}

// per-stream scratch of the device-pointer entry points (grow-only)
int workspace(SaIndex &s, void *stream, size_t bytes, void **out) {
    std::lock_guard<std::mutex> lock(s.ws_mutex);
    auto &slot = s.ws[stream];
    if (slot.second < bytes) {
        if (slot.first) {
            FMX_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
            (void)hipFree(slot.first);
            slot = {nullptr, 0};
        }
        FMX_HIP_TRY(hipMalloc(&slot.first, bytes));
        slot.second = bytes;
    }
    *out = slot.first;
    return FMX_OK;
}

// SA:100-129 over one batch whose operands lie in HBM: counts and / or the locate rows (max_matches < 0: count only)
int query_dev(SaIndex &s, const uint16_t *d_pat, const int32_t *d_pat_off, int32_t n, int32_t max_matches, int32_t *d_locs,
              int32_t *d_found, int32_t *d_counts, void *d_scratch, size_t scratch_bytes, void *stream) {
    const SaView v = s.view();
    const bool locate = max_matches >= 0;
    int32_t *d_left = locate ? static_cast<int32_t *>(d_scratch) : nullptr;
    int e = launch_sa_search(v, s.fence_keys(), s.n_cu, d_pat, d_pat_off, n, locate ? max_matches : 0, d_counts, d_left,
                             locate ? d_found : nullptr, stream);
    if (e) return api_fail(FMX_E_HIP, std::string("k_sa_search launch: ") + hipGetErrorString((hipError_t)e));
    if (locate && max_matches > 0) {
        const size_t left_bytes = ((size_t)n * 4 + 255) / 256 * 256;
        e = launch_sa_locate_copy(v, s.n_cu, d_left, d_found, n, max_matches, d_locs,
                                  static_cast<uint8_t *>(d_scratch) + left_bytes, scratch_bytes - left_bytes, stream);
        if (e) return api_fail(FMX_E_HIP, std::string("k_sa_locate_copy launch: ") + hipGetErrorString((hipError_t)e));
    }
    return FMX_OK;
}

size_t query_scratch_bytes(int32_t n, int32_t max_matches) {
    if (max_matches < 0) return 0;
    return ((size_t)n * 4 + 255) / 256 * 256 + sa_locate_scratch_bytes(n);
}

int check_batch(int32_t n, int32_t max_matches, bool operands) {
    if (n < 0 || !operands) return api_fail(FMX_E_ARG, "bad arguments");
    if (max_matches > 0 && (int64_t)n * max_matches >= ((int64_t)1 << 31))
        return api_fail(FMX_E_ARG, "n * max_matches must stay below 2^31");
    return FMX_OK;
}

// the host-buffer form: operands staged through per-call device buffers, on the null stream
int query_host(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, int32_t max_matches,
               int32_t *locs, int32_t *found, int32_t *counts) {
    SaIndex *s = nullptr;
    int rc = resident(idx, &s);
    if (rc) return rc;
    const bool locate = max_matches >= 0;
    rc = check_batch(n, max_matches, n == 0 || (pat_off && (counts || (locate && found && (locs || max_matches == 0)))));
    if (rc) return rc;
    if (n == 0) return FMX_OK;
    if (pat_off[0] < 0) return api_fail(FMX_E_ARG, "pattern offsets must start at >= 0 and never decrease");
    for (int32_t i = 0; i < n; ++i)
        if (pat_off[i + 1] < pat_off[i]) return api_fail(FMX_E_ARG, "pattern offsets must start at >= 0 and never decrease");
    const size_t chars = (size_t)pat_off[n];
    if (chars && !pat) return api_fail(FMX_E_ARG, "bad arguments");
    FMX_HIP_TRY(hipSetDevice(s->device));
    const size_t n_locs = locate ? (size_t)n * (size_t)max_matches : 0;
    DevBuf d_pat, d_off, d_counts, d_found, d_locs, d_scratch;
    FMX_HIP_TRY(d_pat.alloc(chars * 2));
    FMX_HIP_TRY(d_off.alloc(((size_t)n + 1) * 4));
    if (counts) FMX_HIP_TRY(d_counts.alloc((size_t)n * 4));
    if (locate) {
        FMX_HIP_TRY(d_found.alloc((size_t)n * 4));
        FMX_HIP_TRY(d_locs.alloc(n_locs * 4));
        FMX_HIP_TRY(d_scratch.alloc(query_scratch_bytes(n, max_matches)));
        if (n_locs) FMX_HIP_TRY(hipMemcpy(d_locs.p, locs, n_locs * 4, hipMemcpyHostToDevice));  // slots past `found` keep their values
    }
    if (chars) FMX_HIP_TRY(hipMemcpy(d_pat.p, pat, chars * 2, hipMemcpyHostToDevice));
    FMX_HIP_TRY(hipMemcpy(d_off.p, pat_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice));
    rc = query_dev(*s, d_pat.as<uint16_t>(), d_off.as<int32_t>(), n, max_matches, d_locs.as<int32_t>(), d_found.as<int32_t>(),
                   d_counts.as<int32_t>(), d_scratch.p, query_scratch_bytes(n, max_matches), nullptr);
    if (rc) return rc;
    FMX_HIP_TRY(hipDeviceSynchronize());
    if (counts) FMX_HIP_TRY(hipMemcpy(counts, d_counts.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (locate) {
        FMX_HIP_TRY(hipMemcpy(found, d_found.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (n_locs) FMX_HIP_TRY(hipMemcpy(locs, d_locs.p, n_locs * 4, hipMemcpyDeviceToHost));
    }
    return FMX_OK;
}

}  // namespace

SaView SaIndex::view() const {
    SaView v;
    v.text = d_text;
    v.sa = d_sa;
    v.n = length();
    v.fence_len = d_fences ? static_cast<const uint8_t *>(d_fences) + fence_key_bytes(n_fences, fence_chars) : nullptr;
    v.n_fences = d_fences ? n_fences : 0;
    v.fence_shift = fence_shift;
    v.fence_chars = fence_chars;
    return v;
}

void SaIndex::release_device() {
    if (device >= 0) (void)hipSetDevice(device);
    for (auto &kv : ws)
        if (kv.second.first) (void)hipFree(kv.second.first);
    ws.clear();
    for (void *p : {(void *)d_text, (void *)d_sa, d_fences})
        if (p) (void)hipFree(p);
    d_text = nullptr;
    d_sa = nullptr;
    d_fences = nullptr;
    n_fences = 0;
    device = -1;
}

int sa_map_text(const uint16_t *text, int64_t n, std::vector<int32_t> &codes) {
    std::vector<int32_t> code(65536, 0);
    for (int64_t i = 0; i < n; ++i) code[text[i]] = 1;
    int32_t sigma = 0;
    for (int c = 0; c < 65536; ++c)
        if (code[(size_t)c]) code[(size_t)c] = ++sigma;
    codes.resize((size_t)n + 1);
    for (int64_t i = 0; i < n; ++i) codes[(size_t)i] = code[text[i]];
    codes[(size_t)n] = 0;
    return sigma;
}

int sa_sort(const std::vector<int32_t> &codes, int alphabet, int device, int32_t *sa, int32_t **d_sa_out, std::string &err) {
    const int32_t L = (int32_t)codes.size();
    if (d_sa_out) *d_sa_out = nullptr;
    // the device stage takes 16-bit codes: a text with all 65,536 char values (and the terminator) is sorted on the host
    if (device >= 0 && alphabet <= 65536) {
        if (!device_suffix_array) {
            err = "library built without the device stage";
            return FMX_E_UNSUPPORTED;
        }
        std::vector<int16_t> seq((size_t)L);
        for (int32_t i = 0; i < L; ++i) seq[(size_t)i] = (int16_t)(uint16_t)codes[(size_t)i];
        uint32_t *d = nullptr;
        const int rc = device_suffix_array(seq.data(), L, alphabet, device, &d, nullptr, err);
        if (rc) return stage_code(rc);
        hipError_t e = hipSuccess;
        if (sa) e = hipMemcpy(sa, d, (size_t)L * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            err = std::string("hipMemcpy of the suffix array: ") + hipGetErrorString(e);
            device_release(d);
            return FMX_E_HIP;
        }
        if (d_sa_out)
            *d_sa_out = reinterpret_cast<int32_t *>(d);
        else
            device_release(d);
        return FMX_OK;
    }
    sais_detail::sais<int32_t>(codes.data(), sa, L, alphabet);
    return FMX_OK;
}

int sa_to_device(SaIndex &s, int device, std::string &err) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        err = "no HIP device visible";
        return FMX_E_NO_DEVICE;
    }
    if (device < 0 || device >= n_dev) {
        err = "device ordinal out of range";
        return FMX_E_ARG;
    }
    int32_t n_fences, shift, chars;
    if (sa_fence_settings(s.length(), &n_fences, &shift, &chars)) {
        err = "fence table (sa_fences x sa_fence_chars x 2 bytes) larger than 64 KiB";
        return FMX_E_ARG;
    }
    if (s.device >= 0 && s.device != device) {
        (void)hipSetDevice(s.device);
        (void)hipDeviceSynchronize();
        s.release_device();
    }
    auto hip = [&](hipError_t e, const char *what) {
        if (e == hipSuccess) return false;
        (void)hipGetLastError();
        err = std::string(what) + ": " + hipGetErrorString(e);
        return true;
    };
    if (hip(hipSetDevice(device), "hipSetDevice")) return FMX_E_HIP;
    s.device = device;
    hipDeviceProp_t prop;
    if (hip(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties")) return FMX_E_HIP;
    s.n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const size_t n = (size_t)s.length();
    if (!s.d_sa) {
        if (hip(hipMalloc((void **)&s.d_sa, (n + 1) * 4), "hipMalloc") ||
            hip(hipMemcpy(s.d_sa, s.sa.data(), (n + 1) * 4, hipMemcpyHostToDevice), "hipMemcpy")) {
            s.release_device();
            return FMX_E_HIP;
        }
    }
    if (!s.d_text) {
        if (hip(hipMalloc((void **)&s.d_text, n ? n * 2 : 2), "hipMalloc") ||
            (n && hip(hipMemcpy(s.d_text, s.text.data(), n * 2, hipMemcpyHostToDevice), "hipMemcpy"))) {
            s.release_device();
            return FMX_E_HIP;
        }
    }
    if (!s.d_fences || s.n_fences != n_fences || s.fence_shift != shift || s.fence_chars != chars) {
        if (s.d_fences) (void)hipFree(s.d_fences);
        s.d_fences = nullptr;
        s.n_fences = n_fences;
        s.fence_shift = shift;
        s.fence_chars = chars;
        if (n_fences > 0) {
            const size_t key_bytes = fence_key_bytes(n_fences, chars);
            if (hip(hipMalloc(&s.d_fences, key_bytes + (size_t)n_fences), "hipMalloc")) {
                s.release_device();
                return FMX_E_HIP;
            }
            const SaView v = s.view();
            const int e = launch_sa_fences(v, static_cast<uint16_t *>(s.d_fences), const_cast<uint8_t *>(v.fence_len), nullptr);
            if (hip((hipError_t)e, "k_sa_fences") || hip(hipDeviceSynchronize(), "k_sa_fences")) {
                s.release_device();
                return FMX_E_HIP;
            }
        }
    }
    return FMX_OK;
}

}  // namespace fmx

using fmx::api_fail;
using fmx::guarded;

extern "C" {

int fmx_sa_build(const uint16_t *text, int32_t n, int build_device, fmx_index **out) {
    return guarded([&]() -> int {
        if (!out || n < 0 || n > INT32_MAX - 1 || (n > 0 && !text) || build_device < -1)
            return api_fail(FMX_E_ARG, "bad arguments");
        std::unique_ptr<fmx::SaIndex> s(new fmx::SaIndex());
        s->text.assign(text, text + n);
        s->sa.assign((size_t)n + 1, 0);
        s->sa[0] = n;
        std::string err;
        if (n > 0) {
            std::vector<int32_t> codes;
            const int sigma = fmx::sa_map_text(text, n, codes);
            int32_t *d_sa = nullptr;
            const int rc = fmx::sa_sort(codes, sigma + 1, build_device, s->sa.data(), build_device >= 0 ? &d_sa : nullptr, err);
            if (rc) return api_fail(rc, err);
            if (d_sa) {  // the array stays where it was made
                s->d_sa = d_sa;
                s->device = build_device;
            }
        }
        if (build_device >= 0) {
            const int rc = fmx::sa_to_device(*s, build_device, err);
            if (rc) return api_fail(rc, err);
        }
        *out = fmx::sa_handle(std::move(s));
        return FMX_OK;
    });
}

int fmx_sa_load(const uint8_t *ser, size_t len, fmx_index **out) {
    return guarded([&]() -> int {
        if (!out || (!ser && len)) return api_fail(FMX_E_ARG, "null argument");
        std::unique_ptr<fmx::SaIndex> s(new fmx::SaIndex());
        std::string err;
        const int rc = fmx::sa_parse(ser, len, *s, err);
        if (rc) return api_fail(rc, err);
        *out = fmx::sa_handle(std::move(s));
        return FMX_OK;
    });
}

int fmx_sa_save(const fmx_index *idx, int framed, uint8_t **buf, size_t *len) {
    return guarded([&]() -> int {
        const fmx::SaIndex *s = fmx::sa_of(idx);
        if (!s || !buf || !len) return api_fail(FMX_E_ARG, "not a SuffixArray handle");
        std::vector<uint8_t> bytes;
        fmx::sa_emit(*s, framed != 0, bytes);
        uint8_t *p = static_cast<uint8_t *>(malloc(bytes.size() ? bytes.size() : 1));
        if (!p) return api_fail(FMX_E_NOMEM, "out of memory");
        memcpy(p, bytes.data(), bytes.size());
        *buf = p;
        *len = bytes.size();
        return FMX_OK;
    });
}

int64_t fmx_sa_get(const fmx_index *idx, int32_t *sa, int64_t cap) {
    const fmx::SaIndex *s = fmx::sa_of(idx);
    if (!s || cap < 0 || (cap > 0 && !sa)) return api_fail(FMX_E_ARG, "bad arguments");
    const int64_t rows = (int64_t)s->sa.size();
    memcpy(sa, s->sa.data(), (size_t)(cap < rows ? cap : rows) * 4);
    return rows;
}

int fmx_sa_hash_code(const fmx_index *idx, int32_t *hash) {
    const fmx::SaIndex *s = fmx::sa_of(idx);
    if (!s || !hash) return api_fail(FMX_E_ARG, "bad arguments");
    *hash = fmx::sa_hash_code(*s);
    return FMX_OK;
}

int fmx_sa_count_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, int32_t *counts) {
    return guarded([&]() -> int { return fmx::query_host(idx, pat, pat_off, n, -1, nullptr, nullptr, counts); });
}

int fmx_sa_locate_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, int32_t max_matches,
                        int32_t *locs, int32_t *found, int32_t *counts) {
    return guarded([&]() -> int {
        if (max_matches < 0) return api_fail(FMX_E_ARG, "max_matches < 0");
        return fmx::query_host(idx, pat, pat_off, n, max_matches, locs, found, counts);
    });
}

int fmx_sa_count_batch_dev(const fmx_index *idx, const uint16_t *d_pat, const int32_t *d_pat_off, int32_t n, int32_t *d_counts,
                           void *stream) {
    return guarded([&]() -> int {
        fmx::SaIndex *s = nullptr;
        int rc = fmx::resident(idx, &s);
        if (rc) return rc;
        rc = fmx::check_batch(n, -1, n == 0 || (d_pat_off && d_counts));
        if (rc || n == 0) return rc;
        FMX_HIP_TRY(hipSetDevice(s->device));
        return fmx::query_dev(*s, d_pat, d_pat_off, n, -1, nullptr, nullptr, d_counts, nullptr, 0, stream);
    });
}

int fmx_sa_locate_batch_dev(const fmx_index *idx, const uint16_t *d_pat, const int32_t *d_pat_off, int32_t n,
                            int32_t max_matches, int32_t *d_locs, int32_t *d_found, int32_t *d_counts, void *stream) {
    return guarded([&]() -> int {
        fmx::SaIndex *s = nullptr;
        int rc = fmx::resident(idx, &s);
        if (rc) return rc;
        if (max_matches < 0) return api_fail(FMX_E_ARG, "max_matches < 0");
        rc = fmx::check_batch(n, max_matches, n == 0 || (d_pat_off && d_found && (d_locs || max_matches == 0)));
        if (rc || n == 0) return rc;
        FMX_HIP_TRY(hipSetDevice(s->device));
        const size_t bytes = fmx::query_scratch_bytes(n, max_matches);
        void *scratch = nullptr;
        rc = fmx::workspace(*s, stream, bytes, &scratch);
        if (rc) return rc;
        return fmx::query_dev(*s, d_pat, d_pat_off, n, max_matches, d_locs, d_found, d_counts, scratch, bytes, stream);
    });
}

int fmx_bwt(const uint16_t *text, int32_t n, int build_device, uint16_t *bwt) {
    return guarded([&]() -> int {
        if (!bwt || n < 0 || n > INT32_MAX - 2 || (n > 0 && !text) || build_device < -1)
            return api_fail(FMX_E_ARG, "bad arguments");
        std::vector<uint16_t> text1(text, text + n);  // BWT:45-47: text + '\0'
        text1.push_back(0);
        const int32_t n1 = n + 1;
        std::vector<int32_t> codes;
        const int sigma = fmx::sa_map_text(text1.data(), n1, codes);
        if (sigma > 32767) return api_fail(FMX_E_ALPHABET, "Charset has more than 32767 different characters.");  // BWT:64-67
        std::string err;
        if (build_device >= 0) {  // the array stays in HBM; one gather makes the transform there
            int32_t *d_sa = nullptr;
            int rc = fmx::sa_sort(codes, sigma + 1, build_device, nullptr, &d_sa, err);
            if (rc) return api_fail(rc, err);
            fmx::DevBuf owner, d_text1, d_out;
            owner.p = d_sa;
            FMX_HIP_TRY(d_text1.alloc((size_t)n1 * 2));
            FMX_HIP_TRY(d_out.alloc((size_t)n1 * 2));
            FMX_HIP_TRY(hipMemcpy(d_text1.p, text1.data(), (size_t)n1 * 2, hipMemcpyHostToDevice));
            const int e = fmx::launch_bwt_gather(d_sa, d_text1.as<uint16_t>(), n1, d_out.as<uint16_t>(), nullptr);
            if (e) return api_fail(FMX_E_HIP, std::string("k_bwt_gather launch: ") + hipGetErrorString((hipError_t)e));
            FMX_HIP_TRY(hipMemcpy(bwt, d_out.p, (size_t)n1 * 2, hipMemcpyDeviceToHost));
            return FMX_OK;
        }
        std::vector<int32_t> sa((size_t)n1 + 1);
        const int rc = fmx::sa_sort(codes, sigma + 1, -1, sa.data(), nullptr, err);
        if (rc) return api_fail(rc, err);
        for (int32_t i = 0; i < n1; ++i) {  // BWT:100-108, the terminator's row dropped
            const int32_t p = sa[(size_t)i + 1];
            bwt[i] = p == 0 ? (uint16_t)0 : text1[(size_t)p - 1];
        }
        return FMX_OK;
    });
}

}  // extern "C"
