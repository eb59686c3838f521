// fmx_sa_index.hpp — index4j's SuffixArray (suffixarray/SuffixArray.java, "SA") and the suffix-array core of its
// BurrowsWheelerTransform (encoding/BurrowsWheelerTransform.java, "BWT"): the host object behind an fmx_index handle
// made by fmx_sa_build / fmx_sa_load, its stream form, and the launchers of fmx_sa_query.hip.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include <memory>

#include "fmx_sa_device.hpp"

struct fmx_index;

namespace fmx {

struct SaIndex {
    std::vector<uint16_t> text;
    std::vector<int32_t> sa;  // n + 1 entries, sa[0] = n (SA:89-91)
    // resident form (fmx_to_device; a device build leaves the array where it was made)
    int device = -1;
    int n_cu = 256;
    uint16_t *d_text = nullptr;
    int32_t *d_sa = nullptr;
    void *d_fences = nullptr;  // [n_fences * K chars][n_fences lengths]
    int32_t n_fences = 0, fence_shift = 0, fence_chars = 0;
    // per-stream scratch of the query calls (grow-only, freed with the handle)
    std::mutex ws_mutex;
    std::map<void *, std::pair<void *, size_t>> ws;

    ~SaIndex() { release_device(); }
    int32_t length() const { return (int32_t)text.size(); }
    SaView view() const;
    const uint16_t *fence_keys() const { return static_cast<const uint16_t *>(d_fences); }
    void release_device();
};

// SA:89-91 / BWT:43-113: the suffix array of `codes` (L symbols below `alphabet`, 0 at L-1 only) — by prefix doubling in
// HBM (device >= 0; *d_sa_out, if given, receives the device copy, else it is freed) or by host SA-IS (device = -1).
// 0 or an FMX_E_* code.
int sa_sort(const std::vector<int32_t> &codes, int alphabet, int device, int32_t *sa, int32_t **d_sa_out,
            std::string &err);
// text -> 1 + rank(char) (order-keeping), with a unique 0 appended; returns the number of distinct chars
int sa_map_text(const uint16_t *text, int64_t n, std::vector<int32_t> &codes);

// fmx_serial.cpp: the ObjectOutputStream framing of SER:67-79 (unframe_stream: false = `buf` is a raw stream; corrupt_tail = the
// block data ended at a header that is no type code)
void frame_stream(const std::vector<uint8_t> &raw, std::vector<uint8_t> &out);
bool unframe_stream(const uint8_t *buf, size_t len, std::vector<uint8_t> &plain, bool &corrupt_tail);
// SA:172-199 (+ that framing)
void sa_emit(const SaIndex &s, bool framed, std::vector<uint8_t> &out);
// 0, or FMX_E_FORMAT / FMX_E_VERSION with `err` set; validates len(sa) == n + 1, every entry in [0, n], UTF-8
int sa_parse(const uint8_t *buf, size_t len, SaIndex &s, std::string &err);
// SA:202-204: String.hashCode(text) + Arrays.hashCode(sa), int32 arithmetic
int32_t sa_hash_code(const SaIndex &s);
// Java's String.getBytes(UTF_8) / new String(bytes, UTF_8) for well-formed input; decode returns false on malformed bytes
void utf16_to_utf8(const uint16_t *s, size_t n, std::vector<uint8_t> &out);
bool utf8_to_utf16(const uint8_t *b, size_t n, std::vector<uint16_t> &out);

// the resident form on `device` (the array is uploaded unless it already lies there; the fence table is made from the options)
int sa_to_device(SaIndex &s, int device, std::string &err);
// fmx_api.cpp: the handle of a SuffixArray, and the SuffixArray of a handle (nullptr: another kind of handle)
fmx_index *sa_handle(std::unique_ptr<SaIndex> sa);
SaIndex *sa_of(const fmx_index *idx);

// fmx_sa_query.hip
int sa_fence_settings(int32_t n, int32_t *n_fences, int32_t *shift, int32_t *chars);  // from the options; -1: too big for LDS
int launch_sa_fences(const SaView &v, uint16_t *keys, uint8_t *lens, void *stream);
// per pattern: counts[i] = right - left (nullable), left[i] and found[i] = min(count, max_matches) (both nullable)
int launch_sa_search(const SaView &v, const uint16_t *keys, int n_cu, const uint16_t *pat, const int32_t *pat_off,
                     int32_t n, int32_t max_matches, int32_t *counts, int32_t *left, int32_t *found, void *stream);
// locs[i * max_matches + k] = sa[left[i] + k] for k < found[i], flattened over an inclusive scan of found
size_t sa_locate_scratch_bytes(int32_t n);
int launch_sa_locate_copy(const SaView &v, int n_cu, const int32_t *left, const int32_t *found, int32_t n,
                          int32_t max_matches, int32_t *locs, void *scratch, size_t scratch_bytes, void *stream);
// BWT:100-108 from the suffix array of text' + unique terminator (L = n1 + 1 rows; row 0 is dropped)
int launch_bwt_gather(const int32_t *d_sa, const uint16_t *d_text1, int32_t n1, uint16_t *d_out, void *stream);

}  // namespace fmx
