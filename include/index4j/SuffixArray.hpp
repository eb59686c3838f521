// index4j/SuffixArray.hpp — host-side C++ mirror of com.dynatrace.suffixarray.SuffixArray and
// com.dynatrace.encoding.BurrowsWheelerTransform over the C ABI of libfmx.so (include/fmx.h).  Header-only; the
// error mapping of FmIndex.hpp.  count / locate run on the GPU (construct() leaves the array resident on `device`).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "FmIndex.hpp"

namespace index4j {

class SuffixArray {
public:
    // new SuffixArray(CharSequence) SA:47-49; buildDevice -1 = sort the suffixes on the host (default: on `device`)
    explicit SuffixArray(std::u16string input, int device = 0, int buildDevice = -2)
        : text_(std::move(input)), device_(device), build_(buildDevice == -2 ? device : buildDevice) {}
    SuffixArray(const SuffixArray &) = delete;
    SuffixArray &operator=(const SuffixArray &) = delete;
    ~SuffixArray() {
        if (h_) fmx_free(h_);
    }

    void construct() {  // SA:89-91
        if (h_) fmx_free(h_);
        h_ = nullptr;
        detail::check(fmx_sa_build(reinterpret_cast<const uint16_t *>(text_.data()), (int32_t)text_.size(), build_, &h_),
                      "fmx_sa_build");
        if (device_ >= 0 && fmx_device_of(h_) != device_) detail::check(fmx_to_device(h_, device_), "fmx_to_device");
    }

    int count(const std::u16string &pattern) const {  // SA:100-104
        const int32_t off[2] = {0, (int32_t)pattern.size()};
        int32_t c = 0;
        detail::check(fmx_sa_count_batch(handle(), reinterpret_cast<const uint16_t *>(pattern.data()), off, 1, &c),
                      "fmx_sa_count_batch");
        return c;
    }

    int locate(const std::u16string &pattern, std::vector<int32_t> &offsets) const {  // SA:116-129
        const int32_t off[2] = {0, (int32_t)pattern.size()};
        int32_t found = 0;
        detail::check(fmx_sa_locate_batch(handle(), reinterpret_cast<const uint16_t *>(pattern.data()), off, 1,
                                          (int32_t)offsets.size(), offsets.data(), &found, nullptr),
                      "fmx_sa_locate_batch");
        return found;
    }

    std::vector<int32_t> getSuffixArray() const {  // SA:164-166
        std::vector<int32_t> out((size_t)fmx_sa_get(handle(), nullptr, 0));
        fmx_sa_get(handle(), out.data(), (int64_t)out.size());
        return out;
    }

    std::vector<uint8_t> write(bool framed = true) const {  // SA:172-184
        uint8_t *buf = nullptr;
        size_t len = 0;
        detail::check(fmx_sa_save(handle(), framed ? 1 : 0, &buf, &len), "fmx_sa_save");
        std::vector<uint8_t> out(buf, buf + len);
        fmx_free_buffer(buf);
        return out;
    }

    static SuffixArray read(const std::vector<uint8_t> &bytes, int device = 0) {  // SA:186-199
        SuffixArray s(std::u16string(), device, -1);
        detail::check(fmx_sa_load(bytes.data(), bytes.size(), &s.h_), "fmx_sa_load");
        if (device >= 0) detail::check(fmx_to_device(s.h_, device), "fmx_to_device");
        return s;
    }

    int hashCode() const {  // SA:202-204
        int32_t h = 0;
        detail::check(fmx_sa_hash_code(handle(), &h), "fmx_sa_hash_code");
        return h;
    }

    SuffixArray(SuffixArray &&o) noexcept : text_(std::move(o.text_)), device_(o.device_), build_(o.build_), h_(o.h_) {
        o.h_ = nullptr;
    }

private:
    fmx_index *handle() const {
        if (!h_) throw std::runtime_error("SuffixArray: call construct() first");
        return h_;
    }
    std::u16string text_;
    int device_, build_;
    fmx_index *h_ = nullptr;
};

struct BurrowsWheelerTransform {
    // BWT:43-113 (buildDevice -1: on the host)
    static std::u16string createBurrowsWheelerTransform(const std::u16string &text, int buildDevice = 0) {
        std::u16string out(text.size() + 1, u'\0');
        const int rc = fmx_bwt(reinterpret_cast<const uint16_t *>(text.data()), (int32_t)text.size(), buildDevice,
                               reinterpret_cast<uint16_t *>(&out[0]));
        if (rc == FMX_E_ALPHABET) throw std::invalid_argument("Charset has more than 32767 different characters.");
        detail::check(rc, "fmx_bwt");
        return out;
    }
    // BWT:116-135
    template <class C>
    static double computeRedundancyOfText(const std::basic_string<C> &input) {
        if (input.empty()) throw std::out_of_range("Index 0 out of bounds for length 0");
        int r = 1;
        for (size_t i = 1; i < input.size(); ++i) r += input[i] != input[i - 1];
        return (double)input.size() / (double)r;
    }
};

}  // namespace index4j
