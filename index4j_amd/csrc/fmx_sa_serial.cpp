// fmx_sa_serial.cpp — the stream form of index4j's SuffixArray (SA:172-199) and its hashCode (SA:202-204).  Host code only:
// the sanitizer build of the tests compiles it without the HIP runtime.
//
//   byte 0 | int UTF-8 byte length | the UTF-8 bytes of cs.toString() | int n + 1 | n + 1 ints     (all big-endian)
//
// Writing follows String.getBytes(UTF_8): a surrogate pair becomes one 4-byte sequence, an unpaired surrogate '?'.  Reading
// follows new String(bytes) under Java >= 18's UTF-8 default, except that malformed UTF-8 is refused (FMX_E_FORMAT) where
// Java would put U+FFFD in its place.
#include "../../include/fmx.h"
#include "fmx_sa_index.hpp"

namespace fmx {
namespace {

void put32(std::vector<uint8_t> &o, uint32_t v) {
    o.push_back((uint8_t)(v >> 24));
    o.push_back((uint8_t)(v >> 16));
    o.push_back((uint8_t)(v >> 8));
    o.push_back((uint8_t)v);
}
uint32_t get32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

}  // namespace

void utf16_to_utf8(const uint16_t *s, size_t n, std::vector<uint8_t> &out) {
    out.clear();
    out.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t c = s[i];
        if (c >= 0xD800 && c <= 0xDFFF) {
            if (c <= 0xDBFF && i + 1 < n && s[i + 1] >= 0xDC00 && s[i + 1] <= 0xDFFF) {
                c = 0x10000 + ((c - 0xD800) << 10) + (s[++i] - 0xDC00u);
            } else {
                out.push_back('?');
                continue;
            }
        }
        if (c < 0x80) {
            out.push_back((uint8_t)c);
        } else if (c < 0x800) {
            out.push_back((uint8_t)(0xC0 | (c >> 6)));
            out.push_back((uint8_t)(0x80 | (c & 0x3F)));
        } else if (c < 0x10000) {
            out.push_back((uint8_t)(0xE0 | (c >> 12)));
            out.push_back((uint8_t)(0x80 | ((c >> 6) & 0x3F)));
            out.push_back((uint8_t)(0x80 | (c & 0x3F)));
        } else {
            out.push_back((uint8_t)(0xF0 | (c >> 18)));
            out.push_back((uint8_t)(0x80 | ((c >> 12) & 0x3F)));
            out.push_back((uint8_t)(0x80 | ((c >> 6) & 0x3F)));
            out.push_back((uint8_t)(0x80 | (c & 0x3F)));
        }
    }
}

bool utf8_to_utf16(const uint8_t *b, size_t n, std::vector<uint16_t> &out) {
    out.clear();
    out.reserve(n);
    for (size_t i = 0; i < n;) {
        const uint32_t c0 = b[i];
        if (c0 < 0x80) {
            out.push_back((uint16_t)c0);
            ++i;
            continue;
        }
        int len;
        uint32_t c, min;
        if ((c0 & 0xE0) == 0xC0) {
            len = 2, c = c0 & 0x1F, min = 0x80;
        } else if ((c0 & 0xF0) == 0xE0) {
            len = 3, c = c0 & 0x0F, min = 0x800;
        } else if ((c0 & 0xF8) == 0xF0) {
            len = 4, c = c0 & 0x07, min = 0x10000;
        } else {
            return false;
        }
        if (n - i < (size_t)len) return false;
        for (int k = 1; k < len; ++k) {
            if ((b[i + k] & 0xC0) != 0x80) return false;
            c = (c << 6) | (b[i + k] & 0x3F);
        }
        if (c < min || c > 0x10FFFF || (c >= 0xD800 && c <= 0xDFFF)) return false;  // overlong, out of range, a surrogate
        if (c >= 0x10000) {
            out.push_back((uint16_t)(0xD800 + ((c - 0x10000) >> 10)));
            out.push_back((uint16_t)(0xDC00 + ((c - 0x10000) & 0x3FF)));
        } else {
            out.push_back((uint16_t)c);
        }
        i += (size_t)len;
    }
    return true;
}

void sa_emit(const SaIndex &s, bool framed, std::vector<uint8_t> &out) {
    std::vector<uint8_t> utf8, raw;
    utf16_to_utf8(s.text.data(), s.text.size(), utf8);
    raw.reserve(1 + 4 + utf8.size() + 4 + s.sa.size() * 4);
    raw.push_back(0);  // SERIAL_VERSION_V0
    put32(raw, (uint32_t)utf8.size());
    raw.insert(raw.end(), utf8.begin(), utf8.end());
    put32(raw, (uint32_t)s.sa.size());
    for (int32_t v : s.sa) put32(raw, (uint32_t)v);
    if (framed)
        frame_stream(raw, out);
    else
        out.swap(raw);
}

int sa_parse(const uint8_t *buf, size_t len, SaIndex &s, std::string &err) {
    std::vector<uint8_t> plain;
    bool corrupt_tail = false;
    if (unframe_stream(buf, len, plain, corrupt_tail)) {
        buf = plain.data();
        len = plain.size();
    }
    auto malformed = [&](const char *what) {
        err = std::string("suffix array stream: ") + what;
        return FMX_E_FORMAT;
    };
    if (len < 1) return malformed("truncated");
    if (buf[0] != 0) {  // SER:35-36
        err = "Incompatible serial versions! Expected version 0 but was " + std::to_string((int)(int8_t)buf[0]) + ".";
        return FMX_E_VERSION;
    }
    size_t pos = 1;
    if (len - pos < 4) return malformed("truncated");
    const int32_t n_bytes = (int32_t)get32(buf + pos);
    pos += 4;
    if (n_bytes < 0 || (size_t)n_bytes > len - pos) return malformed(n_bytes < 0 ? "negative text length" : "truncated");
    if (!utf8_to_utf16(buf + pos, (size_t)n_bytes, s.text)) return malformed("text is not well-formed UTF-8");
    pos += (size_t)n_bytes;
    if (len - pos < 4) return malformed("truncated");
    const int32_t rows = (int32_t)get32(buf + pos);
    pos += 4;
    const int64_t n = (int64_t)s.text.size();
    if ((int64_t)rows != n + 1) return malformed("the array does not have text length + 1 entries");
    if ((uint64_t)rows * 4 > len - pos) return malformed("truncated");
    s.sa.resize((size_t)rows);
    for (int32_t i = 0; i < rows; ++i, pos += 4) {
        const int32_t v = (int32_t)get32(buf + pos);
        if (v < 0 || v > n) return malformed("an entry lies outside [0, text length]");
        s.sa[(size_t)i] = v;
    }
    return FMX_OK;
}

int32_t sa_hash_code(const SaIndex &s) {
    uint32_t h = 0;  // String.hashCode
    for (uint16_t c : s.text) h = 31u * h + c;
    uint32_t a = 1;  // Arrays.hashCode(int[])
    for (int32_t v : s.sa) a = 31u * a + (uint32_t)v;
    return (int32_t)(h + a);
}

}  // namespace fmx
