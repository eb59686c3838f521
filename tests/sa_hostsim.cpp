// sa_hostsim.cpp — TEST-ONLY host build of the SuffixArray search routines (index4j_amd/csrc/fmx_sa_device.hpp).
//
// g++ compiles the header's FMX_HD functions as plain C++, so that the CPU suite checks the very source the kernels of
// fmx_sa_query.hip run against a restatement of SA:100-157 (tests/test_suffix_array_cpu.py).  The fence table is made here
// exactly as k_sa_fences makes it.  Built with -DSA_FUZZ_MAIN it is the sanitizer campaign over damaged streams instead:
// whatever the product's loader (fmx_sa_serial.cpp) accepts is searched, under AddressSanitizer.  Never part of libfmx.so.
#include "../index4j_amd/csrc/fmx_sa_device.hpp"

#include <cstddef>
#include <cstdint>
#include <vector>

using namespace fmx;

namespace {

// k_sa_fences on the host: n_fences, shift and K as sa_fence_settings derives them from (most, chars)
void make_fences(const uint16_t *text, int32_t n, const int32_t *sa, int32_t most, int32_t chars, std::vector<uint16_t> &keys,
                 std::vector<uint8_t> &lens, SaView &v) {
    int32_t s = 0;
    while (most > 0 && (((int64_t)n + (1ll << s) - 1) >> s) > most) ++s;
    const int32_t nf = most > 0 ? (int32_t)(((int64_t)n + (1ll << s) - 1) >> s) : 0;
    keys.assign((size_t)nf * chars + 1, 0);
    lens.assign((size_t)nf + 1, 0);
    for (int32_t j = 0; j < nf; ++j) {
        const int32_t pos = sa[(int64_t)j << s];
        const int32_t len = sa_min(chars, n - pos);
        for (int32_t u = 0; u < chars; ++u) keys[(size_t)j * chars + u] = u < len ? text[pos + u] : 0;
        lens[(size_t)j] = (uint8_t)len;
    }
    v.text = text;
    v.sa = sa;
    v.n = n;
    v.fence_len = lens.data();
    v.n_fences = nf;
    v.fence_shift = s;
    v.fence_chars = chars;
}

}  // namespace

extern "C" {

// left / right of every pattern, searched as k_sa_search does with a fence table of at most `most` fences of `chars` chars
// (most = 0: none); returns the number of fences
int32_t sim_sa_search(const uint16_t *text, int32_t n, const int32_t *sa, int32_t most, int32_t chars, const uint16_t *pat,
                      const int32_t *pat_off, int32_t n_pat, int32_t *left, int32_t *right) {
    std::vector<uint16_t> keys;
    std::vector<uint8_t> lens;
    SaView v;
    make_fences(text, n, sa, most, chars, keys, lens, v);
    for (int32_t i = 0; i < n_pat; ++i) {
        const SaRange r = sa_search(v, keys.data(), pat + pat_off[i], pat_off[i + 1] - pat_off[i]);
        left[i] = r.left;
        right[i] = r.right;
    }
    return v.n_fences;
}

}  // extern "C"

#ifdef SA_FUZZ_MAIN
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../index4j_amd/csrc/fmx_sa_index.hpp"
#include "../index4j_amd/csrc/fmx_sais.hpp"

void fmx::SaIndex::release_device() {}  // (nothing is resident in this build)

// argv: iterations, seed
int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 2000;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    int accepted = 0, refused = 0;
    for (int it = 0; it < iters; ++it) {
        // a valid stream of a small random text (some surrogates, some '\0'), then damage
        const int32_t n = (int32_t)(rng() % 200);
        fmx::SaIndex s;
        s.text.resize((size_t)n);
        for (auto &c : s.text) {
            const uint64_t r = rng() % 16;
            c = r == 0 ? 0 : r == 1 ? (uint16_t)(0xD800 + rng() % 0x800) : (uint16_t)('a' + rng() % 4);
        }
        std::vector<int32_t> codes;
        std::vector<int32_t> code(65536, 0);
        for (uint16_t c : s.text) code[c] = 1;
        int32_t sigma = 0;
        for (auto &c : code)
            if (c) c = ++sigma;
        for (uint16_t c : s.text) codes.push_back(code[c]);
        codes.push_back(0);
        s.sa.resize((size_t)n + 1);
        fmx::sais_detail::sais<int32_t>(codes.data(), s.sa.data(), n + 1, sigma + 1);
        std::vector<uint8_t> bytes;
        fmx::sa_emit(s, rng() & 1, bytes);
        const int kind = (int)(rng() % 5);
        const size_t tail = bytes.size() - (size_t)(n + 1) * 4;  // where the entries start (raw streams; framed: near it)
        if (kind == 4 && n > 0) {  // entries that stay in [0, n]: an array the loader accepts but no suffix array
            for (int f = 0; f < 3; ++f) {
                const size_t at = tail + 4 * (rng() % (size_t)(n + 1));
                const uint32_t v = (uint32_t)(rng() % (uint64_t)(n + 1));
                if (at + 4 > bytes.size()) continue;
                for (int b = 0; b < 4; ++b) bytes[at + b] = (uint8_t)(v >> (24 - 8 * b));
            }
        } else if (kind == 0 && !bytes.empty()) {
            bytes.resize(rng() % bytes.size());
        } else {
            const int flips = 1 + (int)(rng() % 4);
            for (int f = 0; f < flips && !bytes.empty(); ++f) {
                size_t at = rng() % bytes.size();
                if (kind == 3 && bytes.size() > 8) at = bytes.size() - 1 - rng() % (bytes.size() / 2);  // the array's entries
                bytes[at] = (uint8_t)(kind == 2 ? bytes[at] ^ (1u << (rng() % 8)) : rng());
            }
        }
        fmx::SaIndex t;
        std::string err;
        if (fmx::sa_parse(bytes.data(), bytes.size(), t, err)) {
            ++refused;
            continue;
        }
        ++accepted;
        // the loaded array may be any entries in [0, n]: the searches must stay inside text and array
        std::vector<uint16_t> pat;
        std::vector<int32_t> off{0};
        for (int p = 0; p < 24; ++p) {
            const int len = (int)(rng() % 12);
            for (int k = 0; k < len; ++k) pat.push_back((uint16_t)(rng() % 3 == 0 ? 0 : 'a' + rng() % 4));
            off.push_back((int32_t)pat.size());
        }
        pat.push_back(0);
        const int32_t m = (int32_t)t.text.size();
        std::vector<int32_t> left(off.size()), right(off.size());
        for (int32_t most : {0, 4, 64})
            sim_sa_search(t.text.data(), m, t.sa.data(), most, 1 + (int32_t)(rng() % 8), pat.data(), off.data(),
                          (int32_t)off.size() - 1, left.data(), right.data());
    }
    printf("sa fuzz ok: %d accepted, %d refused\n", accepted, refused);
    return 0;
}
#endif
