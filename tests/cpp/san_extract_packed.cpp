// san_extract_packed.cpp — sanitizer driver of "extract, packed": tests/extract_packed_hostsim.cpp (the device header's piece
// geometry, seek, piece walk, redo list and the mirrors of the three kernels of fmx_extract_packed.hip) as a stand-alone program
// for -fsanitize=address,undefined.  Every array has exactly the size the contract gives it, so a store outside a range's slice,
// the redo list or the flags is a report.  Two texts — a synthetic log (no quirk rows: nothing is redone) and runs of wide symbols
// (quirk Q1: ranges ARE redone) — at sample rates 1, 5, 32 and 64, over the tree and the three directory forms; the answer must
// equal the literal fm_extract of every range (sim_extract).  Prints one " ok: " line per index; exit code 0 = clean.
#include "../extract_packed_hostsim.cpp"

#include <cstdio>
#include <string>

#include "fmx_model.hpp"

extern "C" int fmx_synth_log(uint64_t seed, int32_t n, uint16_t *out);

namespace {

uint64_t g_rng = 88172645463325252ull;
uint32_t below(uint32_t n) {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng % n);
}

// random wide symbols, a long run of one wide symbol, short lines — three times (the shape of the suite's run-block text)
std::vector<uint16_t> run_block_text() {
    std::vector<uint16_t> t;
    for (int part = 0; part < 3; ++part) {
        for (int i = 0; i < 1500; ++i) t.push_back((uint16_t)(0x4E00 + below(900) * 7));
        t.insert(t.end(), 70000, (uint16_t)(0x30A1 + part));
        for (int i = 0; i < 50; ++i)
            for (const char *p = "log line\n"; *p; ++p) t.push_back((uint16_t)*p);
    }
    return t;
}

void ranges_for(int32_t text_len, int32_t sr, std::vector<int32_t> &a, std::vector<int32_t> &b) {
    const int32_t p = sr >= 32 ? sr : (31 / sr + 1) * sr, L = text_len;
    auto add = [&](int64_t x, int64_t y) {
        a.push_back((int32_t)x);
        b.push_back((int32_t)y);
    };
    add(7, 7);
    for (int32_t ln : {0, 1, p - 1, p, p + 1})
        for (int32_t s0 : {0, 3 * p, 3 * p + 1, 5 * sr - 1, (int32_t)below((uint32_t)(L - p - 2))}) add(s0, s0 + ln);
    const int32_t k = L / 2 / sr;
    for (int da = -1; da <= 1; ++da)
        for (int db = -1; db <= 1; ++db)
            for (int span : {0, 1, 3}) add((int64_t)k * sr + da, (int64_t)(k + span) * sr + db);
    add(L - 50, L);
    add(L - 1, L);
    add(0, L);  // the whole text: crosses tiles
    for (int i = 0; i < 75; ++i) add(i * 3, i * 3 - (i & 1));
    add(L - 3000, L);
    add(-1, 5);
    add(10, L + 1);
    add(0, -2147483647);
    for (int i = 0; i < 120; ++i) {
        const int32_t s0 = (int32_t)below((uint32_t)L);
        add(s0, std::min<int64_t>(L, (int64_t)s0 + below((uint32_t)(4 * p))));
    }
    add(L / 2, L / 2);
}

}  // namespace

int main() {
    std::vector<uint16_t> log_text(60000);
    fmx_synth_log(42, (int32_t)log_text.size(), log_text.data());
    const std::vector<uint16_t> runs = run_block_text();
    int64_t redone_in_runs = 0;
    for (int which = 0; which < 2; ++which) {
        const std::vector<uint16_t> &text = which ? runs : log_text;
        for (int sr : {1, 5, 32, 64}) {
            fmx::FmModel m;
            std::string err;
            std::vector<uint8_t> blob;
            if (fmx::build_model(text.data(), (int32_t)text.size(), sr, true, m, err) || fmx::flatten_model(m, blob, err)) {
                printf("build failed: %s\n", err.c_str());
                return 1;
            }
            std::vector<int32_t> a, b;
            ranges_for((int32_t)text.size(), sr, a, b);
            const int32_t n = (int32_t)a.size();
            // the judge here: the literal fm_extract of every range (the oracle judges IT in the CPU suite)
            std::vector<std::vector<uint16_t>> want((size_t)n);
            std::vector<int32_t> want_status((size_t)n);
            for (int32_t i = 0; i < n; ++i) {
                const int32_t len = b[i] > a[i] ? b[i] - a[i] : 0;
                std::vector<uint16_t> row((size_t)len + 1, 0xFFFE);
                int32_t out_len = 0, lf = 0;
                sim_extract(blob.data(), &a[i], &b[i], 1, row.data(), len, 0, &out_len, &lf, &want_status[(size_t)i]);
                const bool early = want_status[(size_t)i] >= ST_NOT_ENABLED && want_status[(size_t)i] <= ST_STOP_TOO_LONG;
                const bool negative_index = want_status[(size_t)i] == ST_JAVA_AIOOBE && b[i] < 0;
                want[(size_t)i].assign(row.begin(), row.begin() + ((early || negative_index) ? 0 : len));
            }
            int64_t redone = 0, tiles = 0;
            for (int form : {0, 4, 6, -1}) {
                if (form) {
                    sim_set_entry_bytes(form);
                    sim_win_attach(blob.data(), nullptr);
                    sim_set_entry_bytes(0);
                }
                std::vector<int64_t> text_off((size_t)n + 1), piece_off((size_t)n + 1);
                std::vector<int32_t> status((size_t)n), redo((size_t)n + kPackedRedoHead), flags((size_t)n);
                sim_packed_offsets(blob.data(), a.data(), b.data(), n, text_off.data(), piece_off.data(), status.data());
                std::vector<uint16_t> chars((size_t)text_off[(size_t)n], 0xFFFE);  // exactly the answer: one unit more is a report
                int64_t info[6];
                sim_packed_fill(blob.data(), a.data(), b.data(), n, text_off.data(), piece_off.data(), chars.data(), status.data(), redo.data(),
                                flags.data(), form == 4 ? 1024 : 512, 3, form == 6 ? 8 : kLocateAllSlice, info);
                for (int32_t i = 0; i < n; ++i) {
                    const size_t len = (size_t)(text_off[(size_t)i + 1] - text_off[(size_t)i]);
                    if (status[(size_t)i] != want_status[(size_t)i] || len != want[(size_t)i].size() ||
                        (len && memcmp(chars.data() + text_off[(size_t)i], want[(size_t)i].data(), len * 2))) {
                        printf("text %d sr %d form %d: range %d (%d, %d) differs\n", which, sr, form, i, a[i], b[i]);
                        return 1;
                    }
                }
                redone += info[0];
                tiles = info[5];
                if (form) sim_win_detach(blob.data());
            }
            if (which == 0 && redone) {
                printf("the synthetic log redid %lld ranges\n", (long long)redone);
                return 1;
            }
            if (which) redone_in_runs += redone;
            printf("text %d sr %d ok: %d ranges, %lld tiles, %lld redone over four forms\n", which, sr, n, (long long)tiles, (long long)redone);
        }
    }
    if (!redone_in_runs) {
        printf("no range of the run-block text was redone\n");
        return 1;
    }
    return 0;
}
