// fuzz_rows.cpp — TEST-ONLY: the mutation campaign of fuzz_load.cpp (same doors, same mutations: that file is included as it
// stands, its main() renamed) aimed at the ROW TABLE of a resident index (fmx_device.hpp DevIndex.rows; option locate_rows).
// For every image the validators accept, the table is filled — over the tree and over a window directory grown from that very
// image — into an EXACT-SIZE heap block, and ranges as a count phase over a damaged image may hand them back are located through
// it, with the device code compiled for the host (tests/rows_hostsim.cpp) under AddressSanitizer and the watchdog.  A damaged
// image may answer wrongly or with a status; a read outside the table here would be a read outside it on the GPU.
// Usage: fuzz_rows <iterations> <seed>; prints one summary line, exit code 0 = clean.  -DFMX_COMPACT=1: compact images.
#define main fuzz_load_main
#include "fuzz_load.cpp"
#undef main
// (hostsim.cpp is in through fuzz_load.cpp: only the row table's own functions are taken from here)
#define ROWS_HOSTSIM_NO_BASE 1
#include "../rows_hostsim.cpp"

namespace {

long g_filled = 0, g_replay = 0, g_rows_total = 0;

void locate_through_rows(const std::vector<uint8_t> &blob, const std::vector<uint16_t> &text, Rng &r, int directory) {
    uint8_t *img = new uint8_t[blob.size()];
    memcpy(img, blob.data(), blob.size());
    if (directory) {
        g_where = "growing the window directory";
        sim_set_entry_bytes(directory);
        (void)sim_win_attach(img, nullptr);
        sim_set_entry_bytes(0);
    }
    BlobHeader h;
    memcpy(&h, img, sizeof h);
    const size_t n_rows = (size_t)sim_rows_size(img);
    uint32_t *rows = new uint32_t[n_rows];  // exact size: ASan sees the first word past it
    g_where = "filling the row table";
    g_replay += (long)sim_rows_fill(img, rows);
    g_rows_total += (long)n_rows;
    ++g_filled;
    const int n = 24;
    std::vector<uint16_t> pat;
    std::vector<int32_t> off(1, 0);
    for (int q = 0; q < n; ++q) {
        const int m = 1 + (int)r.below(6);
        const size_t from = r.below((uint32_t)(text.size() - 16));
        for (int i = 0; i < m; ++i) pat.push_back(text[from + i]);
        off.push_back((int32_t)pat.size());
    }
    std::vector<int32_t> counts(n), lf(n), st(n), range(2 * n);
    g_where = "count";
    sim_count(img, pat.data(), off.data(), n, counts.data(), lf.data(), st.data(), range.data());
    // what count left, a few arbitrary rows around the table's ends, and ranges no table has
    const int32_t length = h.length;
    for (int q = 0; q < n; q += 3) {
        range[2 * q] = (int32_t)r.below((uint32_t)length + 8) - 4;
        range[2 * q + 1] = range[2 * q] + (int32_t)r.below(40);
    }
    range[2] = 0x7ffffff0;
    range[3] = 0x7ffffff8;
    range[8] = -40;
    range[9] = 3;
    for (const int cap : {1, 4, 16, 100}) {
        for (const int mm : {-1, 1, 16}) {
            std::vector<int32_t> locs((size_t)n * cap), found(n);
            std::fill(lf.begin(), lf.end(), 0);
            std::fill(st.begin(), st.end(), 0);
            g_where = "locate through the row table";
            (void)sim_locate_rows(img, rows, range.data(), n, mm, locs.data(), cap, found.data(), lf.data(), st.data(), nullptr, nullptr,
                                  nullptr, 0);
        }
    }
    delete[] rows;
    if (directory) sim_win_detach(img);
    delete[] img;
}

}  // namespace

int main(int argc, char **argv) {
    const long iterations = argc > 1 ? atol(argv[1]) : 1000;
    Rng r{argc > 2 ? strtoull(argv[2], nullptr, 10) * 0x9e3779b97f4a7c15ull + 1 : 88172645463325252ull};
    signal(SIGALRM, on_alarm);
#if FMX_COMPACT
    fmx::set_image_compact(1);
#endif
    struct Base {
        std::vector<uint16_t> text;
        std::vector<uint8_t> ser, blob;
        fmx::FmModel model;
    };
    std::vector<Base> bases;
    const int kinds[][3] = {{12000, 0, 8}, {5000, 0, 1}, {14000, 0, 32}, {10000, 700, 4}, {4000, 1, 2}};  // n, alphabet kind, sampleRate
    for (const auto &k : kinds) {
        Base b;
        b.text.resize(k[0]);
        if (k[1] == 0)
            fmx_synth_log(7 + k[2], k[0], b.text.data());
        else if (k[1] == 1)
            for (auto &c : b.text) c = (uint16_t)('a' + r.below(3));
        else
            fmx_synth_log_multichar(11, k[0], k[1], b.text.data());
        std::string err;
        if (fmx::build_model(b.text.data(), k[0], k[2], true, b.model, err)) return printf("build failed: %s\n", err.c_str()), 2;
        fmx::emit_model(b.model, false, b.ser);
        if (fmx::flatten_model(b.model, b.blob, err)) return printf("flatten failed: %s\n", err.c_str()), 2;
        for (const int directory : {0, 4, 6, -1}) locate_through_rows(b.blob, b.text, r, directory);  // the undamaged image first
        bases.push_back(std::move(b));
    }
    const long undamaged = g_filled;
    for (g_iter = 0; g_iter < iterations; ++g_iter) {
        const Base &base = bases[r.below((uint32_t)bases.size())];
        std::string err;
        std::vector<uint8_t> blob;
        alarm(30);
        if (g_iter % 3 == 1) {  // door A: a stream written from a damaged model
            fmx::FmModel damaged = base.model;
            mutate_model(damaged, r);
            if (damaged.wt.sb.size() != base.model.wt.sb.size()) continue;
            std::vector<uint8_t> ser;
            g_where = "emit_model";
            fmx::emit_model(damaged, false, ser);
            fmx::FmModel m;
            g_where = "parse_model";
            if (fmx::parse_model(ser.data(), ser.size(), m, err) || fmx::validate_model(m, err)) continue;
            g_where = "flatten_model";
            if (fmx::flatten_model(m, blob, err) || fmx::validate_blob(blob.data(), blob.size(), err)) continue;
        } else if (g_iter % 3 == 2) {  // ... from damaged bytes
            std::vector<uint8_t> ser = base.ser;
            mutate(ser, r, true);
            fmx::FmModel m;
            g_where = "parse_model";
            if (fmx::parse_model(ser.data(), ser.size(), m, err) || fmx::validate_model(m, err)) continue;
            g_where = "flatten_model";
            if (fmx::flatten_model(m, blob, err) || fmx::validate_blob(blob.data(), blob.size(), err)) continue;
        } else {  // door B: a damaged image with a matching checksum
            blob = base.blob;
            mutate(blob, r, false);
            BlobHeader h;
            memcpy(&h, blob.data(), sizeof h);
            h.checksum = 0;
            memcpy(blob.data(), &h, sizeof h);
            h.checksum = fmx::image_checksum(blob.data(), blob.size());
            memcpy(blob.data(), &h, sizeof h);
            g_where = "validate_blob";
            if (fmx::validate_blob(blob.data(), blob.size(), err)) continue;
        }
        locate_through_rows(blob, base.text, r, 0);
        const int forms[3] = {4, 6, -1};
        locate_through_rows(blob, base.text, r, forms[r.below(3)]);
    }
    alarm(0);
    printf("rows fuzz ok: %ld damaged images accepted, filled and located (%ld undamaged before them); %ld of %ld rows marked replay\n",
           (g_filled - undamaged) / 2, undamaged, g_replay, g_rows_total);
    return 0;
}
