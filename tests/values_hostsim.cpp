// values_hostsim.cpp — TEST-ONLY host build of the device code of "the values that follow a pattern, with counts"
// (fmx_values_of_hits_dev / fmx_values_fill_dev): index4j_amd/csrc/fmx_hit_values.hpp's fm_val_window, fm_val_length over both forms
// of the stop set, fm_val_same, fm_val_chunk_key, fm_val_lower_bound — with fm_hit_pattern for a hit's pattern — driven by a mirror
// of the stages of fmx_hit_values.hip with the lanes run one after the other (every radix_sort_pairs pass = std::stable_sort on
// that pass's keys over all n_hits slots, the scans = running sums).  g++ compiles the header's functions as plain C++, so the CPU
// suite checks the source of those FUNCTIONS (tests/test_field_values_cpu.py).  NOT mirrored: k_val_ranges' tile loop, which is
// k_hit_line_keys' (tests/locate_all_hostsim.cpp mirrors that loop), and the packed extract between the first stage and the rest
// (tests/extract_packed_hostsim.cpp): the windows' text comes in with the input, made by the judge for the windows this program
// must find itself.  The kernels' own route runs in tests/test_gpu_field_values.py only.  Never part of libfmx.so.
//
// A stand-alone program:  values_hostsim IN OUT [list]   ("list": the sorted units as the stop set's form, else the bitmap)
//   IN   int64 {n, n_hits, n_stop, max_len, text_len}, int32 term_len[n], uint16 stop[n_stop], int64 hit_off[n + 1],
//        int32 locs[n_hits], int64 win_off[n_hits + 1], uint16 win[win_off[n_hits]]
//   OUT  int64 {G, R, units}, int64 val_off[n + 1], int32 count[G], int64 text_off[G + 1], uint16 chars[units],
//        int32 start[n_hits], int32 stop[n_hits]
// Exit status 3: a window of the input does not have the length this program's first stage finds for it.
#include "../index4j_amd/csrc/fmx_hit_values.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace fmx;

namespace {

template <class T>
bool get(FILE *f, std::vector<T> &v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}
template <class T>
void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

// one radix_sort_pairs pass: stable, by `key` of the slot's run
template <class Key>
void pass(std::vector<uint32_t> &perm, Key key) {
    std::vector<decltype(key(0u))> keys(perm.size());
    for (size_t j = 0; j < perm.size(); ++j) keys[j] = key(perm[j]);
    std::vector<uint32_t> order(perm.size());
    for (size_t j = 0; j < order.size(); ++j) order[j] = (uint32_t)j;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    std::vector<uint32_t> out(perm.size());
    for (size_t j = 0; j < order.size(); ++j) out[j] = perm[order[j]];
    perm.swap(out);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const bool list = argc > 3 && !strcmp(argv[3], "list");
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<int64_t> head, hit_off, win_off;
    std::vector<int32_t> term_len, locs;
    std::vector<uint16_t> stop, win;
    if (!get(in, head, 5)) return 2;
    const int32_t n = (int32_t)head[0], n_stop = (int32_t)head[2], max_len = (int32_t)head[3], text_len = (int32_t)head[4];
    const int64_t n_hits = head[1];
    if (!get(in, term_len, (size_t)n) || !get(in, stop, (size_t)n_stop) || !get(in, hit_off, (size_t)n + 1) || !get(in, locs, (size_t)n_hits) ||
        !get(in, win_off, (size_t)n_hits + 1) || !get(in, win, (size_t)win_off[(size_t)n_hits]))
        return 2;
    fclose(in);
    const size_t H = (size_t)n_hits;
    // launch_values_ranges: the stop set sorted, a hit's pattern and window
    std::sort(stop.begin(), stop.end());
    std::vector<uint32_t> bitmap(kStopBitmapWords, 0);
    for (uint16_t u : stop) bitmap[u >> 5] |= 1u << (u & 31);
    const int64_t total = hit_off[(size_t)n] < n_hits ? hit_off[(size_t)n] : n_hits;
    std::vector<int32_t> pat(H), start(H), stop_at(H);
    for (int64_t t = 0; t < n_hits; ++t) {  // k_val_ranges
        if (t >= total) {
            pat[(size_t)t] = n;
            start[(size_t)t] = stop_at[(size_t)t] = 0;
            continue;
        }
        const int32_t p = fm_hit_pattern(hit_off.data(), n, t);
        fm_val_window(locs[(size_t)t], term_len[(size_t)p], max_len, text_len, start[(size_t)t], stop_at[(size_t)t]);
        pat[(size_t)t] = p;
        if (win_off[(size_t)t + 1] - win_off[(size_t)t] != stop_at[(size_t)t] - start[(size_t)t]) return 3;
    }
    std::vector<int32_t> vlen(H);
    for (size_t t = 0; t < H; ++t) {  // k_val_lengths
        const uint16_t *w = win.data() + win_off[t];
        const int32_t len = (int32_t)(win_off[t + 1] - win_off[t]);
        vlen[t] = pat[t] >= n ? 0 : list ? fm_val_length<false>(w, len, stop.data(), n_stop) : fm_val_length<true>(w, len, bitmap.data(), n_stop);
    }
    std::vector<int32_t> flag(H + 1, 0), scan(H + 1), run_start(H + 1, -7);
    for (size_t i = 0; i < H; ++i)  // k_val_run_flags
        if (pat[i] < n)
            flag[i] = i == 0 || pat[i - 1] != pat[i] || !fm_val_same(win.data() + win_off[i - 1], vlen[i - 1], win.data() + win_off[i], vlen[i]);
    int32_t sum = 0;
    for (size_t i = 0; i <= H; ++i) {  // the scan
        scan[i] = sum;
        sum += flag[i];
    }
    const uint32_t R = (uint32_t)scan[H];
    for (size_t i = 0; i <= H; ++i) {  // k_val_run_starts
        if (i == H)
            run_start[R] = (int32_t)total;
        else if (flag[i])
            run_start[(size_t)scan[i]] = (int32_t)i;
    }
    // the exact grouping: stable passes over all n_hits slots, the least significant first
    std::vector<uint32_t> perm(H);
    for (size_t j = 0; j < H; ++j) perm[j] = (uint32_t)j;
    pass(perm, [&](uint32_t r) { return r < R ? (uint32_t)vlen[(size_t)run_start[r]] : 0u; });
    for (int32_t c = fm_val_chunks(max_len) - 1; c >= 0; --c)
        pass(perm, [&](uint32_t r) {
            if (r >= R) return (uint64_t)0;
            const size_t h = (size_t)run_start[r];
            return fm_val_chunk_key(win.data() + win_off[h], vlen[h], c);
        });
    pass(perm, [&](uint32_t r) { return r < R ? (uint32_t)pat[(size_t)run_start[r]] : (uint32_t)n; });
    std::vector<uint32_t> skeys(H);
    for (size_t j = 0; j < H; ++j) skeys[j] = perm[j] < R ? (uint32_t)pat[(size_t)run_start[perm[j]]] : (uint32_t)n;
    std::vector<int32_t> head_flag(H + 1, 0), weight(H + 1, 0), hscan(H + 1), wscan(H + 1);
    std::vector<int64_t> hlen(H + 1, 0), lscan(H + 1);
    for (size_t j = 0; j < H; ++j) {  // k_val_heads
        if (skeys[j] >= (uint32_t)n) continue;
        const uint32_t r = perm[j];
        const size_t h = (size_t)run_start[r];
        weight[j] = run_start[r + 1] - (int32_t)h;
        int32_t f = 1;
        if (j > 0 && skeys[j - 1] == skeys[j]) {
            const size_t g = (size_t)run_start[perm[j - 1]];
            f = !fm_val_same(win.data() + win_off[g], vlen[g], win.data() + win_off[h], vlen[h]);
        }
        head_flag[j] = f;
        if (f) hlen[j] = vlen[h];
    }
    int32_t hs = 0, wsum = 0;
    int64_t ls = 0;
    for (size_t j = 0; j <= H; ++j) {  // the three scans
        hscan[j] = hs;
        wscan[j] = wsum;
        lscan[j] = ls;
        hs += head_flag[j];
        wsum += weight[j];
        ls += hlen[j];
    }
    const size_t G = (size_t)hscan[H];
    std::vector<int32_t> group_start(H + 1, -7), count(G);
    std::vector<int64_t> text_off(G + 1), val_off((size_t)n + 1);
    std::vector<const uint16_t *> src(G);
    for (size_t j = 0; j <= H; ++j) {  // k_val_groups
        if (j == H) {
            group_start[G] = (int32_t)H;
            text_off[G] = lscan[H];
        } else if (head_flag[j]) {
            const size_t g = (size_t)hscan[j];
            group_start[g] = (int32_t)j;
            text_off[g] = lscan[j];
            src[g] = win.data() + win_off[(size_t)run_start[perm[j]]];
        }
    }
    for (size_t g = 0; g < G; ++g) count[g] = wscan[(size_t)group_start[g + 1]] - wscan[(size_t)group_start[g]];  // k_val_counts
    for (int32_t p = 0; p <= n; ++p) val_off[(size_t)p] = hscan[(size_t)fm_val_lower_bound(skeys.data(), n_hits, (uint32_t)p)];  // k_val_offsets
    std::vector<uint16_t> chars((size_t)text_off[G]);
    for (size_t g = 0; g < G; ++g)  // k_val_fill
        for (int64_t k = 0; k < text_off[g + 1] - text_off[g]; ++k) chars[(size_t)(text_off[g] + k)] = src[g][k];
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    put(out, std::vector<int64_t>{(int64_t)G, (int64_t)R, text_off[G]});
    put(out, val_off);
    put(out, count);
    put(out, text_off);
    put(out, chars);
    put(out, start);
    put(out, stop_at);
    return fclose(out) == 0 ? 0 : 2;
}
