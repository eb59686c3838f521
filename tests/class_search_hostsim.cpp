// class_search_hostsim.cpp — TEST-ONLY host build of the device code of the class search (fmx_class_*):
// index4j_amd/csrc/fmx_device.hpp's fm_class_keep / _rank / _first / _candidate / _advance / _survives / _slot, driven by a serial
// mirror of k_class_search (fmx_class_search.hip): a team per pattern, the position's alternatives mapped, freed of code 0 and
// duplicates and ordered as the team's lanes do it, the candidates code-major and range-minor in rounds of kClassPairs lane pairs
// (both roles of a pair evaluated in turn), the survivors appended from the round's bit mask, both stages with the exclusive scan
// between them.  g++ compiles the header's FMX_HD functions as plain C++, so the CPU suite checks the very source the kernel runs
// against the oracle (tests/test_class_search_cpu.py).  The image's view and the literal search (sim_count) come from
// tests/hostsim.cpp, included as it stands.  Never part of libfmx.so.
#include "hostsim.cpp"

#include <vector>

namespace {

struct ClassTeam {  // what a team keeps in LDS: exactly as large as fm_class_team_bytes says
    std::vector<int32_t> front[2];  // {start, end} pairs
    std::vector<int16_t> code, kept;
    explicit ClassTeam(int32_t max_ranges)
        : front{std::vector<int32_t>((size_t)max_ranges * 2), std::vector<int32_t>((size_t)max_ranges * 2)},
          code((size_t)kClassAltsMax),
          kept((size_t)kClassAltsMax) {}
};

struct ClassAnswer {
    int32_t n_ranges = 0, count = 0, status = ST_OK, cur = 0;
};

// one pattern, as its team runs it; info (nullable, 3 slots) += {candidates, rank calls}, [2] = max(the largest frontier)
ClassAnswer class_search_one(const DevIndex &ix, const uint16_t *alt, const int32_t *pos_off, int32_t first_pos, int32_t m, int32_t max_ranges,
                             ClassTeam &T, int64_t *info) {
    ClassAnswer A;
    if (m <= 0) {
        A.status = ST_JAVA_AIOOBE;
        return A;
    }
    bool too_many = false;
    for (int32_t j = 0; j < m; ++j) too_many |= pos_off[first_pos + j + 1] - pos_off[first_pos + j] > kClassAltsMax;
    int status = ST_OK;
    int32_t n_cur = 0;
    int cur = 0;
    bool go = !too_many;
    for (int32_t k = 0; go && k < m; ++k) {
        const int32_t j = first_pos + m - 1 - k;
        const int32_t a0 = pos_off[j];
        int32_t n_alt = pos_off[j + 1] - a0;
        if (n_alt < 0) n_alt = 0;
        for (int32_t t = 0; t < n_alt; ++t) T.code[(size_t)t] = (int16_t)fm_map(ix, alt[a0 + t]);
        for (int32_t t = 0; t < n_alt; ++t) T.kept[(size_t)t] = fm_class_keep(T.code.data(), n_alt, t) ? T.code[(size_t)t] : (int16_t)0;
        int32_t n_codes = 0;
        for (int32_t t = 0; t < n_alt; ++t)
            if (T.kept[(size_t)t]) {
                T.code[(size_t)fm_class_rank(T.kept.data(), n_alt, t)] = T.kept[(size_t)t];
                ++n_codes;
            }
        const std::vector<int32_t> &src = T.front[cur];
        std::vector<int32_t> &dst = T.front[cur ^ 1];
        const int32_t n_cand = k == 0 ? n_codes : n_codes * n_cur;
        int32_t n_next = 0;
        for (int32_t q0 = 0; q0 < n_cand && !too_many; q0 += kClassPairs) {
            int32_t start[kClassPairs], end[kClassPairs];
            uint32_t bits = 0;
            for (int pair = 0; pair < kClassPairs; ++pair) {
                const int32_t q = q0 + pair;
                if (q >= n_cand) continue;
                if (k == 0) {
                    fm_class_first(ix, T.code[(size_t)q], start[pair], end[pair]);
                } else {
                    int32_t a, r;
                    fm_class_candidate(q, n_cur, a, r);
                    const int32_t s0 = src[(size_t)2 * r], e0 = src[(size_t)2 * r + 1];
                    start[pair] = fm_class_advance(ix, ix.inv_global, s0, e0, 0, T.code[(size_t)a], status);
                    end[pair] = fm_class_advance(ix, ix.inv_global, s0, e0, 1, T.code[(size_t)a], status);
                    if (info) info[1] += 2;
                }
                if (info) ++info[0];
                if (fm_class_survives(start[pair], end[pair])) bits |= 1u << (2 * pair);  // (the pair's role-0 lane)
            }
            const int32_t total = fmx_popc(bits);
            for (int pair = 0; pair < kClassPairs; ++pair) {
                if (!(bits >> (2 * pair) & 1u)) continue;
                const int32_t slot = fm_class_slot(n_next, fmx_popc(bits & ((1u << (2 * pair)) - 1u)), total, max_ranges);
                if (slot < 0) continue;
                dst[(size_t)2 * slot] = start[pair];
                dst[(size_t)2 * slot + 1] = end[pair];
            }
            if (fm_class_slot(n_next, 0, total, max_ranges) < 0)
                too_many = true;
            else
                n_next += total;
        }
        if (too_many) break;
        n_cur = n_next;
        cur ^= 1;
        if (info && n_cur > info[2]) info[2] = n_cur;
        if (n_cur == 0) go = false;
    }
    if (too_many) {
        A.status = ST_TOO_MANY_RANGES;
        return A;
    }
    A.status = status;
    A.n_ranges = n_cur;
    A.cur = cur;
    for (int32_t i = 0; i < n_cur; ++i) A.count += T.front[cur][(size_t)2 * i + 1] - T.front[cur][(size_t)2 * i];
    return A;
}

}  // namespace

extern "C" {

int32_t sim_class_team() { return kClassTeam; }
int32_t sim_class_ranges_max() { return kClassRangesMax; }
int32_t sim_class_alts_max() { return kClassAltsMax; }
int64_t sim_class_team_bytes(int32_t max_ranges) { return (int64_t)fm_class_team_bytes(max_ranges); }

// stage 1 + the exclusive scan: range_off (n + 1), counts, status (n each); `teams` patterns per workgroup of `grid` workgroups,
// in the kernel's grid-stride order.  info: 3 slots, see class_search_one.
void sim_class_count(const uint8_t *blob, const uint16_t *alt, const int32_t *pos_off, const int32_t *pat_off, int32_t n, int32_t max_ranges,
                     int32_t teams, int32_t grid, int64_t *range_off, int32_t *counts, int32_t *status_out, int64_t *info) {
    const DevIndex ix = make_index(blob);
    for (int i = 0; i < 3; ++i) info[i] = 0;
    std::vector<int64_t> cnt((size_t)n + 1, 0);
    std::vector<ClassTeam> lds((size_t)teams, ClassTeam(max_ranges));
    for (int64_t group = 0; group < grid; ++group)
        for (int64_t p0 = group * teams; p0 < n; p0 += (int64_t)grid * teams)
            for (int team = 0; team < teams; ++team) {
                const int64_t p = p0 + team;
                if (p >= n) continue;
                const ClassAnswer A = class_search_one(ix, alt, pos_off, pat_off[p], pat_off[p + 1] - pat_off[p], max_ranges, lds[(size_t)team], info);
                cnt[(size_t)p] = A.n_ranges;
                counts[p] = A.count;
                status_out[p] = A.status;
            }
    int64_t sum = 0;
    for (int32_t i = 0; i <= n; ++i) {
        range_off[i] = sum;
        sum += cnt[(size_t)i];
    }
}

// stage 2: the search again, the ranges of pattern i at ranges[2 * range_off[i] ..)
void sim_class_fill(const uint8_t *blob, const uint16_t *alt, const int32_t *pos_off, const int32_t *pat_off, int32_t n, int32_t max_ranges,
                    int32_t teams, int32_t grid, const int64_t *range_off, int32_t *ranges) {
    const DevIndex ix = make_index(blob);
    std::vector<ClassTeam> lds((size_t)teams, ClassTeam(max_ranges));
    for (int64_t group = 0; group < grid; ++group)
        for (int64_t p0 = group * teams; p0 < n; p0 += (int64_t)grid * teams)
            for (int team = 0; team < teams; ++team) {
                const int64_t p = p0 + team;
                if (p >= n) continue;
                ClassTeam &T = lds[(size_t)team];
                const ClassAnswer A = class_search_one(ix, alt, pos_off, pat_off[p], pat_off[p + 1] - pat_off[p], max_ranges, T, nullptr);
                const int64_t at = range_off[p], room = range_off[p + 1] - at;
                for (int32_t i = 0; i < A.n_ranges && i < room; ++i) {
                    ranges[2 * (at + i)] = T.front[A.cur][(size_t)2 * i];
                    ranges[2 * (at + i) + 1] = T.front[A.cur][(size_t)2 * i + 1];
                }
            }
}

// fmx_class_hit_offsets_dev: k_hit_counts + scan over the m ranges (every hit), then the gather
void sim_class_hit_offsets(const int64_t *range_off, int32_t n, const int32_t *ranges, int64_t m, int64_t *range_hit_off, int64_t *hit_off) {
    int64_t sum = 0;
    for (int64_t r = 0; r <= m; ++r) {
        range_hit_off[r] = sum;
        if (r < m) sum += fm_locate_all_hits(ranges[2 * r], ranges[2 * r + 1], -1);
    }
    for (int32_t i = 0; i <= n; ++i) {
        int64_t r = range_off[i];
        r = r < 0 ? 0 : (r > m ? m : r);
        hit_off[i] = range_hit_off[r];
    }
}
}
