// fmx_host_batch.cpp — the HOST arrays of the where, histogram, stats, top and keyed forms (fmx_host_stage.hpp): their checks — the
// offsets, where_of and the window of lines, by_of, the edges, the shape of the values and of the numbers, term_len, the limits of
// the hits — and the merge of the filter terms and the value patterns into ONE batch, literal and class, with the key patterns
// between them for the keyed forms.  Plain C++: no HIP runtime call and nothing of a handle, so that the CPU suite links this file
// alone, under sanitizers (tests/cpp/san_merged_batch.cpp).
#include "fmx_hit_numbers.hpp"
#include "fmx_host_stage.hpp"

namespace fmx {

int no_line_table() { return api_fail(FMX_E_ARG, "the index has no line table (call fmx_line_table_build)"); }

int check_offsets(const int32_t *off, int32_t n, const char *what) {
    if (off[0] < 0) return api_fail(FMX_E_ARG, std::string(what) + " offsets start below 0");
    for (int32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return api_fail(FMX_E_ARG, std::string(what) + " offsets decrease");
    return FMX_OK;
}

int check_literal_batches(const int32_t *pat_off, int32_t n, const int32_t *term_off, int32_t n_terms) {
    int rc;
    if ((n > 0 && (rc = check_offsets(pat_off, n, "pattern"))) || (n_terms > 0 && (rc = check_offsets(term_off, n_terms, "term")))) return rc;
    return FMX_OK;
}

int check_class_batches(const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n, const uint16_t *term_alt,
                        const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off, int32_t n_terms) {
    int rc;
    if ((rc = check_offsets(pos_off, n_pos, "position")) || (rc = check_offsets(pat_off, n, "pattern"))) return rc;
    if (pat_off[n] > n_pos) return api_fail(FMX_E_ARG, "pattern offsets end behind the positions");
    if (pos_off[n_pos] > 0 && !alt) return api_fail(FMX_E_ARG, "bad arguments");
    if (n_terms > 0) {
        if ((rc = check_offsets(term_pos_off, term_n_pos, "term position")) || (rc = check_offsets(term_off, n_terms, "term"))) return rc;
        if (term_off[n_terms] > term_n_pos) return api_fail(FMX_E_ARG, "term offsets end behind the positions");
        if (term_pos_off[term_n_pos] > 0 && !term_alt) return api_fail(FMX_E_ARG, "bad arguments");
    }
    return FMX_OK;
}

int merge_literal_batch(const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat, const int32_t *term_off,
                        int32_t n_terms, MergedBatch *m, ValuesBatch *batch) {
    const int64_t term_chars = n_terms > 0 ? (int64_t)term_off[n_terms] - term_off[0] : 0, pat_chars = (int64_t)pat_off[n] - pat_off[0];
    if (term_chars + pat_chars > INT32_MAX) return api_fail(FMX_E_ARG, "more than 2^31 - 1 characters in one batch");
    if ((term_chars > 0 && !term_pat) || (pat_chars > 0 && !pat)) return api_fail(FMX_E_ARG, "bad arguments");
    m->chars.assign((size_t)(term_chars + pat_chars) + 1, 0);
    m->off.assign((size_t)n_terms + n + 1, 0);
    for (int32_t t = 0; t < n_terms; ++t) m->off[(size_t)t] = term_off[t] - term_off[0];
    for (int32_t i = 0; i <= n; ++i) m->off[(size_t)n_terms + i] = (int32_t)(term_chars + (pat_off[i] - pat_off[0]));
    for (int64_t k = 0; k < term_chars; ++k) m->chars[(size_t)k] = term_pat[term_off[0] + k];
    for (int64_t k = 0; k < pat_chars; ++k) m->chars[(size_t)(term_chars + k)] = pat[pat_off[0] + k];
    *batch = ValuesBatch{m->chars.data(), nullptr, 0, m->off.data(), n_terms, n, 0};
    return FMX_OK;
}

// ... position by position
int merge_class_batch(const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n, const uint16_t *term_alt,
                      const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off, int32_t n_terms, int32_t max_ranges,
                      MergedBatch *m, ValuesBatch *batch) {
    if ((int64_t)(n_terms > 0 ? term_pos_off[term_n_pos] : 0) + pos_off[n_pos] > INT32_MAX)
        return api_fail(FMX_E_ARG, "more than 2^31 - 1 alternatives in one batch");
    m->chars.clear();
    m->pos.assign(1, 0);
    m->off.assign(1, 0);
    auto append = [&](const uint16_t *a, const int32_t *pos, const int32_t *off, int32_t count) {
        for (int32_t i = 0; i < count; ++i) {
            for (int32_t j = off[i]; j < off[i + 1]; ++j) {
                m->chars.insert(m->chars.end(), a + pos[j], a + pos[j + 1]);
                m->pos.push_back((int32_t)m->chars.size());
            }
            m->off.push_back((int32_t)m->pos.size() - 1);
        }
    };
    if (n_terms > 0) append(term_alt, term_pos_off, term_off, n_terms);
    append(alt, pos_off, pat_off, n);
    m->chars.push_back(0);  // (never an empty array)
    *batch = ValuesBatch{m->chars.data(), m->pos.data(), (int32_t)m->pos.size() - 1, m->off.data(), n_terms, n, max_ranges};
    return FMX_OK;
}

// the m + n lengths of the keys and the numbers from the offsets of their batch
static void lengths_of(const std::vector<int32_t> &off, std::vector<int32_t> *len) {
    len->clear();
    for (size_t i = 0; i + 1 < off.size(); ++i) len->push_back(off[i + 1] - off[i]);
}

// ... the keys take the terms' slot of the first merge, the numbers lie behind them; then the terms in front
int merge_keyed_literal_batch(const uint16_t *key_pat, const int32_t *key_off, int32_t m, const uint16_t *pat, const int32_t *pat_off, int32_t n,
                              const uint16_t *term_pat, const int32_t *term_off, int32_t n_terms, MergedBatch *merged, ValuesBatch *batch,
                              std::vector<int32_t> *term_len) {
    MergedBatch both;
    ValuesBatch both_batch;
    int rc;
    if ((rc = merge_literal_batch(pat, pat_off, n, key_pat, key_off, m, &both, &both_batch)) ||
        (rc = merge_literal_batch(both.chars.data(), both.off.data(), m + n, term_pat, term_off, n_terms, merged, batch)))
        return rc;
    lengths_of(both.off, term_len);
    return FMX_OK;
}

int merge_keyed_class_batch(const uint16_t *key_alt, const int32_t *key_pos_off, int32_t key_n_pos, const int32_t *key_off, int32_t m,
                            const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n, const uint16_t *term_alt,
                            const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off, int32_t n_terms, int32_t max_ranges,
                            MergedBatch *merged, ValuesBatch *batch, std::vector<int32_t> *term_len) {
    MergedBatch both;
    ValuesBatch both_batch;
    int rc;
    if ((rc = merge_class_batch(alt, pos_off, n_pos, pat_off, n, key_alt, key_pos_off, key_n_pos, key_off, m, max_ranges, &both, &both_batch)) ||
        (rc = merge_class_batch(both.chars.data(), both.pos.data(), both_batch.n_pos, both.off.data(), m + n, term_alt, term_pos_off, term_n_pos,
                                term_off, n_terms, max_ranges, merged, batch)))
        return rc;
    lengths_of(both.off, term_len);  // (a position is a character)
    return FMX_OK;
}

bool hits_filter_asked(int32_t n, const int32_t *where_of, int32_t line_lo, int32_t line_hi) {
    if (line_lo != 0 || line_hi != INT32_MAX) return true;
    for (int32_t i = 0; i < n; ++i)
        if (where_of[i] >= 0) return true;
    return false;
}

int check_where_of(int32_t n, const int32_t *where_of, int32_t q) {
    for (int32_t i = 0; i < n; ++i)
        if (where_of[i] < -1 || where_of[i] >= q) return api_fail(FMX_E_ARG, "where_of[" + std::to_string(i) + "] is outside -1 .. q - 1");
    return FMX_OK;
}

int check_where(int32_t n, const int32_t *where_of, int32_t q, int32_t line_lo, int32_t line_hi) {
    if (n < 0 || q < 0 || line_lo < 0 || line_hi < 0 || (n > 0 && !where_of)) return api_fail(FMX_E_ARG, "bad arguments");
    if (line_lo > line_hi) return api_fail(FMX_E_ARG, "the window of lines ends in front of its start");
    return check_where_of(n, where_of, q);
}

int check_values_shape(const uint16_t *stop, int32_t n_stop, int32_t max_len) {
    if (max_len < 1 || max_len > kValuesMaxLen) return api_fail(FMX_E_ARG, "max_len is outside [1, 64]");
    if (n_stop < 0 || n_stop > kValuesMaxStop || (n_stop > 0 && !stop)) return api_fail(FMX_E_ARG, "the stop set is outside [0, 64] code units");
    return FMX_OK;
}

int check_values_hits(int64_t n_hits, int32_t max_len) {
    if (n_hits > 0x7fffffff) return api_fail(FMX_E_ARG, "more than 2^31 - 1 hits in one call");
    if (n_hits * max_len > kValuesMaxUnits) return api_fail(FMX_E_ARG, "the windows of the hits hold more than 2^35 code units");
    return FMX_OK;
}

int check_term_len(int32_t n, const int32_t *term_len) {
    for (int32_t i = 0; i < n; ++i)
        if (term_len[i] < 0) return api_fail(FMX_E_ARG, "term_len[" + std::to_string(i) + "] is negative");
    return FMX_OK;
}

int check_numbers_shape(int32_t frac_digits, const int32_t *permille, int32_t n_permille) {
    if (frac_digits < 0 || frac_digits > kNumFracMax) return api_fail(FMX_E_ARG, "frac_digits is outside [0, 9]");
    switch (fm_num_permille_bad(permille, n_permille)) {
        case 0: return FMX_OK;
        case 1: return api_fail(FMX_E_ARG, "n_permille is outside [0, 16]");
        default: return api_fail(FMX_E_ARG, "a permille is outside [0, 1000]");
    }
}

int check_by_of(int32_t n, const int32_t *by_of, int32_t m) {
    if (n > 0 && m <= 0) return api_fail(FMX_E_ARG, "number patterns without a key pattern (m == 0 with n > 0)");
    for (int32_t i = 0; i < n; ++i)
        if (by_of[i] < 0 || by_of[i] >= m) return api_fail(FMX_E_ARG, "by_of[" + std::to_string(i) + "] is outside 0 .. m - 1");
    return FMX_OK;
}

int check_edges_array(const int32_t *edges, int32_t n_edges) {
    switch (fm_hist_edges_bad(edges, n_edges)) {
        case 0: return FMX_OK;
        case 1: return api_fail(FMX_E_ARG, "fewer than 2 edges");
        case 2: return api_fail(FMX_E_ARG, "the first edge is negative");
        default: return api_fail(FMX_E_ARG, "the edges decrease");
    }
}

}  // namespace fmx
