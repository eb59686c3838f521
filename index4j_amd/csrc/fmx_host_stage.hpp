// fmx_host_stage.hpp — the host-stage layer of the C ABI: what the feature files (fmx_class_api.cpp, fmx_where_api.cpp,
// fmx_hist_api.cpp, fmx_stats_api.cpp, fmx_range_api.cpp, fmx_by_api.cpp, fmx_value_hist_api.cpp, fmx_top_api.cpp,
// fmx_by_hist_api.cpp) see of a handle and of the packed host sequence of fmx_api.cpp, and what they share among themselves, each
// piece defined ONCE.  Host code only: no .hip file includes it.
//   fmx_api.cpp          the views of a handle, extract_windows, check_query_arrays, values_between_call, hits_stage_call
//   fmx_host_batch.cpp   the checks of a call's HOST arrays (offsets, where_of, by_of, edges, the values' and the numbers' shape,
//                        term_len, the limits of the hits) and the merges into ONE batch, terms | value patterns and terms | key
//                        patterns | number patterns: no HIP runtime call, so that the CPU suite links it as plain C++
//                        (tests/cpp/san_merged_batch.cpp)
//   fmx_host_stage.cpp   the stages on the device: the number filter over the terms' hits, the lines of the queries, the filter
//                        over the value patterns' hits, the groups of hits; the statistics arrays and the packed result of a
//                        stage; the keyed forms' call plumbing and their front half, from the filter to the group offsets
// Every function that returns int returns an FMX_* code (fmx::api_fail has set the message).
#pragma once

#include "fmx_abi.hpp"
#include "fmx_plan.hpp"

#include <climits>
#include <cstdlib>
#include <initializer_list>
#include <vector>

namespace fmx {

// ---- fmx_api.cpp: a resident FM handle after the checks of every FM device entry point (0 = *view is filled) -------------------
// the image a class search launches over
struct ClassView {
    const DevIndex *dev;
    int n_cu, device;
    bool compact;
};
int class_view(const ::fmx_index *idx, ClassView *view);
// the line table (table == nullptr: fmx_line_table_build has not run)
struct LineView {
    const int32_t *table;
    int32_t count;  // boundaries in the table
    int n_cu;
};
int line_view(const ::fmx_index *idx, LineView *view);
// what the windows of hits need
struct TextView {
    int32_t text_len;  // getInputLength() - 1
    bool extract;      // built with extraction
};
int text_view(const ::fmx_index *idx, TextView *view);
// both stages of the packed extract over n ranges on the device (the launcher the values stage uses), into the regions of a
// ValuesWindows
int extract_windows(const ::fmx_index *idx, const ValuesWindows &w, int32_t n, void *stream);
// the HOST arrays that cut n terms into q queries, as fmx_match_query_batch judges them (its return value)
int check_query_arrays(int32_t n, int32_t q, const int32_t *query_off, const uint8_t *term_kind);

// ---- fmx_api.cpp: the packed host sequence over a MERGED batch -----------------------------------------------------------------
// values_between_call: a range stage, the fill, the values stages, ONE result allocation, the per-pattern arrays, the last wait,
// over n_terms filter terms in front and n value patterns behind them — literal (pos_off == nullptr: chars / pat_off are
// fmx_count_batch's) or class (alt / pos_off / pat_off are fmx_count_class_batch's) — with a stage of the caller's between the fill
// and the values stages.  `between` sees every hit of the merged batch on the device and leaves the value patterns' kept hits as
// (kept_off, kept_locs), asynchronously on `stream`; its device blocks come from block() and live until the call has synchronised.
struct HitsBetween {
    const LineView *view;
    void *stream;
    int32_t n_terms, n;
    const int64_t *hit_off;      // n_terms + n + 1 (device)
    const int32_t *locs;         // `total` hits (device)
    int64_t term_hits, total;    // hit_off[n_terms], hit_off[n_terms + n]
    int64_t *kept_off;           // n + 1 (device, out)
    int32_t *kept_locs;          // room for total - term_hits (device, out)
    void *call;
    int (*block)(void *call, size_t bytes, void **out);
    const ::fmx_index *idx;      // the handle of the call
    int32_t *status;             // the value patterns' statuses (device, n; nullptr: the call asks for none)
    int32_t *term_status;        // the terms' statuses (device, n_terms; nullptr likewise)
};
struct ValuesBatch {
    const uint16_t *chars;
    const int32_t *pos_off;  // nullptr: literal patterns
    int32_t n_pos;
    const int32_t *pat_off;
    int32_t n_terms, n, max_ranges;
};
typedef int (*ValuesBetweenFn)(const HitsBetween &hits, void *arg);
int values_between_call(const ::fmx_index *idx, const ValuesBatch &batch, const uint16_t *stop, int32_t n_stop, int32_t max_len,
                        ValuesBetweenFn between, void *arg, int64_t *val_off, int32_t **counts, int64_t **text_off, uint16_t **chars,
                        int32_t *occurrences, int32_t *status, int32_t *kept, int32_t *term_status);
// hits_stage_call: the same sequence up to the caller's stage and no further — ONE range stage over the merged batch, every hit
// into one block, `stage`, the per-pattern arrays, the last wait.  kept_off / kept_locs of HitsBetween are NULL: the stage takes
// what it needs from block().  What it copies to the host asynchronously on `stream` has arrived when the call returns FMX_OK.
// occurrences / status are the value patterns', term_occurrences / term_status the terms' (each nullable).
int hits_stage_call(const ::fmx_index *idx, const ValuesBatch &batch, ValuesBetweenFn stage, void *arg, int32_t *occurrences, int32_t *status,
                    int32_t *term_occurrences, int32_t *term_status);

// ---- fmx_host_batch.cpp: the HOST arrays of a call ------------------------------------------------------------------------------
int no_line_table();  // the refusal of a call that needs the line table of an index without one
// offsets that start at or above 0 and never decrease (what the range stages ask of theirs: judged ahead of the merge)
int check_offsets(const int32_t *off, int32_t n, const char *what);
// the offset arrays of the value patterns and of the terms, literal and class
int check_literal_batches(const int32_t *pat_off, int32_t n, const int32_t *term_off, int32_t n_terms);
int check_class_batches(const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n, const uint16_t *term_alt,
                        const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off, int32_t n_terms);
// ONE batch, the terms in front, the value patterns behind them; *batch points into *m.  The offsets have been judged.
struct MergedBatch {
    std::vector<uint16_t> chars;
    std::vector<int32_t> pos, off;
};
int merge_literal_batch(const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat, const int32_t *term_off,
                        int32_t n_terms, MergedBatch *m, ValuesBatch *batch);
int merge_class_batch(const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n, const uint16_t *term_alt,
                      const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off, int32_t n_terms, int32_t max_ranges,
                      MergedBatch *m, ValuesBatch *batch);
// the same with m key patterns and n number patterns for value patterns: ONE batch terms | keys | numbers (to values_between_call /
// hits_stage_call the last two are m + n value patterns) and *term_len, the m + n lengths of the keys and the numbers (a position of
// a class pattern is a character).  The two merges above, one behind the other, and their refusals.
int merge_keyed_literal_batch(const uint16_t *key_pat, const int32_t *key_off, int32_t m, const uint16_t *pat, const int32_t *pat_off, int32_t n,
                              const uint16_t *term_pat, const int32_t *term_off, int32_t n_terms, MergedBatch *merged, ValuesBatch *batch,
                              std::vector<int32_t> *term_len);
int merge_keyed_class_batch(const uint16_t *key_alt, const int32_t *key_pos_off, int32_t key_n_pos, const int32_t *key_off, int32_t m,
                            const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off, int32_t n, const uint16_t *term_alt,
                            const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off, int32_t n_terms, int32_t max_ranges,
                            MergedBatch *merged, ValuesBatch *batch, std::vector<int32_t> *term_len);
// the number filter over the TERMS' hits (fmx_hit_range.hpp: term t is ranged iff num_lo[t] >= 0); the default is "none"
struct NumberTerms {
    const int64_t *num_lo = nullptr, *num_hi = nullptr;  // n_terms each (host)
    const int32_t *term_len = nullptr;                   // n_terms (host), none negative
    int32_t frac_digits = 0;                             // in [0, 9]
    bool ranged = false;                                 // number_terms_ranged
    // n_terms each (host, out, nullable): what the stage stores has arrived when the call has synchronised; a call whose terms have
    // no hit stores nothing
    int32_t *kept = nullptr, *not_number = nullptr, *overflow = nullptr;
};
inline bool number_terms_ranged(int32_t n_terms, const int64_t *num_lo) {
    for (int32_t t = 0; t < n_terms && num_lo; ++t)
        if (num_lo[t] >= 0) return true;
    return false;
}
// the queries, which query each value pattern asks for and the window of lines
struct HitsFilter {
    const int32_t *query_off;
    const uint8_t *term_kind;
    int32_t q;
    const int32_t *where_of;   // n entries, each -1 .. q - 1
    int32_t line_lo, line_hi;  // the window of lines (0 .. INT32_MAX: every line)
    bool filters;              // hits_filter_asked
    NumberTerms number{};      // query_lines_stage: a ranged term holds on a line iff one of its PASSING hits lies there
};
// the call filters at all: a pattern asks for a query, or the window is not 0 .. INT32_MAX
bool hits_filter_asked(int32_t n, const int32_t *where_of, int32_t line_lo = 0, int32_t line_hi = INT32_MAX);
int check_where_of(int32_t n, const int32_t *where_of, int32_t q);
// where_of and the window of lines 0 <= line_lo <= line_hi of a call that takes one
int check_where(int32_t n, const int32_t *where_of, int32_t q, int32_t line_lo, int32_t line_hi);
// the values stages' shape (fmx_hit_values.hpp): max_len in [1, 64], a stop set of [0, 64] code units
int check_values_shape(const uint16_t *stop, int32_t n_stop, int32_t max_len);
// their limits: at most 2^31 - 1 hits in one call and 2^35 code units in the hits' windows
int check_values_hits(int64_t n_hits, int32_t max_len);
int check_term_len(int32_t n, const int32_t *term_len);  // none negative
// the numbers stages' shape (fmx_hit_numbers.hpp): frac_digits in [0, 9], at most 16 permilles, each in [0, 1000]
int check_numbers_shape(int32_t frac_digits, const int32_t *permille, int32_t n_permille);
// by_of (n entries, each 0 .. m - 1): the key pattern each number pattern is grouped by (fmx_number_stats_by_batch); n > 0 needs m > 0
int check_by_of(int32_t n, const int32_t *by_of, int32_t m);
// edges by fmx_line_hist.hpp's rules (n_edges >= 2, edges[0] >= 0, never decreasing)
int check_edges_array(const int32_t *edges, int32_t n_edges);

// kept[i] = kept_off[i + 1] - kept_off[i] (kept nullable); a[0, count) = 0 (a nullable)
inline void kept_of(const int64_t *kept_off, int32_t n, int32_t *kept) {
    for (int32_t i = 0; i < n && kept; ++i) kept[i] = (int32_t)(kept_off[(size_t)i + 1] - kept_off[(size_t)i]);
}
template <class T>
void zero(T *a, size_t count) {
    for (size_t i = 0; i < count && a; ++i) a[i] = 0;
}

// ---- fmx_host_stage.cpp: inside a stage of values_between_call / hits_stage_call ------------------------------------------------
// the refusal of queries whose sort key query | line | term is wider than 64 bits (count: the boundaries of the line table)
int check_query_key_width(int32_t q, int32_t count, const int32_t *query_off);
// the lines of the f.q > 0 queries from the terms' hits, no limit: *d_line_off (q + 1) and *d_lines on the device, from block();
// d_line_count (device, q entries; nullable).  With f.number.ranged the terms' hits first go through number_range_run — the ONE
// launcher of that filter — and ONE 8-byte read and wait brings the kept total down, which sizes the line stage.  max_lines: the
// line stages' limit per query (0: none).
int query_lines_stage(const HitsBetween &h, const HitsFilter &f, int64_t **d_line_off, int32_t **d_lines, int32_t *d_line_count,
                      int32_t max_lines = 0);
// packed hits -> the packed hits whose number lies in a range (fmx_hit_range.hip's launchers around the packed extract): n > 0,
// n_hits in [1, 2^31 - 1], the host arrays judged (fm_range_args_bad).  An index built without extraction: no launch over the image,
// every ranged pattern gets FMX_ST_NOT_ENABLED and keeps no hit, unranged patterns are copied through.  kept, not_number, overflow
// and status are nullable device arrays of n ints.
struct NumberRangeOut {
    int64_t *kept_off;   // n + 1
    int32_t *kept_locs;  // room for n_hits
    int32_t *kept, *not_number, *overflow, *status;
};
int number_range_run(const ::fmx_index *idx, int n_cu, const TextView &text, int32_t n, const int32_t *term_len, const int64_t *num_lo,
                     const int64_t *num_hi, int32_t frac_digits, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits,
                     const NumberRangeOut &out, void *ws, size_t ws_bytes, void *stream);
// the value patterns' hits that pass the filter, into (kept_off: n + 1, kept_locs: room for total - term_hits): the lines of the
// queries where the call filters and has queries, then fmx_hits_in_lines_dev's launcher.  A call that does not filter runs it
// without a line table (every hit is kept), so an index without one still answers.  h.n > 0 and a value pattern has a hit.
int hits_in_lines_stage(const HitsBetween &h, const HitsFilter &f, int64_t *kept_off, int32_t *kept_locs);
// the same for a stage that reads the hits where they lie: (*d_off: n + 1, *d_locs, *n_hits slots) — the packed block's own part
// when the call does not filter, else what hits_in_lines_stage keeps, in blocks from block()
int kept_hits_stage(const HitsBetween &h, const HitsFilter &f, const int64_t **d_off, const int32_t **d_locs, int64_t *n_hits);

// ---- fmx_host_stage.cpp: what the stages of the feature files share ----------------------------------------------------------------
int hip_fail(const char *what, int e);  // FMX_E_HIP, "<what>: <the text of HIP error e>"
// the value patterns' statuses of a stage (h.status, h.n; nullable) = value, asynchronously
int status_all(const HitsBetween &h, int32_t value, const char *what);
// stage b of the keyed forms and fmx_values_of_hits_groups_dev behind its checks: the windows, their text, the groups and the group
// of every hit (n > 0, n_hits > 0, an index with extraction)
int values_groups_run(const ::fmx_index *idx, const LineView &view, const TextView &text, int32_t n, const int32_t *term_len, const uint16_t *stop,
                      int32_t n_stop, int32_t max_len, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, int64_t *d_val_off,
                      int32_t *d_count, int64_t *d_text_off, int32_t *d_group_of_hit, int32_t *d_status, void *ws, size_t ws_bytes, void *stream);
// the statistics arrays of the numbers stages, on the device or on the host: `cells` rows (pct: cells * P) and n counters per
// pattern; an array that is not wanted is nullptr
struct StatRows {
    int32_t *count;
    uint64_t *sum_lo, *sum_hi;
    int64_t *min, *max, *pct;
    int32_t *no_key, *not_number, *overflow;
};
// *d: device blocks from h.block for the arrays `wanted` has (nullptr: every one); pct only where P > 0
int stat_rows_blocks(const HitsBetween &h, const StatRows *wanted, size_t cells, size_t P, int32_t n, StatRows *d);
// the arrays `host` has, copied down asynchronously; the arrays `d` has, zeroed asynchronously
int stat_rows_down(const StatRows &host, const StatRows &d, size_t cells, size_t P, int32_t n, void *stream);
int stat_rows_zero(const StatRows &d, size_t cells, size_t P, int32_t n, void *stream);
// the ONE zeroed allocation of a host form's answer: region i holds bytes[i], each region at a multiple of 8, 8 spare bytes behind
// the last.  The caller owns it (fmx_free_buffer on region 0) once release() has run.
struct PackedResult {
    uint8_t *p = nullptr;
    std::vector<size_t> at;
    ~PackedResult() { free(p); }
    bool alloc(std::initializer_list<size_t> bytes);
    template <class T>
    T *region(size_t i) const { return reinterpret_cast<T *>(p + at[i]); }
    void release() { p = nullptr; }
};

// ---- fmx_host_stage.cpp: the keyed forms (statistics by key, and by key per bucket) ---------------------------------------------------
// what their host forms take besides their patterns and what they hand back per pattern (each output nullable) ...
struct KeyedCall {
    int32_t m, n;
    const int32_t *by_of;
    int32_t n_terms;
    const int32_t *query_off;
    const uint8_t *term_kind;
    int32_t q;
    const int32_t *key_where_of, *where_of;
    const uint16_t *stop;
    int32_t n_stop, max_len, frac_digits;
    const int32_t *permille;
    int32_t n_permille;
    int64_t **text_off;  // these eight point into the ONE allocation of the answer
    uint16_t **chars;
    int32_t **count;
    uint64_t **sum_lo, **sum_hi;
    int64_t **min, **max, **pct;
    int32_t *no_key, *not_number, *overflow, *occurrences, *kept, *status, *key_occurrences, *key_kept, *key_status, *term_status;
};
void keyed_null_results(const KeyedCall &c);     // the eight that are there = NULL
bool keyed_results_missing(const KeyedCall &c);  // one of the eight is not there
// ... and what their stage needs of that, and leaves on the host (arrived when the call has synchronised)
struct KeyedArgs {
    int32_t m = 0, n = 0;
    const int32_t *by_of = nullptr;
    HitsFilter filter{};
    std::vector<int32_t> where_all, term_len;  // m + n each: the key patterns', then the number patterns'
    const uint16_t *stop = nullptr;
    int32_t n_stop = 0, max_len = 0, frac_digits = 0;
    const int32_t *permille = nullptr;
    int32_t P = 0;
    TextView text{};
    std::vector<int64_t> kept_off, val_off;             // m + n + 1; m + 2: the group offsets, the units of the groups' text behind
    std::vector<int64_t> part_off;                      // the key part's and the number part's own offsets (copied to the device)
    std::vector<int32_t> no_key, not_number, overflow;  // n each
    PackedResult result;
};
// the checks of the HOST arrays the forms share (behind their own batches'); the handle's views (keys are per line: no line table
// is a refusal); *a from c with the window of the filter — false: n == 0, nothing is searched and the call is answered
int keyed_call_checks(const KeyedCall &c);
int keyed_call_views(const ::fmx_index *idx, TextView *text);
bool keyed_call_fill(const KeyedCall &c, int32_t line_lo, int32_t line_hi, KeyedArgs *a);
// the fill alone, for a form whose n == 0 is a call of its own (the pairs and their lines of fmx_number_stats_by_pair_batch)
void keyed_args_fill(const KeyedCall &c, int32_t line_lo, int32_t line_hi, KeyedArgs *a);
// the call over the merged batch terms | keys | numbers with `stage` (its argument: arg), then the per-pattern outputs of c
int keyed_call_run(const ::fmx_index *idx, const KeyedCall &c, const ValuesBatch &batch, ValuesBetweenFn stage, void *arg, const KeyedArgs &a);
// the host side of the statistics for stat_rows_down: count .. pct are regions first .. first + 5 of a.result, the counters a's
StatRows keyed_host_rows(KeyedArgs &a, size_t first);
// the caller's eight pointers: text_off, chars, count .. pct are regions first .. first + 7; the allocation is the caller's now
void keyed_hand_over(const KeyedCall &c, KeyedArgs &a, size_t first);
// the front half of their stages: the filter (kept_hits_stage), ONE read of the kept offsets, the two parts of the kept block with
// offsets of their own, stage a (the first hit of every line) over the keys' part, stage b (values_groups_run) over the first hits,
// ONE read of the m + 1 group offsets with the units of the groups' text behind them.  It leaves a.kept_off, a.val_off, K and N,
// and the device arrays below (blocks of h.block).  *done: answered, nothing more to run — no key or number hit, an index without
// extraction (FMX_ST_NOT_ENABLED), or K == 0: every kept number hit is a.no_key.
struct KeyedFront {
    int64_t K, N;                                      // the kept key hits, the kept number hits
    const int64_t *key_off, *num_off;                  // m + 1, n + 1: the parts' own offsets, from 0
    const int32_t *key_locs, *num_locs;
    int64_t *first_off;                                // m + 1
    int32_t *first_lines, *first_locs, *lines, *group;  // K slots each: stage a's lines and hits, stage b's count and group of hit
    int64_t *text_off;                                 // K + 1
    void *ws_b;                                        // stage b's workspace: launch_values_fill reads it
    size_t b_bytes;
};
int keyed_front_stage(const HitsBetween &h, KeyedArgs &a, const char *what, KeyedFront *f, bool *done);

// ---- fmx_host_stage.cpp: the forms over the groups of the kept hits (top values per bucket, distinct values per bucket) -------------
// what their stage needs of a call, and leaves on the host (arrived when the call has synchronised)
struct GroupsArgs {
    HitsFilter filter{};
    TextView text{};
    std::vector<int32_t> term_len;  // the value patterns'
    const uint16_t *stop = nullptr;
    int32_t n_stop = 0, max_len = 0;
    std::vector<int64_t> kept_off, part_off, val_off;  // n + 1, n + 1, n + 2 (the units of the groups' text behind, where asked for)
    void sized(int32_t n) {
        kept_off.assign((size_t)n + 1, 0);
        part_off.assign((size_t)n + 1, 0);
        val_off.assign((size_t)n + 2, 0);
    }
};
// the front half of their stages: the filter (kept_hits_stage), ONE read of the kept offsets, the kept block with offsets of its own
// that start at 0, fmx_values_of_hits_groups_dev over it, ONE read of the n + 1 group offsets — with `units` the units of the groups'
// text behind them (text_off[G], picked on the device).  It leaves a.kept_off, a.part_off, a.val_off, K and the device arrays below
// (blocks of h.block).  *done: answered, nothing more to run — no value pattern has a hit, an index without extraction
// (FMX_ST_NOT_ENABLED), or no hit is kept.
struct GroupsFront {
    int64_t K;                // the kept hits
    const int64_t *part_off;  // n + 1: the kept block's own offsets, from 0
    const int32_t *locs;
    int32_t *count, *group;   // K slots each: the groups' counts, the group of every hit
    int64_t *text_off;        // K + 1
    void *ws_b;               // the values stage's workspace: fmx_values_fill_dev reads it
    size_t b_bytes;
};
int groups_front_stage(const HitsBetween &h, GroupsArgs &a, bool units, const char *what, GroupsFront *f, bool *done);

}  // namespace fmx
