// fmx_plan.hpp — what the plan stage of a batch (fmx_kernels.hip: k_plan_codes, k_plan_scatter) hands to k_count, and the
// launchers of the .hip files that are compiled once.  Shared by the launchers and the C-ABI layer; what only the C-ABI layer
// sees — the views of a handle, the packed host sequence, the merged batch — lives in fmx_host_stage.hpp.
#pragma once

#include <cstddef>
#include <cstdint>

namespace fmx {

struct SortShape {
    int bits;         // bits per alphabet code
    int chars;        // trailing characters in the full key
    int total_bits;   // chars * bits (<= 32); with sa_key: bits of an SA row number of this index
    int coarse_bits;  // top bits used by the bucket pass
    int sa_key;       // 1: a pattern's key is the first SA row of its tabulated suffix (the suffix table's answer) — neighbours
                      // in that order read neighbouring BWT positions in their first step, and LF-mapping keeps rows that are
                      // preceded by the same character in order: the locality survives the steps; 0: the trailing characters'
                      // codes, the last character most significant (indexes without a suffix table)
};

struct CountPlan {
    const void *recs = nullptr;  // PlanRec[n] in processing order (device memory); nullptr = the caller's order
    int32_t n = 0;
    int code_bits = 8;           // width of one code in a record's code word (8, or 16 when sigma > 256)
    SortShape shape = {1, 1, 1, 1, 0};
    // the alphabet the code words are written in (the index the plan was made with): code -> char, alphabet size
    const int32_t *look_up = nullptr;
    int32_t sigma = 0;
    // *mixed == epoch: the batch holds patterns of different lengths (k_plan_codes stores the plan's epoch there when it sees
    // two lengths; never reset — the next plan has another epoch).  k_count regroups its workgroups by length only then.
    const uint32_t *mixed = nullptr;
    uint32_t epoch = 0;
    // k_count_lean's redo list (patterns that met a route it does not carry: room for n indices) and its counters {entries,
    // workgroups of the list pass that are done} — both zero between launches; nullptr = no room (the general k_count runs)
    int32_t *redo_list = nullptr;
    uint32_t *redo_count = nullptr;
};

// head of the plan workspace: histogram, cursors, ticket — all zero between plans (k_plan_scatter restores that)
constexpr size_t kPlanHeadBytes = 2 * ((size_t)4 << 14) + 256;

// fmx_hit_offsets.hip — the packed layout of fmx_locate_all_*: hit_off[i] = hits of patterns 0 .. i - 1 (n + 1 entries) from the
// {start, end} ranges of a batch.  It does not depend on the image form, so it is compiled once, outside the two namespaces of
// fmx_kernels.hip.  scratch: hit_offsets_scratch_bytes(n).  The launcher returns a hipError_t as int; `stream` a hipStream_t.
size_t hit_offsets_scratch_bytes(int32_t n);
int launch_hit_offsets(const int32_t *range, int32_t n, int32_t max_matches, int64_t *hit_off, void *scratch, size_t scratch_bytes,
                       void *stream);

// fmx_extract_packed.hip — the packed layout of fmx_extract_packed_*: status[i], text_off[i] = characters of ranges 0 .. i - 1 and
// piece_off[i] = their pieces (n + 1 entries each) from the ranges themselves.  It looks at the index's length, sample rate and
// enableExtract only.  scratch: extract_packed_scratch_bytes(n), ONE workspace for both stages of a call — the fill (declared in
// fmx_kernel_api.hpp: it walks the image) keeps its redo list {count, 0, 0, 0, ranges...} at extract_packed_redo and a flag per
// range at extract_packed_flags.  The launcher returns a hipError_t as int; `stream` a hipStream_t.
struct DevIndex;
size_t extract_packed_scratch_bytes(int32_t n);
int32_t *extract_packed_redo(void *scratch);
int32_t *extract_packed_flags(void *scratch, int32_t n);
int launch_extract_packed_offsets(const DevIndex &ix, const int32_t *start, const int32_t *stop, int32_t n, int64_t *text_off,
                                  int64_t *piece_off, int32_t *status, void *scratch, size_t scratch_bytes, void *stream);

// fmx_class_search.hip — what the class search (fmx_class_*) does outside the image: the exclusive scan of the patterns' range
// counts (stage 1 leaves them at class_ranges_counts of the workspace, n + 1 int64), the hit offsets of the patterns from those of
// their ranges (launch_hit_offsets over the m ranges, every hit, then one gather; scratch: hit_offsets_scratch_bytes(m)) and the
// fold of the ranges' walk statuses into their patterns'.  The launchers return a hipError_t as int; `stream` a hipStream_t.
size_t class_ranges_scratch_bytes(int32_t n);
int64_t *class_ranges_counts(void *scratch);
int launch_class_range_offsets(void *scratch, size_t scratch_bytes, int32_t n, int64_t *range_off, void *stream);
int launch_class_hit_offsets(const int32_t *ranges, int32_t m, const int64_t *range_off, int32_t n, int64_t *range_hit_off,
                             int64_t *hit_off, void *scratch, size_t scratch_bytes, void *stream);
int launch_class_fold_status(const int64_t *range_off, int32_t n, int32_t m, const int32_t *range_status, int32_t *status, void *stream);

// fmx_hit_lines.hip — the line table of a resident index and packed hits -> packed distinct lines (fmx_line_table_build,
// fmx_line_bounds_*, fmx_lines_of_hits_dev).  Compiled once, like fmx_hit_offsets.hip.  The launchers return a hipError_t as int;
// `stream` is a hipStream_t; nothing is synchronised or allocated.
// launch_line_table: T[0 .. count) = locs sorted ascending (scratch: line_table_scratch_bytes), *n_lines (device) = fm_line_total.
size_t line_table_scratch_bytes(int32_t count);
int launch_line_table(const int32_t *locs, int32_t count, int32_t text_len, int32_t *T, int64_t *n_lines, void *scratch, size_t scratch_bytes,
                      void *stream);
int launch_line_bounds(const int32_t *T, int32_t count, int64_t n_lines, int32_t text_len, int n_cu, const int32_t *ids, int32_t n,
                       int32_t *start, int32_t *stop, void *stream);
// the workspace of launch_lines_of_hits (0: nothing to do, or n_hits beyond 2^31 - 1); too small a workspace: hipErrorInvalidValue
// before anything is launched
size_t lines_of_hits_scratch_bytes(int32_t n, int64_t n_hits);
int launch_lines_of_hits(const int32_t *T, int32_t count, int n_cu, int32_t n, const int64_t *hit_off, const int32_t *locs, int64_t n_hits,
                         int32_t max_lines, int64_t *line_off, int32_t *lines, int32_t *line_count, void *ws, size_t ws_bytes, void *stream);
// workgroups per CU the grids stop at (the rest of the hits by grid-stride loops): k_hit_line_keys takes tiles of kLocateAllTile
// hits with 1,024 lanes, the element-wise kernels 256 lanes; hit_lines_geometry: the two grids of a call over n_hits hits
constexpr int kHitLinesKeyGroupsPerCu = 2, kHitLinesFlatGroupsPerCu = 8;
void hit_lines_geometry(int64_t n_hits, int n_cu, int32_t *key_grid, int32_t *flat_grid);

// fmx_query_lines.hip — packed hits of a batch of terms -> the packed distinct lines of each QUERY (fmx_query_lines_of_hits_dev).
// Compiled once.  query_off (q + 1) and term_kind (n) are HOST arrays the caller has validated; the tables made from them are
// copied into the workspace before the launcher returns.  The grids are hit_lines_geometry's.  hipErrorInvalidValue before anything
// is launched or written: too small a workspace, n_hits beyond 2^31 - 1, a key of more than 64 bits (fm_query_key_width).
size_t query_lines_scratch_bytes(int32_t n, int32_t q, int64_t n_hits);
int32_t query_lines_max_terms(int32_t q, const int32_t *query_off);  // the largest number of terms of one query
int launch_query_lines(const int32_t *T, int32_t count, int n_cu, int32_t n, int32_t q, const int32_t *query_off, const uint8_t *term_kind,
                       const int64_t *hit_off, const int32_t *locs, int64_t n_hits, int32_t max_lines, int64_t *line_off, int32_t *lines,
                       int32_t *line_count, void *ws, size_t ws_bytes, void *stream);

// fmx_sequence_lines.hip — packed hits of a batch of terms -> the packed lines of each SEQUENCE of terms in order
// (fmx_sequence_lines_of_hits_dev).  Compiled once.  query_off (q + 1) and term_len (n, none negative) are HOST arrays the caller
// has validated; the tables made from them are copied into the workspace before the launcher returns.  n_lines, text_len: the
// line bounds' (fm_line_bounds).  spans (nullable): two ints per stored line.  The grids are hit_lines_geometry's.
// hipErrorInvalidValue before anything is launched or written: too small a workspace, n_hits beyond 2^31 - 1.
size_t sequence_lines_scratch_bytes(int32_t n, int32_t q, int64_t n_hits);
int launch_sequence_lines(const int32_t *T, int32_t count, int64_t n_lines, int32_t text_len, int n_cu, int32_t n, int32_t q,
                          const int32_t *query_off, const int32_t *term_len, const int64_t *hit_off, const int32_t *locs, int64_t n_hits,
                          int32_t max_lines, int64_t *line_off, int32_t *lines, int32_t *line_count, int32_t *spans, void *ws, size_t ws_bytes,
                          void *stream);

// fmx_hit_values.hip — packed hits of a batch of patterns -> the distinct values that follow each pattern, with counts
// (fmx_values_of_hits_dev / fmx_values_fill_dev; fmx_hit_values.hpp has the definition).  Compiled once.  term_len (n, none
// negative) and stop (n_stop units) are HOST arrays the caller has validated; they are copied into the workspace before
// launch_values_ranges returns.  The C-ABI layer runs three steps on one stream over one workspace:
//   launch_values_ranges   pattern and window [s, e) of every hit, into the regions values_windows names;
//   the packed extract     launch_extract_packed_offsets and the image form's launch_extract_packed_fill over those n_hits ranges;
//   launch_values_groups   lengths, runs, the sorting passes, heads: val_off (n + 1), count and text_off (one per group, text_off one
//                          more), status (nullable: a window the extract ran literally hands its status to its pattern).
// launch_values_fill: the groups' code units into chars (groups = val_off[n], read by the caller).  The grids are hit_lines_geometry's.  hipErrorInvalidValue
// before anything is launched or written: too small a workspace, a shape outside values_of_hits_scratch_bytes' (which is 0 then).
struct ValuesWindows {
    int32_t *start, *stop, *status;
    int64_t *text_off, *piece_off;
    uint16_t *chars;
    void *scratch;
    size_t scratch_bytes;
};
size_t values_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t max_len);
bool values_windows(void *ws, size_t ws_bytes, int32_t n, int64_t n_hits, int32_t max_len, ValuesWindows *out);
int launch_values_ranges(int32_t text_len, int n_cu, int32_t n, const int32_t *term_len, const uint16_t *stop, int32_t n_stop, int32_t max_len,
                         const int64_t *hit_off, const int32_t *locs, int64_t n_hits, void *ws, size_t ws_bytes, void *stream);
int launch_values_groups(int n_cu, int32_t n, int32_t n_stop, int32_t max_len, int64_t n_hits, const int64_t *hit_off,
                         int64_t *val_off, int32_t *count, int64_t *text_off, int32_t *status, void *ws, size_t ws_bytes, void *stream);
int launch_values_fill(int n_cu, int64_t groups, const int64_t *text_off, uint16_t *chars, const void *ws, void *stream);
int launch_values_status_all(int n_cu, int32_t *status, int32_t n, int32_t value, void *stream);  // status[0, n) = value

// fmx_hit_filter.hip — packed hits -> the packed hits that lie in given lines, in the order they had (fmx_hits_in_lines_dev;
// fmx_hit_filter.hpp has the keep rule).  Compiled once.  where_of (n, each -1 .. q - 1) is a HOST array the caller has validated;
// it is copied into the workspace before the launcher returns.  T == nullptr (no line table): the caller holds every where_of
// negative and the window 0 .. INT32_MAX — every hit is kept, the block is moved to the front.  kept_locs must not overlap locs.
// The grids are hit_lines_geometry's.  hipErrorInvalidValue before anything is launched or written: too small a workspace,
// n_hits beyond 2^31 - 1.  n <= 0 or n_hits <= 0: nothing is done.
size_t hits_in_lines_scratch_bytes(int32_t n, int64_t n_hits);
int launch_hits_in_lines(const int32_t *T, int32_t count, int n_cu, int32_t n, const int32_t *where_of, const int64_t *line_off,
                         const int32_t *lines, int32_t line_lo, int32_t line_hi, const int64_t *hit_off, const int32_t *locs, int64_t n_hits,
                         int64_t *kept_off, int32_t *kept_locs, void *ws, size_t ws_bytes, void *stream);
// the stable store alone, for a stage that makes flags of its own (fmx_hit_range.hip): flag and pos = its exclusive scan, n_hits + 1
// int32 each, the flags in front of hit_off[0] and behind hit_off[n] being 0; flat_grid: hit_lines_geometry's over n_hits
int launch_hit_keep_store(int32_t flat_grid, const int32_t *flag, const int32_t *pos, const int64_t *hit_off, int32_t n, const int32_t *locs,
                          int64_t n_hits, int64_t *kept_off, int32_t *kept_locs, void *stream);

// fmx_hit_range.hip — packed hits -> the packed hits whose number lies in a range, in the order they had
// (fmx_hits_in_number_range_dev; fmx_hit_range.hpp has the definition).  Compiled once.  term_len (n, none negative), num_lo and
// num_hi (n int64 each; num_lo[i] < 0: pattern i is not ranged) are HOST arrays the caller has validated; they are copied into the
// workspace before launch_range_windows returns.  The C-ABI layer runs three steps on one stream over one workspace, as for the
// numbers stage:
//   launch_range_windows   pattern and window [s, e) of every slot, into the regions range_windows names — an empty window for a
//                          slot of an unranged pattern and for a slot that is no hit: the extract walks nothing for them;
//   the packed extract     extract_windows (fmx_host_stage.hpp) over those n_hits ranges; skipped with extract == false;
//   launch_range_keep      the codes (extract == false: a ranged pattern keeps nothing and gets the status not_enabled), the two
//                          exclusive scans, launch_hit_keep_store, and a lane per pattern for kept, not_number and overflow (each
//                          nullable); status (nullable): a window the extract ran literally hands its status to its pattern.
// The grids are hit_lines_geometry's.  hipErrorInvalidValue before anything is launched or written: too small a workspace, n <= 0,
// n_hits <= 0 or beyond 2^31 - 1, frac_digits outside [0, 9].
size_t hits_in_number_range_scratch_bytes(int32_t n, int64_t n_hits);
bool range_windows(void *ws, size_t ws_bytes, int32_t n, int64_t n_hits, ValuesWindows *out);
int launch_range_windows(int32_t text_len, int n_cu, int32_t n, const int32_t *term_len, const int64_t *num_lo, const int64_t *num_hi,
                         const int64_t *hit_off, const int32_t *locs, int64_t n_hits, void *ws, size_t ws_bytes, void *stream);
int launch_range_keep(int n_cu, int32_t n, bool extract, int32_t not_enabled, int32_t frac_digits, const int64_t *hit_off, const int32_t *locs,
                      int64_t n_hits, int64_t *kept_off, int32_t *kept_locs, int32_t *kept, int32_t *not_number, int32_t *overflow,
                      int32_t *status, void *ws, size_t ws_bytes, void *stream);

// fmx_line_hist.hip — matching lines and hits per bucket of lines (fmx_lines_histogram_dev, fmx_hits_histogram_dev;
// fmx_line_hist.hpp has the definitions).  Compiled once.  edges (n_edges >= 2, edges[0] >= 0, never decreasing) is a HOST array; it
// is judged again and copied into the workspace before the launcher returns.  hist gets rows * (n_edges - 1) int32, nothing behind
// them.  The grids are hit_lines_geometry's.  hipErrorInvalidValue before anything is launched or written: too small a workspace,
// bad edges, rows * B beyond 2^27, n_hits beyond 2^31 - 1, no line table (hits form).  q <= 0, n <= 0 or n_hits <= 0: nothing is done.
size_t lines_histogram_scratch_bytes(int32_t q, int32_t n_edges);
size_t hits_histogram_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_edges);
int launch_lines_histogram(int n_cu, int32_t q, const int64_t *line_off, const int32_t *lines, const int32_t *edges, int32_t n_edges,
                           int32_t *hist, void *ws, size_t ws_bytes, void *stream);
int launch_hits_histogram(const int32_t *T, int32_t count, int n_cu, int32_t n, const int64_t *hit_off, const int32_t *locs, int64_t n_hits,
                          const int32_t *edges, int32_t n_edges, int32_t *hist, void *ws, size_t ws_bytes, void *stream);

// fmx_hit_numbers.hip — packed hits of a batch of patterns -> statistics of the number behind each hit, per bucket of lines
// (fmx_numbers_of_hits_dev; fmx_hit_numbers.hpp has the definition).  Compiled once.  term_len (n, none negative), edges (n_edges >= 2
// by fmx_line_hist.hpp's rules, or none at all: n_edges == 0, B = 1, no line table needed) and permille (n_permille <= 16, each in
// [0, 1000]) are HOST arrays; they are judged again and copied into the workspace before launch_numbers_ranges returns.  The C-ABI
// layer runs three steps on one stream over one workspace, as for the values stage:
//   launch_numbers_ranges  window [s, e) and key pattern | bucket of every slot, into the regions numbers_windows names;
//   the packed extract     extract_windows (fmx_host_stage.hpp) over those n_hits ranges;
//   launch_numbers_rows    the parse, the two sorts, the two running sums, the rows (count is required, every other output
//                          nullable) and the per-pattern counters; status (nullable): a window the extract ran literally hands its
//                          status to its pattern.
// The grids are hit_lines_geometry's.  hipErrorInvalidValue before anything is launched or written: too small a workspace, a shape
// outside numbers_of_hits_scratch_bytes' (which is 0 then).
bool numbers_shape_ok(int32_t n, int64_t n_hits, int32_t n_edges, int32_t n_permille);
size_t numbers_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_edges, int32_t n_permille);
bool numbers_windows(void *ws, size_t ws_bytes, int32_t n, int64_t n_hits, int32_t n_edges, int32_t n_permille, ValuesWindows *out);
int launch_numbers_ranges(const int32_t *T, int32_t count, int32_t text_len, int n_cu, int32_t n, const int32_t *term_len, const int64_t *hit_off,
                          const int32_t *locs, int64_t n_hits, const int32_t *edges, int32_t n_edges, const int32_t *permille, int32_t n_permille,
                          void *ws, size_t ws_bytes, void *stream);
int launch_numbers_rows(int n_cu, int32_t n, const int64_t *hit_off, int64_t n_hits, int32_t n_edges, int32_t frac_digits, int32_t n_permille,
                        int32_t *count, uint64_t *sum_lo, uint64_t *sum_hi, int64_t *min, int64_t *max, int64_t *pct, int32_t *not_number,
                        int32_t *overflow, int32_t *status, void *ws, size_t ws_bytes, void *stream);


// "STATS ... BY KEY" (fmx_hit_by.hpp has the definition): the three stages of fmx_first_hits_of_lines_dev,
// fmx_values_of_hits_groups_dev and fmx_numbers_by_key_dev.  Each compiled once; the grids are hit_lines_geometry's; the launchers
// return a hipError_t as int, `stream` is a hipStream_t, nothing is synchronised or allocated.  hipErrorInvalidValue before anything
// is launched or written: too small a workspace, a shape outside the stage's scratch-size function (which is 0 then).
// fmx_hit_first.hip — packed hits of m patterns -> first_off (m + 1), first_lines and first_locs (first_off[m] entries each, nothing
// behind them): per pattern its distinct lines ascending, each with the smallest position of a hit on it.  T: the line table (required).
size_t first_hits_scratch_bytes(int32_t m, int64_t n_hits);
int launch_first_hits(const int32_t *T, int32_t count, int32_t text_len, int n_cu, int32_t m, const int64_t *hit_off, const int32_t *locs,
                      int64_t n_hits, int64_t *first_off, int32_t *first_lines, int32_t *first_locs, void *ws, size_t ws_bytes, void *stream);
// fmx_hit_values.hip — launch_values_groups with one more output: group_of_hit (n_hits ints) = the index of each hit's group within
// its pattern, -1 for a slot that is no hit.  Its workspace is larger than launch_values_groups' (a group per run behind it); the
// ranges and the fill are launch_values_ranges / launch_values_fill over the same workspace, values_windows over its front part.
size_t values_groups_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t max_len);
int launch_values_groups_of_hits(int n_cu, int32_t n, int32_t n_stop, int32_t max_len, int64_t n_hits, const int64_t *hit_off, int64_t *val_off,
                                 int32_t *count, int64_t *text_off, int32_t *status, int32_t *group_of_hit, void *ws, size_t ws_bytes,
                                 void *stream);
// fmx_hit_numbers.hip — the numbers stage with the code of a hit = the group of its line's key.  term_len, by_of (n, each in [0, m)),
// val_off (m + 1: the key patterns' group offsets, stage b's answer read by the caller) and permille are HOST arrays, judged again
// (fm_by_rows_bad) and copied into the workspace before launch_numbers_by_key_ranges returns; row_off_out (device, n + 1; nullable)
// gets the rows' offsets.  Three steps on one stream over one workspace, as launch_numbers_ranges / extract_windows /
// launch_numbers_rows; count is required when there are rows, every other output nullable.
size_t numbers_by_key_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_permille);
bool numbers_by_key_windows(void *ws, size_t ws_bytes, int32_t n, int64_t n_hits, int32_t n_permille, ValuesWindows *out);
int launch_numbers_by_key_ranges(const int32_t *T, int32_t count, int32_t text_len, int n_cu, int32_t n, const int32_t *term_len,
                                 const int32_t *by_of, int32_t m, const int64_t *val_off, const int64_t *hit_off, const int32_t *locs,
                                 int64_t n_hits, const int64_t *first_off, const int32_t *first_lines, const int32_t *group_of_first,
                                 const int32_t *permille, int32_t n_permille, int64_t *row_off_out, void *ws, size_t ws_bytes, void *stream);
int launch_numbers_by_key_rows(int n_cu, int32_t n, const int32_t *by_of, int32_t m, const int64_t *val_off, const int64_t *hit_off,
                               int64_t n_hits, int32_t frac_digits, int32_t n_permille, int32_t *count, uint64_t *sum_lo, uint64_t *sum_hi,
                               int64_t *min, int64_t *max, int64_t *pct, int32_t *no_key, int32_t *not_number, int32_t *overflow,
                               int32_t *status, void *ws, size_t ws_bytes, void *stream);

// fmx_hit_pairs.hip — "STATS ... BY TWO KEYS" (fmx_pairs_of_first_hits_dev; fmx_hit_pairs.hpp has the definition): stage a's and b's
// answers joined through the line.  Compiled once; the grids are hit_lines_geometry's over n_slots; the launcher returns a
// hipError_t as int, `stream` is a hipStream_t, nothing is synchronised or allocated.  val_off (m + 1), pair_a and pair_b (c, each in
// [0, m)) are HOST arrays, judged again (fm_pair_args_bad) and copied into the workspace before the launcher returns.  n_slots: at
// least the first hits of the a-sides, pair after pair.  pair_off and joined_off get c + 1 entries; pair_group_a, pair_group_b and
// pair_lines pair_off[c] entries, joined_lines and joined_group joined_off[c], nothing behind them (each has room for n_slots).
// hipErrorInvalidValue before anything is launched or written: too small a workspace, a shape outside the scratch-size function's
// (which is 0 then: m, c or n_slots <= 0, n_slots beyond 2^31 - 1), a key of more than 64 bits.
size_t pairs_of_first_hits_scratch_bytes(int32_t m, int32_t n_pairs, int64_t n_slots);
int launch_pairs_of_first_hits(int n_cu, int32_t m, const int64_t *val_off, int32_t c, const int32_t *pair_a, const int32_t *pair_b,
                               const int64_t *first_off, const int32_t *first_lines, const int32_t *group_of_first, int64_t n_slots,
                               int64_t *pair_off, int32_t *pair_group_a, int32_t *pair_group_b, int32_t *pair_lines, int64_t *joined_off,
                               int32_t *joined_lines, int32_t *joined_group, void *ws, size_t ws_bytes, void *stream);

// fmx_value_hist.hip — THE TOP VALUES OF A FIELD PER BUCKET OF LINES (fmx_values_top_histogram_dev, fmx_values_gather_rows_dev;
// fmx_value_hist.hpp has the definition).  Compiled once; the grids are hit_lines_geometry's; the launchers return a hipError_t as
// int, `stream` is a hipStream_t, nothing is synchronised or allocated.  val_off (n + 1: the values stage's group offsets, read by the
// caller, val_off[0] = 0) and edges (n_edges >= 2 by fmx_line_hist.hpp's rules, or none at all: n_edges == 0, B = 1, T not needed)
// are HOST arrays; they are judged again (fm_vh_shape_bad) and copied into the workspace before the launcher returns.
// hipErrorInvalidValue before anything is launched or written: too small a workspace, a shape outside the scratch-size function's
// (which is 0 then), top outside [1, 65536], n * (top + 1) * B beyond 2^27.  n <= 0 or n_hits <= 0: nothing is done.
// launch_values_top_histogram: group_count (G = val_off[n] ints) and group_of_hit (n_hits ints) are launch_values_groups_of_hits'
// over the same packed hits; row_off_out (n + 1), row_group and row_count (R each), hist (R * B), other (n * B): nothing behind them.
size_t values_top_histogram_scratch_bytes(int32_t n, int64_t n_groups, int64_t n_hits, int32_t n_edges);
int launch_values_top_histogram(const int32_t *T, int32_t count, int n_cu, int32_t n, const int64_t *val_off, int32_t top, const int32_t *edges,
                                int32_t n_edges, const int64_t *hit_off, const int32_t *locs, int64_t n_hits, const int32_t *group_count,
                                const int32_t *group_of_hit, int64_t *row_off_out, int32_t *row_group, int32_t *row_count, int32_t *hist,
                                int32_t *other, void *ws, size_t ws_bytes, void *stream);
// launch_values_gather_rows: the text of the R rows (row r of pattern p: group val_off[p] + row_group[r]) out of the text of ALL
// groups (text_off: G + 1, chars: launch_values_fill's) into row_text_off (R + 1) and row_chars; max_units: a bound of the packed
// length that sizes the grid (the units of all groups will do); nothing is stored behind row_text_off[R] units.
// launch_values_groups_units: *out (device) = text_off[val_off[n]], the code units of all groups' text (val_off, text_off: the values
// stage's, on the device), so that ONE read brings the group offsets and that size down
int launch_values_groups_units(const int64_t *val_off, int32_t n, const int64_t *text_off, int64_t *out, void *stream);
size_t values_gather_rows_scratch_bytes(int32_t n, int64_t n_rows);
int launch_values_gather_rows(int n_cu, int32_t n, const int64_t *val_off, int32_t top, int64_t max_units, const int32_t *row_group,
                              const int64_t *text_off, const uint16_t *chars, int64_t *row_text_off, uint16_t *row_chars, void *ws,
                              size_t ws_bytes, void *stream);

// fmx_distinct.hip — THE DISTINCT VALUES OF A FIELD PER BUCKET OF LINES (fmx_values_distinct_histogram_dev; fmx_distinct.hpp has the
// definition).  Compiled once; the grids are hit_lines_geometry's; the launcher returns a hipError_t as int, `stream` is a
// hipStream_t, nothing is synchronised or allocated.  val_off and edges are HOST arrays as launch_values_top_histogram takes them,
// judged again (fm_dv_shape_bad) and copied into the workspace before the launcher returns; group_of_hit (n_hits ints) is
// launch_values_groups_of_hits' over the same packed hits; distinct and first_seen: n * B ints each, nothing behind them.
// hipErrorInvalidValue before anything is launched or written: too small a workspace, a shape outside the scratch-size function's
// (which is 0 then), n * B beyond 2^27.  n <= 0 or n_hits <= 0: nothing is done.
size_t values_distinct_histogram_scratch_bytes(int32_t n, int64_t n_groups, int64_t n_hits, int32_t n_edges);
int launch_values_distinct_histogram(const int32_t *T, int32_t count, int n_cu, int32_t n, const int64_t *val_off, const int32_t *edges,
                                     int32_t n_edges, const int64_t *hit_off, const int32_t *locs, int64_t n_hits, const int32_t *group_of_hit,
                                     int32_t *distinct, int32_t *first_seen, void *ws, size_t ws_bytes, void *stream);

// fmx_by_hist.hip — "STATS ... BY KEY" PER BUCKET OF LINES (fmx_numbers_by_key_buckets_dev; fmx_by_hist.hpp has the definition).
// Compiled once; the grids are hit_lines_geometry's; the launchers return a hipError_t as int, `stream` is a hipStream_t, nothing is
// synchronised or allocated.  term_len, by_of (n, each in [0, m)), val_off (m + 1: the key patterns' group offsets, stage b's answer
// read by the caller, val_off[0] = 0), edges (n_edges >= 2 by fmx_line_hist.hpp's rules, or none at all: n_edges == 0, B = 1) and
// permille are HOST arrays, judged again (fm_bh_shape_bad) and copied into the workspace before launch_by_hist_codes returns.  Three
// steps on one stream over one workspace, as launch_numbers_by_key_ranges / extract_windows / launch_numbers_by_key_rows:
//   launch_by_hist_codes   the rank of every group by its lines (group_lines: stage b's counts, G ints), the key rows
//                          (key_row_off_out: m + 1, key_row_group and key_row_lines: R = the sum of min(top, G_k); cell_off_out:
//                          n + 1; the two offset arrays nullable), then window [s, e) and key pattern | code of every slot, into the
//                          regions numbers_by_key_buckets_windows names; n_hits == 0: the key rows alone;
//   the packed extract     extract_windows (fmx_host_stage.hpp) over those n_hits ranges;
//   launch_by_hist_cells   launch_numbers_sorted, the cells (count is required, every other output nullable) and the per-pattern
//                          counters; status (nullable) as in launch_numbers_rows.  n_hits > 0.
// hipErrorInvalidValue before anything is launched or written: too small a workspace, a shape outside the scratch-size function's
// (which is 0 then), top outside [1, 65536], n * (top + 1) * B beyond 2^27 (or that times max(n_permille, 1)).
// launch_numbers_sorted (fmx_hit_numbers.hip): that file's k_num_parse over the windows' text and the keys pattern | code in key_a
// (codes in [0, B]; code_bits = fm_num_code_bits(B)), its two stable sorts (key_a / val_a leave sorted by (key, value)) and, with
// `sums`, its two running sums of the values' halves (low in val_b, high in key_b); tmp: numbers_sorted_tmp_bytes(n_hits).
size_t numbers_sorted_tmp_bytes(int64_t n_hits);
int launch_numbers_sorted(int n_cu, int32_t n, int64_t n_hits, int32_t B, int32_t frac_digits, const int64_t *win_off, const uint16_t *win,
                          const int32_t *win_status, uint64_t *key_a, uint64_t *key_b, uint64_t *val_a, uint64_t *val_b, bool sums, int32_t *status,
                          void *tmp, size_t tmp_bytes, void *stream);
size_t numbers_by_key_buckets_scratch_bytes(int32_t n, int32_t m, int64_t n_groups, int64_t n_hits, int32_t n_edges, int32_t n_permille);
bool numbers_by_key_buckets_windows(void *ws, size_t ws_bytes, int32_t n, int32_t m, int64_t n_groups, int64_t n_hits, int32_t n_edges,
                                    int32_t n_permille, ValuesWindows *out);
int launch_by_hist_codes(const int32_t *T, int32_t count, int32_t text_len, int n_cu, int32_t n, const int32_t *term_len, const int32_t *by_of,
                         int32_t m, const int64_t *val_off, int32_t top, const int32_t *edges, int32_t n_edges, const int64_t *hit_off,
                         const int32_t *locs, int64_t n_hits, const int64_t *first_off, const int32_t *first_lines, const int32_t *group_of_first,
                         const int32_t *group_lines, const int32_t *permille, int32_t n_permille, int64_t *key_row_off_out,
                         int32_t *key_row_group, int32_t *key_row_lines, int64_t *cell_off_out, void *ws, size_t ws_bytes, void *stream);
int launch_by_hist_cells(int n_cu, int32_t n, const int32_t *by_of, int32_t m, const int64_t *val_off, int32_t top, int32_t n_edges,
                         const int64_t *hit_off, int64_t n_hits, int32_t frac_digits, int32_t n_permille, int32_t *count, uint64_t *sum_lo,
                         uint64_t *sum_hi, int64_t *min, int64_t *max, int64_t *pct, int32_t *no_key, int32_t *not_number, int32_t *overflow,
                         int32_t *status, void *ws, size_t ws_bytes, void *stream);

// fmx_hit_top.hip — packed hits of a batch of patterns -> the lines ranked by the number behind each hit (fmx_top_lines_of_hits_dev;
// fmx_hit_top.hpp has the definition).  Compiled once; the grids are hit_lines_geometry's; the launchers return a hipError_t as int,
// `stream` is a hipStream_t, nothing is synchronised or allocated.  term_len (n, none negative) and descending (n bytes) are HOST
// arrays; they are copied into the workspace before launch_top_lines_windows returns.  The C-ABI layer runs three steps on one
// stream over one workspace, as for the numbers stage:
//   launch_top_lines_windows  window [s, e) and key pattern | position of every slot, into the regions top_lines_windows names;
//   the packed extract        extract_windows (fmx_host_stage.hpp) over those n_hits ranges;
//   launch_top_lines_rows     the parse, the sort by position, the lines, the reduction per (pattern, line), the two ranking sorts,
//                             the per-pattern counters (rows is required, every other output nullable) and the rows of n x top;
//                             status (nullable): a window the extract ran literally hands its status to its pattern.  T: the line
//                             table (required).
// hipErrorInvalidValue before anything is launched or written: too small a workspace, a shape outside
// top_lines_of_hits_scratch_bytes' (which is 0 then: n <= 0, n_hits <= 0 or beyond 2^31 - 1, top < 1, n * top beyond 2^27).
bool top_lines_shape_ok(int32_t n, int64_t n_hits, int32_t top);
size_t top_lines_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t top);
bool top_lines_windows(void *ws, size_t ws_bytes, int32_t n, int64_t n_hits, int32_t top, ValuesWindows *out);
int launch_top_lines_windows(int32_t text_len, int n_cu, int32_t n, const int32_t *term_len, const uint8_t *descending, const int64_t *hit_off,
                             const int32_t *locs, int64_t n_hits, int32_t top, void *ws, size_t ws_bytes, void *stream);
int launch_top_lines_rows(const int32_t *T, int32_t count, int32_t text_len, int n_cu, int32_t n, const int64_t *hit_off, int64_t n_hits,
                          int32_t frac_digits, int32_t first, int32_t top, int32_t *rows, int32_t *row_line, int64_t *row_value, int32_t *row_loc,
                          int32_t *lines, int32_t *numbers, int32_t *not_number, int32_t *overflow, int32_t *status, void *ws, size_t ws_bytes,
                          void *stream);

}  // namespace fmx
