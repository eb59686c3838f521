// fmx_kernel_api.hpp — the launchers of fmx_kernels.hip, as the C-ABI layer calls them.
//
// NO include guard, on purpose: the file is included INSIDE a namespace, more than once.  fmx_kernels.hip is compiled twice
// (namespace fmx for expanded images, fmxc for compact ones) and includes it inside the namespace it defines, so that every
// definition sees its prototype; fmx_api.cpp includes it once inside `namespace fmx` and once inside `namespace fmxc`.
// Needs fmx_device.hpp, fmx_plan.hpp and <hip/hip_runtime.h> in front.  Every launcher returns a hipError_t as int.

// growing the suffix table, the window directory and the row table of an index that becomes resident
int launch_suffix_level1(const fmx::DevIndex &ix, fmx::SuffixSlot *out, uint32_t *count, uint32_t cap, hipStream_t st);
int launch_suffix_expand(const fmx::DevIndex &ix, int n_cu, const fmx::SuffixSlot *in, uint32_t n_in, int depth, int key_bits,
                         fmx::SuffixSlot *out, uint32_t *count, uint32_t cap, hipStream_t st);
int launch_suffix_insert(const fmx::DevIndex &geometry, const fmx::SuffixSlot *in, uint32_t n_in, int len, fmx::SuffixSlot *slots,
                         hipStream_t st);
int launch_suffix_order1(const fmx::DevIndex &ix, float *out, hipStream_t st);
// ... its deepest level as child lists: parents' slots and counts, exclusive scan (one workgroup), runs per parent, sorted runs and
// their entries, the lists themselves
int launch_suffix_child_parents(const fmx::DevIndex &hashed, const fmx::SuffixSlot *kids, uint32_t n_kids, int len,
                                fmx::SuffixSlot *table, uint32_t *kid_slot, uint32_t *per_slot, hipStream_t st);
int launch_suffix_child_scan(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *total, hipStream_t st);
int launch_suffix_child_place(const fmx::SuffixSlot *kids, uint32_t n_kids, const uint32_t *kid_slot, uint32_t *cursor,
                              fmx::SuffixSlot *placed, hipStream_t st);
int launch_suffix_child_sort(uint32_t slots, const uint32_t *per_slot, const uint32_t *run_end, fmx::SuffixSlot *placed,
                             uint32_t *entries, hipStream_t st);
int launch_suffix_child_write(uint32_t slots, const uint32_t *per_slot, const uint32_t *run_end, const fmx::SuffixSlot *placed,
                              const uint32_t *first, fmx::SuffixSlot *table, uint32_t *rows, uint8_t *codes, hipStream_t st);
int launch_win_build(const fmx::DevIndex &ix, int n_cu, uint32_t n_win, fmx::Quad *out, uint32_t *others, hipStream_t st);
int launch_win_other(const fmx::DevIndex &ix, int n_cu, uint32_t n_win, fmx::Quad *cells, const uint32_t *first, uint16_t *entries,
                     uint32_t *open_entries, int entry4, uint64_t *full, uint32_t full_cap, hipStream_t st);
int launch_win_flat(const fmx::DevIndex &ix, int n_cu, uint32_t n_pos, uint32_t *flat, uint32_t *tail, uint64_t *full,
                    uint32_t full_cap, hipStream_t st);
int launch_rows_fill(const fmx::DevIndex &ix, int n_cu, uint32_t n_rows, uint32_t *rows, uint32_t *replay, hipStream_t st);

// count
size_t count_workspace_bytes(const fmx::DevIndex &ix, int32_t n);
int launch_count_plan(const fmx::DevIndex &ix, int n_cu, const uint16_t *pat, const int32_t *off, int32_t n, void *workspace,
                      size_t workspace_bytes, bool head_is_zero, fmx::CountPlan *plan, hipStream_t st);
int launch_count(const fmx::DevIndex &ix, int n_cu, const uint16_t *pat, const int32_t *off, const fmx::CountPlan *plan,
                 bool plan_is_foreign, int32_t n, int32_t *counts, int32_t *lf, int32_t *status, int32_t *range, hipStream_t st);

// locate
size_t walk_workspace_bytes(const fmx::DevIndex &ix, int32_t n);
int launch_locate_walk(const fmx::DevIndex &ix, int n_cu, const int32_t *range, int32_t n, int32_t max_matches, int32_t *locs,
                       int32_t loc_cap, int32_t *found, int32_t *lf, int32_t *status, const int32_t *taken, void *workspace,
                       size_t workspace_bytes, bool head_is_zero, hipStream_t st, int64_t *set_locs, int64_t set_base);
// "all occurrences", packed: hits [first_hit, first_hit + n_hits) of the layout hit_off describes (n + 1 entries), cut at hit_off[n]
int launch_locate_all(const fmx::DevIndex &ix, int n_cu, const int32_t *range, const int64_t *hit_off, int32_t n, int64_t first_hit,
                      int64_t n_hits, int32_t *locs, int32_t *lf, int32_t *status, hipStream_t st);

// extract, extractUntilBoundary
int launch_extract(const fmx::DevIndex &ix, int n_cu, const int32_t *start, const int32_t *stop, int64_t n, uint16_t *dst,
                   int32_t dst_len, int32_t offset, int32_t *out_len, int32_t *lf, int32_t *status, const int32_t *slot_found,
                   int32_t slots, int32_t fixed_len, void *order_ws, size_t order_ws_bytes, bool head_is_zero, hipStream_t st);
size_t boundary_workspace_bytes(const fmx::DevIndex &ix, int64_t n, int n_cu);
size_t boundary_order_bytes(const fmx::DevIndex &ix, int64_t n);
int launch_extract_boundary(const fmx::DevIndex &ix, int n_cu, const int32_t *from, int64_t n, uint16_t boundary, int mode,
                            uint16_t *dst, int32_t dst_len, int32_t offset, int32_t *out_len, int32_t *lf, int32_t *status,
                            int32_t *aux, void *workspace, size_t workspace_bytes, const int32_t *slot_found, int32_t slots,
                            void *order_ws, size_t order_ws_bytes, bool head_is_zero, hipStream_t st);

// extract, packed (fmx_extract_packed.hip, compiled per image form like fmx_kernels.hip): the pieces of the layout text_off /
// piece_off describe into chars, then the ranges a piece put on the redo list, literally.  redo / flags: fmx_plan.hpp
int launch_extract_packed_fill(const fmx::DevIndex &ix, int n_cu, const int32_t *start, const int32_t *stop, int32_t n,
                               const int64_t *text_off, const int64_t *piece_off, int64_t pieces, uint16_t *chars, int32_t *status,
                               int32_t *redo, int32_t *flags, hipStream_t st);

// class patterns (fmx_class_search.hip, compiled per image form like fmx_kernels.hip): the frontier search of a batch.  Stage 1
// (ranges == nullptr): range_cnt = n + 1 int64 (class_ranges_counts of the call's workspace: fmx_plan.hpp), counts / status
// nullable; stage 2: the ranges of pattern i at range_off[i]
int launch_class_search(const fmx::DevIndex &ix, int n_cu, const uint16_t *alt, const int32_t *pos_off, const int32_t *pat_off, int32_t n,
                        int32_t max_ranges, int64_t *range_cnt, int32_t *counts, int32_t *status, const int64_t *range_off,
                        int32_t *ranges, hipStream_t st);

// the stand-alone structures: RrrVector, WaveletFixedBlockBoosting
int launch_rrr_rank_ones(const fmx::DevIndex &ix, int n_cu, const int32_t *pos, int32_t n, int32_t *out, hipStream_t st);
int launch_rrr_access(const fmx::DevIndex &ix, int n_cu, const int32_t *pos, int32_t n, uint8_t *out, int32_t *status,
                      hipStream_t st);
int launch_wt_rank(const fmx::DevIndex &ix, int n_cu, const int64_t *pos, const int32_t *sym, int32_t n, int64_t *out,
                   int32_t *status, hipStream_t st);
int launch_wt_inverse_select(const fmx::DevIndex &ix, int n_cu, const int64_t *pos, int32_t n, int64_t *out, int32_t *status,
                             hipStream_t st);

// merging the answers of a segment set
int launch_fill_offsets(int32_t *off, int32_t first, int32_t m, int32_t count, hipStream_t st);
int launch_segment_add_counts(int64_t *total, int64_t *lf_total, int32_t *status_total, const int32_t *counts, const int32_t *lf,
                              const int32_t *status, int32_t n, int first, hipStream_t st);
int launch_segment_append_hits(int64_t *locs, int32_t *found, int32_t *status_total, const int32_t *seg_locs,
                               const int32_t *seg_found, const int32_t *seg_status, int32_t n, int32_t cap, int64_t base, int first,
                               hipStream_t st);
int launch_segment_commit(int32_t *found, int32_t *status_total, const int32_t *seg_found, const int32_t *seg_status, int32_t n,
                          int32_t cap, int first, hipStream_t st);
