// fmx_options.cpp — the table of fmx_set_option's options: the complete list, with defaults and accepted values.
// A row is ONE source line `{"name", default, where it is stored, what it accepts, "description"}` (tests/test_option_ranges.py
// reads names and defaults from these lines and compares them with its own list).  The notes above a row record why its default
// is what it is.  "Afterwards" = the option is read when an index is flattened / becomes resident, not by later launches.
#include "fmx_options.hpp"

#include <string_view>

#include "fmx_model.hpp"

namespace fmx {
namespace {

bool is_block(int v) { return v == 512 || v == 1024; }
bool is_boundary_group(int v) { return v == 0 || v == 1 || v == 2 || v == 4 || v == 8 || v == 16; }
bool is_first_fill(int v) { return v == 0 || v == 2; }  // (1, half-width windows, was measured slower in round 3 and is gone)
bool is_entry_bytes(int v) { return v == 0 || v == 4 || v == 6; }
bool is_fence_count(int v) { return v >= 0 && v <= 32768 && !(v & (v - 1)); }  // a power of two, or 0

using O = Options;
constexpr Accept any = range(INT_MIN, INT_MAX);

constexpr OptionRow kOptions[] = {
    // ---- launch shape: the FM kernels (both image forms) and the suffix-array kernels ----
    {"block", 512, &O::block, one_of(is_block), "threads per workgroup"},
    {"groups_per_cu", 16, &O::groups_per_cu, range(1, 64), "grid cap: workgroups per CU, the rest grid-stride"},
    {"lds_pad_kb", 0, &O::lds_pad_kb, range(0, 96), "experiment knob: extra dynamic LDS per workgroup (lowers occupancy)"},

    // ---- count() and its plan stage ----
    {"sort_min", 16384, &O::sort_min, at_least(0), "batches at least this large are processed in suffix-sorted order (0 = never)"},
    {"sort_bits", 28, &O::sort_bits, range(1, 32), "full key width: floor(sort_bits / bits-per-code) trailing characters"},
    // bins of the bucket pass = 2^coarse_bits (k_plan_scatter keeps two arrays of 2^bits words in LDS).  Measured on configs[1]
    // (tools/tune_coarse.py): 14 bits: plan 0.091 ms, step 0.304 ms; 12 bits: 0.075 / 0.286 ms; 10 bits: 0.071 / 0.286 ms;
    // 8 bits: 0.069 / 0.294 ms
    {"coarse_bits", 12, &O::coarse_bits, range(4, kCoarseBitsMax - 1), "bins of the plan stage's bucket pass = 2^coarse_bits"},
    {"plan_fine", 1, &O::plan_fine, range(0, 2), "the window-local fine order: 0 = skipped (A/B), 1 = unless ordered by SA row, 2 = always"},
    {"plan_sa_key", 2, &O::plan_sa_key, range(0, 2), "order by: 0 = the trailing characters' codes, 1 = the SA row the suffix table answers, 2 = an estimate of that row (SortShape.sa_key)"},
    {"plan_sa_min", 786432, &O::plan_sa_min, at_least(0), "under plan_sa_key != 0: smallest batch over a suffix table that is planned (plan_pays)"},
    // The plan stage (suffix order of a batch) pays while MANY patterns share the table string they start from — their first
    // steps then read the same lines.  Measured (tools/depth_sort_probe.py, tools/nosort_probe.py): 1 M patterns over 26 K strings
    // (depth 4): planned 0.168 ms, caller's order 0.179; over 227 K strings (depth 5): 0.150 / 0.141; 65,536 patterns over
    // 227 K: 0.045 / 0.023.
    {"plan_min_per_string", 16, &O::plan_min_per_string, at_least(0), "under plan_sa_key = 0: planned only with this many patterns per string of the table's deepest level (0 = always)"},
    // Measured (round 5, configs[1]): step 0.1365 -> 0.1339 ms (-2 %), with two batches in flight 0.109 -> 0.117 (+7 %:
    // workgroups waiting at the barrier hold their CUs) — not worth a spinning kernel by default.
    {"plan_fused", 0, &O::plan_fused, flag(), "1 = the plan stage of a batch of at most one tile per CU is ONE launch (k_plan_fused), not k_plan_codes + k_plan_scatter"},
    {"plan_spin_limit", 4096, &O::plan_spin_limit, at_least(0), "polls of k_plan_fused's barrier before a workgroup aborts the order (~1 us each)"},
    {"code_bits_12", 1, &O::code_bits_12, flag(), "0 = alphabets of 257 .. 4,096 codes get 16-bit codes, not 12 (A/B; plan_code_bits, and the key width of suffix tables grown afterwards)"},
    {"suffix_table", 1, &O::suffix_table, flag(), "0 = launches ignore the index's suffix table, and batches are planned as if there were none (A/B)"},
    {"regroup_by_length", 1, &O::regroup_by_length, flag(), "k_count: workgroups with mixed pattern lengths hand their records out again by length (0: A/B)"},
    {"lf_steps_executed_only", 0, &O::lf_steps_executed_only, flag(), "1 = the LF-step output of count() leaves out what the suffix table answered"},
    // planned k_count: decided on the device from the plan's flag.  Tried first (round 5): tiles taken from a counter on a grid of
    // 8 workgroups per CU — the barrier that hands a tile to a workgroup's eight waves ties them together: headline 0.138 ->
    // 0.151 ms, series count +3 %.  Dropped.
    {"count_halve_uniform", 1, &O::count_halve_uniform, flag(), "a planned batch of one pattern length runs on half the grid (0: A/B)"},
    // Default OFF, by measurement (round 6, profiles/r06_experiments.txt 1): the lean kernel issues 20 % fewer vector instructions
    // (26.0 M against 32.5 M per headline launch, no spill at all) and takes the SAME time (89.0 against 90.9 us; + 4.6 us for the
    // list pass that finds its list empty) — k_count is not bound by instruction issue.  Kept as the A/B that showed it.
    {"count_lean", 0, &O::count_lean, flag(), "1 = planned batches over expanded images run k_count_lean + k_count's list mode instead of k_count"},

    // ---- locate() ----
    {"walk_pack", 1, &O::walk_pack, range(0, 3), "locate over a window directory packs the walks still under way into fewer waves: 0 = k_locate_walk (A/B), 1 / 2 = two packings, 3 = three"},
    {"walk_queue", 8, &O::walk_queue, range(0, 64), "locate over a window directory hands its tickets out per wave, this many per lane and run (0: the packed form)"},
    {"walk_queue_min_slots", 32, &O::walk_queue_min_slots, at_least(0), "... for calls with at least this many hit slots per pattern"},
    {"walk_burst", 0, &O::walk_burst, range(0, 1024), "LF-steps between two hand-outs of walk_queue (0 = sample_rate / 4, at least 2)"},
    // Measured on configs[1]'s index, <= 16 hits per pattern (tools/locate_order_probe.py): 16,384 patterns +8 % (the two or
    // three short kernels in front), 32,768 -5 %, 100,000 -24 %, 1,048,576 -43 %.
    {"walk_order_min", 32768, &O::walk_order_min, at_least(0), "locate: batches at least this large walk their hits by the first row of the patterns' SA ranges (0 = always the caller's order)"},
    {"walk_fine", 1, &O::walk_fine, flag(), "the window-local fine order on top of the walk order's buckets (k_plan_fine; 0: A/B)"},
    // 0 by measurement (profiles/r08_locate_rows.json): a gather reads one or two sectors per pattern whatever the order, and the
    // three short kernels in front cost more than the locality they buy: configs[2] 0.062 -> 0.044 ms, series locate(1)
    // 0.85 -> 0.77, locate(100) 0.47 -> 0.45
    {"rows_order", 0, &O::rows_order, range(0, 1), "1 = locate over a row table (k_locate_rows) still takes large batches by the first row of their ranges; 0 = the caller's order"},

    // ---- extractUntilBoundary ----
    {"boundary_accel", 1, &O::boundary_accel, flag(), "0 = literal right walk of extractUntilBoundary (A/B and fallback)"},
    {"boundary_group", 4, &O::boundary_group, one_of(is_boundary_group), "lanes per query of extractUntilBoundary (0 = one lane per query)"},
    {"boundary_first_fill", 2, &O::boundary_first_fill, one_of(is_first_fill), "first fill of the two text windows: 0 = a lane walks its intervals one after the other, 2 = its two walks interleaved (fm_lf_step2)"},
    // Default OFF, by measurement (round 6, profiles/r06_experiments.txt 2): the narrow first round walks 37.8 M LF-steps where the
    // wide form walks 50.9 M on configs[3] and takes 0.855 ms against 0.808: every pass costs a wave's lifetime (64 dependent steps
    // of one or two HBM round trips: ~0.35 ms whatever the batch), and the second pass pays it again for a quarter of the queries
    {"boundary_narrow", 0, &O::boundary_narrow, flag(), "1 = a narrow first round in front of the wide one"},
    {"boundary_narrow_min", 4096, &O::boundary_narrow_min, at_least(0), "... for batches at least this large"},
    {"boundary_rounds", 1, &O::boundary_rounds, flag(), "the group of four fetches the four sample intervals next to `from` first, the four further out only where needed (window_fill_round)"},
    // 100,000 hit locations of configs[3] (40,024 distinct) 1.93 -> 1.74 ms sorted on the host (tools/boundary_order_probe.py)
    {"boundary_order_min", 32768, &O::boundary_order_min, at_least(0), "batches at least this large take their queries by text position (0 = always the caller's order)"},

    // ---- what an index grows when it becomes resident afterwards ----
    {"sb_cache_limit", 320, &O::sb_cache_limit, range(0, 320), "superblocks whose headers the kernels stage in LDS (tests: 0 = no LDS cache)"},
    {"suffix_table_mb", 256, &O::suffix_table_mb, range(0, 1 << 16), "budget of the suffix table (0 = none)"},
    {"suffix_table_chars", 8, &O::suffix_table_chars, range(0, 8), "its depth (characters; the size limit and the key width may cut it)"},
    {"suffix_table_image_fraction", 8, &O::suffix_table_image_fraction, at_least(0), "the table stays below image bytes / this (0 = only the budget counts)"},
    // the window directory (fmx_device.hpp: 64 bytes per 112 text characters + 8 per position no class holds, beside the image).
    // window_cells_mb is per index: a process that holds many indexes lowers it, or the quarter rule shrinks what is free geometrically
    {"window_cells", 2, &O::window_cells, range(0, 3), "window directory: 0 = none, 1 = always, 2 = where it fits a quarter of the device's free memory and window_cells_mb, 3 = the flat form"},
    {"window_cells_mb", 65536, &O::window_cells_mb, at_least(0), "absolute budget (MiB) of one index's window directory under window_cells = 2, and of its row table"},
    {"window_entry_bytes", 0, &O::window_entry_bytes, one_of(is_entry_bytes), "the directory's entries: 0 = four bytes where the alphabet fits LDS (kWinSymbolSearchMax), else six; 4 / 6 = that form (tests, A/B)"},
    {"window_flat_fraction", 128, &O::window_flat_fraction, at_least(0), "under window_cells = 2 the FLAT form (4 bytes per text byte) where it costs at most 1 / this of the device's memory (0 = never by itself)"},
    {"locate_rows", 0, &O::locate_rows, range(0, 1), "row table (4 bytes per text character; locate() gathers its hits instead of walking): 0 = never, 1 = below 2^31 characters and where it fits"},
    {"sa_fences", 4096, &O::sa_fences, one_of(is_fence_count), "suffix arrays: most fences of the table staged in LDS (a power of two; 0 = no fence table)"},
    {"sa_fence_chars", 8, &O::sa_fence_chars, range(1, 16), "... and the characters per fence"},
    {"wavelet_on_device", 1, &O::wavelet_on_device, flag(), "0 = fmx_build_on_device encodes the wavelet tree on the host"},

    // ---- the image layer: images flattened afterwards (state and defaults live in fmx_blob.cpp, behind these setters) ----
    {"image_compact", 0, set_image_compact, flag(), "1 = the bit vectors stay compressed as RRR records (BlobHeader.compact; fmx.h)"},
    {"map_by_symbol", -1, set_map_by_symbol, range(-1, 1), "row layout of the mapping tables: -1 = by alphabet size, 0 = by superblock code, 1 = by global symbol"},
    {"map_fast", 1, set_map_fast, flag(), "0 = every present mapping entry takes the reference's own route (tests)"},
    {"inv_fast", 1, set_inv_fast, flag(), "0 = inverseSelect takes the reference's own route in every block (tests)"},
    {"cells_split_blocks", 1048576, +[](int v) { set_split_blocks(v); }, any, "bit vectors above this many 15-bit blocks are decoded in chunks (at least 64; tests lower it: same image)"},

    // ---- host-buffer entry points ----
    {"host_small_max", 2048, &O::host_small_max, at_least(0), "host-array calls of at most this many patterns / queries go through one mapped pinned block (0: off)"},
    {"host_pipeline_min", 131072, &O::host_pipeline_min, at_least(0), "host-buffer count(): batches at least this large go through the pipeline (0 = never)"},
    {"host_pipeline_chunk", 262144, &O::host_pipeline_chunk, at_least(65536), "patterns per stage of that pipeline"},
    {"host_mapped", 1, &O::host_mapped, flag(), "every array of a host-buffer count registered -> one launch over the mapped arrays, no copies"},
    {"host_direct_stores", 1, &O::host_direct_stores, flag(), "the pipeline's kernels store results straight into registered arrays"},
    // 0 BY MEASUREMENT: with the result copies gone a 1 M-pattern call takes 0.58 ms with the runtime's staging and 0.70-0.73 with
    // 3-6 threads of the copy pool: the runtime's copy is not what the call was waiting for (profiles/r06_experiments.txt 4)
    {"host_stage_threads", 0, &O::host_stage_threads, range(0, 64), "host threads that stage a pageable array into pinned memory (0 / 1 = the runtime's own staging)"},

    // ---- segment sets ----
    {"segments_direct", 1, &O::segments_direct, flag(), "0 = every segment's hits staged and appended (A/B)"},
    {"segments_overlap", 1, &O::segments_overlap, flag(), "0 = a segment set's kernels all on the caller's stream (A/B)"},
    {"segments_overlap_min", 262144, &O::segments_overlap_min, at_least(0), "... and only for batches at least this large"},
};
static_assert(sizeof(kOptions) / sizeof(kOptions[0]) == 58, "a new option needs its entry in tests/test_option_ranges.py too");

}  // namespace

Options::Options() {
    for (const OptionRow &row : kOptions)
        if (row.store.member) (this->*row.store.member).store(row.def);
}

Options &options() {
    static Options instance;
    return instance;
}

const OptionRow *find_option(const char *name) {
    for (const OptionRow &row : kOptions)
        if (std::string_view(row.name) == name) return &row;
    return nullptr;
}

bool OptionRow::set(int value) const {
    if (value < accept.lo || value > accept.hi || (accept.one_of && !accept.one_of(value))) return false;
    if (accept.flag) value = value != 0;
    if (store.member)
        (options().*store.member).store(value);
    else
        store.setter(value);
    return true;
}

}  // namespace fmx
