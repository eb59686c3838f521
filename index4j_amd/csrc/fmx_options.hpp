// fmx_options.hpp — the runtime options of fmx_set_option: one struct of atomics (one member per option, one instance per
// process) and one table (fmx_options.cpp: name, default, accepted values, description of every option).
//
// Atomics: a launch on one host thread may read an option while another thread sets one (results are identical for every
// setting, so a launch that sees a mix of old and new values is still correct).  Where a decision depends on an option, the
// reader takes ONE reading per decision.  Only host code reads the struct: launchers hand the values to their kernels as arguments.
#pragma once

#include <atomic>
#include <climits>

namespace fmx {

constexpr int kCoarseBitsMax = 14;  // bins of the plan stage's bucket pass: 16,384 LDS bins (64 KiB)

// One member per option that is stored here, named as the option is.  The values come from the table's defaults (Options()).
struct Options {
    // launch shape (FM, compact-FM and suffix-array kernels alike)
    std::atomic<int> block, groups_per_cu, lds_pad_kb;
    // count() and its plan stage
    std::atomic<int> sort_min, sort_bits, coarse_bits, plan_fine, plan_sa_key, plan_sa_min, plan_min_per_string, plan_fused,
        plan_spin_limit, code_bits_12, suffix_table, regroup_by_length, lf_steps_executed_only, count_halve_uniform, count_lean;
    // locate()
    std::atomic<int> walk_pack, walk_queue, walk_queue_min_slots, walk_burst, walk_order_min, walk_fine, rows_order;
    // extractUntilBoundary
    std::atomic<int> boundary_accel, boundary_group, boundary_first_fill, boundary_narrow, boundary_narrow_min, boundary_rounds,
        boundary_order_min;
    // what an index grows when it becomes resident
    std::atomic<int> sb_cache_limit, suffix_table_mb, suffix_table_chars, suffix_table_image_fraction, window_cells,
        window_cells_mb, window_entry_bytes, window_flat_fraction, locate_rows, sa_fences, sa_fence_chars, wavelet_on_device;
    // host-buffer entry points and segment sets
    std::atomic<int> host_small_max, host_pipeline_min, host_pipeline_chunk, host_mapped, host_direct_stores, host_stage_threads,
        segments_direct, segments_overlap, segments_overlap_min;
    Options();
};
Options &options();  // the process's instance

// What an option accepts: a range [lo, hi], or "anything, normalised to 0 / 1", or the values a captureless predicate names.
struct Accept {
    int lo, hi;
    bool flag;
    bool (*one_of)(int);
};
constexpr Accept range(int lo, int hi) { return {lo, hi, false, nullptr}; }
constexpr Accept at_least(int lo) { return {lo, INT_MAX, false, nullptr}; }
constexpr Accept flag() { return {INT_MIN, INT_MAX, true, nullptr}; }
constexpr Accept one_of(bool (*pred)(int)) { return {INT_MIN, INT_MAX, false, pred}; }

// Where an accepted value goes: a member of Options, or a setter of the image layer (fmx_blob.cpp keeps that state itself:
// it is compiled into host-only test builds without this table).
struct Store {
    std::atomic<int> Options::*member = nullptr;
    void (*setter)(int) = nullptr;
    constexpr Store(std::atomic<int> Options::*m) : member(m) {}
    constexpr Store(void (*s)(int)) : setter(s) {}
};

struct OptionRow {
    const char *name;
    int def;
    Store store;
    Accept accept;
    const char *what;
    bool set(int value) const;  // false: the value is refused and the option keeps what it had
};
const OptionRow *find_option(const char *name);  // nullptr: no option of that name

}  // namespace fmx
