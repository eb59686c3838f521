"""The values fmx_set_option takes and refuses for the launch-shape and plan-stage options that tests/test_gpu_launch_shapes.py
and tools/fuzz_gpu.py sweep.  The setter only stores a value (no device needed); a sweep over a value the library refuses would
silently test the previous setting instead, so the ranges are pinned here.

Since the options live in one table (index4j_amd/csrc/fmx_options.cpp) RANGES lists every option, and test_table_matches_ranges
holds the table's names and defaults against it: results are identical for every setting by design, so a default that slipped
would pass every parity test and cost only speed.  A new option needs its entry here."""
import pathlib
import re

import pytest

import index4j_amd as ia

BIG = 2**31 - 1
SWITCH = [0, 1, -1, 2, BIG]
# name -> (library default, values it takes, values it refuses)
RANGES = {
    "block": (512, [512, 1024], [768, 256, 0, 2048, -512]),
    "groups_per_cu": (16, list(range(1, 65)), [0, -1, 65, 1024]),
    "coarse_bits": (12, list(range(4, 14)), [3, 14, 0, -4]),
    "sort_bits": (28, list(range(1, 33)), [0, 33, -1, 64]),
    "plan_fine": (1, [0, 1, 2], [-1, 3]),
    "walk_pack": (1, [0, 1, 2, 3], [-1, 4]),
    "walk_queue": (8, list(range(0, 65)), [-1, 65, 128]),
    "boundary_group": (4, [0, 1, 2, 4, 8, 16], [3, 5, 6, 7, 12, 32, -1]),
    # the remaining options, typed from the setter's source (NOT generated from the table in csrc/fmx_options.cpp: the double entry
    # is what test_table_matches_ranges checks).  BIG: no upper bound; a 0 / 1 switch takes any value (normalised) and refuses none.
    "lds_pad_kb": (0, [0, 1, 64, 96], [-1, 97, 1024]),
    "sort_min": (16384, [0, 1, 16384, BIG], [-1, -16384]),
    "plan_sa_key": (2, [0, 1, 2], [-1, 3]),
    "plan_sa_min": (786432, [0, 1, 786432, BIG], [-1]),
    "plan_min_per_string": (16, [0, 1, 16, BIG], [-1]),
    "plan_fused": (0, SWITCH, []),
    "plan_spin_limit": (4096, [0, 1, 4096, BIG], [-1]),
    "code_bits_12": (1, SWITCH, []),
    "suffix_table": (1, SWITCH, []),
    "regroup_by_length": (1, SWITCH, []),
    "lf_steps_executed_only": (0, SWITCH, []),
    "count_halve_uniform": (1, SWITCH, []),
    "count_lean": (0, SWITCH, []),
    "walk_queue_min_slots": (32, [0, 1, 32, BIG], [-1]),
    "walk_burst": (0, [0, 1, 16, 1024], [-1, 1025, 4096]),
    "walk_order_min": (32768, [0, 1, 32768, BIG], [-1]),
    "walk_fine": (1, SWITCH, []),
    "rows_order": (0, [0, 1], [-1, 2]),
    "boundary_accel": (1, SWITCH, []),
    "boundary_first_fill": (2, [0, 2], [1, 3, 4, -1]),
    "boundary_narrow": (0, SWITCH, []),
    "boundary_narrow_min": (4096, [0, 1, 4096, BIG], [-1]),
    "boundary_rounds": (1, SWITCH, []),
    "boundary_order_min": (32768, [0, 1, 32768, BIG], [-1]),
    "sb_cache_limit": (320, [0, 1, 319, 320], [-1, 321, 1024]),
    "suffix_table_mb": (256, [0, 1, 256, 65536], [-1, 65537, BIG]),
    "suffix_table_chars": (8, list(range(0, 9)), [-1, 9, 16]),
    "suffix_table_image_fraction": (8, [0, 1, 8, BIG], [-1]),
    "window_cells": (2, [0, 1, 2, 3], [-1, 4]),
    "window_cells_mb": (65536, [0, 1, 65536, BIG], [-1]),
    "window_entry_bytes": (0, [0, 4, 6], [1, 2, 3, 5, 7, 8, -4]),
    "window_flat_fraction": (128, [0, 1, 128, BIG], [-1]),
    "locate_rows": (0, [0, 1], [-1, 2]),
    "sa_fences": (4096, [0, 1, 2, 4096, 32768], [-1, 3, 4095, 4097, 65536, BIG]),
    "sa_fence_chars": (8, list(range(1, 17)), [0, -1, 17]),
    "wavelet_on_device": (1, SWITCH, []),
    "image_compact": (0, SWITCH, []),
    "map_by_symbol": (-1, [-1, 0, 1], [-2, 2]),
    "map_fast": (1, SWITCH, []),
    "inv_fast": (1, SWITCH, []),
    "cells_split_blocks": (1048576, [-1, 0, 63, 64, 1048576, BIG], []),  # (anything; below 64 becomes 64)
    "host_small_max": (2048, [0, 1, 2048, BIG], [-1]),
    "host_pipeline_min": (131072, [0, 1, 131072, BIG], [-1]),
    "host_pipeline_chunk": (262144, [65536, 262144, BIG], [65535, 0, -1]),
    "host_mapped": (1, SWITCH, []),
    "host_direct_stores": (1, SWITCH, []),
    "host_stage_threads": (0, [0, 1, 6, 64], [-1, 65]),
    "segments_direct": (1, SWITCH, []),
    "segments_overlap": (1, SWITCH, []),
    "segments_overlap_min": (262144, [0, 1, 262144, BIG], [-1]),
}


@pytest.mark.parametrize("name", sorted(RANGES))
def test_launch_and_plan_option_ranges(name):
    default, good, bad = RANGES[name]
    key = name.encode()
    try:
        for v in good:
            assert ia.lib.fmx_set_option(key, v) == 0, (name, v)
        assert ia.lib.fmx_set_option(key, good[0]) == 0
        for v in bad:
            assert ia.lib.fmx_set_option(key, v) == ia._lib.E_ARG, (name, v)
    finally:
        assert ia.lib.fmx_set_option(key, ia._lib.ENV_OPTIONS.get(name, default)) == 0


def test_table_matches_ranges():
    """The option table's rows — one source line `{"name", default, ...}` each — name exactly RANGES' options, with its defaults."""
    src = pathlib.Path(ia.__file__).resolve().parent / "csrc" / "fmx_options.cpp"
    rows = re.findall(r'^\s*\{"(\w+)",\s*(-?\d+),', src.read_text(), flags=re.M)
    assert len(rows) == len({name for name, _ in rows}), "an option has two rows"
    assert {name for name, _ in rows} == set(RANGES)
    assert {name: int(default) for name, default in rows} == {name: r[0] for name, r in RANGES.items()}
