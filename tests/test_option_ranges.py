"""The values fmx_set_option takes and refuses for the launch-shape and plan-stage options that tests/test_gpu_launch_shapes.py
and tools/fuzz_gpu.py sweep.  The setter only stores a value (no device needed); a sweep over a value the library refuses would
silently test the previous setting instead, so the ranges are pinned here."""
import pytest

import index4j_amd as ia

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
