"""The judge of the distinct-values stage (fmx_values_distinct_histogram_dev) over what the stage itself takes, in plain numpy: a packed
block of slots (hit_off, locs, n_hits), the group of every slot, the group offsets, the line table and the edges.  It needs no index
and no oracle, so it judges made-up hits too; tests/test_distinct_values_cpu.py holds it to the oracle-based judge on the fixture."""
import numpy as np


def judge_distinct_slots(hit_off, locs, n_hits, group_of_hit, val_off, T, edges):
    """(distinct, first_seen), each (n, B): per pattern the different (group, bucket) pairs of its slots that are hits, have a group
    inside the pattern's groups and a line inside the edges; a group's first is the pair with its smallest bucket.  edges None: one
    bucket, every line, T unused."""
    hit_off, val_off = np.asarray(hit_off, np.int64), np.asarray(val_off, np.int64)
    n = len(hit_off) - 1
    B = 1 if edges is None else len(edges) - 1
    distinct, first_seen = np.zeros((n, B), np.int32), np.zeros((n, B), np.int32)
    slot = np.clip(hit_off, 0, n_hits)
    for i in range(n):
        a, b = int(slot[i]), int(slot[i + 1])
        g = np.asarray(group_of_hit[a:b], np.int64)
        if edges is None:
            bucket = np.zeros(b - a, np.int64)
        else:
            e = np.asarray(edges, np.int64)
            L = np.searchsorted(np.asarray(T, np.int64), np.asarray(locs[a:b], np.int64), side="left")  # the entries of T below the hit
            below = np.searchsorted(e, L, side="right")  # the edges <= L; of equal edges the last one: an empty bucket stays empty
            bucket = np.where((below == 0) | (below == len(e)), B, below - 1)
        ok = (g >= 0) & (g < val_off[i + 1] - val_off[i]) & (bucket < B)
        pairs = np.unique(g[ok] * B + bucket[ok])  # ascending: by group, then by bucket
        head = np.ones(len(pairs), bool)
        head[1:] = pairs[1:] // B != pairs[:-1] // B
        distinct[i] = np.bincount(pairs % B, minlength=B)
        first_seen[i] = np.bincount(pairs[head] % B, minlength=B)
    return distinct, first_seen
