"""The neighbour table of a label volume in numpy - the reference of tests/test_gpu_neighbours.py, pinned against an all-voxel-pairs
brute force in tests/test_neighbours_cpu.py.  It depends on neither pruning of csrc/cc_neighbours.hip: for every offset of the FULL
box (both signs on every axis) with 0 < d2 <= R2 the label array is compared with its shifted self, the pairs a < b are taken and
reduced by key with np.minimum.at.

A voxel takes part when 1 <= L(v) <= n.  gap2(a, b) = the smallest (wz dz)^2 + (wy dy)^2 + (wx dx)^2 between a voxel of a and a
voxel of b; the table is every a < b with gap2 <= R2."""
import math

import numpy as np

NO_GAP = np.iinfo(np.int64).max


def reach(radius_sq, spacing):
    """floor(sqrt(R2) / w) per axis"""
    root = math.isqrt(int(radius_sq))
    return tuple(root // int(w) for w in spacing)


def neighbour_table(labels, n, spacing, radius_sq):
    """-> {(a, b): gap2} for every pair a < b of labels 1..n with gap2 <= radius_sq"""
    lab = np.asarray(labels).astype(np.int64)
    assert lab.ndim == 3
    lab = np.where((lab >= 1) & (lab <= int(n)), lab, 0)
    Z, Y, X = lab.shape
    wz, wy, wx = (int(w) for w in spacing)
    R2 = int(radius_sq)
    rz, ry, rx = (min(r, d - 1) for r, d in zip(reach(R2, spacing), lab.shape))  # (a larger offset leaves the volume)
    keys, gaps = [], []
    for dz in range(-rz, rz + 1):
        for dy in range(-ry, ry + 1):
            for dx in range(-rx, rx + 1):
                d2 = (wz * dz) ** 2 + (wy * dy) ** 2 + (wx * dx) ** 2
                if not 0 < d2 <= R2:
                    continue
                # v in `here`, v + (dz, dy, dx) in `there`
                here = lab[max(0, -dz):Z - max(0, dz), max(0, -dy):Y - max(0, dy), max(0, -dx):X - max(0, dx)]
                there = lab[max(0, dz):Z - max(0, -dz), max(0, dy):Y - max(0, -dy), max(0, dx):X - max(0, -dx)]
                hit = (here > 0) & (there > 0) & (here < there)  # (a < b; the offset with the other sign brings b < a)
                if hit.any():
                    k = np.unique(here[hit] << 32 | there[hit])
                    keys.append(k)
                    gaps.append(np.full(len(k), d2, dtype=np.int64))
    if not keys:
        return {}
    keys, gaps = np.concatenate(keys), np.concatenate(gaps)
    uniq, inverse = np.unique(keys, return_inverse=True)
    best = np.full(len(uniq), NO_GAP, dtype=np.int64)
    np.minimum.at(best, inverse, gaps)
    return {(int(k >> 32), int(k & 0xFFFFFFFF)): int(g) for k, g in zip(uniq.tolist(), best.tolist())}


def brute_force_table(labels, n, spacing, radius_sq):
    """the definition itself, over all pairs of voxels that take part: for hand-made volumes of a few hundred foreground voxels"""
    lab = np.asarray(labels).astype(np.int64)
    at = np.argwhere((lab >= 1) & (lab <= int(n)))
    who = lab[tuple(at.T)]
    w = np.asarray(spacing, dtype=np.int64)
    table = {}
    for i in range(len(at)):
        d2 = (((at - at[i]) * w) ** 2).sum(axis=1)
        for j in np.flatnonzero((who > who[i]) & (d2 <= int(radius_sq))).tolist():
            key = (int(who[i]), int(who[j]))
            table[key] = min(table.get(key, NO_GAP), int(d2[j]))
    return table


def as_arrays(table):
    """{(a, b): gap2} -> (pairs uint32 (P, 2) sorted by (a, b), gap_sq uint32 (P)): HipEngine.cc_neighbours' order"""
    items = sorted(table.items())
    pairs = np.array([k for k, _ in items], dtype=np.uint32).reshape(-1, 2)
    return pairs, np.array([g for _, g in items], dtype=np.uint32)


def assert_table_equal(got, table):
    """HipEngine.cc_neighbours' dict against {(a, b): gap2}: the keys, the types, the order, every gap; S bounds P"""
    assert list(got) == ["a", "b", "gap_sq", "segments"]
    pairs, gaps = as_arrays(table)
    for k in ("a", "b", "gap_sq"):
        assert got[k].dtype == np.uint32 and got[k].shape == (len(gaps),), (k, got[k].dtype, got[k].shape, len(gaps))
    np.testing.assert_array_equal(np.stack([got["a"], got["b"]], axis=1), pairs, err_msg="pairs")
    np.testing.assert_array_equal(got["gap_sq"], gaps, err_msg="gap_sq")
    assert isinstance(got["segments"], int) and got["segments"] >= len(gaps)
    assert (got["segments"] == 0) == (len(gaps) == 0)
