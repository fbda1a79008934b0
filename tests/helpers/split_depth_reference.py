"""numpy restatement of dlv_cc_split_depth_dev's definition (include/delivr_hip.h; INTEGRATION "Splitting fused cells"), for
tests/test_split_depth_cpu.py and tests/test_gpu_split_depth.py.  Built from the two references that are pinned already: the
distance map of depth_reference.py (scipy's exact transform, one label at a time) and the labelling, growth and numbering of
split_reference.py.  Only the threshold T(l) is new, in Python integers."""
import importlib.util
import os

import numpy as np


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


depth = _helper("depth_reference")
split = _helper("split_reference")


def thresholds(L: np.ndarray, n: int, d2: np.ndarray, core_d2: int, fraction: int) -> np.ndarray:
    """T(l) = max(core_d2, ceil(fraction^2 * m(l) / 10000), 1) for the rows 0..n, m(l) the largest D2 of label l, as uint64"""
    m = depth.depth_rows(L, n, d2)["depth_max_sq"]
    return np.array([max(int(core_d2), -(-int(fraction) * int(fraction) * int(v) // 10000), 1) for v in m], dtype=np.uint64)


def cores(L: np.ndarray, n: int, spacing, core_d2: int, fraction: int) -> np.ndarray:
    """C: the voxels of a label 1..n whose D2 reaches their label's threshold, as a bool volume"""
    d2 = depth.depth_map(L, n, spacing)
    T = thresholds(L, n, d2, core_d2, fraction)
    inside = (L >= 1) & (L <= n)
    return inside & (d2.astype(np.uint64) >= T[np.where(inside, L, 0)])


def split_depth_reference(L: np.ndarray, n: int, spacing, core_d2: int, fraction: int, min_core: int = 1) -> dict:
    """The whole definition -> split_reference's dict: {"out": uint32 volume, "K", "parent": uint32 (K+1), "n_split", "M" (cores),
    "steps" (growth steps that changed a voxel), "max_cores" (the most cores in one label)}"""
    L = np.asarray(L).astype(np.uint32)
    assert 0 <= fraction <= 99 and core_d2 >= 0 and (core_d2 or fraction)
    Q, M = split.label26(cores(L, n, spacing, core_d2, fraction))
    if min_core > 1 and M:  # (split_reference.core_labels' rule: cores of fewer voxels are dropped, the rest renumbered in order)
        sizes = np.bincount(Q.ravel(), minlength=M + 1)
        keep = sizes >= min_core
        keep[0] = False
        lut = np.where(keep, np.cumsum(keep), 0).astype(np.uint32)
        Q, M = lut[Q], int(keep.sum())
    Q = Q.astype(np.uint32)
    G, steps = split.grow(L, Q)
    out, K, parent, n_split = split.pieces(L, G, Q, M, n)
    comp = np.zeros(M + 1, dtype=np.int64)
    comp[Q[Q != 0]] = L[Q != 0]
    max_cores = int(np.bincount(comp[1:], minlength=n + 1).max()) if M else 0
    return {"out": out, "K": K, "parent": parent, "n_split": n_split, "M": M, "steps": steps, "max_cores": max_cores}
