"""The reference of the per-label quantile tests (dlv_cc_quantiles_dev / HipEngine.cc_quantiles), numpy only: the voxels with a
label 1..n sorted by (label, value) with np.lexsort, the segment starts from np.bincount, and per label with m >= 1 voxels and
level p (per cent) the value at index (p * (m - 1)) // 100 of its segment - the lower quantile.  Labels above n and the background
are not measured; row 0 and an absent label read 0 with a count of 0."""
import numpy as np


def quantile_reference(labels: np.ndarray, raw: np.ndarray, n: int, levels=(25, 50, 75)):
    """labels: unsigned integers, raw: uint16 of the same shape -> (uint16 (n+1, len(levels)), uint32 counts (n+1,))"""
    assert labels.shape == raw.shape and raw.dtype == np.uint16
    lab, val = labels.ravel().astype(np.int64), raw.ravel()
    sel = (lab >= 1) & (lab <= n)
    lab, val = lab[sel], val[sel]
    order = np.lexsort((val, lab))  # (last key first: by label, then by value)
    val = val[order]
    counts = np.bincount(lab, minlength=n + 1).astype(np.int64)
    starts = np.cumsum(counts) - counts
    out = np.zeros((n + 1, len(levels)), dtype=np.uint16)
    present = counts > 0
    for k, p in enumerate(levels):
        idx = starts[present] + (int(p) * (counts[present] - 1)) // 100
        out[present, k] = val[idx]
    return out, counts.astype(np.uint32)
