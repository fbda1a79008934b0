"""The reference of dlv_cc_depth_dev / HipEngine.cc_depth: scipy's exact Euclidean distance transform, one label at a time.

For a label l: the bounding box of scipy.ndimage.find_objects, grown by one voxel and clipped to the volume; `crop == l` padded
with one plane of zeros on each side where the box touches a face of the volume (the outside of the volume is background);
distance_transform_edt(mask, sampling=w); np.rint(d * d) as uint64 - d is the correctly rounded root of an integer below 2^32, so
the square rounds back to that integer.  The grown box always contains a nearest foreign voxel: clamping any foreign voxel to the
box gives a position that is at least as near on every axis and still outside the label (inside the box but off the label's own
bounding box, or on the zero padding).  The per-label rows follow from the map with np.maximum.at, np.add.at and the first argmax
in raster order."""
import numpy as np
from scipy import ndimage

NO_PEAK = 2**64 - 1


def depth_map(labels: np.ndarray, n: int, spacing=(1, 1, 1)) -> np.ndarray:
    """D2 of every voxel as uint32 (Z, Y, X): 0 where the label is 0 or above n"""
    labels = np.asarray(labels)
    assert labels.ndim == 3
    w = tuple(int(v) for v in spacing)
    out = np.zeros(labels.shape, dtype=np.uint64)
    # (find_objects takes int labels; labels above n are other labels here, so the volume is handed over whole)
    boxes = ndimage.find_objects(labels.astype(np.int64), max_label=int(n)) if n > 0 else []
    for l, box in enumerate(boxes, 1):
        if box is None:
            continue
        grown = tuple(slice(max(s.start - 1, 0), min(s.stop + 1, dim)) for s, dim in zip(box, labels.shape))
        mask = labels[grown] == l
        pad = tuple((int(g.start == 0), int(g.stop == dim)) for g, dim in zip(grown, labels.shape))
        d = ndimage.distance_transform_edt(np.pad(mask, pad, constant_values=False), sampling=w)
        d2 = np.rint(d * d).astype(np.uint64)
        inner = tuple(slice(p[0], d2.shape[a] - p[1]) for a, p in enumerate(pad))
        view = out[grown]
        view[mask] = d2[inner][mask]
    assert int(out.max(initial=0)) < 2**32
    return out.astype(np.uint32)


def depth_rows(labels: np.ndarray, n: int, d2: np.ndarray) -> dict:
    """the ABI's rows 0..n from the map: depth_max_sq uint32, depth_sum_sq uint64, depth_peak_index uint64"""
    flat_l = np.asarray(labels).ravel()
    flat_d = np.asarray(d2).ravel()
    sel = np.flatnonzero((flat_l >= 1) & (flat_l <= n))
    lab = flat_l[sel].astype(np.int64)
    val = flat_d[sel]
    mx = np.zeros(n + 1, dtype=np.uint32)
    sm = np.zeros(n + 1, dtype=np.uint64)
    np.maximum.at(mx, lab, val.astype(np.uint32))
    np.add.at(sm, lab, val.astype(np.uint64))
    peak = np.full(n + 1, NO_PEAK, dtype=np.uint64)
    at_max = val == mx[lab]  # (sel ascends: the first hit per label is the first in raster order)
    first = np.unique(lab[at_max], return_index=True)
    peak[first[0]] = sel[at_max][first[1]].astype(np.uint64)
    return {"depth_max_sq": mx, "depth_sum_sq": sm, "depth_peak_index": peak}


def depth_reference(labels: np.ndarray, n: int, spacing=(1, 1, 1)):
    """-> (D2 map uint32, the rows 0..n)"""
    d2 = depth_map(labels, n, spacing)
    return d2, depth_rows(labels, n, d2)


def scan_reference(labels: np.ndarray, n: int, spacing=(1, 1, 1)) -> np.ndarray:
    """the three passes of csrc/cc_depth.hip in numpy, voxel by voxel (small volumes only): an independent check of the separable
    formulation against depth_map"""
    L = np.asarray(labels).astype(np.int64)
    Z, Y, X = L.shape
    wz, wy, wx = (int(v) for v in spacing)
    g = np.zeros(L.shape, dtype=np.int64)
    for z in range(Z):
        for y in range(Y):
            x = 0
            while x < X:
                x1 = x
                while x1 + 1 < X and L[z, y, x1 + 1] == L[z, y, x]:
                    x1 += 1
                for k in range(x, x1 + 1):
                    g[z, y, k] = (wx * min(k - x + 1, x1 - k + 1)) ** 2
                x = x1 + 1
    for axis, w in ((1, wy), (0, wz)):
        src = np.moveaxis(g, axis, 0).copy()
        lab = np.moveaxis(L, axis, 0)
        dst = src.copy()
        dim = src.shape[0]
        for p in range(dim):
            for q in range(dim):  # every position of the line; a foreign voxel stands for distance 0 in its row / plane
                cand = (w * (p - q)) ** 2 + np.where(lab[q] == lab[p], src[q], 0)
                dst[p] = np.minimum(dst[p], cand)
            edge = (w * min(p + 1, dim - p)) ** 2
            dst[p] = np.minimum(dst[p], edge)
        g = np.moveaxis(dst, 0, axis).copy()
    g[(L < 1) | (L > n)] = 0
    return g.astype(np.uint32)
