"""A label volume described by a short list of cells, and what every per-cell kernel family must give on it, computed from that
list alone - for tests/test_sparse_cells_cpu.py (which pins this file on small volumes against the dense references applied to the
whole volume) and tests/test_gpu_index_limits.py (which runs the same layouts at 2^32 voxels, where nothing dense fits the host).

The cells are few and lie far apart: the CROP of a cell group - its voxels and MARGIN voxels around them, clipped at the faces of
the volume - meets no other crop, and MARGIN exceeds the largest shell radius / split depth used (MAX_REACH) by two.  So every
kernel's answer decomposes: the dense numpy reference runs on each crop (a crop that touches a face of the volume is clipped there,
so the face is the crop's face too; every other crop face lies in MARGIN voxels of background), and the result is translated to
volume coordinates and 64-bit linear indices.  Whole-volume outputs come back as Sparse(coords, values): the non-zero voxels only;
`k = len(values)` is the number the output's count_nonzero must give.

raw (uint16) and prob (float32) are zero outside the crops and seeded random inside them; the probabilities are multiples of 2^-24,
and two voxels of the cell LAYOUT.peak_label hold 1.0 (the peak is the first of them in raster order).

numpy only, apart from the references it calls: tests/helpers/{split,fill,quantile,paint}_reference.py, label_runs.encode_runs and
compare_cells.overlap_table_np."""
import importlib.util
import itertools
import os
from collections import namedtuple

import numpy as np

MARGIN = 5
MAX_REACH = 3  # the largest shell radius / split depth the expectations may be asked for
NONE = np.uint32(0xFFFFFFFF)
NO_PEAK = np.uint64(0xFFFFFFFFFFFFFFFF)

Sparse = namedtuple("Sparse", "coords values")  # coords: int64 (k, 3) z, y, x in raster order; values: (k,) non-zero
Crop = namedtuple("Crop", "lo hi labels raw prob")  # lo, hi: the half-open box in the volume; the arrays have shape hi - lo


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


split_ref = _helper("split_reference")
fill_ref = _helper("fill_reference")
quantile_ref = _helper("quantile_reference")
paint_ref = _helper("paint_reference")


# ---- the dense references: a volume (or a crop at `origin` of a volume of `shape`) -> tables over the labels 0..n ------------------
def dense_counts(L, n):
    """voxels per label 0..n (row 0: the background of L)"""
    return np.bincount(L.ravel().astype(np.int64), minlength=n + 1)[:n + 1].astype(np.uint64)


def dense_stats(L, n, origin=(0, 0, 0)):
    """HipEngine.cc_stats_raw's rows 1..n: counts u32, bbmin (absent: 0xFFFFFFFF) / bbmax u32 (n+1, 3), sums u64 (n+1, 3); row 0 is
    left absent (the caller knows the background)"""
    out = {"counts": np.zeros(n + 1, np.uint32), "bbmin": np.full((n + 1, 3), NONE, np.uint32), "bbmax": np.zeros((n + 1, 3), np.uint32),
           "sums": np.zeros((n + 1, 3), np.uint64)}
    idx = np.nonzero(L)
    lab = L[idx].astype(np.int64)
    out["counts"][:] = np.bincount(lab, minlength=n + 1)
    for a in range(3):
        c = idx[a].astype(np.uint64) + np.uint64(origin[a])
        np.add.at(out["sums"][:, a], lab, c)
        np.minimum.at(out["bbmin"][:, a], lab, c.astype(np.uint32))
        np.maximum.at(out["bbmax"][:, a], lab, c.astype(np.uint32))
    return out


def dense_intensity(L, raw, n):
    """HipEngine.cc_intensity's rows: absent labels - and row 0 - read 0, 0, 0xFFFF, 0"""
    out = {"intensity_sum": np.zeros(n + 1, np.uint64), "intensity_sumsq": np.zeros(n + 1, np.uint64),
           "intensity_min": np.full(n + 1, 0xFFFF, np.uint16), "intensity_max": np.zeros(n + 1, np.uint16)}
    sel = (L >= 1) & (L <= n)
    lab, v = L[sel].astype(np.int64), raw[sel].astype(np.uint64)
    np.add.at(out["intensity_sum"], lab, v)
    np.add.at(out["intensity_sumsq"], lab, v * v)
    np.minimum.at(out["intensity_min"], lab, v.astype(np.uint16))
    np.maximum.at(out["intensity_max"], lab, v.astype(np.uint16))
    return out


def quantise(prob):
    """q = rint(clamp(p, 0, 1) * 2^24), NaN as 0 (hostlogic.quantise_confidence's definition)"""
    p = np.asarray(prob, dtype=np.float32)
    return np.rint(np.clip(np.where(np.isnan(p), 0, p), 0, 1).astype(np.float32) * np.float32(2 ** 24)).astype(np.uint32)


def dense_confidence(L, prob, n, origin=(0, 0, 0), shape=None):
    """HipEngine.cc_confidence's rows; the peak is a linear index in the volume of `shape` (default: L's own)"""
    shape = L.shape if shape is None else shape
    out = {"confidence_sum": np.zeros(n + 1, np.uint64), "confidence_min_q": np.full(n + 1, NONE, np.uint32),
           "confidence_max_q": np.zeros(n + 1, np.uint32), "confidence_peak_index": np.full(n + 1, NO_PEAK, np.uint64)}
    idx = np.nonzero((L >= 1) & (L <= n))
    lab, q = L[idx].astype(np.int64), quantise(prob)[idx]
    lin = linear_index(np.stack(idx, axis=1) + np.asarray(origin, np.int64), shape)
    np.add.at(out["confidence_sum"], lab, q.astype(np.uint64))
    np.minimum.at(out["confidence_min_q"], lab, q)
    np.maximum.at(out["confidence_max_q"], lab, q)
    top = q == out["confidence_max_q"][lab]
    np.minimum.at(out["confidence_peak_index"], lab[top], lin[top])  # the first in raster order among the largest
    return out


def dense_expand(L, r):
    """E_r of cc_shell.hip: r synchronous steps of the 26-neighbourhood minimum into the background"""
    E = L.astype(np.uint32)
    Z, Y, X = E.shape
    for _ in range(r):
        P = np.pad(np.where(E == 0, NONE, E), 1, constant_values=NONE)
        m = np.full(E.shape, NONE, dtype=np.uint32)
        for dz, dy, dx in itertools.product(range(3), repeat=3):
            np.minimum(m, P[dz:dz + Z, dy:dy + Y, dx:dx + X], out=m)
        E = np.where(E != 0, E, np.where(m == NONE, 0, m)).astype(np.uint32)
    return E


def dense_shell(L, raw, r):
    """S: the expanded voxels that are background in L and (raw given) not 0 in raw"""
    keep = L == 0
    if raw is not None:
        keep = keep & (raw != 0)
    return np.where(keep, dense_expand(L, r), 0).astype(np.uint32)


SHAPE_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # zz, yy, xx, zy, zx, yx


def dense_shape(L, n, planes=None, origin=(0, 0, 0)):
    """HipEngine.cc_shape's accumulators of the buffer L: the planes [planes[0], planes[1]) measured, the rest neighbours only; what
    lies outside L differs from every label; coordinates are L's own plus `origin` (z: the caller folds z_abs0 in)"""
    lo, hi = planes or (0, L.shape[0])
    pad = np.pad(L.astype(np.int64), 1, constant_values=-1)
    core = pad[1:-1, 1:-1, 1:-1]
    exposed = [(np.roll(pad, 1, a)[1:-1, 1:-1, 1:-1] != core).astype(np.uint64) + (np.roll(pad, -1, a)[1:-1, 1:-1, 1:-1] != core)
               for a in range(3)]
    sel = np.zeros(L.shape, dtype=bool)
    sel[lo:hi] = (L[lo:hi] >= 1) & (L[lo:hi] <= n)
    lab = L[sel].astype(np.int64)
    c = [v[sel].astype(np.int64) + int(o) for v, o in zip(np.indices(L.shape), origin)]
    assert all((v >= 0).all() for v in c)
    c = [v.astype(np.uint64) for v in c]
    out = {"shape_counts": np.bincount(lab, minlength=n + 1).astype(np.uint32), "shape_sums": np.zeros((n + 1, 3), np.uint64),
           "shape_moments": np.zeros((n + 1, 6), np.uint64), "shape_faces": np.zeros((n + 1, 3), np.uint64),
           "shape_surface_voxels": np.zeros(n + 1, np.uint32)}
    for a in range(3):
        np.add.at(out["shape_sums"][:, a], lab, c[a])
        np.add.at(out["shape_faces"][:, a], lab, exposed[a][sel])
    for j, (a, b) in enumerate(SHAPE_PAIRS):
        np.add.at(out["shape_moments"][:, j], lab, c[a] * c[b])
    np.add.at(out["shape_surface_voxels"], lab, ((exposed[0] + exposed[1] + exposed[2])[sel] > 0).astype(np.uint32))
    return out


def dense_boxes(bin_img, boxes, values):
    """blob_highlighter's sequential loop: every box (z0, z1, y0, y1, x0, x1, half-open) in order writes bin_img * value over itself"""
    out = np.zeros(bin_img.shape, dtype=values.dtype)
    for b, v in zip(boxes, values):
        sl = (slice(b[0], b[1]), slice(b[2], b[3]), slice(b[4], b[5]))
        out[sl] = (bin_img[sl].astype(np.int64) * int(v)).astype(values.dtype)
    return out


def linear_index(coords, shape):
    """uint64 C-order linear indices of int64 (k, 3) coordinates in a volume of `shape`"""
    c = np.asarray(coords).astype(np.uint64)
    return (c[:, 0] * np.uint64(shape[1]) + c[:, 1]) * np.uint64(shape[2]) + c[:, 2]


def sparse_of(volume):
    """a dense volume as Sparse"""
    idx = np.nonzero(volume)
    return Sparse(np.stack(idx, axis=1).astype(np.int64), volume[idx])


# ---- the layout ---------------------------------------------------------------------------------------------------------------------
def _box(lo, hi):
    """the inclusive box lo..hi as (origin, bool block)"""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    return lo, np.ones(tuple(hi - lo + 1), dtype=bool)


def _dumbbell(axis):
    """two 5^3 cubes joined by a one-voxel neck along `axis`: (5, 5, 5) stretched to 11 along it"""
    shape = [5, 5, 5]
    shape[axis] = 11
    m = np.ones(shape, dtype=bool)
    gap = [slice(None)] * 3
    gap[axis] = 5
    m[tuple(gap)] = False
    neck = [2, 2, 2]
    neck[axis] = 5
    m[tuple(neck)] = True
    return m


def _hollow():
    m = np.ones((5, 5, 5), dtype=bool)
    m[1:4, 1:4, 1:4] = False
    return m


def _cup_far_z():
    """a 5^3 cube whose 3 x 3 cavity is open towards +z: pushed against the far z face it is no hole"""
    m = np.ones((5, 5, 5), dtype=bool)
    m[1:5, 1:4, 1:4] = False
    return m


class Layout:
    """shape, half (the linear index the cells straddle: 2^31 at the full sizes), n labels, the groups [(name, origin, uint32 block)]
    and their crops; label k is the k-th cell of the list, NOT its raster rank"""

    def __init__(self, shape, half, seed=0):
        Z, Y, X = self.shape = tuple(int(v) for v in shape)
        self.nvox = Z * Y * X
        self.half = int(half)
        hz, hy, hx = (int(v) for v in np.unravel_index(self.half, self.shape))
        self.hz = hz
        assert 0 < self.half < self.nvox and hz >= 14 and Z - hz >= 21, "the three z groups need room"
        bar_len = min(1800, (7 * Y) // 8)
        self.bar = (hz + 3, Y // 16, (2 * X) // 3, bar_len)  # z, first y, x, voxels along y
        cells = [("origin", *_box((0, 0, 0), (2, 3, 4))),
                 ("bar", *_box((self.bar[0], self.bar[1], self.bar[2]), (self.bar[0], self.bar[1] + bar_len - 1, self.bar[2]))),
                 ("end", *_box((Z - 3, Y - 4, X - 5), (Z - 1, Y - 1, X - 1)))]
        if hy == 0 and hx == 0:  # the index is a plane's first voxel: one box ends plane hz - 1, one starts plane hz
            cells += [("below", *_box((hz - 1, Y - 8, X - 8), (hz + 1, Y - 1, X - 1))), ("above", *_box((hz - 1, 0, 0), (hz + 1, 2, 8)))]
        else:  # inside a row: one box, whose run in row (hz, hy) covers hx - 8 .. hx + 8
            assert 2 <= hy < Y - 2 and 8 <= hx < X - 8
            cells += [("across", *_box((hz - 1, hy - 2, hx - 8), (hz + 1, hy + 2, hx + 8)))]
        cells += [("dumbbell_mid", np.array((hz - 5, Y // 2 - 2, X // 4 - 2)), _dumbbell(0)),
                  ("hollow_mid", np.array((hz - 2, Y // 2 - 2, X // 2 - 2)), _hollow())]
        groups = [(name, lo, blk.astype(np.uint32) * np.uint32(k)) for k, (name, lo, blk) in enumerate(cells, 1)]
        k = len(cells)
        # two 3^3 cubes two voxels apart, above `half`: the one that comes LATER in raster order holds the smaller label
        pair = np.zeros((3, 3, 8), dtype=np.uint32)
        pair[:, :, 0:3] = k + 2
        pair[:, :, 5:8] = k + 1
        groups.append(("pair", np.array((hz + 1, Y // 4 - 1, X // 2 - 4)), pair))
        k += 2
        for name, lo, blk in (("dumbbell_end", (Z - 5, Y // 4 - 2, X // 2 - 5), _dumbbell(2)),
                              ("hollow_end", (Z - 5, Y // 2 - 2, X // 2 - 2), _hollow()),
                              ("cup", (Z - 5, Y // 2 - 2, X // 4 - 2), _cup_far_z())):
            k += 1
            groups.append((name, np.array(lo), blk.astype(np.uint32) * np.uint32(k)))
        self.n = k
        self.groups = [(name, np.asarray(lo, np.int64), blk) for name, lo, blk in groups]
        self.label_of = {}
        for name, _, blk in self.groups:
            self.label_of[name] = [int(v) for v in np.unique(blk[blk != 0])]
        self.peak_label = self.label_of["across" if "across" in self.label_of else "below"][0]
        self.crops = self._make_crops(seed)
        self._check()

    def _make_crops(self, seed):
        rng = np.random.default_rng(seed)
        crops = []
        for name, lo, blk in self.groups:
            clo = np.maximum(lo - MARGIN, 0)
            chi = np.minimum(lo + np.array(blk.shape) + MARGIN, self.shape)
            labels = np.zeros(tuple(chi - clo), dtype=np.uint32)
            off = lo - clo
            labels[off[0]:off[0] + blk.shape[0], off[1]:off[1] + blk.shape[1], off[2]:off[2] + blk.shape[2]] = blk
            raw = rng.integers(0, 65536, labels.shape).astype(np.uint16)
            raw[rng.random(labels.shape) < 0.2] = 0  # (the shell's raw condition must matter)
            prob = (rng.integers(0, 2 ** 24, labels.shape).astype(np.float64) * 2.0 ** -24).astype(np.float32)  # (< 1, exact)
            if self.peak_label in self.label_of[name]:
                at = np.argwhere(labels == self.peak_label)
                lin = linear_index(at + clo, self.shape)
                below, above = at[lin < self.half], at[lin >= self.half]
                # two voxels hold the largest value, both at or above `half`: the first in raster order wins
                for v in (above[len(above) // 3], above[-1]) if len(above) >= 3 else (at[0], at[-1]):
                    prob[tuple(v)] = 1.0
            for a in (labels, raw, prob):
                a.setflags(write=False)
            crops.append(Crop(clo, chi, labels, raw, prob))
        return crops

    def _check(self):
        assert MARGIN >= MAX_REACH + 2
        for a, b in itertools.combinations(self.crops, 2):
            assert ((a.hi <= b.lo) | (b.hi <= a.lo)).any(), "two crops meet: the cells are not far enough apart for this shape"
        for c in self.crops:
            assert (c.lo >= 0).all() and (c.hi <= self.shape).all()
            fg = np.argwhere(c.labels != 0)
            for a in range(3):  # a cell may touch a crop face only where that is a face of the volume
                assert fg[:, a].min() >= MARGIN or c.lo[a] == 0
                assert fg[:, a].max() < c.labels.shape[a] - MARGIN or c.hi[a] == self.shape[a]
        lin = self.linear(self.labels().coords)
        assert lin.min() == 0 and lin.max() == self.nvox - 1
        assert ((lin >= self.half - 64) & (lin <= self.half + 64)).any() and (lin >= self.half).any()

    # -- plumbing ------------------------------------------------------------------------------------------------------------------
    def linear(self, coords):
        return linear_index(coords, self.shape)

    def gather(self, volumes, z_lo=0, z_hi=None):
        """per-crop dense volumes (None: skipped) -> Sparse in volume coordinates, in raster order; only planes [z_lo, z_hi), with z
        counted from z_lo"""
        z_hi = self.shape[0] if z_hi is None else z_hi
        cs, vs = [], []
        for c, v in zip(self.crops, volumes):
            if v is None:
                continue
            assert v.shape[:3] == c.labels.shape
            s = sparse_of(v)
            co = s.coords[:, :3] + c.lo
            keep =(co[:, 0] >= z_lo) & (co[:, 0] < z_hi)
            cs.append(co[keep] - np.array((z_lo, 0, 0)))
            vs.append(s.values[keep])
        coords, values = np.concatenate(cs), np.concatenate(vs)
        order = np.argsort(linear_index(coords, (z_hi - z_lo,) + self.shape[1:]), kind="stable")
        return Sparse(coords[order], values[order])

    def dense(self, which="labels"):
        """the whole volume (small layouts only): "labels", "raw" or "prob\""""
        dtype = {"labels": np.uint32, "raw": np.uint16, "prob": np.float32}[which]
        out = np.zeros(self.shape, dtype=dtype)
        for c in self.crops:
            out[c.lo[0]:c.hi[0], c.lo[1]:c.hi[1], c.lo[2]:c.hi[2]] = getattr(c, which)
        return out

    @staticmethod
    def _merge(parts, how):
        """per-crop tables over the labels 0..n -> one: a label lives in one crop, so sums add and extrema combine"""
        out = {}
        for k, op in how.items():
            acc = parts[0][k].copy()
            for p in parts[1:]:
                acc = op(acc, p[k])
            out[k] = acc
        return out

    # -- the expectations ------------------------------------------------------------------------------------------------------------
    def labels(self):
        return self.gather([c.labels for c in self.crops])

    def counts(self, volumes=None):
        """uint32 (n+1): cc_counts of the labels (or of per-crop volumes, the shells); row 0 is the background of the WHOLE volume,
        modulo 2^32 as the device's uint32 counter wraps"""
        volumes = [c.labels for c in self.crops] if volumes is None else volumes
        total = sum(dense_counts(v, self.n) for v in volumes)
        total[0] = (self.nvox - int(total[1:].sum())) % (1 << 32)
        return total.astype(np.uint32)

    def size_filter(self, lo, hi):
        """(K, lut uint32 (n+1), Sparse of the filtered labels): labels with lo <= voxels <= hi (negative: no bound) renumbered in order"""
        counts = self.counts().astype(np.int64)
        keep = np.ones(self.n + 1, dtype=bool)
        if lo >= 0:
            keep &= counts >= lo
        if hi >= 0:
            keep &= counts <= hi
        keep[0] = False
        lut = np.where(keep, np.cumsum(keep), 0).astype(np.uint32)
        return int(keep.sum()), lut, self.relabel(lut)

    def relabel(self, lut):
        return self.gather([np.asarray(lut, np.uint32)[c.labels] for c in self.crops])

    def stats_raw(self):
        ident = {"counts": np.add, "bbmin": np.minimum, "bbmax": np.maximum, "sums": np.add}
        out = self._merge([dense_stats(c.labels, self.n, c.lo) for c in self.crops], ident)
        out["bbmin"][0] = 0  # the background reaches every face; its count and sums are not accumulated
        out["bbmax"][0] = np.array(self.shape) - 1
        return out

    def intensity(self, volumes=None):
        volumes = [c.labels for c in self.crops] if volumes is None else volumes
        how = {"intensity_sum": np.add, "intensity_sumsq": np.add, "intensity_min": np.minimum, "intensity_max": np.maximum}
        return self._merge([dense_intensity(v, c.raw, self.n) for v, c in zip(volumes, self.crops)], how)

    def quantiles(self, levels=(25, 50, 75)):
        parts = [quantile_ref.quantile_reference(c.labels, c.raw, self.n, levels) for c in self.crops]
        values, counts = np.zeros_like(parts[0][0]), np.zeros_like(parts[0][1])
        for v, cnt in parts:  # (a label's voxels lie in one crop)
            assert not (counts[cnt > 0] > 0).any()
            values[cnt > 0] = v[cnt > 0]
            counts += cnt
        return values, counts

    def confidence(self):
        how = {"confidence_sum": np.add, "confidence_min_q": np.minimum, "confidence_max_q": np.maximum, "confidence_peak_index": np.minimum}
        return self._merge([dense_confidence(c.labels, c.prob, self.n, c.lo, self.shape) for c in self.crops], how)

    def shell(self, radius, with_raw):
        """(Sparse of S, the per-crop volumes of S for counts() / intensity())"""
        assert 1 <= radius <= MAX_REACH
        vols = [dense_shell(c.labels, c.raw if with_raw else None, radius) for c in self.crops]
        return self.gather(vols), vols

    def shape_stats(self, buffer=None, keep=None, z_abs0=0):
        """cc_shape of the planes `buffer` = (b0, b1) of the volume handed over as one buffer (default: all), of which the planes
        keep = (first, planes) - counted inside the buffer - are measured, the buffer's first plane standing at absolute z_abs0"""
        b0, b1 = buffer or (0, self.shape[0])
        first, planes = keep or (0, b1 - b0)
        parts = []
        for c in self.crops:
            z0, z1 = max(int(c.lo[0]), b0), min(int(c.hi[0]), b1)
            if z0 >= z1:
                continue
            sub = c.labels[z0 - c.lo[0]:z1 - c.lo[0]]
            m0, m1 = max(b0 + first, z0), min(b0 + first + planes, z1)
            if m0 >= m1:
                continue
            parts.append(dense_shape(sub, self.n, (m0 - z0, m1 - z0), (z_abs0 + z0 - b0, c.lo[1], c.lo[2])))
        keys = ("shape_counts", "shape_sums", "shape_moments", "shape_faces", "shape_surface_voxels")
        return self._merge(parts, {k: np.add for k in keys})

    def split(self, depth, min_core=1):
        """(K, parent uint32 (K+1), number of labels split, Sparse of the renumbered pieces): the pieces of all crops numbered in
        raster order of their first voxel in the volume"""
        assert 1 <= depth <= MAX_REACH
        found, n_split = [], 0  # (first linear index, parent, crop, local piece)
        outs = []
        for i, c in enumerate(self.crops):
            r = split_ref.split_reference(c.labels, self.n, depth, min_core)
            outs.append(r["out"])
            n_split += r["n_split"]
            s = sparse_of(r["out"])
            lin = self.linear(s.coords + c.lo)
            for j in range(1, r["K"] + 1):
                found.append((int(lin[s.values == j].min()), int(r["parent"][j]), i, j))
        found.sort()
        parent = np.zeros(len(found) + 1, dtype=np.uint32)
        luts = [np.zeros(int(o.max()) + 1, dtype=np.uint32) for o in outs]
        for new, (_, par, i, j) in enumerate(found, 1):
            parent[new] = par
            luts[i][j] = new
        return len(found), parent, n_split, self.gather([lut[o] for lut, o in zip(luts, outs)])

    def runs(self, volumes=None):
        """label_runs.encode_runs' dict of the whole volume, from the runs of the crops (row_start: Z * Y + 1 uint64 - rows, not
        voxels)"""
        from delivr_cfos_amd import label_runs

        Z, Y, X = self.shape
        volumes = [c.labels for c in self.crops] if volumes is None else volumes
        rows, x0, x1, lab = [], [], [], []
        for c, v in zip(self.crops, volumes):
            r = label_runs.encode_runs(v)
            per_row = np.diff(r["row_start"].astype(np.int64))
            local = np.repeat(np.arange(len(per_row), dtype=np.int64), per_row)
            z, y = local // v.shape[1] + c.lo[0], local % v.shape[1] + c.lo[1]
            rows.append(z * Y + y)
            x0.append(r["x0"].astype(np.int64) + c.lo[2])
            x1.append(r["x1"].astype(np.int64) + c.lo[2])
            lab.append(r["label"])
        rows, x0, x1, lab = (np.concatenate(a) for a in (rows, x0, x1, lab))
        order = np.lexsort((x0, rows))
        row_start = np.zeros(Z * Y + 1, dtype=np.uint64)
        np.cumsum(np.bincount(rows, minlength=Z * Y).astype(np.uint64), out=row_start[1:])
        return {"row_start": row_start, "x0": x0[order].astype(np.uint16), "x1": x1[order].astype(np.uint16),
                "label": lab[order].astype(np.uint32), "shape": (Z, Y, X)}

    def painted(self, lut, z_lo=0, z_hi=None):
        """Sparse of lut[labels] on the planes [z_lo, z_hi) (paint_labels / paint_runs; a lut of (n_lut, 3): three of them)"""
        lut = np.asarray(lut)
        if lut.ndim == 2:
            return [self.painted(lut[:, k], z_lo, z_hi) for k in range(lut.shape[1])]
        return self.gather([paint_ref.paint_by_label(c.labels, lut) for c in self.crops], z_lo, z_hi)

    def decoded(self, z_lo=0, z_hi=None):
        return self.gather([c.labels for c in self.crops], z_lo, z_hi)

    def boxes(self):
        """(n_boxes, 6) int32 half-open boxes in painting order: a large one around the bar (above the painter's own-launch
        threshold at the full sizes), then the bounding boxes of the bar and of the cells at the limits"""
        Z, Y, X = self.shape
        bz, _, bx, _ = self.bar
        out = [[bz - 3, bz + 4, 0, Y, bx - 3, bx + 4]]
        for name in ("bar", "origin", "below", "above", "across", "end"):
            for _, lo, blk in (g for g in self.groups if g[0] == name):
                hi = lo + np.array(blk.shape)
                out.append([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]])
        return np.array(out, dtype=np.int32)

    def boxed(self, values):
        """Sparse of paint_boxes(labels != 0, boxes(), values)"""
        boxes = self.boxes().astype(np.int64)
        vols = []
        for c in self.crops:
            local = boxes.copy()
            for a in range(3):
                local[:, 2 * a] = np.clip(boxes[:, 2 * a] - c.lo[a], 0, c.labels.shape[a])
                local[:, 2 * a + 1] = np.clip(boxes[:, 2 * a + 1] - c.lo[a], 0, c.labels.shape[a])
            vols.append(dense_boxes((c.labels != 0).astype(np.uint8), local, np.asarray(values)))
        return self.gather(vols)

    def second(self):
        """(per-crop volumes of a second labelling, n_b): every cell moved by one voxel along each axis (what leaves the volume is
        lost; the bar, one voxel wide, no longer meets itself), and the dumbbell across `half` cut in two: the second half of its
        voxels in raster order is the new label n + 1"""
        cut_label = self.label_of["dumbbell_mid"][0]
        vols = []
        for c in self.crops:
            b = np.zeros_like(c.labels)
            b[1:, 1:, 1:] = c.labels[:-1, :-1, :-1]
            at = np.argwhere(b == cut_label)
            if len(at):
                cut = at[len(at) // 2:]
                b[cut[:, 0], cut[:, 1], cut[:, 2]] = self.n + 1
            vols.append(b)
        return vols, self.n + 1

    def overlap(self):
        """compare_cells.overlap_table_np's dict of the labels against second()"""
        from delivr_cfos_amd.compare_cells import overlap_table_np

        vols, n_b = self.second()
        pairs, segments = {}, 0
        for c, b in zip(self.crops, vols):
            t = overlap_table_np(c.labels, b, self.n, n_b)
            segments += t["segments"]
            for a_, b_, v in zip(t["a"], t["b"], t["voxels"]):
                pairs[(int(a_), int(b_))] = pairs.get((int(a_), int(b_)), 0) + int(v)
        keys = sorted(pairs)
        return {"a": np.array([k[0] for k in keys], np.uint32), "b": np.array([k[1] for k in keys], np.uint32),
                "voxels": np.array([pairs[k] for k in keys], np.uint64), "segments": segments}

    def filled(self, fill_value=2):
        """(voxels_filled, holes, Sparse of the mask (labels != 0) after fill_holes): a crop's faces inside the volume lie in
        background that reaches the volume's faces around the crops, a clipped face is the volume's own"""
        voxels = holes = 0
        vols = []
        for c in self.crops:
            mask = (c.labels != 0).astype(np.uint8)
            _, v, h = fill_ref.fill_reference(mask)
            voxels, holes = voxels + v, holes + h
            vols.append(fill_ref.expected_bytes(mask, fill_value))
        return voxels, holes, self.gather(vols)
