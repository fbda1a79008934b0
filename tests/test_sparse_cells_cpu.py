"""tests/helpers/sparse_cells.py pinned on the host: the cell layouts of tests/test_gpu_index_limits.py scaled down to a few hundred
thousand voxels - the same relative positions: at the origin, across the middle index (a plane's first voxel in one shape, inside a
row in the other), at the last voxel, against the faces - and every sparse expectation compared with the dense reference applied to
the whole small volume.  The full-size layouts are built too (a layout never holds a volume) and the facts the GPU tests rely on are
asserted about them."""
import importlib.util
import os

import numpy as np
import pytest

from delivr_cfos_amd import label_runs
from delivr_cfos_amd.compare_cells import overlap_table_np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, *parts, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sc = _load("sparse_cells", "helpers")

# (shape, half): the middle index starts a plane / lies inside a row with an odd X
SMALL = {"plane": ((44, 96, 100), 22 * 96 * 100), "row": ((42, 90, 109), (21 * 90 + 8) * 109 + 97)}
FULL = {"plane": ((1024, 2048, 2048), 1 << 31), "row": ((1000, 2050, 2095), 1 << 31)}


@pytest.fixture(scope="module", params=sorted(SMALL))
def small(request):
    lay = sc.Layout(*SMALL[request.param])
    dense = {k: lay.dense(k) for k in ("labels", "raw", "prob")}
    for a in dense.values():
        a.setflags(write=False)
    return lay, dense


def _same_sparse(got, dense_volume):
    want = sc.sparse_of(dense_volume)
    assert got.coords.dtype == np.int64 and got.values.dtype == dense_volume.dtype
    np.testing.assert_array_equal(got.coords, want.coords)
    np.testing.assert_array_equal(got.values, want.values)
    assert len(got.values) == int(np.count_nonzero(dense_volume))


def _same_tables(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_the_layout_holds_the_cells_the_limits_need(small):
    lay, d = small
    L = d["labels"]
    Z, Y, X = lay.shape
    assert 2e5 < lay.nvox < 5e5
    _same_sparse(lay.labels(), L)
    assert L[0, 0, 0] == 1 and L[-1, -1, -1] == lay.label_of["end"][0]
    flat = L.ravel()
    assert flat[lay.half] != 0 and flat[lay.half - 1] != 0  # both sides of the middle index are foreground
    if lay.half % (Y * X):
        assert flat[lay.half] == flat[lay.half - 1] and flat[lay.half - 8] == flat[lay.half + 8]  # one run holds the crossing
    assert sorted(np.unique(L)) == list(range(lay.n + 1))
    assert int((d["raw"] != 0).sum()) > 0 and int((d["prob"] != 0).sum()) > 0
    q = d["prob"].astype(np.float64) * 2 ** 24
    assert (q == np.rint(q)).all() and d["prob"].max() == 1.0
    top = np.flatnonzero((d["prob"].ravel() == 1.0) & (flat == lay.peak_label))
    assert len(top) == 2 and top.min() >= lay.half  # the tie is decided above the middle index


def test_the_full_size_layouts_reach_the_index_limits():
    for name, (shape, half) in FULL.items():
        lay = sc.Layout(shape, half)
        lin = lay.linear(lay.labels().coords)
        assert lin.dtype == np.uint64 and int(lin.max()) == lay.nvox - 1 and int(lin.min()) == 0
        assert half in set(int(v) for v in lin) and half - 1 in set(int(v) for v in lin)
        assert int((lin >= half).sum()) > 1800  # the bar and everything in the last planes
        b = lay.boxes().astype(np.int64)
        assert (b[0, 1] - b[0, 0]) * (b[0, 3] - b[0, 2]) * (b[0, 5] - b[0, 4]) > 1 << 16  # the painter's own-launch threshold
    assert sc.Layout(*FULL["plane"]).nvox == 1 << 32
    row = sc.Layout(*FULL["row"])
    assert row.nvox == 4294750000 and np.unravel_index(1 << 31, row.shape) == (500, 51, 1803)
    run = [g for g in row.groups if g[0] == "across"][0]
    assert run[1][2] == 1795 and run[1][2] + run[2].shape[2] - 1 == 1811


def test_counts_size_filter_and_relabel(small):
    lay, d = small
    L = d["labels"]
    counts = np.bincount(L.ravel(), minlength=lay.n + 1)
    np.testing.assert_array_equal(lay.counts(), counts.astype(np.uint32))
    lo, hi = 60, 200
    keep = (counts >= lo) & (counts <= hi)
    keep[0] = False
    assert 2 <= keep.sum() < lay.n  # some stay, some go
    lut = np.where(keep, np.cumsum(keep), 0).astype(np.uint32)
    K, got_lut, sp = lay.size_filter(lo, hi)
    assert K == int(keep.sum())
    np.testing.assert_array_equal(got_lut, lut)
    _same_sparse(sp, lut[L])
    K2, _, sp2 = lay.size_filter(-1, 100)
    keep2 = counts <= 100
    keep2[0] = False
    assert K2 == int(keep2.sum())
    _same_sparse(sp2, np.where(keep2, np.cumsum(keep2), 0).astype(np.uint32)[L])
    perm = np.r_[0, np.random.default_rng(1).permutation(lay.n) + 1].astype(np.uint32)
    _same_sparse(lay.relabel(perm), perm[L])


def test_stats_intensity_quantiles_confidence(small):
    lay, d = small
    L, raw, prob = d["labels"], d["raw"], d["prob"]
    want = sc.dense_stats(L, lay.n)
    want["bbmin"][0], want["bbmax"][0] = 0, np.array(lay.shape) - 1
    _same_tables(lay.stats_raw(), want)
    # the dense statistics against numpy's own words for one label
    k = lay.label_of["bar"][0]
    at = np.argwhere(L == k)
    assert want["counts"][k] == len(at) and (want["bbmin"][k] == at.min(0)).all() and (want["bbmax"][k] == at.max(0)).all()
    assert (want["sums"][k] == at.sum(0)).all()
    _same_tables(lay.intensity(), sc.dense_intensity(L, raw, lay.n))
    v = raw[L == k].astype(np.int64)
    got = lay.intensity()
    assert (got["intensity_sum"][k], got["intensity_sumsq"][k], got["intensity_min"][k], got["intensity_max"][k]) == (
        v.sum(), (v * v).sum(), v.min(), v.max())
    for levels in ((25, 50, 75), (0, 100)):
        gv, gc = lay.quantiles(levels)
        wv, wc = sc.quantile_ref.quantile_reference(L, raw, lay.n, levels)
        np.testing.assert_array_equal(gv, wv)
        np.testing.assert_array_equal(gc, wc)
    conf = lay.confidence()
    _same_tables(conf, sc.dense_confidence(L, prob, lay.n))
    p = lay.peak_label
    q = sc.quantise(prob).ravel()
    mine = np.flatnonzero(L.ravel() == p)
    assert conf["confidence_max_q"][p] == 1 << 24 and conf["confidence_peak_index"][p] == mine[np.argmax(q[mine])] >= lay.half
    assert conf["confidence_peak_index"][0] == sc.NO_PEAK and conf["confidence_min_q"][0] == 0xFFFFFFFF


@pytest.mark.parametrize("radius,with_raw", [(1, False), (3, True)])
def test_shell(small, radius, with_raw):
    lay, d = small
    L, raw = d["labels"], d["raw"]
    S = sc.dense_shell(L, raw if with_raw else None, radius)
    sp, vols = lay.shell(radius, with_raw)
    _same_sparse(sp, S)
    want_counts = np.bincount(S.ravel(), minlength=lay.n + 1).astype(np.uint32)
    np.testing.assert_array_equal(lay.counts(vols), want_counts)
    _same_tables(lay.intensity(vols), sc.dense_intensity(S, raw, lay.n))
    if radius == 3:  # between the two cells of the pair the smaller label wins, and it is the cell that comes later in the row
        a, b = sorted(lay.label_of["pair"])
        name, lo, blk = [g for g in lay.groups if g[0] == "pair"][0]
        between = sc.dense_expand(L, 3)[lo[0] + 1, lo[1] + 1, lo[2] + 3:lo[2] + 5]
        assert blk[0, 0, 0] == b and blk[0, 0, -1] == a and list(between) == [b, a]
        far = sc.dense_expand(L, 3)[lo[0] + 1, lo[1] + 4, lo[2] + 3:lo[2] + 5]  # ... and at equal distance from both
        assert list(far) == [a, a]


def test_shape_whole_and_slab(small):
    lay, d = small
    L = d["labels"]
    shape_cpu = _load("test_shape_cpu")
    _same_tables(lay.shape_stats(), sc.dense_shape(L, lay.n))
    _same_tables(sc.dense_shape(L, lay.n), shape_cpu._accumulate(L, lay.n))
    b0, b1, first, planes, z_abs0 = lay.hz - 8, lay.hz + 8, 3, 10, 40000
    got = lay.shape_stats((b0, b1), (first, planes), z_abs0)
    _same_tables(got, shape_cpu._accumulate(L[b0:b1], lay.n, (first, first + planes), z_abs0))
    k = lay.label_of["dumbbell_mid"][0]  # cut by the measured planes: its last plane is a neighbour only
    assert 0 < got["shape_counts"][k] < int((L == k).sum())


def test_split(small):
    lay, d = small
    L = d["labels"]
    want = sc.split_ref.split_reference(L, lay.n, 2)
    K, parent, n_split, sp = lay.split(2)
    assert (K, n_split) == (want["K"], want["n_split"]) == (lay.n + 2, 2)
    np.testing.assert_array_equal(parent, want["parent"])
    _same_sparse(sp, want["out"])
    halves = np.flatnonzero(parent == lay.label_of["dumbbell_mid"][0])
    first = [int(lay.linear(sp.coords[sp.values == j]).min()) for j in halves]
    assert len(halves) == 2 and first[0] < lay.half < first[1]  # the two cores lie on either side of the middle index


def test_runs_decode_and_paint(small):
    lay, d = small
    L = d["labels"]
    want = label_runs.encode_runs(L)
    got = lay.runs()
    assert got["shape"] == want["shape"]
    for k in ("row_start", "x0", "x1", "label"):
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    z0 = lay.hz + 1
    _same_sparse(lay.decoded(), L)
    _same_sparse(lay.decoded(z0, lay.shape[0]), L[z0:])
    rng = np.random.default_rng(2)
    rgb = rng.integers(1, 256, (lay.n + 1, 3)).astype(np.uint8)
    u16 = rng.integers(1, 65536, lay.n + 1).astype(np.uint16)
    for c, sp in enumerate(lay.painted(rgb)):
        _same_sparse(sp, sc.paint_ref.paint_by_label(L, rgb[:, c]))
    _same_sparse(lay.painted(u16), sc.paint_ref.paint_by_label(L, u16))
    _same_sparse(lay.painted(u16, z0, lay.shape[0]), sc.paint_ref.paint_by_label(L[z0:], u16))
    short = u16[:lay.n - 1]  # labels at or beyond the table paint 0
    _same_sparse(lay.painted(short), sc.paint_ref.paint_by_label(L, short))


def test_boxes(small):
    lay, d = small
    L = d["labels"]
    boxes = lay.boxes()
    assert boxes.dtype == np.int32 and (boxes[:, 0::2] >= 0).all() and (boxes[:, 1::2] <= np.array(lay.shape)).all()
    rng = np.random.default_rng(3)
    for dtype, top in ((np.uint8, 256), (np.uint16, 65536)):
        values = rng.integers(1, top, len(boxes)).astype(dtype)
        want = sc.dense_boxes((L != 0).astype(np.uint8), boxes, values)
        _same_sparse(lay.boxed(values), want)
        bar = L == lay.label_of["bar"][0]
        assert (want[bar] == values[1]).all()  # the bar's own box is painted over the large one
        assert not want[L == lay.label_of["hollow_mid"][0]].any()


def test_overlap(small):
    lay, d = small
    L = d["labels"]
    vols, n_b = lay.second()
    B = np.zeros(lay.shape, dtype=np.uint32)
    for c, v in zip(lay.crops, vols):
        B[c.lo[0]:c.hi[0], c.lo[1]:c.hi[1], c.lo[2]:c.hi[2]] = v
    shifted = np.zeros_like(L)
    shifted[1:, 1:, 1:] = L[:-1, :-1, :-1]
    assert ((B != 0) == (shifted != 0)).all() and n_b == lay.n + 1 and int((B == n_b).sum()) == 251 - 251 // 2
    want = overlap_table_np(L, B, lay.n, n_b)
    got = lay.overlap()
    assert got["segments"] == want["segments"] > 0
    cut, bar = lay.label_of["dumbbell_mid"][0], lay.label_of["bar"][0]
    assert [int(b) for a, b in zip(want["a"], want["b"]) if a == cut] == [cut, n_b]  # the cell that was cut meets both halves
    assert bar not in want["a"] and len(want["a"]) == lay.n  # the bar meets nothing, every other cell its own shifted self
    for k in ("a", "b", "voxels"):
        assert got[k].dtype == want[k].dtype
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_fill_holes(small):
    lay, d = small
    mask = (d["labels"] != 0).astype(np.uint8)
    _, voxels, holes = sc.fill_ref.fill_reference(mask)
    gv, gh, sp = lay.filled(2)
    assert (gv, gh) == (voxels, holes) == (54, 2)
    want = sc.fill_ref.expected_bytes(mask, 2)
    _same_sparse(sp, want)
    name, lo, blk = [g for g in lay.groups if g[0] == "cup"][0]
    assert lo[0] + blk.shape[0] == lay.shape[0] and want[lo[0] + 2, lo[1] + 2, lo[2] + 2] == 0  # open to the far z face: not filled
    mid = [g for g in lay.groups if g[0] == "hollow_mid"][0]
    cavity = lay.linear(np.argwhere(want == 2))
    assert cavity.min() < lay.half <= cavity[cavity < lay.linear([mid[1] + 5])[0]].max()  # the first cavity straddles the middle
