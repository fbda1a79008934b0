"""The per-cell kernels of count_blobs, compare_cells and blob_highlighter at the 32-bit index limits: label volumes of
(1024, 2048, 2048) = 2^32 voxels exactly and of (1000, 2050, 2095) = 4 294 750 000 voxels with rows of odd length, where index 2^31
lies inside row (500, 51).  Every voxel index in [2^31, 2^32) needs unsigned or 64-bit arithmetic there, and the voxel count of the
first shape wraps to 0 in 32 bits - what the small volumes of the other test files cannot see.

The labels are painted straight into a zeroed device tensor from the cell list of tests/helpers/sparse_cells.py (a box at linear
index 0, boxes across index 2^31, a box that ends at the last voxel, a long bar, dumbbells, hollow cubes, a cup, two cells closer than
the shell radius), not produced by ccl26, so that a failure names the kernel under test.  The expectations come from that list alone
(tests/test_sparse_cells_cpu.py pins them on the host); a whole-volume output is proven equal with two device reductions:
count_nonzero(out) == k and out[coords] == values.  Everything is integer work and compared exactly.

Needs one MI355X with 64 GiB of free HBM for torch tensors (the shared labels and raw volume are 24 GiB of it; the engine's own
workspaces come on top) - a device that cannot hold them FAILS the tests."""
import importlib.util
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GIB = 1 << 30
NEED_GIB = 64
SHAPES = {"plane": ((1024, 2048, 2048), 1 << 31), "row": ((1000, 2050, 2095), 1 << 31)}
SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.uint8): np.uint8, np.dtype(np.float32): np.float32}


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sc = _helper("sparse_cells")


def _dev(a):
    """a host array on the device, unsigned payloads in torch's signed types"""
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(SIGNED[a.dtype]).copy()).cuda()


def _paint(t, lay, volumes):
    """the per-crop volumes written into the device tensor t (zero elsewhere already)"""
    for c, v in zip(lay.crops, volumes):
        t[c.lo[0]:c.hi[0], c.lo[1]:c.hi[1], c.lo[2]:c.hi[2]] = _dev(v)


def _signed(t):
    import torch

    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _check_sparse(out, sp, what):
    """out == the volume sp describes: as many non-zero voxels, and the listed ones hold the listed values"""
    import torch

    out = _signed(out)
    # (64 planes at a time: count_nonzero's temporaries take nine bytes per element of its input)
    k = int(sum(torch.count_nonzero(out[z:z + 64]) for z in range(0, out.shape[0], 64)))
    assert k == len(sp.values), f"{what}: {k} non-zero voxels, expected {len(sp.values)}"
    at = torch.from_numpy(sp.coords).cuda()
    got = out[at[:, 0], at[:, 1], at[:, 2]]
    want = _dev(sp.values)
    bad = torch.nonzero(got != want).flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {len(sp.values)} listed voxels differ, the first at (z, y, x) = "
                              f"{sp.coords[int(bad[0])].tolist()}: {int(got[bad[0]])} != {int(want[bad[0]])}")


def _reaches_the_limits(lay, sp=None, z_lo=0):
    """the cell list reaches the last voxel and the 64 voxels either side of index 2^31; an output (sp) has voxels at or above it"""
    lin = lay.linear(lay.labels().coords)
    assert int(lin.max()) == lay.nvox - 1 and lay.nvox > (1 << 32) - (1 << 20)
    assert ((lin >= (1 << 31) - 64) & (lin <= (1 << 31) + 64)).any()
    if sp is not None:
        assert int(lay.linear(sp.coords + np.array((z_lo, 0, 0))).max()) >= 1 << 31


def _same_tables(got, want, keys=None):
    for k in keys or want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _free():
    import torch

    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=sorted(SHAPES))
def vol(request, eng):
    """the layout of one shape, its labels (16 GiB) and raw volume (8 GiB) on the device - shared, counted in NEED_GIB; a test that
    changes the labels in place puts them back with restore()"""
    import torch

    lay = sc.Layout(*SHAPES[request.param])
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_GIB * GIB:
        pytest.fail(f"the index-limit tests need {NEED_GIB} GiB of free device memory for volumes of {lay.nvox} voxels, "
                    f"{free / GIB:.1f} GiB are free")
    v = types.SimpleNamespace(lay=lay, name=request.param)
    v.labels = torch.zeros(lay.shape, dtype=torch.int32, device="cuda")
    v.raw = torch.zeros(lay.shape, dtype=torch.uint16, device="cuda")
    _paint(v.raw, lay, [c.raw for c in lay.crops])

    def restore():
        v.labels.zero_()
        _paint(v.labels, lay, [c.labels for c in lay.crops])

    v.restore = restore
    restore()
    torch.cuda.synchronize()
    yield v
    del v.labels, v.raw
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def peak(request):
    """prints the peak of torch's allocations during the test (the engine's workspaces are not torch's: not in it)"""
    import torch

    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"\nPEAK {request.node.name}: {torch.cuda.max_memory_allocated() / GIB:.2f} GiB")
    assert torch.cuda.max_memory_allocated() <= NEED_GIB * GIB


def test_the_painted_labels_are_the_layout(vol):
    _reaches_the_limits(vol.lay, vol.lay.labels())
    _check_sparse(vol.labels, vol.lay.labels(), "labels")
    _check_sparse(vol.raw, vol.lay.gather([c.raw for c in vol.lay.crops]), "raw")


def test_cc_counts_and_size_filter(vol, eng):
    lay = vol.lay
    _reaches_the_limits(lay)
    counts = eng.cc_counts(vol.labels, lay.n)
    np.testing.assert_array_equal(counts.cpu().numpy().view(np.uint32), lay.counts())
    try:
        for lo, hi in ((60, 200), (-1, 100)):
            K, lut, sp = lay.size_filter(lo, hi)
            assert 2 <= K < lay.n
            _reaches_the_limits(lay, sp)
            assert eng.cc_size_filter(vol.labels, lay.n, lo, hi) == K
            _check_sparse(vol.labels, sp, f"size filter [{lo}, {hi}]")
            vol.restore()
    finally:
        vol.restore()
        del counts
        _free()


def test_cc_stats_raw_on_painted_labels(vol, eng):
    _reaches_the_limits(vol.lay)
    _same_tables(eng.cc_stats_raw(vol.labels, vol.lay.n), vol.lay.stats_raw())


@pytest.mark.parametrize("padded", [False, True])
def test_cc_intensity_and_quantiles(vol, eng, padded):
    """raw contiguous, and as a view into a buffer one row and eight voxels larger: pitch_y > X, pitch_z > Y * pitch_y"""
    import torch

    lay = vol.lay
    Z, Y, X = lay.shape
    _reaches_the_limits(lay)
    raw = vol.raw
    try:
        if padded:
            buf = torch.zeros((Z, Y + 1, X + 8), dtype=torch.uint16, device="cuda")
            raw = buf[:, :Y, :X]
            _paint(raw, lay, [c.raw for c in lay.crops])
            assert raw.stride(1) > X and raw.stride(0) > Y * raw.stride(1)
        _same_tables(eng.cc_intensity(vol.labels, raw, lay.n), lay.intensity())
        for levels in ((25, 50, 75), (0, 100)):
            values, counts = eng.cc_quantiles(vol.labels, raw, lay.n, levels)
            want_values, want_counts = lay.quantiles(levels)
            np.testing.assert_array_equal(values, want_values)
            np.testing.assert_array_equal(counts, want_counts)
    finally:
        buf = raw = None
        _free()


def test_cc_confidence(vol, eng):
    import torch

    lay = vol.lay
    _reaches_the_limits(lay)
    prob = torch.zeros(lay.shape, dtype=torch.float32, device="cuda")
    try:
        _paint(prob, lay, [c.prob for c in lay.crops])
        got = eng.cc_confidence(vol.labels, prob, lay.n)
        want = lay.confidence()
        assert got["confidence_peak_index"].dtype == np.uint64
        peak_at = int(want["confidence_peak_index"][lay.peak_label])
        assert 1 << 31 <= peak_at < lay.nvox and int(want["confidence_max_q"][lay.peak_label]) == 1 << 24  # the tie, above 2^31
        assert int(want["confidence_peak_index"][1:].max()) >= lay.nvox - 5 * lay.shape[2] * lay.shape[1]  # a peak in the last planes
        _same_tables(got, want)
    finally:
        del prob
        _free()


@pytest.mark.parametrize("radius,with_raw", [(1, False), (3, True)])
def test_cc_shell(vol, eng, radius, with_raw):
    lay = vol.lay
    sp, vols = lay.shell(radius, with_raw)
    _reaches_the_limits(lay, sp)
    shell = eng.cc_shell(vol.labels, radius, vol.raw if with_raw else None)
    try:
        _check_sparse(shell, sp, f"shell of radius {radius}")
        np.testing.assert_array_equal(eng.cc_counts(shell, lay.n).cpu().numpy().view(np.uint32), lay.counts(vols))
        _same_tables(eng.cc_intensity(shell, vol.raw, lay.n), lay.intensity(vols))
    finally:
        del shell
        _free()


def test_cc_shape_whole_and_slab(vol, eng):
    lay = vol.lay
    _reaches_the_limits(lay)
    _same_tables(eng.cc_shape(vol.labels, lay.n), lay.shape_stats())
    b0, b1, keep, z_abs0 = lay.hz - 8, lay.hz + 8, (3, 10), 40000  # a slab around plane hz = 512 / 500, its own absolute z
    assert b0 + keep[0] <= lay.hz < b0 + keep[0] + keep[1]
    want = lay.shape_stats((b0, b1), keep, z_abs0)
    assert int(want["shape_counts"].sum()) > 0
    _same_tables(eng.cc_shape(vol.labels[b0:b1], lay.n, keep=keep, z_abs0=z_abs0), want)


def test_cc_split(vol, eng):
    lay = vol.lay
    K, parent, n_split, sp = lay.split(2)
    _reaches_the_limits(lay, sp)
    assert (K, n_split) == (lay.n + 2, 2)
    try:
        got_K, got_parent, got_split = eng.cc_split(vol.labels, lay.n, 2)
        assert (got_K, got_split) == (K, n_split)
        assert got_parent.dtype == np.uint32
        np.testing.assert_array_equal(got_parent, parent)
        _check_sparse(vol.labels, sp, "split pieces")
    finally:
        vol.restore()
        _free()


def test_cc_runs_encode_decode_and_paint_runs(vol, eng):
    lay = vol.lay
    Z = lay.shape[0]
    _reaches_the_limits(lay)
    want = lay.runs()
    runs = eng.cc_runs_encode(vol.labels)
    assert runs["row_start"].dtype == np.uint64 and tuple(runs["shape"]) == lay.shape
    for k in ("row_start", "x0", "x1", "label"):
        assert runs[k].dtype == want[k].dtype and runs[k].shape == want[k].shape, k
        np.testing.assert_array_equal(runs[k], want[k], err_msg=k)
    rng = np.random.default_rng(4)
    rgb = rng.integers(1, 256, (lay.n + 1, 3)).astype(np.uint8)
    u16 = rng.integers(1, 65536, lay.n + 1).astype(np.uint16)
    z0 = lay.hz + 1  # a plane range that starts above index 2^31
    assert z0 * lay.shape[1] * lay.shape[2] > 1 << 31
    for lo, hi in ((0, Z), (z0, Z)):
        out = planes = gray = None
        try:
            sp = lay.decoded(lo, hi)
            _reaches_the_limits(lay, sp, lo)
            out = eng.cc_runs_decode(want, lo, hi)
            _check_sparse(out, sp, f"decoded planes [{lo}, {hi})")
            out = None
            _free()
            planes, gray = eng.paint_runs(want, lo, hi, rgb=rgb, u16=u16)
            for c, spc in enumerate(lay.painted(rgb, lo, hi)):
                _check_sparse(planes[c], spc, f"paint_runs [{lo}, {hi}) channel {c}")
            _check_sparse(gray, lay.painted(u16, lo, hi), f"paint_runs [{lo}, {hi}) uint16")
        finally:
            out = planes = gray = None
            _free()


def test_paint_labels(vol, eng):
    lay = vol.lay
    rng = np.random.default_rng(5)
    rgb = rng.integers(1, 256, (lay.n + 1, 3)).astype(np.uint8)
    u16 = rng.integers(1, 65536, lay.n + 1).astype(np.uint16)
    _reaches_the_limits(lay, lay.painted(u16))
    planes, gray = eng.paint_labels(vol.labels, rgb=rgb, u16=u16)
    try:
        for c, sp in enumerate(lay.painted(rgb)):
            _check_sparse(planes[c], sp, f"paint_labels channel {c}")
        _check_sparse(gray, lay.painted(u16), "paint_labels uint16")
    finally:
        del planes, gray
        _free()


def test_paint_boxes(vol, eng):
    import torch

    lay = vol.lay
    boxes = lay.boxes()
    b = boxes.astype(np.int64)
    sizes = (b[:, 1] - b[:, 0]) * (b[:, 3] - b[:, 2]) * (b[:, 5] - b[:, 4])
    assert sizes[0] > 1 << 16 and (sizes[1:] < 1 << 16).all()  # one box above the painter's own-launch threshold, small ones at the limits
    rng = np.random.default_rng(6)
    v8 = rng.integers(1, 256, len(boxes)).astype(np.uint8)
    v16 = rng.integers(1, 65536, len(boxes)).astype(np.uint16)
    sp8, sp16 = lay.boxed(v8), lay.boxed(v16)
    _reaches_the_limits(lay, sp8)
    assert int(lay.linear(sp8.coords).max()) == lay.nvox - 1 and int(lay.linear(sp8.coords).min()) == 0
    bin_img = torch.zeros(lay.shape, dtype=torch.uint8, device="cuda")
    o8 = o16 = None
    try:
        _paint(bin_img, lay, [(c.labels != 0).astype(np.uint8) for c in lay.crops])
        o8, o16 = eng.paint_boxes(bin_img, boxes, [v8, v16])
        _check_sparse(o8, sp8, "paint_boxes uint8")
        _check_sparse(o16, sp16, "paint_boxes uint16")
    finally:
        del bin_img, o8, o16
        _free()


def test_cc_overlap(vol, eng):
    import torch

    lay = vol.lay
    _reaches_the_limits(lay)
    vols, n_b = lay.second()
    want = lay.overlap()
    assert len(want["a"]) == lay.n and int(want["b"].max()) == n_b and want["segments"] > len(want["a"])  # (the cut cell: two partners)
    other = torch.zeros(lay.shape, dtype=torch.int32, device="cuda")
    try:
        _paint(other, lay, vols)
        got = eng.cc_overlap(vol.labels, lay.n, other, n_b)
        assert got["segments"] == want["segments"]
        _same_tables(got, want, ("a", "b", "voxels"))
    finally:
        del other
        _free()


def test_fill_holes_and_count_marked(vol, eng):
    import torch

    lay = vol.lay
    voxels, holes, sp = lay.filled(2)
    _reaches_the_limits(lay, sp)
    assert (voxels, holes) == (54, 2)
    mask = torch.zeros(lay.shape, dtype=torch.uint8, device="cuda")
    marked = None
    try:
        _paint(mask, lay, [(c.labels != 0).astype(np.uint8) for c in lay.crops])
        assert eng.fill_holes(mask, 2) == (voxels, holes)
        _check_sparse(mask, sp, "filled mask")
        name, lo, blk = [g for g in lay.groups if g[0] == "cup"][0]
        assert lo[0] + blk.shape[0] == lay.shape[0]
        assert int(mask[lo[0] + 1:, lo[1] + 1:lo[1] + 4, lo[2] + 1:lo[2] + 4].sum()) == 0  # the cup's cavity, open to the far z face
        marked = eng.cc_count_marked(vol.labels, mask, lay.n, 2).cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(marked, np.r_[voxels, np.zeros(lay.n)].astype(np.uint32))  # the holes are background in the labels
        cells = lay.counts()
        cells[0] = 0
        marked = eng.cc_count_marked(vol.labels, mask, lay.n, 1).cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(marked, cells)
    finally:
        del mask
        _free()


def test_relabel(vol, eng):
    lay = vol.lay
    lut = np.r_[0, np.random.default_rng(7).permutation(lay.n) + 1].astype(np.uint32)
    sp = lay.relabel(lut)
    _reaches_the_limits(lay, sp)
    try:
        eng.relabel(vol.labels, lut)
        _check_sparse(vol.labels, sp, "relabelled")
    finally:
        vol.restore()
        _free()
