"""Painting from the labels on the device (dlv_paint_labels_dev / dlv_paint_runs_dev, HipEngine.paint_labels / paint_runs) and
blob_highlighter's settings["mi355x"]["paint_from"] = "labels".

The reference of every case is tests/helpers/paint_reference.py (numpy: lut[label], 0 for label 0 and for labels beyond the table) on
the dense labels - never the device's own output.  Integer work only: every comparison is exact equality.  Every test asserts the
property of its input that it is there for.

The kernels walk rows with one wave per row in sweeps of 512 voxels (csrc/cc_paint.hip): a lane takes the quads [4l, 4l + 4) and
[256 + 4l, 256 + 4l + 4) of a sweep and stores a quad of a plane at once where the plane's row starts on the store's boundary; a
launch has at most 8192 workgroups.  The run painter's waves take 64 consecutive rows at a time and fill every stretch of rows
without a run with zeros in one go."""
import ctypes as C
import importlib.util
import os
import pickle

import numpy as np
import pytest

from delivr_cfos_amd import label_runs as lr

pytestmark = pytest.mark.gpu

MAX_WORKGROUPS = 8192  # PAINT_MAX_WG of csrc/cc_paint.hip
RUN_ROWS_PER_WAVE = 64  # RB: the run painter's waves take 64 consecutive rows at a time


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("paint_reference")


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def _dev(labels):
    import torch

    return torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint32).view(np.int32).copy()).cuda()


def _luts(n_lut, seed=0):
    """(n_lut, 3) uint8 and (n_lut,) uint16 tables without a zero from label 1 on (so a painted voxel shows), entry 0 = 0"""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(1, 256, size=(n_lut, 3), dtype=np.uint8)
    u16 = rng.integers(1, 65536, size=n_lut, dtype=np.uint16)
    rgb[0], u16[0] = 0, 0
    return rgb, u16


def _host_planes(result):
    """((r, g, b), image) of the engine -> (Z, Y, X, 3) uint8, (Z, Y, X) uint16 on the host"""
    chans, gray = result
    return np.stack([c.cpu().numpy() for c in chans], axis=-1), gray.cpu().numpy()


def _assert_both_painters(eng, labels, rgb, u16):
    want_rgb, want_u16 = ref.paint_by_label(labels, rgb), ref.paint_by_label(labels, u16)
    got_rgb, got_u16 = _host_planes(eng.paint_labels(_dev(labels), rgb=rgb, u16=u16))
    np.testing.assert_array_equal(got_rgb, want_rgb, err_msg="paint_labels rgb")
    np.testing.assert_array_equal(got_u16, want_u16, err_msg="paint_labels u16")
    got_rgb, got_u16 = _host_planes(eng.paint_runs(lr.encode_runs(labels), rgb=rgb, u16=u16))
    np.testing.assert_array_equal(got_rgb, want_rgb, err_msg="paint_runs rgb")
    np.testing.assert_array_equal(got_u16, want_u16, err_msg="paint_runs u16")
    return want_rgb, want_u16


# ---- 1. boundaries of the sweep -------------------------------------------------------------------------------------------------
def _boundary_volume(X):
    """Z = 2, Y = 3: [runs at x = 0 and x = X - 1 | empty | one run over the row] [empty | touching runs over the row | random runs]"""
    rng = np.random.default_rng(100 + X)
    v = np.zeros((6, X), dtype=np.uint32)
    v[0, 0] = 1
    v[0, X - 1] = 2
    v[2] = 3
    v[4] = 4 + (np.arange(X) // 3) % 5  # labels 4..8 in stretches of three, no gap
    x = int(rng.integers(0, 3))
    while x < X:
        n = int(rng.integers(1, 9))
        v[5, x:x + n] = rng.integers(9, 60)
        x += n + int(rng.integers(1, 7))
    return v.reshape(2, 3, X)


@pytest.mark.parametrize("X", [1, 3, 4, 5, 511, 512, 513, 1030])
def test_boundaries_of_the_sweep(eng, X):
    v = _boundary_volume(X)
    flat = v.reshape(6, X)
    # what the input is there for
    assert flat[0, 0] != 0 and flat[0, X - 1] != 0 and (X < 3 or not flat[0, 1:X - 1].any())  # runs at x = 0 and at x = X - 1
    assert not flat[1].any() and not flat[3].any()  # empty rows between full ones
    assert (flat[2] == 3).all()  # one run filling a row
    assert flat[4].all() and (X < 4 or (np.diff(flat[4].astype(np.int64)) != 0).sum() >= 1)  # touching runs of different labels
    runs = lr.encode_runs(v)
    per_row = np.diff(runs["row_start"].astype(np.int64))
    assert per_row[1] == per_row[3] == 0 and per_row[2] == 1 and per_row[4] == -(-X // 3)
    rgb, u16 = _luts(60, seed=X)
    want_rgb, want_u16 = _assert_both_painters(eng, v, rgb, u16)
    assert (want_u16 != 0).sum() == (v != 0).sum() and (want_rgb != 0).all(axis=-1).sum() == (v != 0).sum()


# ---- 2. the run painter's addressing ----------------------------------------------------------------------------------------------
def _call_runs(eng, row_start, n_rows, X, x0, x1, label, n_runs, n_lut, lut_rgb, lut_u16, outs):
    """dlv_paint_runs_dev on the caller's own device buffers (None: NULL) -> its return code"""
    p = lambda t: C.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None  # noqa: E731
    eng._enter()
    try:
        return eng.lib.dlv_paint_runs_dev(eng.ctx, p(row_start), n_rows, X, p(x0), p(x1), p(label), n_runs, n_lut, p(lut_rgb), p(lut_u16),
                                          *(p(o) for o in outs))
    finally:
        eng._leave()
        eng.sync()


def _call_labels(eng, labels, shape, n_lut, lut_rgb, lut_u16, outs):
    p = lambda t: C.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None  # noqa: E731
    eng._enter()
    try:
        return eng.lib.dlv_paint_labels_dev(eng.ctx, p(labels), *shape, n_lut, p(lut_rgb), p(lut_u16), *(p(o) for o in outs))
    finally:
        eng._leave()
        eng.sync()


def _filled_outs(shape):
    """r, g, b, image on the device, every byte 0xFF"""
    import torch

    outs = [torch.full(shape, 0xFF, dtype=torch.uint8, device="cuda") for _ in range(3)]
    gray = torch.empty(shape, dtype=torch.uint16, device="cuda")
    gray.view(torch.uint8).fill_(0xFF)
    return outs + [gray]


def _dev_luts(rgb, u16):
    import torch

    wide = rgb.astype(np.uint32)
    packed = (wide[:, 0] | (wide[:, 1] << 8) | (wide[:, 2] << 16)).view(np.int32)
    return torch.from_numpy(packed.copy()).cuda(), torch.from_numpy(u16.view(np.int16).copy()).cuda()


def test_a_volume_without_a_run_is_painted_with_zeros(eng):
    import torch

    Z, Y, X = 2, 3, 37  # (odd: the rows of every plane start off the 16-byte boundaries of the zero fill)
    rgb, u16 = _luts(8)
    lut_rgb, lut_u16 = _dev_luts(rgb, u16)
    row_start = torch.zeros(Z * Y + 1, dtype=torch.int64, device="cuda")
    outs = _filled_outs((Z, Y, X))
    assert all(int(o.view(torch.uint8).min()) == 0xFF for o in outs)
    rc = _call_runs(eng, row_start, Z * Y, X, None, None, None, 0, 8, lut_rgb, lut_u16, outs)  # R = 0, NULL run arrays
    assert rc == 0
    for o in outs:
        assert not o.cpu().numpy().any()
    # and through the engine, from the coding of an empty label volume
    empty = lr.encode_runs(np.zeros((Z, Y, X), dtype=np.uint32))
    assert len(empty["label"]) == 0
    got_rgb, got_u16 = _host_planes(eng.paint_runs(empty, rgb=rgb, u16=u16))
    assert got_rgb.shape == (Z, Y, X, 3) and not got_rgb.any() and not got_u16.any()


@pytest.fixture(scope="module")
def scattered():
    """(6, 4, 37) labels 0..49, about a third of the voxels labelled, one plane empty"""
    rng = np.random.default_rng(5)
    v = rng.integers(1, 50, size=(6, 4, 37), dtype=np.uint32)
    v[rng.random(v.shape) < 0.66] = 0
    v[3] = 0
    v[4, 1] = 0
    v.setflags(write=False)
    return v


def test_an_inner_range_of_planes_equals_the_same_planes_of_the_whole(eng, scattered):
    v = scattered
    rgb, u16 = _luts(50, seed=1)
    runs = lr.encode_runs(v)
    assert runs["row_start"][2 * 4] > 0 and runs["row_start"][5 * 4] < len(runs["label"])  # the origin moves; runs follow the range
    full_rgb, full_u16 = _host_planes(eng.paint_runs(runs, rgb=rgb, u16=u16))
    np.testing.assert_array_equal(full_rgb, ref.paint_by_label(v, rgb))
    np.testing.assert_array_equal(full_u16, ref.paint_by_label(v, u16))
    part_rgb, part_u16 = _host_planes(eng.paint_runs(runs, 2, 5, rgb=rgb, u16=u16))
    assert part_u16.shape == (3, 4, 37)
    np.testing.assert_array_equal(part_rgb, full_rgb[2:5])
    np.testing.assert_array_equal(part_u16, full_u16[2:5])
    last = eng.paint_runs(runs, 5, u16=u16)  # (z1 defaults to the end)
    np.testing.assert_array_equal(last.cpu().numpy(), full_u16[5:])
    for z0, z1 in ((-1, 2), (2, 2), (3, 7)):
        with pytest.raises(ValueError, match="planes"):
            eng.paint_runs(runs, z0, z1, u16=u16)


def test_stretches_of_empty_rows_across_the_blocks_of_rows(eng):
    rng = np.random.default_rng(9)
    Z, Y, X = 5, 40, 21  # 200 rows: three blocks of 64 and one of 8; odd X: no stretch starts on a boundary of the zero fill
    v = np.zeros((Z * Y, X), dtype=np.uint32)
    for r in (0, 1, 5, 63, 64, 130, 191, 199):  # rows with runs at both ends of blocks; [65, 130) and [131, 191) cross block ends
        v[r, rng.random(X) < 0.5] = rng.integers(1, 20)
        v[r, int(rng.integers(0, X))] = 7
    v = v.reshape(Z, Y, X)
    per_row = np.diff(lr.encode_runs(v)["row_start"].astype(np.int64))
    assert (np.flatnonzero(per_row) == (0, 1, 5, 63, 64, 130, 191, 199)).all()
    rgb, u16 = _luts(20, seed=9)
    want_rgb, want_u16 = _assert_both_painters(eng, v, rgb, u16)
    runs = lr.encode_runs(v)
    for z0, z1 in ((1, 4), (3, 5), (2, 3)):  # a range starts a new count of blocks at its first row; (2, 3) holds no run at all
        got_rgb, got_u16 = _host_planes(eng.paint_runs(runs, z0, z1, rgb=rgb, u16=u16))
        np.testing.assert_array_equal(got_rgb, want_rgb[z0:z1])
        np.testing.assert_array_equal(got_u16, want_u16[z0:z1])
    assert not want_u16[2].any() and want_u16[1].any()


@pytest.mark.parametrize("shape, first_strided_row", [((3, 3000, 5), MAX_WORKGROUPS), ((3, 174800, 1), MAX_WORKGROUPS * RUN_ROWS_PER_WAVE)])
def test_more_rows_than_workgroups_are_painted_completely(eng, shape, first_strided_row):
    """the dense painter walks rows grid-stride from row 8192 on, the run painter blocks of 64 rows from row 8192 * 64 on"""
    rng = np.random.default_rng(8)
    Z, Y, X = shape
    assert Z * Y > first_strided_row and Z * Y % RUN_ROWS_PER_WAVE != 0  # (and the last block of rows is a partial one)
    v = rng.integers(1, 30, size=(Z, Y, X), dtype=np.uint32)
    v[rng.random(v.shape) < 0.7] = 0
    per_row = np.diff(lr.encode_runs(v)["row_start"].astype(np.int64))
    assert (per_row[first_strided_row:] > 0).any() and (per_row[first_strided_row:] == 0).any()  # both paths beyond the grid
    rgb, u16 = _luts(30, seed=2)
    _assert_both_painters(eng, v, rgb, u16)


# ---- 3. the look-up tables --------------------------------------------------------------------------------------------------------
def test_labels_beyond_the_table_and_entries_of_zero_paint_zero(eng, scattered):
    v = scattered.copy()
    v[0, 0, :4] = (2**32 - 2, 33, 32, 2**31)
    rgb, u16 = _luts(33, seed=3)  # the labels 33..49 and the two large ones lie beyond the table
    rgb[[5, 6]], u16[[5, 7]] = 0, 0
    assert (v >= 33).sum() > 20 and (v == 5).any() and (v == 6).any() and (v == 7).any() and (v == 32).any()
    want_rgb, want_u16 = _assert_both_painters(eng, v, rgb, u16)
    assert not want_rgb[v >= 33].any() and not want_u16[v >= 33].any() and not want_rgb[v == 5].any() and not want_u16[v == 7].any()
    assert want_u16[v == 6].all() and want_rgb[v == 7].all() and want_u16[0, 0, 2] == u16[32]


def test_one_table_alone_paints_what_both_paint_together(eng, scattered):
    v = scattered
    rgb, u16 = _luts(50, seed=4)
    runs = lr.encode_runs(v)
    for paint in (lambda **kw: eng.paint_labels(_dev(v), **kw), lambda **kw: eng.paint_runs(runs, **kw)):
        both_rgb, both_u16 = _host_planes(paint(rgb=rgb, u16=u16))
        only_rgb = paint(rgb=rgb)
        assert isinstance(only_rgb, tuple) and len(only_rgb) == 3
        np.testing.assert_array_equal(np.stack([c.cpu().numpy() for c in only_rgb], axis=-1), both_rgb)
        np.testing.assert_array_equal(paint(u16=u16).cpu().numpy(), both_u16)
        np.testing.assert_array_equal(both_u16, ref.paint_by_label(v, u16))
        with pytest.raises(ValueError, match="neither"):
            paint()


def test_the_argument_errors_return_an_error_and_paint_nothing(eng, scattered):
    import torch

    from delivr_cfos_amd._lib import DLV_EINVAL

    v = scattered
    Z, Y, X = v.shape
    rgb, u16 = _luts(50, seed=6)
    lut_rgb, lut_u16 = _dev_luts(rgb, u16)
    labels = _dev(v)
    runs = lr.encode_runs(v)
    R = len(runs["label"])
    row_start = torch.from_numpy(runs["row_start"].view(np.int64).copy()).cuda()
    x0, x1 = (torch.from_numpy(runs[k].view(np.int16).copy()).cuda() for k in ("x0", "x1"))
    label = torch.from_numpy(runs["label"].view(np.int32).copy()).cuda()
    outs = _filled_outs((Z, Y, X))
    r, g, b, gray = outs
    cases = {
        "neither table": (None, None, [None] * 4),
        "neither table, planes given": (None, None, outs),
        "the RGB table without its planes": (lut_rgb, None, [None] * 4),
        "the RGB table with two of its planes": (lut_rgb, None, [r, g, None, None]),
        "byte planes without the RGB table": (None, lut_u16, outs),
        "the uint16 table without its plane": (lut_rgb, lut_u16, [r, g, b, None]),
        "the uint16 plane without its table": (lut_rgb, None, outs),
        "a uint16 plane off its alignment": (None, lut_u16, [None, None, None, gray.data_ptr() + 1]),
        "a uint16 table off its alignment": (None, lut_u16.data_ptr() + 1, [None, None, None, gray]),
        "an RGB table off its alignment": (lut_rgb.data_ptr() + 2, None, [r, g, b, None]),
    }
    for what, (t_rgb, t_u16, planes) in cases.items():
        assert _call_labels(eng, labels, (Z, Y, X), 50, t_rgb, t_u16, planes) == DLV_EINVAL, what
        assert _call_runs(eng, row_start, Z * Y, X, x0, x1, label, R, 50, t_rgb, t_u16, planes) == DLV_EINVAL, what
    assert _call_labels(eng, labels.data_ptr() + 2, (Z, Y, X), 50, lut_rgb, lut_u16, outs) == DLV_EINVAL
    assert _call_runs(eng, row_start.data_ptr() + 4, Z * Y, X, x0, x1, label, R, 50, lut_rgb, lut_u16, outs) == DLV_EINVAL
    assert _call_runs(eng, row_start, Z * Y, X, x0.data_ptr() + 1, x1, label, R, 50, lut_rgb, lut_u16, outs) == DLV_EINVAL
    assert _call_runs(eng, row_start, Z * Y, X, x0, x1, label.data_ptr() + 2, R, 50, lut_rgb, lut_u16, outs) == DLV_EINVAL
    for o in outs:  # nothing was painted
        assert int(o.view(torch.uint8).min()) == 0xFF
    # the same buffers with sound arguments are painted in full
    assert _call_runs(eng, row_start, Z * Y, X, x0, x1, label, R, 50, lut_rgb, lut_u16, outs) == 0
    np.testing.assert_array_equal(gray.cpu().numpy(), ref.paint_by_label(v, u16))
    np.testing.assert_array_equal(b.cpu().numpy(), ref.paint_by_label(v, rgb)[..., 2])


# ---- 4. agreement with the box painter --------------------------------------------------------------------------------------------
def _paint_both_ways(eng, mask, ids, rgb_of_id, region_of_id):
    """the cells `ids` (labels of the device's labelling of mask, in painting order) painted by boxes as blob_highlighter does
    (padded once for RGB, twice for the region ids) and by labels -> (labels, boxes rgb, boxes region, labels rgb, labels region)"""
    import torch

    from delivr_cfos_amd.hostlogic import padded_boxes, paint_luts

    bin_dev = torch.from_numpy(mask).cuda()
    labels_dev, n = eng.ccl26(bin_dev)
    stats = eng.cc_stats(labels_dev, n)
    r, g, b = (rgb_of_id[:, c].astype(np.uint8) for c in range(3))
    chans = eng.paint_boxes(bin_dev, padded_boxes(stats["bounding_boxes"], ids, mask.shape, 1), [r, g, b])
    (rid,) = eng.paint_boxes(bin_dev, padded_boxes(stats["bounding_boxes"], ids, mask.shape, 2), [region_of_id.astype(np.uint16)])
    lut_rgb, lut_region = paint_luts(ids, r, g, b, region_of_id, n)
    got = _host_planes(eng.paint_labels(labels_dev, rgb=lut_rgb, u16=lut_region))
    labels = labels_dev.cpu().numpy().view(np.uint32)
    want = ref.paint_by_label(labels, lut_rgb), ref.paint_by_label(labels, lut_region)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    return labels, np.stack([c.cpu().numpy() for c in chans], axis=-1), rid.cpu().numpy(), got[0], got[1], stats, n


def test_cells_far_apart_are_painted_alike_from_boxes_and_from_labels(eng):
    from delivr_cfos_amd.hostlogic import padded_boxes

    mask = np.zeros((40, 40, 40), dtype=np.uint8)
    rng = np.random.default_rng(12)
    for k in range(4):  # a 4^3 cube with a few voxels missing (its centre plane stays: one component), every 9 voxels along the diagonal
        cube = (rng.random((4, 4, 4)) < 0.8).astype(np.uint8)
        cube[1:3] = 1
        mask[1 + 9 * k:5 + 9 * k, 1 + 9 * k:5 + 9 * k, 1 + 9 * k:5 + 9 * k] = cube
    ids = np.array([3, 1, 4, 2])
    colours = np.array([[255, 1, 7], [2, 255, 8], [3, 4, 255], [90, 91, 92]])
    regions = np.array([65535, 1, 300, 17])
    labels, box_rgb, box_rid, lab_rgb, lab_rid, stats, n = _paint_both_ways(eng, mask, ids, colours, regions)
    assert n == 4
    boxes = padded_boxes(stats["bounding_boxes"], np.arange(1, 5), mask.shape, 2).astype(np.int64)
    for i in range(4):
        for j in range(i + 1, 4):
            for ax in range(3):  # padded twice, still 3 voxels apart on every axis
                gap = max(boxes[i, 2 * ax] - boxes[j, 2 * ax + 1], boxes[j, 2 * ax] - boxes[i, 2 * ax + 1])
                assert gap >= 3, (i, j, ax, gap)
    np.testing.assert_array_equal(lab_rgb, box_rgb)
    np.testing.assert_array_equal(lab_rid, box_rid)
    assert (lab_rid != 0).sum() == mask.sum()


def test_interlocking_cells_keep_their_own_colours_only_from_the_labels(eng):
    mask = np.zeros((3, 9, 9), dtype=np.uint8)
    mask[1, 1:7, 1] = mask[1, 1, 1:7] = 1  # cell A: an L along x = 1 and y = 1
    mask[1, 3:7, 6] = mask[1, 6, 3:7] = 1  # cell B: an L along x = 6 and y = 6, inside A's bounding box, two voxels from A
    ids = np.array([2, 1])  # A (the first voxel in raster order: label 1) is listed last: its box is painted over B
    colours = np.array([[10, 20, 30], [200, 210, 220]])
    regions = np.array([500, 600])
    labels, box_rgb, box_rid, lab_rgb, lab_rid, stats, n = _paint_both_ways(eng, mask, ids, colours, regions)
    assert n == 2 and labels[1, 1, 1] == 1 and labels[1, 6, 6] == 2
    bb = stats["bounding_boxes"].astype(np.int64)
    assert bb[1, 2] <= bb[2, 2] and bb[2, 3] <= bb[1, 3] and bb[1, 4] <= bb[2, 4] and bb[2, 5] <= bb[1, 5]  # B's box lies in A's
    assert (lab_rid[labels == 1] == 600).all() and (lab_rid[labels == 2] == 500).all()
    assert (lab_rgb[labels == 2] == (10, 20, 30)).all()
    wrong = box_rid != lab_rid
    assert wrong.sum() >= 1 and (labels[wrong] == 2).all() and (box_rid[wrong] == 600).all()  # the boxes colour B as A
    assert (box_rgb != lab_rgb).any()


# ---- 5. blob_highlighter ------------------------------------------------------------------------------------------------------------
CSV_HEAD = ",connected_component_id,acronym,red,green,blue,graph_order\n"


def _folder(tmp_path, brain, mask, cells, paint_from="labels"):
    """the folders of a visualisation run as the reference lays them out; cells: rows (id, acronym, r, g, b, graph_order)"""
    d_bin, d_csv, d_out, d_post = (str(tmp_path / k) for k in ("bin", "csv", "out", "post"))
    os.makedirs(os.path.join(d_bin, brain, "binary_segmentations"))
    for d in (d_csv, d_out, d_post):
        os.makedirs(d)
    np.save(os.path.join(d_bin, brain, "binary_segmentations", "binaries.npy"), mask)
    with open(os.path.join(d_csv, f"cells_{brain}.csv"), "w") as fh:
        fh.write(CSV_HEAD)
        for i, row in enumerate(cells):
            fh.write(f"{i}," + ",".join(str(v) for v in row) + "\n")
    settings = {"visualization": {"input_prediction_location": d_bin + "/", "input_csv_location": d_csv + "/",
                                  "output_location": d_out, "cache_location": str(tmp_path / "cache"),
                                  "no_atlas_depthmap": False, "region_id_rgb": True, "region_id_grayvalues": True},
                "postprocessing": {"output_location": d_post}, "FLAGS": {"LOAD_ALL_RAM": True}}
    if paint_from is not None:
        settings["mi355x"] = {"paint_from": paint_from}
    return settings, d_out, d_post


def _read_planes(d_out, brain, Z):
    from delivr_cfos_amd.downsample.downsample_and_mask import read_tiff_plane

    rgb = np.stack([np.stack([read_tiff_plane(os.path.join(d_out, brain + "_rgb_tiffs", f"{brain}rgb_C0{c}_z{z:04d}.tif")) for z in range(Z)])
                    for c in range(3)], axis=-1)
    rid = np.stack([read_tiff_plane(os.path.join(d_out, brain, brain + "_region_id_tiffs", f"region_id_{z:04d}.tif")) for z in range(Z)])
    assert sorted(os.listdir(os.path.join(d_out, brain + "_rgb_tiffs"))) == sorted(f"{brain}rgb_C0{c}_z{z:04d}.tif" for c in range(3)
                                                                                    for z in range(Z))
    assert sorted(os.listdir(os.path.join(d_out, brain, brain + "_region_id_tiffs"))) == [f"region_id_{z:04d}.tif" for z in range(Z)]
    return rgb, rid


@pytest.fixture(scope="module")
def brain_case(eng):
    """a (9, 20, 37) mask of small blobs, its labels from the engine, a cell table of most labels in a shuffled order (one 'bgr'
    row, which the highlighter drops) and the planes the helper expects"""
    import torch

    from delivr_cfos_amd.hostlogic import paint_luts

    rng = np.random.default_rng(31)
    mask = np.zeros((9, 20, 37), dtype=np.uint8)
    for _ in range(40):
        z, y, x = (int(rng.integers(0, s - 2)) for s in mask.shape)
        mask[z:z + int(rng.integers(1, 3)), y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 4))] = 1
    dev, n = eng.ccl26(torch.from_numpy(mask).cuda())
    labels = dev.cpu().numpy().view(np.uint32).copy()
    assert 10 < n < 65536
    ids = rng.permutation(np.arange(1, n + 1))
    dropped, bgr, ids = ids[:3], ids[3], ids[4:]  # three labels without a row, one in the background region
    cells = [(int(i), "reg", int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(1, 65536)))
             for i in ids]
    cells.insert(2, (int(bgr), "bgr", 9, 9, 9, 9))
    kept = [c for c in cells if c[1] != "bgr"]
    rgb, region = paint_luts(*(np.array([c[k] for c in kept]) for k in (0, 2, 3, 4, 5)), n)
    want = ref.paint_by_label(labels, rgb), ref.paint_by_label(labels, region)
    assert not want[1][np.isin(labels, dropped)].any() and not want[1][labels == bgr].any() and (want[1] != 0).any()
    for a in (mask, labels):
        a.setflags(write=False)
    return mask, labels, n, cells, want


def _run_highlighter(eng, monkeypatch, settings, brain, shape, min_slabs=3):
    """blob_highlighter with slabs of two planes of a dense uint16 file's 11 bytes per voxel -> the paint calls it made"""
    from delivr_cfos_amd import blob_highlighter as bh

    Z, Y, X = shape
    monkeypatch.setattr(bh, "_SLAB_BYTES", 2 * Y * X * 11)
    calls = []
    for name in ("paint_labels", "paint_runs", "paint_boxes"):
        def counted(*a, _f=getattr(eng, name), _n=name, **kw):
            calls.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(eng, name, counted)
    bh.blob_highlighter(settings, [brain, ""], (1, 1, Z, Y, X), engine=eng)
    assert len(calls) >= min_slabs, calls
    return calls


def test_highlighter_paints_from_a_dense_uint16_label_file(eng, monkeypatch, tmp_path, brain_case):
    mask, labels, n, cells, want = brain_case
    settings, d_out, d_post = _folder(tmp_path, "brainA", np.ones_like(mask), cells)  # (binaries.npy full of 1s: it is not read)
    np.save(os.path.join(d_post, f"brainA-{n}-cc3d.npy"), labels.astype(np.uint16))
    calls = _run_highlighter(eng, monkeypatch, settings, "brainA", mask.shape)
    assert set(calls) == {"paint_labels"} and len(calls) == 5  # 9 planes, two per slab; both outputs from one call per slab
    rgb, rid = _read_planes(d_out, "brainA", mask.shape[0])
    np.testing.assert_array_equal(rgb, want[0])
    np.testing.assert_array_equal(rid, want[1])
    # a uint32 file is uploaded as it is: the same planes; a uint64 file is refused
    import shutil

    shutil.rmtree(d_out)
    os.makedirs(d_out)
    np.save(os.path.join(d_post, f"brainA-{n}-cc3d.npy"), labels.astype(np.uint32))
    calls = _run_highlighter(eng, monkeypatch, settings, "brainA", mask.shape)
    assert set(calls) == {"paint_labels"} and len(calls) == 5  # (4 + 5 bytes per voxel: still two planes per slab)
    rgb, rid = _read_planes(d_out, "brainA", mask.shape[0])
    np.testing.assert_array_equal(rgb, want[0])
    np.testing.assert_array_equal(rid, want[1])
    np.save(os.path.join(d_post, f"brainA-{n}-cc3d.npy"), labels.astype(np.uint64))
    with pytest.raises(ValueError, match="uint64"):
        _run_highlighter(eng, monkeypatch, settings, "brainA", mask.shape, min_slabs=0)


def test_highlighter_paints_from_a_run_file_without_reading_the_mask(eng, monkeypatch, tmp_path, brain_case):
    mask, labels, n, cells, want = brain_case
    settings, d_out, d_post = _folder(tmp_path, "brainA", np.ones_like(mask), cells)  # (binaries.npy full of 1s: it is not read)
    lr.save_runs(os.path.join(d_post, lr.runs_name("brainA", n)), lr.encode_runs(labels), n)
    calls = _run_highlighter(eng, monkeypatch, settings, "brainA", mask.shape)
    assert set(calls) == {"paint_runs"} and len(calls) == 3  # no label bytes in HBM: four planes per slab, z0 = 0, 4, 8
    rgb, rid = _read_planes(d_out, "brainA", mask.shape[0])
    np.testing.assert_array_equal(rgb, want[0])
    np.testing.assert_array_equal(rid, want[1])


def test_highlighter_labels_the_mask_again_without_a_label_file(eng, monkeypatch, tmp_path, brain_case):
    mask, labels, n, cells, want = brain_case
    settings, d_out, d_post = _folder(tmp_path, "brainA", mask, cells)
    calls = _run_highlighter(eng, monkeypatch, settings, "brainA", mask.shape)
    assert set(calls) == {"paint_labels"} and len(calls) == 5
    rgb, rid = _read_planes(d_out, "brainA", mask.shape[0])
    np.testing.assert_array_equal(rgb, want[0])
    np.testing.assert_array_equal(rid, want[1])
    # a pickle of that labelling changes nothing; one of another number of components is refused
    with open(os.path.join(d_post, "brainA-stats.pickle"), "wb") as fh:
        pickle.dump({"bounding_boxes": np.zeros((n + 1, 6), dtype=np.uint16)}, fh)
    _run_highlighter(eng, monkeypatch, settings, "brainA", mask.shape)
    np.testing.assert_array_equal(_read_planes(d_out, "brainA", mask.shape[0])[1], want[1])
    with open(os.path.join(d_post, "brainA-stats.pickle"), "wb") as fh:
        pickle.dump({"bounding_boxes": np.zeros((n + 3, 6), dtype=np.uint16)}, fh)
    with pytest.raises(ValueError, match="split or filtered"):
        _run_highlighter(eng, monkeypatch, settings, "brainA", mask.shape, min_slabs=0)


def test_highlighter_gives_the_siblings_of_a_split_their_own_colours(eng, monkeypatch, tmp_path):
    import torch

    mask = np.zeros((20, 20, 24), dtype=np.uint8)
    mask[2:10, 2:10, 2:10] = 1
    mask[8:16, 8:16, 10:18] = 1  # two cubes that touch in a 2 x 2 patch of the face x = 9 | 10: one component
    dev, n = eng.ccl26(torch.from_numpy(mask).cuda())
    assert n == 1
    K, _, n_split = eng.cc_split(dev, n, 2)
    assert (K, n_split) == (2, 1)
    labels = dev.cpu().numpy().view(np.uint32).copy()
    assert ((labels != 0) == (mask != 0)).all() and (labels == 1).sum() > 100 and (labels == 2).sum() > 100
    cells = [(1, "a", 255, 0, 10, 111), (2, "b", 0, 255, 20, 222)]
    settings, d_out, d_post = _folder(tmp_path, "brainS", mask, cells)
    lr.save_runs(os.path.join(d_post, lr.runs_name("brainS", K)), lr.encode_runs(labels), K)
    calls = _run_highlighter(eng, monkeypatch, settings, "brainS", mask.shape)
    assert set(calls) == {"paint_runs"}
    rgb, rid = _read_planes(d_out, "brainS", mask.shape[0])
    np.testing.assert_array_equal(rid, ref.paint_by_label(labels, np.array([0, 111, 222], dtype=np.uint16)))
    np.testing.assert_array_equal(rgb, ref.paint_by_label(labels, np.array([[0, 0, 0], [255, 0, 10], [0, 255, 20]], dtype=np.uint8)))
    assert (rid == 111).sum() == (labels == 1).sum() and (rid == 222).sum() == (labels == 2).sum()


def test_without_the_key_the_golden_planes_are_still_the_reference_s(eng, monkeypatch, tmp_path, golden_dir):
    from delivr_cfos_amd.downsample.downsample_and_mask import read_tiff_plane

    g = np.load(os.path.join(golden_dir, "ref_paint.npz"))
    m = g["mask"]
    cells = [(g["cc_id"][i], g["acronym"][i], g["red"][i], g["green"][i], g["blue"][i], g["graph_order"][i]) for i in range(len(g["cc_id"]))]
    for key in (None, "boxes"):
        settings, d_out, d_post = _folder(tmp_path / str(key), "brainA", m, cells, paint_from=key)
        with open(os.path.join(d_post, "brainA-stats.pickle"), "wb") as fh:
            pickle.dump({"bounding_boxes": g["bounding_boxes"].copy()}, fh)
        calls = _run_highlighter(eng, monkeypatch, settings, "brainA", m.shape, min_slabs=0)
        assert calls == ["paint_boxes", "paint_boxes"]
        p = read_tiff_plane(os.path.join(d_out, "brainA", "brainA_region_id_tiffs", "region_id_0005.tif"))
        np.testing.assert_array_equal(p, g["region_id"][5])
        p = read_tiff_plane(os.path.join(d_out, "brainA_rgb_tiffs", "brainArgb_C01_z0005.tif"))
        np.testing.assert_array_equal(p, g["rgb"][1, 5])
