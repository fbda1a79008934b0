"""The paths of cc_stats_kernel (dlv_cc_stats_dev / dlv_cc_stats_raw_dev; HipEngine.cc_stats / cc_stats_raw): the 16-byte loads of
an aligned volume with X % 8 == 0 across the gap between a thread's quads, a sweep boundary and a partial last sweep, the
element-wise loads of an unaligned volume and of an odd X, many labels per wave, one label in every lane, no background and
nothing but background.

The reference of every case is numpy on the labels dlv_ccl26_dev returned: counts by np.bincount, bounding boxes by minimum /
maximum.reduceat over a stable argsort by label, coordinate sums in uint64 by add.reduceat.  Every integer is compared for
equality, row 0 (the background) included; a centroid of a row >= 1 is float64 equality with sum.astype(float64) / count, the
background's - which the library derives from the totals - is held to rtol 1e-12."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = 0xFFFFFFFF


def _reference(labels: np.ndarray, n: int) -> dict:
    """rows 0..n from numpy alone - row 0 is the background's true count, box and sums; an absent row reads 0, ABSENT / 0, 0"""
    lab = labels.ravel()
    order = np.argsort(lab, kind="stable")
    ls = lab[order]
    starts = np.flatnonzero(np.r_[True, ls[1:] != ls[:-1]])
    present = ls[starts].astype(np.int64)
    assert present.max() <= n
    coords = np.stack(np.unravel_index(order, labels.shape), axis=1).astype(np.uint64)  # (voxels, 3) in label order
    ref = {"counts": np.bincount(lab, minlength=n + 1).astype(np.uint32), "bbmin": np.full((n + 1, 3), ABSENT, dtype=np.uint32),
           "bbmax": np.zeros((n + 1, 3), dtype=np.uint32), "sums": np.zeros((n + 1, 3), dtype=np.uint64)}
    ref["bbmin"][present] = np.minimum.reduceat(coords, starts, axis=0).astype(np.uint32)
    ref["bbmax"][present] = np.maximum.reduceat(coords, starts, axis=0).astype(np.uint32)
    ref["sums"][present] = np.add.reduceat(coords, starts, axis=0)
    assert int(ref["counts"].sum()) == lab.size
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _check(eng, lab_dev, n: int, ref: dict):
    """HipEngine.cc_stats_raw and cc_stats on the device labels against the reference"""
    counts, sums = ref["counts"], ref["sums"]
    bg = int(counts[0])
    # the accumulators: the kernel counts and sums labels 1..n only, the background's row holds its bounding box alone
    raw = eng.cc_stats_raw(lab_dev, n)
    assert list(raw) == ["counts", "bbmin", "bbmax", "sums"]
    want = {"counts": counts.copy(), "bbmin": ref["bbmin"], "bbmax": ref["bbmax"], "sums": sums.copy()}
    want["counts"][0] = 0
    want["sums"][0] = 0
    for k, v in want.items():
        assert raw[k].dtype == v.dtype and raw[k].shape == v.shape, k
        np.testing.assert_array_equal(raw[k], v, err_msg=k)
    # the cc3d.statistics layout
    st = eng.cc_stats(lab_dev, n)
    assert st["voxel_counts"].dtype == np.uint32 and st["bounding_boxes"].dtype == np.uint16 and st["centroids"].dtype == np.float64
    np.testing.assert_array_equal(st["voxel_counts"], counts)
    boxes = np.stack([ref["bbmin"], ref["bbmax"]], axis=2).reshape(n + 1, 6)  # zmin, zmax, ymin, ymax, xmin, xmax
    if bg == 0:
        boxes[0] = 0
    assert boxes.max() <= 0xFFFF
    np.testing.assert_array_equal(st["bounding_boxes"], boxes.astype(np.uint16))
    assert (counts[1:] > 0).all()  # (dlv_ccl26_dev numbers the components 1..n without a gap)
    np.testing.assert_array_equal(st["centroids"][1:], sums[1:].astype(np.float64) / counts[1:, None])
    if bg:
        np.testing.assert_allclose(st["centroids"][0], sums[0].astype(np.float64) / bg, rtol=1e-12, atol=0)
    else:
        assert np.isnan(st["centroids"][0]).all()


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def _label(eng, mask):
    import torch

    lab, n = eng.ccl26(torch.from_numpy(mask).cuda())
    labels = lab.cpu().numpy().view(np.uint32)
    labels.setflags(write=False)
    return labels, n


def _labels_dev(labels):
    import torch

    dev = torch.from_numpy(labels.view(np.int32).copy()).cuda()
    assert dev.data_ptr() % 16 == 0
    return dev


# ---- 1, 2. X % 8 == 0 with a partial third sweep: aligned (16-byte loads) and unaligned (element by element) -----------
@pytest.fixture(scope="module")
def wide(eng):
    """3 x 5 x 4104 = 2 sweeps of 2048 voxels + 8: single cells across the gap between a thread's two quads (x = 1023 | 1024), the
    sweep boundary (2047 | 2048) and into the last sweep (4095 | 4096), one cell that is the last 8 voxels of a row, one box over
    two planes and two rows"""
    mask = np.zeros((3, 5, 4104), dtype=np.uint8)
    mask[0, 0, 1020:1028] = 1
    mask[0, 2, 2040:2056] = 1
    mask[0, 4, 4090:4100] = 1
    mask[2, 0, 4096:4104] = 1
    mask[1:3, 2:4, 1000:1030] = 1
    labels, n = _label(eng, mask)
    assert n == 5 and np.array_equal(labels != 0, mask != 0)
    for z, y, x in ((0, 0, 1023), (0, 2, 2047), (0, 4, 4095), (2, 2, 1023)):
        assert labels[z, y, x] == labels[z, y, x + 1] != 0  # one cell on both sides
    assert (labels[2, 0, 4096:] == labels[2, 0, 4096]).all() and labels[2, 0, 4096] != 0 and labels[2, 0, 4095] == 0
    assert len({int(labels[p]) for p in ((0, 0, 1023), (0, 2, 2047), (0, 4, 4095), (2, 0, 4096), (2, 2, 1023))}) == 5
    return labels, n, _reference(labels, n)


def test_aligned_wide_rows_cells_across_quad_gap_sweep_boundary_and_partial_sweep(eng, wide):
    labels, n, ref = wide
    assert labels.shape[2] % 8 == 0
    lab_dev = _labels_dev(labels)
    _check(eng, lab_dev, n, ref)
    np.testing.assert_array_equal(lab_dev.cpu().numpy().view(np.uint32), labels)  # read, never written


def test_the_same_volume_4_bytes_past_a_16_byte_boundary(eng, wide):
    import torch

    labels, n, ref = wide
    host = np.full(labels.size + 1, 0x7FFFFFF0, dtype=np.int32)  # (the guard in front: a label far above n)
    host[1:] = labels.view(np.int32).ravel()
    buf = torch.from_numpy(host).cuda()
    view = buf[1:].view(labels.shape)
    assert view.data_ptr() % 16 == 4
    _check(eng, view, n, ref)
    np.testing.assert_array_equal(buf.cpu().numpy(), host)


# ---- 3. odd X: a ragged last segment -----------------------------------------------------------------------------------
def test_odd_x_random_mask(eng):
    mask = (np.random.default_rng(17).random((7, 9, 131)) < 0.30).astype(np.uint8)
    labels, n = _label(eng, mask)
    assert n > 1 and np.array_equal(labels != 0, mask != 0) and labels.shape[2] % 8 == 3
    assert mask[:, :, 128:].any()  # the last, 3-voxel segment of some row holds foreground
    _check(eng, _labels_dev(labels), n, _reference(labels, n))


# ---- 4. many labels per wave, two per thread: the leader loop runs many rounds ---------------------------------------------
def test_more_than_64_labels_in_a_wave_two_per_thread(eng):
    mask = np.zeros((2, 3, 1024), dtype=np.uint8)
    mask[0, 1, ::2] = 1  # single voxels at pitch 2: no two touch
    labels, n = _label(eng, mask)
    assert n == 512
    assert np.unique(labels[0, 1, :512]).size - 1 > 64  # more distinct labels in 512 voxels than a wave has lanes
    quads = labels[0, 1].reshape(-1, 4)
    assert all(np.unique(q[q != 0]).size == 2 for q in quads)  # two labels in every quad of four voxels
    _check(eng, _labels_dev(labels), n, _reference(labels, n))


# ---- 5. one label in all 64 lanes of every wave of a plane -----------------------------------------------------------------
def test_a_full_plane_behind_one_label_beside_specks(eng):
    rng = np.random.default_rng(23)
    mask = np.zeros((4, 16, 512), dtype=np.uint8)
    mask[1] = 1
    mask[3, ::2, ::2] = rng.integers(0, 2, size=(8, 256), dtype=np.uint8)  # single voxels, two planes away from the set one
    labels, n = _label(eng, mask)
    plane = int(labels[1, 0, 0])
    assert n == 1 + int(mask[3].sum()) > 100 and plane == 1 and (labels[1] == plane).all() and (labels[3] != plane).all()
    ref = _reference(labels, n)
    assert int(ref["counts"][plane]) == 16 * 512
    assert ref["bbmin"][plane].tolist() == [1, 0, 0] and ref["bbmax"][plane].tolist() == [1, 15, 511]
    assert ref["sums"][plane].tolist() == [16 * 512, 512 * (15 * 16 // 2), 16 * (511 * 512 // 2)]
    lab_dev = _labels_dev(labels)
    _check(eng, lab_dev, n, ref)
    raw = eng.cc_stats_raw(lab_dev, n)  # ... and the plane's row once more against the closed forms
    assert int(raw["counts"][plane]) == 8192 and raw["sums"][plane].tolist() == [8192, 61440, 2093056]
    assert raw["bbmin"][plane].tolist() == [1, 0, 0] and raw["bbmax"][plane].tolist() == [1, 15, 511]


# ---- 6. the background row without and with nothing but background ---------------------------------------------------------
def test_all_background_and_all_foreground(eng):
    empty, n0 = _label(eng, np.zeros((2, 3, 16), dtype=np.uint8))
    assert n0 == 0 and not empty.any()
    ref0 = _reference(empty, 0)
    assert ref0["counts"].tolist() == [96] and ref0["bbmin"].tolist() == [[0, 0, 0]] and ref0["bbmax"].tolist() == [[1, 2, 15]]
    _check(eng, _labels_dev(empty), 0, ref0)
    full, n1 = _label(eng, np.ones((2, 3, 16), dtype=np.uint8))
    assert n1 == 1 and (full == 1).all()
    ref1 = _reference(full, 1)
    assert ref1["counts"].tolist() == [0, 96] and ref1["bbmin"][0].tolist() == [ABSENT] * 3 and ref1["bbmax"][0].tolist() == [0, 0, 0]
    _check(eng, _labels_dev(full), 1, ref1)
    got = eng.cc_stats(_labels_dev(full), 1)
    assert got["voxel_counts"].tolist() == [0, 96] and got["bounding_boxes"].tolist() == [[0] * 6, [0, 1, 0, 2, 0, 15]]
    np.testing.assert_array_equal(got["centroids"][1], [0.5, 1.0, 7.5])
