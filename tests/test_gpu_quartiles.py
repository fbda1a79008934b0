"""Per-cell intensity quartiles on the device (dlv_cc_quantiles_dev / HipEngine.cc_quantiles;
settings["mi355x"]["intensity_quartiles"] in count_blobs).

The reference of every case is tests/helpers/quantile_reference.py, numpy only: the voxels with a label 1..n sorted by (label,
value), per label with m voxels and level p the value at index (p * (m - 1)) // 100 of its segment.  Everything compared is an
integer - equality, no tolerance; contrast_median is float64 equality with the division done in numpy."""
import ctypes as C
import importlib.util
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIVE = (0, 25, 50, 75, 100)
QUARTILE_KEYS = ("intensity_q25", "intensity_median", "intensity_q75")
SHELL_QUARTILE_KEYS = ("shell_q25", "shell_median", "shell_q75", "contrast_median")
INTENSITY_KEYS = {"intensity_sum", "intensity_sumsq", "intensity_min", "intensity_max", "intensity_mean"}
SHELL_KEYS = {"shell_voxels", "shell_sum", "shell_sumsq", "shell_min", "shell_max", "shell_mean", "contrast", "shell_radius"}
STD_KEYS = {"voxel_counts", "bounding_boxes", "centroids"}


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


reference = _helper("quantile_reference").quantile_reference


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def _label(eng, mask):
    import torch

    lab, n = eng.ccl26(torch.from_numpy(mask).cuda())
    return lab.cpu().numpy().view(np.uint32), n


def _labels_dev(labels):
    import torch

    return torch.from_numpy(labels.view(np.int32).copy()).cuda()


def _raw_dev(raw):
    import torch

    return torch.from_numpy(np.array(raw, order="C")).cuda()  # (a writable copy: the fixtures are read-only)


def _assert_pair(got, ref):
    (values, counts), (ref_values, ref_counts) = got, ref
    assert values.dtype == np.uint16 and values.shape == ref_values.shape
    assert counts.dtype == np.uint32 and counts.shape == ref_counts.shape
    np.testing.assert_array_equal(counts, ref_counts)
    np.testing.assert_array_equal(values, ref_values)


# ---- 1. segment sizes around every internal boundary -----------------------------------------------------------------
ROD_SIZES = list(range(1, 131)) + [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049]


@pytest.fixture(scope="module")
def rods(eng):
    """one plane of 284 x 2051 voxels (an odd X: the alignment of the rows changes from row to row); row 2j holds one rod of
    ROD_SIZES[j] voxels - label j + 1 - at a random offset: the lengths around a wave (64), the one-wave selection's registers
    (512: beyond it the workgroup kernel selects) and a sweep of 2048 voxels.  The first 40 rows of raw are heavy in ties."""
    rng = np.random.default_rng(21)
    shape = (1, 284, 2051)
    mask = np.zeros(shape, dtype=np.uint8)
    for j, size in enumerate(ROD_SIZES):
        x0 = int(rng.integers(0, shape[2] - size + 1))
        mask[0, 2 * j, x0:x0 + size] = 1
    raw = rng.integers(0, 65536, size=shape, dtype=np.uint16)
    raw[0, :40] = rng.integers(0, 4, size=(40, shape[2]), dtype=np.uint16)
    labels, n = _label(eng, mask)
    assert n == len(ROD_SIZES) == 142
    assert np.bincount(labels.ravel())[1:].tolist() == ROD_SIZES
    ref = reference(labels, raw, n, FIVE)
    for a in (labels, raw, *ref):
        a.setflags(write=False)
    return labels, n, raw, ref


def test_segment_sizes_around_every_internal_boundary(eng, rods):
    labels, n, raw, ref = rods
    lab_dev, raw_dev = _labels_dev(labels), _raw_dev(raw)
    values, counts = eng.cc_quantiles(lab_dev, raw_dev, n, FIVE)
    _assert_pair((values, counts), ref)
    moments = eng.cc_intensity(lab_dev, raw_dev, n)
    np.testing.assert_array_equal(values[1:, 0], moments["intensity_min"][1:])
    np.testing.assert_array_equal(values[1:, 4], moments["intensity_max"][1:])
    assert (np.diff(values.astype(np.int64), axis=1) >= 0).all()  # the levels of a row do not decrease
    np.testing.assert_array_equal(counts[1:], eng.cc_counts(lab_dev, n).cpu().numpy().view(np.uint32)[1:])
    assert counts[0] == 0 and not values[0].any()
    _assert_pair(eng.cc_quantiles(lab_dev, raw_dev, n), (ref[0][:, 1:4], ref[1]))  # the default levels: the quartiles
    np.testing.assert_array_equal(lab_dev.cpu().numpy().view(np.uint32), labels)
    np.testing.assert_array_equal(raw_dev.cpu().numpy(), raw)


def test_the_same_call_twice_gives_equal_tables(eng, rods):
    labels, n, raw, ref = rods
    lab_dev, raw_dev = _labels_dev(labels), _raw_dev(raw)
    first = eng.cc_quantiles(lab_dev, raw_dev, n, FIVE)
    second = eng.cc_quantiles(lab_dev, raw_dev, n, FIVE)
    _assert_pair(second, first)
    _assert_pair(second, ref)


# ---- 2. odd geometry, padded raw, both alignments ------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd(eng):
    """33 x 67 x 131 labels of the intensity tests' pitch-4 box mask (5049 labels) under a 48 x 80 x 144 raw volume; expected
    from raw[:33, :67, :131]"""
    rng = np.random.default_rng(5)
    shape = (33, 67, 131)
    mask = np.zeros(shape, dtype=np.uint8)
    for z in range(0, shape[0], 4):
        for y in range(0, shape[1], 4):
            ext = rng.integers(1, 4, size=(len(range(0, shape[2], 4)), 3))
            for (dz, dy, dx), x in zip(ext, range(0, shape[2], 4)):
                mask[z:z + dz, y:y + dy, x:x + dx] = 1
    labels, n = _label(eng, mask)
    assert n == 9 * 17 * 33 == 5049
    raw = rng.integers(0, 65536, size=(48, 80, 144), dtype=np.uint16)
    inside = np.argwhere(mask)
    for value, picks in ((0, inside[::7]), (65535, inside[3::11])):
        raw[picks[:, 0], picks[:, 1], picks[:, 2]] = value
    ref = reference(labels, raw[:33, :67, :131], n, FIVE)
    for a in (labels, raw, *ref):
        a.setflags(write=False)
    return labels, n, raw, ref


def test_odd_geometry_padded_raw_fresh_tensors(eng, odd):
    import torch

    labels, n, raw, ref = odd
    lab_dev, raw_dev = _labels_dev(labels), _raw_dev(raw)
    assert lab_dev.data_ptr() % 16 == 0 and raw_dev.data_ptr() % 16 == 0
    _assert_pair(eng.cc_quantiles(lab_dev, raw_dev, n, FIVE), ref)
    _assert_pair(eng.cc_quantiles(lab_dev, raw_dev.view(torch.int16), n, FIVE), ref)  # an int16-viewed volume is the same bytes
    np.testing.assert_array_equal(lab_dev.cpu().numpy().view(np.uint32), labels)
    np.testing.assert_array_equal(raw_dev.cpu().numpy(), raw)


def test_odd_geometry_labels_4_bytes_and_raw_2_bytes_past_a_16_byte_boundary(eng, odd):
    import torch

    labels, n, raw, ref = odd
    lab_host = np.full(labels.size + 2, 0x7FFFFFF0, dtype=np.int32)  # guards: a label far above n
    lab_host[1:-1] = labels.view(np.int32).ravel()
    raw_host = np.full(raw.size + 2, 0xABCD, dtype=np.uint16)
    raw_host[1:-1] = raw.ravel()
    lab_buf, raw_buf = torch.from_numpy(lab_host).cuda(), torch.from_numpy(raw_host).cuda()
    lab_view, raw_view = lab_buf[1:-1].view(labels.shape), raw_buf[1:-1].view(raw.shape)
    assert lab_view.data_ptr() % 16 == 4 and raw_view.data_ptr() % 16 == 2
    _assert_pair(eng.cc_quantiles(lab_view, raw_view, n, FIVE), ref)
    np.testing.assert_array_equal(lab_buf.cpu().numpy(), lab_host)  # guards and payload untouched
    np.testing.assert_array_equal(raw_buf.cpu().numpy(), raw_host)


def test_odd_geometry_tight_raw_and_a_strided_view_of_the_padded_one(eng, odd):
    labels, n, raw, ref = odd
    tight = _raw_dev(raw[:33, :67, :131])
    assert tuple(tight.stride()) == (67 * 131, 131, 1)
    _assert_pair(eng.cc_quantiles(_labels_dev(labels), tight, n, FIVE), ref)
    view = _raw_dev(raw)[:33, :67, :131]
    assert tuple(view.stride()) == (80 * 144, 144, 1)
    _assert_pair(eng.cc_quantiles(_labels_dev(labels), view, n, FIVE), ref)


# ---- 3. one giant component beside specks -----------------------------------------------------------------------------
def test_one_giant_component_beside_specks(eng):
    rng = np.random.default_rng(7)
    mask = np.zeros((64, 64, 96), dtype=np.uint8)
    mask[8:56, 8:56, 16:80] = 1  # 147 456 voxels behind one label: every lane of every wave asks for places of the same segment
    mask[::2, ::2, 84::2] = rng.integers(0, 2, size=(32, 32, 6), dtype=np.uint8)  # isolated voxels, some ahead of the block in raster order
    labels, n = _label(eng, mask)
    block = int(labels[8, 8, 16])
    assert 1 < block < n
    raw = rng.integers(0, 65536, size=mask.shape, dtype=np.uint16)
    lab_dev = _labels_dev(labels)
    ref = reference(labels, raw, n, FIVE)
    assert int(ref[1][block]) == 147456 and len(set(ref[0][block].tolist())) == 5
    _assert_pair(eng.cc_quantiles(lab_dev, _raw_dev(raw), n, FIVE), ref)
    for constant in (65535, 0):  # a true 65535 everywhere, then a true 0 (told from an absent label by its count)
        raw[8:56, 8:56, 16:80] = constant
        values, counts = eng.cc_quantiles(lab_dev, _raw_dev(raw), n, FIVE)
        _assert_pair((values, counts), reference(labels, raw, n, FIVE))
        assert values[block].tolist() == [constant] * 5 and counts[block] == 147456
    specks = np.arange(1, n + 1) != block
    assert (counts[1:][specks] == 1).all() and (values[1:][specks] == values[1:, :1][specks]).all()  # single voxels: every level is the voxel


# ---- 4. more than 2^16 labels ---------------------------------------------------------------------------------------
def test_more_than_2_to_16_labels_every_row_exact(eng):
    rng = np.random.default_rng(6)
    shape = (64, 96, 144)
    mask = np.zeros(shape, dtype=np.uint8)
    mask[::2, ::2, ::3] = 1
    mask[::2, ::2, 1::3] = rng.integers(0, 2, size=(32, 48, 48), dtype=np.uint8)  # singles or x-pairs
    labels, n = _label(eng, mask)
    assert n == 32 * 48 * 48 and n > 65536
    raw = rng.integers(0, 65536, size=shape, dtype=np.uint16)
    _assert_pair(eng.cc_quantiles(_labels_dev(labels), _raw_dev(raw), n), reference(labels, raw, n))


# ---- 5. degenerate cases ----------------------------------------------------------------------------------------------
def test_empty_mask_small_n_level_counts_and_refused_arguments(eng, odd):
    import torch
    from delivr_cfos_amd import _lib

    empty = np.zeros((9, 10, 11), dtype=np.uint8)
    labels0, n0 = _label(eng, empty)
    assert n0 == 0
    raw0 = np.random.default_rng(1).integers(0, 65536, size=(9, 10, 11), dtype=np.uint16)
    values, counts = eng.cc_quantiles(_labels_dev(labels0), _raw_dev(raw0), 0)
    assert values.tolist() == [[0, 0, 0]] and counts.tolist() == [0] and values.dtype == np.uint16 and counts.dtype == np.uint32
    labels, n, raw, ref = odd
    lab_dev, raw_dev = _labels_dev(labels), _raw_dev(raw)
    few = 100  # labels above n are not measured: the rows 0..100 are those of the whole table
    _assert_pair(eng.cc_quantiles(lab_dev, raw_dev, few, FIVE), (ref[0][:few + 1], ref[1][:few + 1]))
    _assert_pair(eng.cc_quantiles(lab_dev, raw_dev, few, FIVE), reference(labels, raw[:33, :67, :131], few, FIVE))
    _assert_pair(eng.cc_quantiles(lab_dev, raw_dev, n, (50,)), (ref[0][:, 2:3], ref[1]))
    eight = (0, 10, 25, 50, 75, 90, 99, 100)
    _assert_pair(eng.cc_quantiles(lab_dev, raw_dev, n, eight), reference(labels, raw[:33, :67, :131], n, eight))
    # the C entry point: bad level lists, then every EINVAL case of the geometry - nothing is written
    out = np.full((n + 1, 9), 0x5A5A, dtype=np.uint16)
    cnt = np.full(n + 1, 0xA5A5A5A5, dtype=np.uint32)
    op, cp = out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)
    lp, rp = C.c_void_p(lab_dev.data_ptr()), C.c_void_p(raw_dev.data_ptr())
    call = eng.lib.dlv_cc_quantiles_dev

    def levels(*p):
        return (C.c_int * max(len(p), 1))(*p)

    good = levels(25, 50, 75)
    for lv in ((), tuple(range(0, 90, 10)), (25, 25, 75), (50, 25), (25, 101), (-1, 50)):
        assert call(eng.ctx, lp, rp, 33, 67, 131, 144, 80 * 144, n, len(lv), levels(*lv), op, cp) == _lib.DLV_EINVAL, lv
    assert call(eng.ctx, lp, rp, 33, 67, 131, 144, 80 * 144, n, 3, None, op, cp) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, rp, 33, 67, 131, 130, 80 * 144, n, 3, good, op, cp) == _lib.DLV_EINVAL  # raw_pitch_y < X
    assert call(eng.ctx, lp, rp, 33, 67, 131, 144, 67 * 144 - 1, n, 3, good, op, cp) == _lib.DLV_EINVAL  # raw_pitch_z < Y * raw_pitch_y
    for dims in ((0, 67, 131), (33, 0, 131), (33, 67, 0)):
        assert call(eng.ctx, lp, rp, *dims, 144, 80 * 144, n, 3, good, op, cp) == _lib.DLV_EINVAL
    assert call(eng.ctx, None, rp, 33, 67, 131, 144, 80 * 144, n, 3, good, op, cp) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, None, 33, 67, 131, 144, 80 * 144, n, 3, good, op, cp) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, rp, 33, 67, 131, 144, 80 * 144, n, 3, good, None, cp) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, rp, 33, 67, 131, 144, 80 * 144, n, 3, good, op, None) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, rp, 33, 67, 131, 144, 80 * 144, 2**32 - 1, 3, good, op, cp) == _lib.DLV_EINVAL
    assert call(eng.ctx, C.c_void_p(lab_dev.data_ptr() + 2), rp, 33, 67, 131, 144, 80 * 144, n, 3, good, op, cp) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, C.c_void_p(raw_dev.data_ptr() + 1), 33, 67, 131, 144, 80 * 144, n, 3, good, op, cp) == _lib.DLV_EINVAL
    assert (out == 0x5A5A).all() and (cnt == 0xA5A5A5A5).all()  # refused: nothing written
    five = levels(*FIVE)
    assert call(eng.ctx, lp, rp, 33, 67, 131, 144, 80 * 144, n, 5, five, op, cp) == 0
    _assert_pair((out.ravel()[:(n + 1) * 5].reshape(n + 1, 5), cnt), ref)  # (n+1) x n_levels, row-major
    assert (out.ravel()[(n + 1) * 5:] == 0x5A5A).all()
    # the engine: a raw volume smaller than the labels on any axis, a wrong dtype, rank, layout or device, bad levels
    for small in (raw[:32], raw[:, :66], raw[:, :, :130]):
        with pytest.raises(ValueError, match="smaller"):
            eng.cc_quantiles(lab_dev, _raw_dev(small), n)
    with pytest.raises(ValueError):
        eng.cc_quantiles(lab_dev, raw_dev.view(torch.uint8), n)
    with pytest.raises(ValueError):
        eng.cc_quantiles(lab_dev.view(torch.float32), raw_dev, n)
    with pytest.raises(ValueError):
        eng.cc_quantiles(lab_dev.reshape(-1), raw_dev, n)
    with pytest.raises(ValueError):
        eng.cc_quantiles(lab_dev, raw_dev.transpose(1, 2), n)  # (last axis not contiguous)
    with pytest.raises(ValueError):
        eng.cc_quantiles(lab_dev.cpu(), raw_dev, n)
    with pytest.raises(ValueError):
        eng.cc_quantiles(lab_dev, raw_dev.cpu(), n)
    for bad in ((), (50, 25), (25, 25), (101,), (25.0, 50), (True,), tuple(range(9))):
        with pytest.raises(ValueError, match="levels"):
            eng.cc_quantiles(lab_dev, raw_dev, n, bad)


# ---- 6. count_blobs end to end ------------------------------------------------------------------------------------------
def _brain_on_disk(tmp_path, mask, raw):
    """step 2's output and the padded raw volume of the brain 'brain' (both .npy with numpy's 128-byte header) -> input folder"""
    d = tmp_path / "in" / "brain"
    os.makedirs(d / "binary_segmentations")
    np.save(str(d / "binary_segmentations" / "binaries.npy"), mask)
    os.makedirs(d / "masked_niftis")
    np.save(str(d / "masked_niftis" / "x.npy"), raw[None, None])
    return str(tmp_path / "in")


def _settings(path_in, post, **mi355x):
    s = {"postprocessing": {"output_location": post + "/"}, "blob_detection": {"input_location": path_in}}
    if mi355x:
        s["mi355x"] = mi355x
    return s


def _read(post, name):
    with open(os.path.join(post, name), "rb") as fh:
        return fh.read()


def _check_outputs(eng, post, shape, raw, n, shell_radius=0, more_keys=(), more_names=()):
    """pickle keys, cell_quartiles/brain.csv and last_quartiles of a run with the switch on against numpy on the label file the
    run wrote (and, with a shell, on HipEngine.cc_shell's volume of those labels) -> the pickle"""
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import cell_quartiles_csv_text

    labels = np.load(os.path.join(post, f"brain-{n}-cc3d.npy")).astype(np.uint32)
    crop = np.ascontiguousarray(raw[:shape[0], :shape[1], :shape[2]])
    values, counts = reference(labels, crop, n)
    stats = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(stats) == STD_KEYS | INTENSITY_KEYS | set(QUARTILE_KEYS) | (SHELL_KEYS | set(SHELL_QUARTILE_KEYS) if shell_radius else set()) | set(more_keys)
    np.testing.assert_array_equal(stats["voxel_counts"][1:], counts[1:])
    expected = {"voxel_counts": stats["voxel_counts"]}
    for k, key in enumerate(QUARTILE_KEYS):
        assert stats[key].dtype == np.uint16 and stats[key].shape == (n + 1,) and stats[key][0] == 0, key
        np.testing.assert_array_equal(stats[key], values[:, k], err_msg=key)
        expected[key] = values[:, k]
    if shell_radius:
        shell = eng.cc_shell(_labels_dev(labels), shell_radius, _raw_dev(raw)).cpu().numpy().view(np.uint32)
        shell_values, shell_counts = reference(shell, crop, n)
        assert (shell_counts[1:] > 0).any() and (crop[shell != 0] != 0).all()
        np.testing.assert_array_equal(stats["shell_voxels"], shell_counts)
        for k, key in enumerate(SHELL_QUARTILE_KEYS[:3]):
            assert stats[key].dtype == np.uint16 and stats[key].shape == (n + 1,), key
            np.testing.assert_array_equal(stats[key], shell_values[:, k], err_msg=key)
            expected[key] = shell_values[:, k]
        contrast = np.zeros(n + 1, dtype=np.float64)
        present = shell_counts > 0
        contrast[present] = values[present, 1].astype(np.float64) / shell_values[present, 1].astype(np.float64)
        assert stats["contrast_median"].dtype == np.float64
        np.testing.assert_array_equal(stats["contrast_median"], contrast)
        expected.update(shell_voxels=shell_counts, contrast_median=contrast)
    text = _read(post, os.path.join("cell_quartiles", "brain.csv")).decode()
    assert text == cell_quartiles_csv_text(expected, n)
    assert text.startswith("Blob,Size,Q25,Median,Q75" + (",ShellSize,ShellQ25,ShellMedian,ShellQ75,ContrastMedian\n" if shell_radius else "\n"))
    assert text.count("\n") == n + 1 and text.endswith("\n")
    assert os.listdir(os.path.join(post, "cell_quartiles")) == ["brain.csv"]
    assert sorted(os.listdir(post)) == sorted([f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle", "cell_intensity",
                                               "cell_quartiles", *more_names])
    assert count_blobs.last_quartiles == {"n": n}
    return stats


@pytest.fixture(scope="module")
def brain():
    rng = np.random.default_rng(11)
    mask = (rng.random((40, 64, 72)) < 0.05).astype(np.uint8)
    raw = rng.integers(0, 65536, size=(48, 64, 96), dtype=np.uint16)
    mask.setflags(write=False)
    raw.setflags(write=False)
    return mask, raw


def test_count_blobs_switch_on_adds_keys_and_table_and_off_changes_nothing(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, raw)
    shape, stack = mask.shape, (1, 1) + mask.shape
    on = str(tmp_path / "on")
    n = count_blobs(_settings(path_in, on, intensity_stats=True, intensity_quartiles=True), path_in, 0, "brain", stack, engine=eng)
    assert n == 4356
    stats_on = _check_outputs(eng, on, shape, raw, n)
    assert stats_on["voxel_counts"][1:].max() == 23
    assert count_blobs.last_timings["quartiles_s"] > 0 and count_blobs.last_timings["intensity_s"] > 0
    # intensity_stats alone (the key absent, and false): no table, no keys - and every file the switch does not add has the same bytes
    base, base2 = str(tmp_path / "base"), str(tmp_path / "base2")
    assert count_blobs(_settings(path_in, base, intensity_stats=True), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_quartiles is None and "quartiles_s" not in count_blobs.last_timings
    assert count_blobs(_settings(path_in, base2, intensity_stats=True, intensity_quartiles=False), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_quartiles is None and "quartiles_s" not in count_blobs.last_timings
    names = sorted([f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle", "cell_intensity"])
    assert sorted(os.listdir(base)) == names and sorted(os.listdir(base2)) == names
    for name in (f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle", os.path.join("cell_intensity", "brain.csv")):
        assert _read(base, name) == _read(base2, name), name
        if name != "brain-stats.pickle":
            assert _read(on, name) == _read(base, name), name
    stats_base = pickle.loads(_read(base, "brain-stats.pickle"))
    assert set(stats_base) == STD_KEYS | INTENSITY_KEYS
    for k in stats_base:
        assert stats_on[k].dtype == stats_base[k].dtype
        np.testing.assert_array_equal(stats_on[k], stats_base[k])
    # without any mi355x key, and with the key false alone: the three files and the three keys
    off, off2 = str(tmp_path / "off"), str(tmp_path / "off2")
    assert count_blobs(_settings(path_in, off), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs(_settings(path_in, off2, intensity_quartiles=False), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_quartiles is None and count_blobs.last_intensity is None
    names = sorted([f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle"])
    assert sorted(os.listdir(off)) == names and sorted(os.listdir(off2)) == names
    for name in names:
        assert _read(off, name) == _read(off2, name), name
    assert set(pickle.loads(_read(off, "brain-stats.pickle"))) == STD_KEYS
    assert _read(off, f"brain-{n}-cc3d.npy") == _read(on, f"brain-{n}-cc3d.npy")


def test_count_blobs_with_a_background_shell_measures_the_shells_too(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, raw = brain
    raw = raw.copy()
    raw[:, :, 40:48] = 0  # "outside the tissue": such voxels belong to no shell, and some cells there have none
    path_in = _brain_on_disk(tmp_path, mask, raw)
    post = str(tmp_path / "post")
    n = count_blobs(_settings(path_in, post, intensity_stats=True, background_shell=2, intensity_quartiles=True), path_in, 0, "brain",
                    (1, 1) + mask.shape, engine=eng)
    stats = _check_outputs(eng, post, mask.shape, raw, n, shell_radius=2)
    assert (stats["shell_median"][1:] > 0).any() and (stats["contrast_median"][1:] > 0).any()
    base = str(tmp_path / "base")
    assert count_blobs(_settings(path_in, base, intensity_stats=True, background_shell=2), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng) == n
    assert _read(post, os.path.join("cell_intensity", "brain.csv")) == _read(base, os.path.join("cell_intensity", "brain.csv"))
    stats_base = pickle.loads(_read(base, "brain-stats.pickle"))
    assert set(stats_base) == STD_KEYS | INTENSITY_KEYS | SHELL_KEYS
    for k in stats_base:
        np.testing.assert_array_equal(stats[k], stats_base[k])


def test_count_blobs_measures_the_final_labels_after_the_size_filter_and_the_split(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, raw)
    post = str(tmp_path / "filtered")
    n = count_blobs(_settings(path_in, post, intensity_stats=True, intensity_quartiles=True, size_filter=True), path_in, 0, "brain",
                    (1, 1) + mask.shape, 3, 20, engine=eng)
    assert count_blobs.last_filter["n_kept"] == n and 1 < n < count_blobs.last_filter["n_before"]
    stats = _check_outputs(eng, post, mask.shape, raw, n)
    assert stats["voxel_counts"][1:].min() >= 3 and stats["voxel_counts"][1:].max() <= 20
    post = str(tmp_path / "split")
    n = count_blobs(_settings(path_in, post, intensity_stats=True, intensity_quartiles=True, split_fused=1), path_in, 0, "brain",
                    (1, 1) + mask.shape, engine=eng)
    assert count_blobs.last_split["n_after"] == n
    _check_outputs(eng, post, mask.shape, raw, n, more_keys=("split_parent", "split_siblings", "split_depth"))


def test_count_blobs_on_cached_labels_completes_a_cached_pickle(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, raw)
    post, stack = str(tmp_path / "post"), (1, 1) + mask.shape
    n = count_blobs(_settings(path_in, post), path_in, 0, "brain", stack, engine=eng)
    label_bytes, csv_bytes = _read(post, f"brain-{n}-cc3d.npy"), _read(post, f"{mask.shape}_brain.csv")
    before = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(before) == STD_KEYS
    both = _settings(path_in, post, intensity_stats=True, intensity_quartiles=True)
    assert count_blobs(both, path_in, 0, "brain", stack, engine=eng) == n
    stats = _check_outputs(eng, post, mask.shape, raw, n)
    for k in STD_KEYS:
        assert stats[k].dtype == before[k].dtype
        np.testing.assert_array_equal(stats[k], before[k])
    assert _read(post, f"brain-{n}-cc3d.npy") == label_bytes and _read(post, f"{mask.shape}_brain.csv") == csv_bytes
    # a third run finds the keys in the cached pickle: nothing is measured again, the pickle keeps its bytes
    pickle_bytes = _read(post, "brain-stats.pickle")
    assert count_blobs(both, path_in, 0, "brain", stack, engine=eng) == n
    assert _read(post, "brain-stats.pickle") == pickle_bytes and "quartiles_s" not in count_blobs.last_timings
    assert count_blobs.last_quartiles == {"n": n}
    # a pickle with the moment statistics and without the quartiles: the quartiles alone are added
    part = str(tmp_path / "part")
    assert count_blobs(_settings(path_in, part, intensity_stats=True), path_in, 0, "brain", stack, engine=eng) == n
    moments = pickle.loads(_read(part, "brain-stats.pickle"))
    assert count_blobs(_settings(path_in, part, intensity_stats=True, intensity_quartiles=True), path_in, 0, "brain", stack, engine=eng) == n
    stats = _check_outputs(eng, part, mask.shape, raw, n)
    for k in moments:
        np.testing.assert_array_equal(stats[k], moments[k])
    # ... and with a shell asked for, the pickle lacks the shell keys: completed with them
    shell = _settings(path_in, part, intensity_stats=True, intensity_quartiles=True, background_shell=2)
    assert count_blobs(shell, path_in, 0, "brain", stack, engine=eng) == n
    _check_outputs(eng, part, mask.shape, raw, n, shell_radius=2)
    pickle_bytes = _read(part, "brain-stats.pickle")
    assert count_blobs(shell, path_in, 0, "brain", stack, engine=eng) == n
    assert _read(part, "brain-stats.pickle") == pickle_bytes


def test_refusals_leave_the_output_location_without_new_files(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, raw)
    post = str(tmp_path / "post")
    os.makedirs(post)
    open(os.path.join(post, "kept.txt"), "w").close()
    stack = (1, 1) + mask.shape
    with pytest.raises(ValueError, match="needs settings.*intensity_stats"):
        count_blobs(_settings(path_in, post, intensity_quartiles=True), path_in, 0, "brain", stack, engine=eng)
    assert os.listdir(post) == ["kept.txt"]
    for bad in (1, "yes"):
        with pytest.raises(ValueError, match="intensity_quartiles"):
            count_blobs(_settings(path_in, post, intensity_stats=True, intensity_quartiles=bad), path_in, 0, "brain", stack, engine=eng)
        assert os.listdir(post) == ["kept.txt"]
    with pytest.raises(MemoryError, match="hbm_budget_gb"):
        count_blobs(_settings(path_in, post, intensity_stats=True, intensity_quartiles=True, hbm_budget_gb=1e-4), path_in, 0, "brain", stack,
                    engine=eng)
    assert os.listdir(post) == ["kept.txt"]
    # a budget that holds what intensity_stats needs (mask, labels, scratch and raw: 7 + 2 bytes per voxel) and not 2 more
    from delivr_cfos_amd.streaming import ccl_bytes_per_voxel

    assert ccl_bytes_per_voxel() == 7
    with pytest.raises(MemoryError, match=r"intensity_quartiles.*2 more bytes per voxel.*hbm_budget_gb"):
        count_blobs(_settings(path_in, post, intensity_stats=True, intensity_quartiles=True, hbm_budget_gb=mask.size * 10 / 2**30), path_in, 0,
                    "brain", stack, engine=eng)
    assert os.listdir(post) == ["kept.txt"]
    assert count_blobs.last_quartiles is None
    # ... and the same for cached labels (4 + 2 bytes per voxel for the moments, 2 more for the quartiles)
    cached = str(tmp_path / "cached")
    n = count_blobs(_settings(path_in, cached), path_in, 0, "brain", stack, engine=eng)
    listing = sorted(os.listdir(cached))
    with pytest.raises(MemoryError, match=r"intensity_quartiles.*cached labels.*hbm_budget_gb"):
        count_blobs(_settings(path_in, cached, intensity_stats=True, intensity_quartiles=True, hbm_budget_gb=mask.size * 7 / 2**30), path_in, 0,
                    "brain", stack, engine=eng)
    assert sorted(os.listdir(cached)) == listing and count_blobs.last_quartiles is None and n > 0
