"""Per-cell raw intensity statistics on the device (dlv_cc_intensity_dev / HipEngine.cc_intensity;
settings["mi355x"]["intensity_stats"] in count_blobs).

The reference of every case is numpy on the labels dlv_ccl26_dev returned: flatten, stable argsort by label, add / minimum /
maximum.reduceat over the runs of equal labels, sums in uint64 (np.bincount(weights=...) would go through float64).  Everything
compared is an integer - equality, no tolerance; the mean is float64 equality with sum.astype(float64) / count."""
import ctypes as C
import importlib.util
import os
import pickle
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("intensity_sum", "intensity_sumsq", "intensity_min", "intensity_max")


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference(labels: np.ndarray, raw: np.ndarray, n: int) -> dict:
    """the ABI's rows 0..n: absent labels - and row 0 - read 0, 0, 0xFFFF, 0; labels above n are left out"""
    assert labels.shape == raw.shape
    lab = labels.ravel()
    order = np.argsort(lab, kind="stable")
    ls, vs = lab[order], raw.ravel()[order].astype(np.uint64)
    starts = np.flatnonzero(np.r_[True, ls[1:] != ls[:-1]])
    present = ls[starts].astype(np.int64)
    sel = (present >= 1) & (present <= n)
    out = {"intensity_sum": np.zeros(n + 1, dtype=np.uint64), "intensity_sumsq": np.zeros(n + 1, dtype=np.uint64),
           "intensity_min": np.full(n + 1, 0xFFFF, dtype=np.uint16), "intensity_max": np.zeros(n + 1, dtype=np.uint16)}
    out["intensity_sum"][present[sel]] = np.add.reduceat(vs, starts)[sel]
    out["intensity_sumsq"][present[sel]] = np.add.reduceat(vs * vs, starts)[sel]
    out["intensity_min"][present[sel]] = np.minimum.reduceat(vs, starts)[sel].astype(np.uint16)
    out["intensity_max"][present[sel]] = np.maximum.reduceat(vs, starts)[sel].astype(np.uint16)
    return out


def _finished(labels, raw, n):
    """what count_blobs stores, from numpy alone: the reference with row 0's minimum 0, the mean and the voxel counts"""
    ref = _reference(labels, raw, n)
    ref["intensity_min"][0] = 0
    counts = np.bincount(labels.ravel(), minlength=n + 1)
    mean = np.zeros(n + 1, dtype=np.float64)
    present = counts > 0
    present[0] = False  # (row 0: the background's count, no sum)
    mean[present] = ref["intensity_sum"][present].astype(np.float64) / counts[present]
    ref["intensity_mean"] = mean
    ref["voxel_counts"] = counts.astype(np.uint32)
    return ref


def _assert_same(got: dict, ref: dict, keys=KEYS):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


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


# ---- 1. odd geometry, padded raw, both alignments ------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd(eng):
    """33 x 67 x 131 labels (x no multiple of 4: the rows of the labels start on a 16-byte boundary every fourth row only) of the
    size-filter tests' pitch-4 box mask under a 48 x 80 x 144 raw volume; expected from raw[:33, :67, :131]"""
    rng = np.random.default_rng(5)
    shape = (33, 67, 131)
    mask = np.zeros(shape, dtype=np.uint8)
    for z in range(0, shape[0], 4):
        for y in range(0, shape[1], 4):
            ext = rng.integers(1, 4, size=(len(range(0, shape[2], 4)), 3))
            for (dz, dy, dx), x in zip(ext, range(0, shape[2], 4)):
                mask[z:z + dz, y:y + dy, x:x + dx] = 1
    labels, n = _label(eng, mask)
    assert n == 9 * 17 * 33
    raw = rng.integers(0, 65536, size=(48, 80, 144), dtype=np.uint16)
    inside = np.argwhere(mask)
    for value, picks in ((0, inside[::7]), (65535, inside[3::11])):
        raw[picks[:, 0], picks[:, 1], picks[:, 2]] = value
    ref = _reference(labels, raw[:33, :67, :131], n)
    assert (ref["intensity_min"][1:] == 0).any() and (ref["intensity_max"][1:] == 65535).any()
    for a in (labels, raw, *ref.values()):
        a.setflags(write=False)
    return labels, n, raw, ref


def test_odd_geometry_padded_raw_fresh_tensors(eng, odd):
    import torch

    labels, n, raw, ref = odd
    lab_dev, raw_dev = _labels_dev(labels), _raw_dev(raw)
    assert lab_dev.data_ptr() % 16 == 0 and raw_dev.data_ptr() % 16 == 0
    got = eng.cc_intensity(lab_dev, raw_dev, n)
    assert list(got) == list(KEYS)
    _assert_same(got, ref)
    assert [int(got[k][0]) for k in KEYS] == [0, 0, 0xFFFF, 0]  # the background is not measured
    _assert_same(eng.cc_intensity(lab_dev, raw_dev.view(torch.int16), n), ref)  # an int16-viewed volume is the same bytes
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
    _assert_same(eng.cc_intensity(lab_view, raw_view, n), ref)
    np.testing.assert_array_equal(lab_buf.cpu().numpy(), lab_host)  # guards and payload untouched
    np.testing.assert_array_equal(raw_buf.cpu().numpy(), raw_host)


def test_odd_geometry_raw_of_exactly_the_labels_shape_with_an_odd_pitch(eng, odd):
    labels, n, raw, ref = odd
    tight = _raw_dev(raw[:33, :67, :131])
    assert tuple(tight.stride()) == (67 * 131, 131, 1)
    _assert_same(eng.cc_intensity(_labels_dev(labels), tight, n), ref)
    # ... and the same voxels as a view into the padded volume: the pitches come from the strides
    view = _raw_dev(raw)[:33, :67, :131]
    assert tuple(view.stride()) == (80 * 144, 144, 1)
    _assert_same(eng.cc_intensity(_labels_dev(labels), view, n), ref)


# ---- 2. one giant component beside specks -----------------------------------------------------------------------------
def test_one_giant_component_beside_specks(eng):
    rng = np.random.default_rng(7)
    mask = np.zeros((64, 64, 96), dtype=np.uint8)
    mask[8:56, 8:56, 16:80] = 1  # 147 456 voxels behind one label: every lane of every wave adds to the same row
    mask[::2, ::2, 84::2] = rng.integers(0, 2, size=(32, 32, 6), dtype=np.uint8)  # isolated voxels, some ahead of the block in raster order
    labels, n = _label(eng, mask)
    block = int(labels[8, 8, 16])
    raw = rng.integers(0, 65536, size=mask.shape, dtype=np.uint16)
    raw[8:56, 8:56, 16:80] = 65535
    ref = _reference(labels, raw, n)
    assert 1 < block < n and int(ref["intensity_sum"][block]) == 147456 * 65535 > 2**32
    assert int(ref["intensity_sumsq"][block]) == 147456 * 65535**2 > 2**49
    got = eng.cc_intensity(_labels_dev(labels), _raw_dev(raw), n)
    _assert_same(got, ref)
    assert got["intensity_min"][block] == got["intensity_max"][block] == 65535  # a true minimum of 65535, not the absent marker
    specks = np.arange(1, n + 1) != block
    np.testing.assert_array_equal(got["intensity_min"][1:][specks], got["intensity_max"][1:][specks])  # single voxels


# ---- 3. more than 2^16 labels ---------------------------------------------------------------------------------------
def test_more_than_2_to_16_labels_every_row_exact(eng):
    rng = np.random.default_rng(6)
    shape = (64, 96, 144)
    mask = np.zeros(shape, dtype=np.uint8)
    mask[::2, ::2, ::3] = 1
    mask[::2, ::2, 1::3] = rng.integers(0, 2, size=(32, 48, 48), dtype=np.uint8)  # singles or x-pairs
    labels, n = _label(eng, mask)
    assert n == 32 * 48 * 48 and n > 65536
    raw = rng.integers(0, 65536, size=shape, dtype=np.uint16)
    _assert_same(eng.cc_intensity(_labels_dev(labels), _raw_dev(raw), n), _reference(labels, raw, n))


# ---- 4. degenerate cases ----------------------------------------------------------------------------------------------
def test_empty_mask_labels_above_n_and_refused_arguments(eng, odd):
    import torch
    from delivr_cfos_amd import _lib

    empty = np.zeros((9, 10, 11), dtype=np.uint8)
    labels0, n0 = _label(eng, empty)
    assert n0 == 0
    raw0 = np.random.default_rng(1).integers(0, 65536, size=(9, 10, 11), dtype=np.uint16)
    got = eng.cc_intensity(_labels_dev(labels0), _raw_dev(raw0), 0)
    assert {k: v.tolist() for k, v in got.items()} == {"intensity_sum": [0], "intensity_sumsq": [0], "intensity_min": [0xFFFF],
                                                       "intensity_max": [0]}
    labels, n, raw, ref = odd
    lab_dev, raw_dev = _labels_dev(labels), _raw_dev(raw)
    few = 100  # labels above n are ignored: the rows 0..100 are those of the whole table
    _assert_same(eng.cc_intensity(lab_dev, raw_dev, few), {k: v[:few + 1] for k, v in ref.items()})
    _assert_same(eng.cc_intensity(lab_dev, raw_dev, few), _reference(labels, raw[:33, :67, :131], few))
    # the C entry point: raw_pitch_y < X, raw_pitch_z < Y * raw_pitch_y, an empty axis, a NULL pointer
    out = {"s": np.zeros(n + 1, np.uint64), "q": np.zeros(n + 1, np.uint64), "lo": np.zeros(n + 1, np.uint16), "hi": np.zeros(n + 1, np.uint16)}
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in out.values()]
    lp, rp = C.c_void_p(lab_dev.data_ptr()), C.c_void_p(raw_dev.data_ptr())
    call = eng.lib.dlv_cc_intensity_dev
    assert call(eng.ctx, lp, rp, 33, 67, 131, 130, 80 * 144, n, *ptrs) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, rp, 33, 67, 131, 144, 67 * 144 - 1, n, *ptrs) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, rp, 33, 0, 131, 144, 80 * 144, n, *ptrs) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, None, 33, 67, 131, 144, 80 * 144, n, *ptrs) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, rp, 33, 67, 131, 144, 80 * 144, n, ptrs[0], ptrs[1], ptrs[2], None) == _lib.DLV_EINVAL
    assert not any(a.any() for a in out.values())  # refused: nothing written
    assert call(eng.ctx, lp, rp, 33, 67, 131, 144, 80 * 144, n, *ptrs) == 0
    _assert_same(dict(zip(KEYS, out.values())), ref)
    # the engine: a raw volume smaller than the labels on any axis, a wrong dtype, rank, layout or device
    for small in (raw[:32], raw[:, :66], raw[:, :, :130]):
        with pytest.raises(ValueError, match="smaller"):
            eng.cc_intensity(lab_dev, _raw_dev(small), n)
    with pytest.raises(ValueError):
        eng.cc_intensity(lab_dev, raw_dev.view(torch.uint8), n)
    with pytest.raises(ValueError):
        eng.cc_intensity(lab_dev.view(torch.float32), raw_dev, n)
    with pytest.raises(ValueError):
        eng.cc_intensity(lab_dev.reshape(-1), raw_dev, n)
    with pytest.raises(ValueError):
        eng.cc_intensity(lab_dev, raw_dev.transpose(1, 2), n)  # (last axis not contiguous)
    with pytest.raises(ValueError):
        eng.cc_intensity(lab_dev.cpu(), raw_dev, n)
    with pytest.raises(ValueError):
        eng.cc_intensity(lab_dev, raw_dev.cpu(), n)


# ---- 5. slabs add up --------------------------------------------------------------------------------------------------
def _seam_volume():
    """the 45 x 40 x 56 volume of the size-filter tests: three even slabs, components across the seams at z = 15 and z = 30"""
    rng = np.random.default_rng(13)
    m = (rng.random((45, 40, 56)) < 0.03).astype(np.uint8)
    m[:, 18:23, 28:33] = 0
    m[10:20, 20, 30] = 1
    m[29:31, 20, 30] = 1
    raw = rng.integers(0, 65536, size=(48, 48, 64), dtype=np.uint16)
    return m, raw


def test_slabs_of_the_global_labels_merge_to_the_whole_volume(eng):
    from delivr_cfos_amd.hostlogic import merge_intensity

    m, raw = _seam_volume()
    labels, n = _label(eng, m)
    assert labels[14, 20, 30] == labels[15, 20, 30] != 0 and labels[29, 20, 30] == labels[30, 20, 30] != 0
    lab_dev, raw_dev = _labels_dev(labels), _raw_dev(raw)
    whole = eng.cc_intensity(lab_dev, raw_dev, n)
    _assert_same(whole, _reference(labels, raw[:45, :40, :56], n))
    parts = [eng.cc_intensity(lab_dev[lo:hi], raw_dev[lo:hi], n) for lo, hi in ((0, 15), (15, 30), (30, 45))]
    assert all((p["intensity_min"][1:] == 0xFFFF).any() for p in parts)  # every slab lacks some labels
    _assert_same(merge_intensity(parts), whole)
    _assert_same(merge_intensity([parts[2], None, parts[0], parts[1]]), whole)


# ---- 6. count_blobs end to end ------------------------------------------------------------------------------------------
STD_KEYS = {"voxel_counts", "bounding_boxes", "centroids"}
ALL_KEYS = STD_KEYS | set(KEYS) | {"intensity_mean"}


def _brain_on_disk(tmp_path, mask, raw):
    """step 2's output and the padded raw volume of the brain 'brain' (both .npy with numpy's 128-byte header) -> input folder"""
    d = tmp_path / "in" / "brain"
    os.makedirs(d / "binary_segmentations")
    np.save(str(d / "binary_segmentations" / "binaries.npy"), mask)
    if raw is not None:
        os.makedirs(d / "masked_niftis")
        np.save(str(d / "masked_niftis" / "x.npy"), raw[None, None])
        assert np.load(str(d / "masked_niftis" / "x.npy"), mmap_mode="r").offset == 128
    return str(tmp_path / "in")


def _settings(path_in, post, **mi355x):
    s = {"postprocessing": {"output_location": post + "/"}, "blob_detection": {"input_location": path_in}}
    if mi355x:
        s["mi355x"] = mi355x
    return s


def _read(post, name):
    with open(os.path.join(post, name), "rb") as fh:
        return fh.read()


def _check_outputs(post, shape, raw, n, raw_file):
    """pickle, table and last_intensity of a run with the switch on against numpy on the label file the run wrote"""
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import cell_intensity_csv_text

    labels = np.load(os.path.join(post, f"brain-{n}-cc3d.npy")).astype(np.uint32)
    ref = _finished(labels, raw[:shape[0], :shape[1], :shape[2]], n)
    stats = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(stats) == ALL_KEYS
    _assert_same(stats, ref, KEYS + ("intensity_mean", "voxel_counts"))
    assert stats["intensity_min"][0] == 0 and stats["intensity_mean"][0] == 0.0
    assert _read(post, os.path.join("cell_intensity", "brain.csv")).decode() == cell_intensity_csv_text(ref, n)
    assert os.listdir(os.path.join(post, "cell_intensity")) == ["brain.csv"]
    assert sorted(os.listdir(post)) == sorted([f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle", "cell_intensity"])
    assert count_blobs.last_intensity == {"n": n, "raw_file": raw_file}
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
    raw_file = os.path.join(path_in, "brain", "masked_niftis", "x.npy")
    shape = mask.shape
    on = str(tmp_path / "on")
    n = count_blobs(_settings(path_in, on, intensity_stats=True), path_in, 0, "brain", (1, 1) + shape, engine=eng)
    stats_on = _check_outputs(on, shape, raw, n, raw_file)
    assert "intensity_s" in count_blobs.last_timings
    # off (the key absent, and false): the parent's files - the same listing, the same bytes in both runs, the three keys
    off, off2 = str(tmp_path / "off"), str(tmp_path / "off2")
    assert count_blobs(_settings(path_in, off), path_in, 0, "brain", (1, 1) + shape, engine=eng) == n
    assert count_blobs.last_intensity is None and "intensity_s" not in count_blobs.last_timings
    assert count_blobs(_settings(path_in, off2, intensity_stats=False), path_in, 0, "brain", (1, 1) + shape, engine=eng) == n
    assert count_blobs.last_intensity is None
    names = sorted([f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle"])
    assert sorted(os.listdir(off)) == names and sorted(os.listdir(off2)) == names
    for name in names:
        assert _read(off, name) == _read(off2, name), name
    stats_off = pickle.loads(_read(off, "brain-stats.pickle"))
    assert set(stats_off) == STD_KEYS
    # ... and the switch changes neither the label file nor the reference's CSV nor the three entries
    assert _read(on, f"brain-{n}-cc3d.npy") == _read(off, f"brain-{n}-cc3d.npy")
    assert _read(on, f"{shape}_brain.csv") == _read(off, f"{shape}_brain.csv")
    for k in STD_KEYS:
        np.testing.assert_array_equal(stats_on[k], stats_off[k])
    assert np.array_equal(np.load(raw_file)[0, 0], raw)  # the raw volume is read, never written


def test_count_blobs_with_the_size_filter_measures_the_filtered_labels(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, raw)
    post = str(tmp_path / "post")
    n = count_blobs(_settings(path_in, post, intensity_stats=True, size_filter=True), path_in, 0, "brain", (1, 1) + mask.shape, 3, 20,
                    engine=eng)
    assert count_blobs.last_filter["n_kept"] == n and 1 < n < count_blobs.last_filter["n_before"]
    stats = _check_outputs(post, mask.shape, raw, n, os.path.join(path_in, "brain", "masked_niftis", "x.npy"))
    assert stats["voxel_counts"][1:].min() >= 3 and stats["voxel_counts"][1:].max() <= 20


def test_count_blobs_on_cached_labels_adds_the_keys_to_a_cached_pickle(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, raw)
    post = str(tmp_path / "post")
    n = count_blobs(_settings(path_in, post), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng)
    label_bytes, csv_bytes = _read(post, f"brain-{n}-cc3d.npy"), _read(post, f"{mask.shape}_brain.csv")
    before = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(before) == STD_KEYS
    assert count_blobs(_settings(path_in, post, intensity_stats=True), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng) == n
    stats = _check_outputs(post, mask.shape, raw, n, os.path.join(path_in, "brain", "masked_niftis", "x.npy"))
    for k in STD_KEYS:
        assert stats[k].dtype == before[k].dtype
        np.testing.assert_array_equal(stats[k], before[k])
    assert _read(post, f"brain-{n}-cc3d.npy") == label_bytes and _read(post, f"{mask.shape}_brain.csv") == csv_bytes
    # a third run finds the keys in the cached pickle: nothing is measured again, the pickle keeps its bytes
    pickle_bytes = _read(post, "brain-stats.pickle")
    assert count_blobs(_settings(path_in, post, intensity_stats=True), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng) == n
    assert _read(post, "brain-stats.pickle") == pickle_bytes and "intensity_s" not in count_blobs.last_timings
    # cached labels without a cached pickle: statistics and intensities both from the label file
    os.remove(os.path.join(post, "brain-stats.pickle"))
    shutil.rmtree(os.path.join(post, "cell_intensity"))
    assert count_blobs(_settings(path_in, post, intensity_stats=True), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng) == n
    _check_outputs(post, mask.shape, raw, n, os.path.join(path_in, "brain", "masked_niftis", "x.npy"))


# ---- 7. sharded -------------------------------------------------------------------------------------------------------
def test_count_blobs_under_torch_distributed_equals_the_single_engine_result(eng, tmp_path, monkeypatch):
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs

    ranks = _helper("thread_ranks")
    m, raw = _seam_volume()
    path_in = _brain_on_disk(tmp_path, m, raw)
    raw_file = os.path.join(path_in, "brain", "masked_niftis", "x.npy")
    single = str(tmp_path / "single")
    n = count_blobs(_settings(path_in, single, intensity_stats=True), path_in, 0, "brain", (1, 1) + m.shape, engine=eng)
    ref = _check_outputs(single, m.shape, raw, n, raw_file)
    fake = ranks.ThreadRanks(3)
    fake.patch(monkeypatch, dist)
    for filtered in (False, True):
        post = str(tmp_path / f"sharded{int(filtered)}")
        settings = _settings(path_in, post, intensity_stats=True, size_filter=filtered)
        results = ranks.run_thread_ranks(fake, lambda rank, e: count_blobs(settings, path_in, 0, "brain", (1, 1) + m.shape, 2, 8, engine=e))
        k = results[0]
        assert results == [k] * 3 and (k < n if filtered else k == n)
        stats = _check_outputs(post, m.shape, raw, k, raw_file)  # rank 0's pickle and table against numpy on the written labels
        if not filtered:
            for key in ALL_KEYS:
                np.testing.assert_array_equal(stats[key], ref[key])
            for name in (f"{m.shape}_brain.csv", os.path.join("cell_intensity", "brain.csv")):
                assert _read(post, name) == _read(single, name), name
            np.testing.assert_array_equal(np.load(os.path.join(post, f"brain-{n}-cc3d.npy")), np.load(os.path.join(single, f"brain-{n}-cc3d.npy")))


# ---- 8. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_location_without_new_files(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, None)
    post = str(tmp_path / "post")
    os.makedirs(post)
    open(os.path.join(post, "kept.txt"), "w").close()
    stack = (1, 1) + mask.shape
    with pytest.raises(FileNotFoundError):  # no masked_niftis folder
        count_blobs(_settings(path_in, post, intensity_stats=True), path_in, 0, "brain", stack, engine=eng)
    assert os.listdir(post) == ["kept.txt"]
    os.makedirs(os.path.join(path_in, "brain", "masked_niftis"))
    with pytest.raises(FileNotFoundError):  # ... and no .npy in it
        count_blobs(_settings(path_in, post, intensity_stats=True), path_in, 0, "brain", stack, engine=eng)
    assert os.listdir(post) == ["kept.txt"]
    raw_file = os.path.join(path_in, "brain", "masked_niftis", "x.npy")
    np.save(raw_file, raw[:, :, :71])  # one voxel short along x
    with pytest.raises(ValueError, match=r"\(48, 64, 71\).*\(40, 64, 72\)"):
        count_blobs(_settings(path_in, post, intensity_stats=True), path_in, 0, "brain", stack, engine=eng)
    assert os.listdir(post) == ["kept.txt"]
    np.save(raw_file, raw.astype(np.int32))
    with pytest.raises(ValueError, match="int32"):
        count_blobs(_settings(path_in, post, intensity_stats=True), path_in, 0, "brain", stack, engine=eng)
    assert os.listdir(post) == ["kept.txt"]
    np.save(raw_file, raw)
    with pytest.raises(MemoryError, match=r"intensity_stats.*hbm_budget_gb"):
        count_blobs(_settings(path_in, post, intensity_stats=True, hbm_budget_gb=1e-4), path_in, 0, "brain", stack, engine=eng)
    assert os.listdir(post) == ["kept.txt"]
    assert count_blobs.last_intensity is None
