"""The run-length coding of a label volume on the device (dlv_cc_runs_count_dev / _emit_dev / _decode_dev, HipEngine.cc_runs_encode /
cc_runs_decode) and count_blobs' settings["mi355x"]["label_file"] = "runs".

The reference of every case is delivr_cfos_amd.label_runs.encode_runs / decode_runs (pinned against a double loop over the voxels by
tests/test_label_runs_cpu.py) or the dense labels - never the device's own output.  Integer work only: every comparison is exact
equality.  Every test asserts the property of its input that it is there for.

The kernels walk rows with one wave per row in sweeps of 512 voxels (csrc/cc_runs.hip): a lane takes the quads [4l, 4l + 4) and
[256 + 4l, 256 + 4l + 4) of a sweep, and a launch has at most 8192 workgroups (RUNS_MAX_WG)."""
import ctypes as C
import os
import pickle
import threading

import numpy as np
import pytest

from delivr_cfos_amd import label_runs as lr

pytestmark = pytest.mark.gpu

MAX_WORKGROUPS = 8192  # RUNS_MAX_WG of csrc/cc_runs.hip
BIG = 2**32 - 2  # the largest label of the format


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def _dev(labels):
    import torch

    return torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint32).view(np.int32).copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _assert_runs_equal(got, want):
    assert tuple(got["shape"]) == tuple(want["shape"])
    for key, dtype in lr.ARRAYS:
        assert got[key].dtype == dtype and got[key].shape == want[key].shape, key
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def _round_trip(eng, labels):
    """device encode == numpy encode, device decode of it == the labels -> the runs"""
    want = lr.encode_runs(labels)
    got = eng.cc_runs_encode(_dev(labels))
    _assert_runs_equal(got, want)
    np.testing.assert_array_equal(_host(eng.cc_runs_decode(want)), labels)
    return want


# ---- 1. boundaries of the sweep layout -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def boundaries():
    rng = np.random.default_rng(11)
    Z, Y, X = 3, 5, 2051
    v = np.zeros((Z * Y, X), dtype=np.uint32)
    v[1] = 3
    v[2] = 1 + (np.arange(X) & 1)
    for k, x in enumerate((4, 256, 1024, 2048)):
        v[3, x - 2:x + 2] = 10 + k
    v[4, 0], v[4, X - 1] = 5, 9
    for r in range(5, Z * Y):
        x = int(rng.integers(0, 6)) if r > 5 else 0
        while x < X:
            n = int(rng.integers(1, 10))
            v[r, x:x + n] = BIG if rng.random() < 0.02 else rng.integers(1, 70001)
            x += n + int(rng.integers(0, 6))
    v[5, 0] = 9
    v = v.reshape(Z, Y, X)
    v.setflags(write=False)
    return v


def test_boundaries_of_the_sweep_layout(eng, boundaries):
    import torch

    v = boundaries
    flat = v.reshape(-1, v.shape[2])
    X = v.shape[2]
    want = lr.encode_runs(v)
    per_row = np.diff(want["row_start"].astype(np.int64))
    # what the input is there for
    assert X % 4 == 3 and X > 4 * 512  # the rows' alignment changes from row to row; more than one sweep, the last one partial
    assert per_row[0] == 0 and per_row[1] == 1 and per_row[2] == X > 512  # empty; one run of 2051; 2051 runs: the rank is carried
    assert want["x1"][want["row_start"][1]] == X - 1
    assert per_row[3] == 4 and want["x0"][want["row_start"][3]:want["row_start"][4]].tolist() == [2, 254, 1022, 2046]
    assert flat[4, X - 1] == flat[5, 0] == 9 and per_row[4] == 2  # a run does not continue into the next row
    assert want["x0"][want["row_start"][5]] == 0 and want["label"][want["row_start"][5]] == 9
    assert (per_row[5:] > 200).all() and (want["label"] == BIG).any() and (want["label"] > 65535).sum() > 10
    touching = (flat[:, 1:] != flat[:, :-1]) & (flat[:, 1:] != 0) & (flat[:, :-1] != 0)
    assert touching[5:].sum() > 100  # runs of different labels without a gap
    got = eng.cc_runs_encode(_dev(v))
    _assert_runs_equal(got, want)
    np.testing.assert_array_equal(_host(eng.cc_runs_decode(got)), v)
    # the same from a buffer that starts 4 bytes past a 16-byte boundary, guards on either side
    host = np.full(v.size + 2, 0x7FFFFFF0, dtype=np.int32)
    host[1:-1] = v.view(np.int32).ravel()
    buf = torch.from_numpy(host).cuda()
    view = buf[1:-1].view(v.shape)
    assert view.data_ptr() % 16 == 4
    _assert_runs_equal(eng.cc_runs_encode(view), want)
    out = torch.full((v.size + 2,), 0x7FFFFFF0, dtype=torch.int32, device="cuda")
    out_view = out[1:-1].view(v.shape)
    assert out_view.data_ptr() % 16 == 4
    eng.cc_runs_decode(want, out=out_view)
    back = out.cpu().numpy()
    assert back[0] == back[-1] == 0x7FFFFFF0
    np.testing.assert_array_equal(back[1:-1].view(np.uint32).reshape(v.shape), v)


# ---- 2. the uint16 limit ---------------------------------------------------------------------------------------------------
def test_rows_of_65536_voxels_and_the_refusal_above(eng):
    import torch

    from delivr_cfos_amd._lib import DLV_EUNSUP

    v = np.zeros((1, 2, 65536), dtype=np.uint32)
    v[0, 0] = 7
    v[0, 1, 65530:] = 2
    for x in (0, 1000, 40000, 65528):
        v[0, 1, x] = 3
    want = _round_trip(eng, v)
    assert want["x0"].tolist() == [0, 0, 1000, 40000, 65528, 65530] and want["x1"].tolist() == [65535, 0, 1000, 40000, 65528, 65535]
    # X = 65537: the error code, and nothing written
    wide = torch.zeros((1, 1, 65537), dtype=torch.int32, device="cuda")
    wide[0, 0, 5:9] = 1
    sentinel = 0x0123456789ABCDEF
    row_start = torch.full((2,), sentinel, dtype=torch.int64, device="cuda")
    n_runs = C.c_uint64(77)
    rc = eng.lib.dlv_cc_runs_count_dev(eng.ctx, C.c_void_p(wide.data_ptr()), 1, 1, 65537, C.c_void_p(row_start.data_ptr()), C.byref(n_runs))
    assert rc == DLV_EUNSUP and n_runs.value == 77
    x0 = torch.full((4,), 0x5A5A, dtype=torch.int16, device="cuda")
    x1, label = x0.clone(), torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc = eng.lib.dlv_cc_runs_emit_dev(eng.ctx, C.c_void_p(wide.data_ptr()), 1, 1, 65537, C.c_void_p(row_start.data_ptr()), 1,
                                      C.c_void_p(x0.data_ptr()), C.c_void_p(x1.data_ptr()), C.c_void_p(label.data_ptr()))
    assert rc == DLV_EUNSUP
    before = wide.clone()
    rc = eng.lib.dlv_cc_runs_decode_dev(eng.ctx, C.c_void_p(row_start.data_ptr()), 1, 65537, C.c_void_p(x0.data_ptr()),
                                        C.c_void_p(x1.data_ptr()), C.c_void_p(label.data_ptr()), 1, C.c_void_p(wide.data_ptr()))
    assert rc == DLV_EUNSUP
    eng.sync()
    assert (row_start.cpu().numpy() == sentinel).all() and (x0.cpu().numpy() == 0x5A5A).all() and (x1.cpu().numpy() == 0x5A5A).all()
    assert (label.cpu().numpy() == 0x5A5A5A5A).all() and torch.equal(wide, before)
    with pytest.raises(Exception) as exc:
        eng.cc_runs_encode(wide)
    assert getattr(exc.value, "code", None) == DLV_EUNSUP


# ---- 3. many rows, few voxels ------------------------------------------------------------------------------------------------
def test_more_rows_than_workgroups_and_the_degenerate_volumes(eng):
    """(40, 300, 37): 12 000 rows for the 8192 workgroups (RUNS_MAX_WG) of a launch - rows are walked grid-stride - and more scan
    groups of 1024 rows than one; a volume without a label (R = 0) and a volume of one label"""
    rng = np.random.default_rng(5)
    v = np.zeros((40, 300, 37), dtype=np.uint32)
    at = rng.random(v.shape) < 0.01
    v[at] = rng.integers(1, 500, size=int(at.sum()))
    pair = np.zeros_like(at)
    pair[:, :, 1:] = at[:, :, :-1] & (rng.random((40, 300, 36)) < 0.3)
    v[pair] = np.roll(v, 1, axis=2)[pair]
    assert v.shape[0] * v.shape[1] == 12000 > MAX_WORKGROUPS
    want = _round_trip(eng, v)
    per_row = np.diff(want["row_start"].astype(np.int64))
    assert (per_row == 0).sum() > 6000 and per_row.max() <= 5 and ((want["x1"] - want["x0"]) == 1).sum() > 100
    zeros = np.zeros((3, 7, 37), dtype=np.uint32)
    runs0 = _round_trip(eng, zeros)
    assert len(runs0["label"]) == 0 and not runs0["row_start"].any()
    one = np.full((3, 7, 37), 5, dtype=np.uint32)
    runs1 = _round_trip(eng, one)
    assert len(runs1["label"]) == 21 and (runs1["x0"] == 0).all() and (runs1["x1"] == 36).all()


def test_more_scan_groups_than_threads_of_the_one_block_step(eng):
    """(1030, 1024, 5): 1 054 720 rows are 1030 scan groups of 1024 rows for the 1024 threads of the scan's one-block step, so a
    thread owns two groups (thread 514 the last two, thread 515 and above none) - with the 64-bit row_start as the output.  X = 5
    keeps the volume small and puts the rows at every alignment."""
    rng = np.random.default_rng(11)
    shape = (1030, 1024, 5)
    v = (rng.integers(1, 4, size=shape, dtype=np.uint32) * (rng.random(shape) < 0.45)).astype(np.uint32)
    rows = shape[0] * shape[1]
    groups = -(-rows // 1024)
    assert groups == 1030 > 1024 and -(-groups // 1024) == 2 and groups % 2 == 0 and groups // 2 == 515
    assert 0.44 < (v != 0).mean() < 0.46 and set(np.unique(v).tolist()) == {0, 1, 2, 3}
    want = _round_trip(eng, v)
    per_row = np.diff(want["row_start"].astype(np.int64))
    assert want["row_start"].dtype == np.uint64 and len(per_row) == rows
    assert per_row.reshape(groups, 1024).sum(axis=1).min() > 1000  # every group adds to the groups behind it


# ---- 4. more than 2^16 runs and labels ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def specks(eng):
    """the (64, 96, 144) mask of test_more_than_2_to_16_labels_down_to_a_uint16_file, labelled on the device"""
    rng = np.random.default_rng(6)
    shape = (64, 96, 144)
    mask = np.zeros(shape, dtype=np.uint8)
    mask[::2, ::2, ::3] = 1
    mask[::2, ::2, 1::3] = rng.integers(0, 2, size=(32, 48, 48), dtype=np.uint8)  # singles or x-pairs
    import torch

    dev, n = eng.ccl26(torch.from_numpy(mask).cuda())
    labels = _host(dev).copy()
    assert n == 32 * 48 * 48 and n > 65536
    mask.setflags(write=False)
    labels.setflags(write=False)
    return mask, labels, n


def test_more_than_2_to_16_runs_and_labels(eng, specks):
    import torch

    _, labels, n = specks
    want = lr.encode_runs(labels)
    assert len(want["label"]) == n > 65536 and int(want["label"].max()) == n
    _assert_runs_equal(eng.cc_runs_encode(_dev(labels)), want)
    out = torch.empty(labels.shape, dtype=torch.int32, device="cuda")
    out.view(torch.uint8).fill_(0xAB)
    assert eng.cc_runs_decode(want, out=out) is out
    np.testing.assert_array_equal(_host(out), labels)  # every voxel written, zeros included
    part = eng.cc_runs_decode(want, 5, 23)
    assert tuple(part.shape) == (18, 96, 144)
    np.testing.assert_array_equal(_host(part), labels[5:23])


# ---- 5. the cells a split leaves touch ---------------------------------------------------------------------------------------
def test_split_cells_whose_runs_touch(eng):
    import torch

    mask = np.zeros((20, 20, 24), dtype=np.uint8)
    mask[2:10, 2:10, 2:10] = 1
    mask[8:16, 8:16, 10:18] = 1  # two cubes that touch in a 2 x 2 patch of the face x = 9 | 10
    dev, n = eng.ccl26(torch.from_numpy(mask).cuda())
    assert n == 1
    K, _, n_split = eng.cc_split(dev, n, 2)
    labels = _host(dev).copy()
    assert (K, n_split) == (2, 1)
    touching = (labels[:, :, 1:] != labels[:, :, :-1]) & (labels[:, :, 1:] != 0) & (labels[:, :, :-1] != 0)
    assert touching.sum() >= 4  # runs of different labels without a gap
    want = lr.encode_runs(labels)
    _assert_runs_equal(eng.cc_runs_encode(dev), want)
    np.testing.assert_array_equal(_host(eng.cc_runs_decode(want)), labels)


# ---- 6. count_blobs ----------------------------------------------------------------------------------------------------------
def _settings(path_in, post, **mi355x):
    s = {"postprocessing": {"output_location": post + "/"}, "blob_detection": {"input_location": path_in}}
    if mi355x:
        s["mi355x"] = mi355x
    return s


def _read(post, name):
    with open(os.path.join(post, name), "rb") as fh:
        return fh.read()


def _stats(post):
    return pickle.loads(_read(post, "brain-stats.pickle"))


def _assert_same_stats(a, b):
    assert set(a) == set(b)
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert a[key].dtype == b[key].dtype, key
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        else:
            assert a[key] == b[key], key


@pytest.fixture(scope="module")
def on_disk(tmp_path_factory, specks):
    """the mask of case 4 as a brain on disk with a raw volume beside it -> (path_in, shape)"""
    mask = specks[0]
    root = tmp_path_factory.mktemp("runs_brain")
    d = root / "in" / "brain"
    os.makedirs(d / "binary_segmentations")
    os.makedirs(d / "masked_niftis")
    np.save(str(d / "binary_segmentations" / "binaries.npy"), mask)
    raw = np.random.default_rng(8).integers(1, 4000, size=mask.shape, dtype=np.uint16)
    np.save(str(d / "masked_niftis" / "raw.npy"), raw)
    return str(root / "in"), mask.shape


def _count(eng, on_disk, post, *size, **kw):
    from delivr_cfos_amd.count_blobs import count_blobs

    path_in, shape = on_disk
    defer = kw.pop("defer_write", False)
    return count_blobs(_settings(path_in, post, **kw), path_in, 0, "brain", (1, 1) + shape, *size, engine=eng, defer_write=defer)


def _refuse(*a, **k):
    raise AssertionError("must not be called")


def test_count_blobs_dense_and_runs_folders(eng, tmp_path, on_disk, specks, monkeypatch):
    from delivr_cfos_amd.count_blobs import count_blobs, load_cached_brain

    _, labels, n = specks
    shape = on_disk[1]
    dense, runs = str(tmp_path / "dense"), str(tmp_path / "runs")
    assert _count(eng, on_disk, dense) == n
    assert "runs_encode_s" not in count_blobs.last_timings
    assert sorted(os.listdir(dense)) == sorted([f"brain-{n}-cc3d.npy", "brain-stats.pickle", f"{shape}_brain.csv"])
    np.testing.assert_array_equal(np.load(os.path.join(dense, f"brain-{n}-cc3d.npy")), labels)
    # the run file in place of the dense one
    assert _count(eng, on_disk, runs, label_file="runs") == n
    assert count_blobs.last_timings["runs_encode_s"] > 0
    assert sorted(os.listdir(runs)) == sorted([f"brain-{n}-cc3d.runs", "brain-stats.pickle", f"{shape}_brain.csv"])
    assert load_cached_brain(_settings(on_disk[0], runs), "brain") is False
    path = os.path.join(runs, f"brain-{n}-cc3d.runs")
    np.testing.assert_array_equal(lr.load_labels(path), labels)
    _assert_runs_equal(lr.load_runs(path), lr.encode_runs(labels))
    _assert_same_stats(_stats(runs), _stats(dense))
    assert _read(runs, f"{shape}_brain.csv") == _read(dense, f"{shape}_brain.csv")
    # again: the run file is the cache, and with a complete pickle nothing is labelled, decoded or uploaded
    with monkeypatch.context() as m:
        m.setattr(eng, "ccl26", _refuse)
        m.setattr(eng, "cc_runs_decode", _refuse)
        assert _count(eng, on_disk, runs, label_file="runs") == n
    # more statistics and no pickle: measured on the labels decoded from the run file (no labelling)
    os.remove(os.path.join(runs, "brain-stats.pickle"))
    with monkeypatch.context() as m:
        m.setattr(eng, "ccl26", _refuse)
        assert _count(eng, on_disk, runs, label_file="runs", shape_stats=True, intensity_stats=True) == n
    assert _count(eng, on_disk, dense, shape_stats=True, intensity_stats=True) == n  # (the dense cache, its pickle completed)
    stats = _stats(runs)
    assert "shape_axes" in stats and "intensity_mean" in stats
    _assert_same_stats(stats, _stats(dense))
    for folder in ("cell_shape", "cell_intensity"):
        assert _read(os.path.join(runs, folder), "brain.csv") == _read(os.path.join(dense, folder), "brain.csv")
    assert not [f for f in os.listdir(runs) if ".npy" in f or f.endswith(".partial")]
    # a file whose header disagrees with its name is refused
    os.replace(path, os.path.join(runs, f"brain-{n - 1}-cc3d.runs"))
    with pytest.raises(ValueError, match="cc3d.runs"):
        _count(eng, on_disk, runs, label_file="runs")


def test_count_blobs_runs_of_the_split_and_filtered_labels(eng, tmp_path, on_disk):
    dense, runs = str(tmp_path / "dense"), str(tmp_path / "runs")
    keys = dict(size_filter=True, split_fused=1)
    k = _count(eng, on_disk, dense, 2, -1, **keys)
    assert 0 < k < 65536
    assert _count(eng, on_disk, runs, 2, -1, label_file="runs", **keys) == k
    filtered = np.load(os.path.join(dense, f"brain-{k}-cc3d.npy"))
    assert filtered.dtype == np.uint16
    got = lr.load_labels(os.path.join(runs, f"brain-{k}-cc3d.runs"))
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, filtered)
    _assert_same_stats(_stats(runs), _stats(dense))


def test_the_default_ignores_a_run_file(eng, tmp_path, on_disk, specks):
    _, labels, n = specks
    post = str(tmp_path / "post")
    os.makedirs(post)
    lr.save_runs(os.path.join(post, f"brain-{n}-cc3d.runs"), lr.encode_runs(np.ones_like(labels)), n)  # (not this brain's labels)
    calls = []
    real = eng.ccl26
    eng.ccl26 = lambda mask: calls.append(1) or real(mask)
    try:
        assert _count(eng, on_disk, post) == n
    finally:
        del eng.ccl26
    assert calls == [1]  # labelled afresh
    np.testing.assert_array_equal(np.load(os.path.join(post, f"brain-{n}-cc3d.npy")), labels)


def test_a_deferred_run_file_is_complete_after_wait_deferred(eng, tmp_path, on_disk, specks, monkeypatch):
    from delivr_cfos_amd import hostio

    _, labels, n = specks
    post = str(tmp_path / "post")
    gate, real = threading.Event(), lr.save_runs

    def gated(path, runs, n_labels=None):
        assert gate.wait(60)
        real(path, runs, n_labels)

    monkeypatch.setattr(lr, "save_runs", gated)
    try:
        assert _count(eng, on_disk, post, label_file="runs", defer_write=True) == n
        assert not [f for f in os.listdir(post) if "cc3d" in f]  # statistics and CSV are there, the label file is still to come
        assert os.path.isfile(os.path.join(post, "brain-stats.pickle"))
    finally:
        gate.set()
    hostio.wait_deferred(eng)
    assert [f for f in os.listdir(post) if "cc3d" in f] == [f"brain-{n}-cc3d.runs"]
    np.testing.assert_array_equal(lr.load_labels(os.path.join(post, f"brain-{n}-cc3d.runs")), labels)


def test_decoded_labels_above_the_budget_are_refused(eng, tmp_path, on_disk, specks):
    _, labels, n = specks
    post = str(tmp_path / "post")
    os.makedirs(post)
    lr.save_runs(os.path.join(post, f"brain-{n}-cc3d.runs"), lr.encode_runs(labels), n)
    with pytest.raises(MemoryError, match=r"label_file'\] = \"runs\" needs the cached labels in HBM"):
        _count(eng, on_disk, post, label_file="runs", hbm_budget_gb=1e-4)
    assert os.listdir(post) == [f"brain-{n}-cc3d.runs"]
    fresh = str(tmp_path / "fresh")
    os.makedirs(fresh)
    with pytest.raises(MemoryError, match="slab-streamed labelling does not write run-length labels"):
        _count(eng, on_disk, fresh, label_file="runs", hbm_budget_gb=1e-4)
    assert os.listdir(fresh) == []
