"""Fused cells split by their erosion cores on the device (dlv_cc_split_dev / HipEngine.cc_split; settings["mi355x"]["split_fused"]
in count_blobs).

The reference of every case is tests/helpers/split_reference.py, the numpy restatement of the definition (pinned on the host by
tests/test_split_cpu.py).  Integer work only: every comparison is exact equality of the whole label volume, K, the number of split
labels and the parent table.  The volumes span two tiles of 8 x 8 x 64 and a remainder on every axis."""
import ctypes as C
import importlib.util
import os
import pickle
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("split_reference")


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def _dev(labels):
    import torch

    return torch.from_numpy(np.ascontiguousarray(labels).view(np.int32).copy()).cuda()


def _run(eng, dev, n, depth, min_core=1):
    K, parent, n_split = eng.cc_split(dev, n, depth, min_core)
    return {"out": dev.cpu().numpy().view(np.uint32), "K": K, "parent": parent, "n_split": n_split}


def _assert_same(got, want):
    assert (got["K"], got["n_split"]) == (want["K"], want["n_split"])
    assert got["parent"].dtype == np.uint32 and got["parent"].shape == (want["K"] + 1,)
    np.testing.assert_array_equal(got["parent"], want["parent"])
    np.testing.assert_array_equal(got["out"], want["out"])


def _check(eng, L, n, depth, min_core=1):
    want = ref.split_reference(L, n, depth, min_core)
    got = _run(eng, _dev(L), n, depth, min_core)
    _assert_same(got, want)
    # the consequences of the definition, directly
    assert ((got["out"] != 0) == (L != 0)).all() and got["K"] >= n
    if want["n_split"] == 0:
        np.testing.assert_array_equal(got["out"], L)
    return want


def _pair(mask, a, b, radius=5):
    mask |= ref.ball(mask.shape, a, radius) | ref.ball(mask.shape, b, radius)


# ---- 1. fused pairs across tile boundaries --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    """27 x 27 x 149: three pairs of balls of radius 5 with centres 8 apart.  Along x: the neck at x = 64, the first core around
    z = y = 8; along y: the neck at y = 16; along z: the neck at z = 16, both cores around x = 128"""
    mask = np.zeros((27, 27, 149), dtype=bool)
    _pair(mask, (8, 8, 60), (8, 8, 68))
    _pair(mask, (13, 12, 100), (13, 20, 100))
    _pair(mask, (12, 8, 128), (20, 8, 128))
    L, n = ref.label26(mask)
    assert n == 3
    L.setflags(write=False)
    return L, n


@pytest.mark.parametrize("depth", [3, 4, 5])
def test_fused_pairs_whose_necks_and_cores_straddle_tile_boundaries(eng, pairs, depth):
    L, n = pairs
    want = _check(eng, L, n, depth)
    assert (want["K"], want["n_split"]) == ((6, 3) if depth > 3 else (3, 0))


def test_labels_4_bytes_past_a_16_byte_boundary(eng, pairs):
    import torch

    L, n = pairs
    host = np.full(L.size + 2, 0x7FFFFFF0, dtype=np.int32)  # guards
    host[1:-1] = L.view(np.int32).ravel()
    buf = torch.from_numpy(host).cuda()
    view = buf[1:-1].view(L.shape)
    assert view.data_ptr() % 16 == 4
    want = ref.split_reference(L, n, 4)
    _assert_same(_run(eng, view, n, 4), want)
    got = buf.cpu().numpy()
    assert got[0] == host[0] and got[-1] == host[-1]


# ---- 2. cells cut by every face of the volume -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def faces():
    """19 x 21 x 149: the cube pair of the definition in the corner at z = y = x = 0 and in the opposite corner, and a pair of balls
    of radius 5 cut by each of the six faces, their centres 4 voxels inside it: what the outside takes away in 4 steps ends just
    short of them"""
    Z, Y, X = 19, 21, 149
    mask = np.zeros((Z, Y, X), dtype=bool)
    mask[0:5, 0:5, 0:5] = mask[0:5, 0:5, 6:11] = True
    mask[2, 2, 5] = True
    mask[Z - 5:, Y - 5:, X - 5:] = mask[Z - 5:, Y - 5:, X - 11:X - 6] = True
    mask[Z - 3, Y - 3, X - 6] = True
    _pair(mask, (4, 10, 40), (4, 10, 48))
    _pair(mask, (14, 10, 70), (14, 10, 78))
    _pair(mask, (9, 4, 100), (9, 4, 108))
    _pair(mask, (9, 16, 120), (9, 16, 128))
    _pair(mask, (10, 6, 4), (10, 14, 4))
    _pair(mask, (8, 6, 144), (8, 14, 144))
    L, n = ref.label26(mask)
    assert n == 8
    L.setflags(write=False)
    return L, n


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_cells_cut_by_every_face_of_the_volume(eng, faces, depth):
    L, n = faces
    want = _check(eng, L, n, depth)
    assert (want["K"], want["n_split"]) == ((10, 2) if depth <= 2 else (14, 6))  # the cube pairs; at depth 4 the ball pairs
    if depth <= 2:  # the cube pairs in the two corners split: the outside counts as background
        assert want["out"][0, 0, 0] != want["out"][0, 0, 6] and want["out"][-1, -1, -1] != want["out"][-1, -1, -7]
        assert want["parent"][want["out"][0, 0, 0]] == want["parent"][want["out"][0, 0, 6]] == L[0, 0, 0]


# ---- 3. a tie ---------------------------------------------------------------------------------------------------------------
def test_the_bridge_of_a_symmetric_dumbbell_goes_to_the_smaller_core_label(eng):
    L = np.zeros((9, 11, 70), dtype=np.uint32)
    L[6:9, 7:10, 61:64] = 1
    L[6:9, 7:10, 65:68] = 1
    L[7, 8, 64] = 1  # the bridge, in the first column of the second x tile
    want = _check(eng, L, 1, 1)
    assert want["K"] == 2 and want["out"][7, 8, 64] == 1 and want["out"][7, 8, 65] == 2


# ---- 4. a long growth -------------------------------------------------------------------------------------------------------
def test_a_tail_of_more_than_100_voxels_and_a_component_that_is_done_in_two_steps(eng):
    L = np.zeros((7, 19, 140), dtype=np.uint32)
    L[0:5, 0:5, 0:5] = L[0:5, 0:5, 6:11] = 1
    L[2, 2, 5] = 1
    L[2, 2, 11:135] = 1   # the tail: along x through three tiles ...
    L[2, 2:17, 134] = 1   # ... along y through three tiles ...
    L[2, 16, 20:135] = 1  # ... and back
    L[4:7, 10:13, 61:64] = L[4:7, 10:13, 65:68] = 2
    L[5, 11, 64] = 2
    L, n = ref.label26(L)
    assert n == 2
    want = _check(eng, L, n, 1)
    assert want["steps"] > 100 and want["K"] == 4 and want["n_split"] == 2
    assert want["out"][2, 16, 20] == want["out"][0, 0, 6]  # the whole tail belongs to the cube it hangs on


# ---- 5. a dense random mask -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    rng = np.random.default_rng(0)
    L, n = ref.label26(rng.random((16, 17, 71)) < 0.62)
    want = ref.split_reference(L, n, 1)
    assert want["max_cores"] >= 50  # one component with many cores
    L.setflags(write=False)
    return L, n, want


def test_a_dense_random_mask_with_many_cores_in_one_component(eng, dense):
    L, n, want = dense
    got = _run(eng, _dev(L), n, 1)
    _assert_same(got, want)
    assert ((got["out"] != 0) == (L != 0)).all() and got["K"] >= n


def test_two_runs_give_identical_bytes(eng, dense):
    L, n, _ = dense
    a, b = _run(eng, _dev(L), n, 1), _run(eng, _dev(L), n, 1)
    assert a["out"].tobytes() == b["out"].tobytes() and a["parent"].tobytes() == b["parent"].tobytes()
    assert (a["K"], a["n_split"]) == (b["K"], b["n_split"])


# ---- 6. min_core ------------------------------------------------------------------------------------------------------------
def test_a_second_core_below_min_core_does_not_split(eng):
    L = np.zeros((9, 10, 75), dtype=np.uint32)
    L[0:5, 0:5, 59:64] = 1  # core at depth 1: 28 voxels
    L[1:4, 1:4, 65:68] = 1  # core at depth 1: 2 voxels
    L[2, 2, 64] = 1
    assert _check(eng, L, 1, 1)["K"] == 2
    assert _check(eng, L, 1, 1, min_core=2)["K"] == 2
    want = _check(eng, L, 1, 1, min_core=3)
    assert want["K"] == 1 and want["n_split"] == 0


# ---- 7. mixed components ------------------------------------------------------------------------------------------------------
def test_components_with_no_one_and_several_cores(eng):
    rng = np.random.default_rng(4)
    mask = rng.random((19, 21, 150)) < 0.01  # specks: no core
    mask[:, :, 30:80] = False
    mask |= ref.ball(mask.shape, (9, 10, 40), 4)  # one core
    _pair(mask, (9, 10, 60), (9, 10, 68))  # two
    L, n = ref.label26(mask)
    want = ref.split_reference(L, n, 4)
    assert want["M"] >= 3 and want["n_split"] >= 1 and (np.bincount(want["parent"][1:]) == 1).sum() > 10
    got = _run(eng, _dev(L), n, 4)
    _assert_same(got, want)
    # the new labels follow the raster order of their first voxels
    labels, first = np.unique(got["out"].ravel(), return_index=True)
    assert labels.tolist() == list(range(got["K"] + 1)) and (np.diff(first[1:]) > 0).all()
    # a component that is not split keeps its voxels
    pieces_of = np.bincount(got["parent"][1:], minlength=n + 1)
    assert pieces_of[1:].min() >= 1 and (pieces_of >= 2).sum() == got["n_split"]
    for j in np.flatnonzero(pieces_of[got["parent"]] == 1):
        if j:
            np.testing.assert_array_equal(got["out"] == j, L == got["parent"][j])


# ---- 8. refused arguments -----------------------------------------------------------------------------------------------------
def test_every_error_path_returns_einval_with_a_message_and_leaves_the_labels(eng, pairs):
    import torch
    from delivr_cfos_amd import _lib

    L, n = pairs
    dev = _dev(L)
    Z, Y, X = L.shape
    wa, wb = torch.empty_like(dev), torch.empty_like(dev)
    big = torch.empty(2 * L.size + 8, dtype=torch.int32, device="cuda")
    parent = torch.zeros(16, dtype=torch.int32, device="cuda")
    k, s = C.c_uint64(77), C.c_uint64(77)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    lp, ap, bp, pp = p(dev), p(wa), p(wb), p(parent)
    ok = (lp, Z, Y, X, n, 4, 1, ap, bp, C.byref(k), C.byref(s), pp, 16)

    def with_(**kw):
        names = ("labels", "Z", "Y", "X", "n", "depth", "min_core", "a", "b", "k", "s", "parent", "cap")
        return tuple(kw.get(name, v) for name, v in zip(names, ok))

    bad = [with_(labels=None), with_(a=None), with_(b=None), with_(k=None), with_(s=None), with_(parent=None),
           with_(Z=0), with_(Y=0), with_(X=-1), with_(depth=0), with_(depth=17), with_(min_core=0), with_(min_core=-5),
           with_(labels=p(dev, 2)), with_(a=p(wa, 1)), with_(b=p(wb, 2)), with_(parent=p(parent, 2)),
           with_(a=lp), with_(b=lp), with_(b=ap), with_(a=p(big), b=p(big, 4 * L.size - 4)),
           with_(Z=1, Y=8 * 65536, X=1),  # beyond the launch grid
           with_(n=2**32 - 1), with_(n=2),  # n beyond the labels; a label above n in the volume
           with_(cap=0), with_(cap=6)]  # K = 6 pieces need 7 rows
    for args in bad:
        assert eng.lib.dlv_cc_split_dev(eng.ctx, *args) == _lib.DLV_EINVAL, args[1:7]
        assert eng.lib.dlv_last_error(eng.ctx).decode().startswith("cc_split:")
    assert k.value == 6  # the capacity error reports K, so that the caller can come again
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), L)  # nothing was rewritten
    assert eng.lib.dlv_cc_split_dev(eng.ctx, *with_(cap=7)) == 0
    want = ref.split_reference(L, n, 4)
    assert (k.value, s.value) == (want["K"], want["n_split"])
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), want["out"])
    np.testing.assert_array_equal(parent.cpu().numpy().view(np.uint32)[:7], want["parent"])
    # the engine
    for args in ((dev.cpu(), n, 4), (L, n, 4), (dev.to(torch.int64), n, 4), (dev.reshape(-1), n, 4), (dev.transpose(1, 2), n, 4),
                 (dev[:0], n, 4), (dev, -1, 4), (dev, n, 0), (dev, n, 17), (dev, n, True), (dev, n, 2.0), (dev, n, 4, 0)):
        with pytest.raises(ValueError, match="cc_split"):
            eng.cc_split(*args)


def test_the_engine_comes_again_with_a_larger_parent_table(eng):
    """the first table has 2 n + 2 rows; the dense component below splits into more pieces than that"""
    L = (np.random.default_rng(1).random((9, 10, 70)) < 0.7).astype(np.uint32)
    L, n = ref.label26(L)
    want = _check(eng, L, n, 1)
    assert want["K"] + 1 > 2 * n + 2


# ---- 9. count_blobs end to end ------------------------------------------------------------------------------------------------
STD_KEYS = {"voxel_counts", "bounding_boxes", "centroids"}


def _brain_on_disk(tmp_path, mask):
    d = tmp_path / "in" / "brain"
    os.makedirs(d / "binary_segmentations")
    np.save(str(d / "binary_segmentations" / "binaries.npy"), mask)
    return str(tmp_path / "in")


def _settings(path_in, post, **mi355x):
    s = {"postprocessing": {"output_location": post + "/"}, "blob_detection": {"input_location": path_in}}
    if mi355x:
        s["mi355x"] = mi355x
    return s


def _read(post, name):
    with open(os.path.join(post, name), "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def brain():
    """24 x 40 x 70: specks, and two fused pairs of balls that split at depth 4"""
    rng = np.random.default_rng(11)
    mask = rng.random((24, 40, 70)) < 0.02
    _pair(mask, (8, 10, 20), (8, 10, 28))
    _pair(mask, (14, 28, 40), (14, 28, 48))
    mask = mask.astype(np.uint8)
    L, n = ref.label26(mask)
    want = ref.split_reference(L, n, 4)
    assert want["n_split"] == 2 and want["K"] == n + 2
    for a in (mask, L, want["out"], want["parent"]):
        a.setflags(write=False)
    return mask, L, n, want


def _expect_files(eng, post, shape, labels, K, parent, n_before, depth, extra_keys=()):
    """label file, pickle and CSV of a run against the existing paths on the labels the reference gives"""
    from delivr_cfos_amd.hostlogic import SPLIT_KEYS, cells_csv_bytes, finish_split

    on_disk = np.load(os.path.join(post, f"brain-{K}-cc3d.npy"))
    assert on_disk.dtype == (np.uint16 if K < 2**16 else np.uint32)
    np.testing.assert_array_equal(on_disk, labels)
    want_stats = eng.cc_stats(_dev(labels), K)
    stats = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(stats) == STD_KEYS | set(SPLIT_KEYS) | {"split_depth"} | set(extra_keys)
    for key in STD_KEYS:
        assert stats[key].dtype == want_stats[key].dtype
        np.testing.assert_array_equal(stats[key], want_stats[key], err_msg=key)
    for key, value in finish_split(parent, n_before).items():
        assert stats[key].dtype == np.uint32
        np.testing.assert_array_equal(stats[key], value, err_msg=key)
    assert stats["split_depth"] == depth
    assert _read(post, f"{shape}_brain.csv") == cells_csv_bytes(want_stats, K)
    return stats


def test_count_blobs_writes_what_the_split_labels_give(eng, tmp_path, brain, capsys):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, L, n, want = brain
    path_in = _brain_on_disk(tmp_path, mask)
    stack = (1, 1) + mask.shape
    post = str(tmp_path / "post")
    K = count_blobs(_settings(path_in, post, split_fused=4), path_in, 0, "brain", stack, engine=eng)
    assert K == want["K"]
    assert sorted(os.listdir(post)) == sorted([f"{mask.shape}_brain.csv", f"brain-{K}-cc3d.npy", "brain-stats.pickle"])
    stats = _expect_files(eng, post, mask.shape, want["out"], K, want["parent"], n, 4)
    assert sorted(stats["split_siblings"].tolist())[-4:] == [2, 2, 2, 2]
    assert count_blobs.last_split == {"depth": 4, "min_core": 1, "n_before": n, "n_after": K, "components_split": 2}
    assert "split_s" in count_blobs.last_timings and count_blobs.last_filter is None
    assert f"split of fused cells (depth 4, min_core 1): 2 of {n} components split, {K} cells" in capsys.readouterr().out
    # a second call finds the cache and does not split again
    before = {name: _read(post, name) for name in os.listdir(post)}
    assert count_blobs(_settings(path_in, post, split_fused=4), path_in, 0, "brain", stack, engine=eng) == K
    assert count_blobs.last_split is None and "split_s" not in count_blobs.last_timings
    assert "the cached labelling is reused as it is, it is not split" in capsys.readouterr().out
    assert {name: _read(post, name) for name in os.listdir(post)} == before


def test_count_blobs_without_the_key_writes_what_it_wrote_before(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import cells_csv_bytes

    mask, L, n, _ = brain
    path_in = _brain_on_disk(tmp_path, mask)
    stack = (1, 1) + mask.shape
    names = sorted([f"{mask.shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle"])
    posts = [str(tmp_path / name) for name in ("absent", "zero", "false")]
    for post, mi in zip(posts, ({}, {"split_fused": 0}, {"split_fused": False})):
        assert count_blobs(_settings(path_in, post, **mi), path_in, 0, "brain", stack, engine=eng) == n
        assert count_blobs.last_split is None and "split_s" not in count_blobs.last_timings
        assert sorted(os.listdir(post)) == names
    for name in names:
        assert _read(posts[0], name) == _read(posts[1], name) == _read(posts[2], name), name
    np.testing.assert_array_equal(np.load(os.path.join(posts[0], f"brain-{n}-cc3d.npy")), L)
    stats = pickle.loads(_read(posts[0], "brain-stats.pickle"))
    assert set(stats) == STD_KEYS
    want_stats = eng.cc_stats(_dev(L), n)
    for key in STD_KEYS:
        np.testing.assert_array_equal(stats[key], want_stats[key], err_msg=key)
    assert _read(posts[0], f"{mask.shape}_brain.csv") == cells_csv_bytes(want_stats, n)


def test_count_blobs_size_filter_acts_on_the_pieces(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, L, n, want = brain
    sizes = np.bincount(want["out"].ravel(), minlength=want["K"] + 1)
    whole = np.bincount(L.ravel(), minlength=n + 1)
    lo, hi = 2, 800
    split_ones = np.flatnonzero(np.bincount(want["parent"][1:], minlength=n + 1) >= 2)
    assert (whole[split_ones] > hi).all()  # unsplit, the fused cells would be removed ...
    keep = (sizes >= lo) & (sizes <= hi)
    keep[0] = False
    assert keep[np.isin(want["parent"], split_ones)].all() and not keep[1:].all()  # ... their pieces stay, specks go
    lut = np.where(keep, np.cumsum(keep), 0).astype(np.uint32)
    labels, K = lut[want["out"]], int(keep.sum())
    parent = np.concatenate([[0], want["parent"][keep]]).astype(np.uint32)
    path_in = _brain_on_disk(tmp_path, mask)
    post = str(tmp_path / "post")
    got = count_blobs(_settings(path_in, post, split_fused=4, size_filter=True), path_in, 0, "brain", (1, 1) + mask.shape, lo, hi, engine=eng)
    assert got == K
    _expect_files(eng, post, mask.shape, labels, K, parent, n, 4)
    assert count_blobs.last_filter["n_before"] == want["K"] and count_blobs.last_filter["n_kept"] == K
    assert count_blobs.last_split["n_after"] == want["K"]


def test_count_blobs_with_the_shape_statistics_as_well(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import SHAPE_KEYS, cell_shape_csv_text, finish_shape

    mask, L, n, want = brain
    path_in = _brain_on_disk(tmp_path, mask)
    post = str(tmp_path / "post")
    K = count_blobs(_settings(path_in, post, split_fused=4, shape_stats=True), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng)
    stats = _expect_files(eng, post, mask.shape, want["out"], K, want["parent"], n, 4, SHAPE_KEYS)
    shape_ref = finish_shape(eng.cc_shape(_dev(want["out"]), K), stats["voxel_counts"])
    for key in SHAPE_KEYS:
        np.testing.assert_array_equal(stats[key], shape_ref[key], err_msg=key)
    shape_ref["voxel_counts"] = stats["voxel_counts"]
    assert _read(os.path.join(post, "cell_shape"), "brain.csv").decode() == cell_shape_csv_text(shape_ref, K)
    assert count_blobs.last_shape == {"n": K}


def test_a_mask_above_the_budget_is_refused_before_any_file_is_written(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask = brain[0]
    path_in = _brain_on_disk(tmp_path, mask)
    post = str(tmp_path / "post")
    os.makedirs(post)
    open(os.path.join(post, "kept.txt"), "w").close()
    with pytest.raises(MemoryError, match=r"split_fused.*8 more bytes.*slab-streamed.*hbm_budget_gb"):
        count_blobs(_settings(path_in, post, split_fused=4, hbm_budget_gb=1e-4), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng)
    assert os.listdir(post) == ["kept.txt"] and count_blobs.last_split is None


def test_two_ranks_raise_the_same_value_error_before_any_collective(eng, tmp_path, monkeypatch, brain):
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs

    ranks = _helper("thread_ranks")
    mask = brain[0]
    path_in = _brain_on_disk(tmp_path, mask)
    post = str(tmp_path / "post")
    fake = ranks.ThreadRanks(2)
    fake.patch(monkeypatch, dist)
    settings = _settings(path_in, post, split_fused=4)
    caught = [None] * 2

    def rank_main(rank):
        fake.bind(rank)
        try:
            count_blobs(settings, path_in, 0, "brain", (1, 1) + mask.shape, engine=eng)  # (refused before the engine is used)
        except BaseException as exc:  # noqa: BLE001
            caught[rank] = exc

    ts = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not any(t.is_alive() for t in ts)  # nobody waits in a collective
    assert all(type(c) is ValueError for c in caught), caught
    assert len({str(c) for c in caught}) == 1 and "split_fused" in str(caught[0]) and "torch.distributed" in str(caught[0])
    assert not os.path.exists(post)
