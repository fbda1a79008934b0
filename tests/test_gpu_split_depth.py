"""Fused cells split by their Euclidean depth cores on the device (dlv_cc_split_depth_dev / HipEngine.cc_split_depth;
settings["mi355x"]["split_radius"] / ["split_fraction"] in count_blobs).

The reference of every case is tests/helpers/split_depth_reference.py: scipy's exact distance map per label, the threshold in Python
integers, and the labelling, growth and numbering of tests/helpers/split_reference.py (pinned on the host by
tests/test_split_depth_cpu.py).  Integer work only: every comparison is exact equality of the whole label volume, K, the number of
split labels and the parent table.  What a case is there for - which labels split - is asserted on the reference before the device
is asked.  The volumes span two tiles of 8 x 8 x 64 and a remainder on every axis."""
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


sd = _helper("split_depth_reference")
ref = sd.split


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def _dev(labels):
    import torch

    return torch.from_numpy(np.ascontiguousarray(labels).view(np.int32).copy()).cuda()


def _run(eng, dev, n, spacing, core_d2=0, fraction=0, min_core=1):
    K, parent, n_split = eng.cc_split_depth(dev, n, spacing, core_d2, fraction, min_core)
    return {"out": dev.cpu().numpy().view(np.uint32), "K": K, "parent": parent, "n_split": n_split}


def _assert_same(got, want):
    assert (got["K"], got["n_split"]) == (want["K"], want["n_split"])
    assert got["parent"].dtype == np.uint32 and got["parent"].shape == (want["K"] + 1,)
    np.testing.assert_array_equal(got["parent"], want["parent"])
    np.testing.assert_array_equal(got["out"], want["out"])


def _check(eng, L, n, spacing, core_d2=0, fraction=0, min_core=1, expect=None):
    """expect: (K, n_split) of the reference, asserted before the device runs"""
    want = sd.split_depth_reference(L, n, spacing, core_d2, fraction, min_core)
    if expect is not None:
        assert (want["K"], want["n_split"]) == expect
    got = _run(eng, _dev(L), n, spacing, core_d2, fraction, min_core)
    _assert_same(got, want)
    # the consequences of the definition, directly
    assert ((got["out"] != 0) == (L != 0)).all() and got["K"] >= n
    if want["n_split"] == 0:
        np.testing.assert_array_equal(got["out"], L)
    return want


def _pair(mask, a, b, radius=5):
    mask |= ref.ball(mask.shape, a, radius) | ref.ball(mask.shape, b, radius)


# ---- 1. the flat pair the erosion split cannot do ---------------------------------------------------------------------------
def test_the_disc_pair_splits_by_depth_and_not_by_erosion(eng):
    """two discs of radius 5, two planes thick, one shared voxel per plane; voxels of 1.62 x 1.62 x 6.0 um"""
    mask = np.zeros((6, 24, 40), dtype=bool)
    yy, xx = np.ogrid[:24, :40]
    for cx in (14, 24):
        mask[2:4] |= ((yy - 12) ** 2 + (xx - cx) ** 2 <= 25)[None]
    L, n = ref.label26(mask)
    assert n == 1
    dev = _dev(L)
    K, parent, n_split = eng.cc_split(dev, n, 1)
    assert (K, n_split, parent.tolist()) == (1, 0, [0, 1])
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), L)
    for radius in (20, 30, 35):
        want = _check(eng, L, n, (37, 10, 10), radius * radius, expect=(2, 1))
        assert np.bincount(want["out"].ravel())[1:].tolist() == [162, 160]


# ---- 2. fused pairs across tile boundaries ----------------------------------------------------------------------------------
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


# (the neck of a pair holds D2 = 16 at spacing 1, the middle of a ball 26: below the neck one core, above the middle none; a
# spacing above 1 along an axis thins the necks of the pairs along the other axes only)
@pytest.mark.parametrize("spacing, core_d2, expect", [((1, 1, 1), 9, (3, 0)), ((1, 1, 1), 20, (6, 3)), ((1, 1, 1), 30, (3, 0)),
                                                      ((3, 1, 1), 16, (4, 1)), ((3, 1, 1), 20, (6, 3)),
                                                      ((2, 3, 1), 16, (4, 1)), ((2, 3, 1), 25, (5, 2))])
def test_fused_pairs_whose_necks_and_cores_straddle_tile_boundaries(eng, pairs, spacing, core_d2, expect):
    L, n = pairs
    _check(eng, L, n, spacing, core_d2, expect=expect)


@pytest.mark.parametrize("fraction, expect", [(50, (3, 0)), (90, (6, 3))])
def test_fused_pairs_by_a_fraction_of_their_own_radius(eng, pairs, fraction, expect):
    L, n = pairs
    _check(eng, L, n, (1, 1, 1), 0, fraction, expect=expect)


# ---- 3. mixed sizes -----------------------------------------------------------------------------------------------------------
def test_an_absolute_radius_a_fraction_and_both_on_cells_of_two_sizes(eng):
    """a pair of balls of radius 7, centres 10 apart (m = 50), and a pair of radius 4, centres 6 apart (m = 17)"""
    mask = np.zeros((20, 21, 90), dtype=bool)
    _pair(mask, (9, 10, 20), (9, 10, 30), 7)
    _pair(mask, (9, 10, 60), (9, 10, 66), 4)
    L, n = ref.label26(mask)
    assert n == 2
    d2 = sd.depth.depth_map(L, n)
    assert sd.depth.depth_rows(L, n, d2)["depth_max_sq"].tolist() == [0, 50, 17]
    # an absolute radius between the two: the small pair has no core at all, the large one two
    want = _check(eng, L, n, (1, 1, 1), 30, expect=(3, 1))
    assert want["parent"].tolist() == [0, 1, 1, 2]
    # a fraction: both
    assert sd.thresholds(L, n, d2, 0, 85).tolist() == [1, 37, 13]
    want = _check(eng, L, n, (1, 1, 1), 0, 85, expect=(4, 2))
    assert want["parent"].tolist() == [0, 1, 1, 2, 2]
    # both keys: per label the larger threshold - the fraction's in the large pair (20 alone leaves it one core), the radius' in
    # the small one (13 alone splits it)
    assert sd.thresholds(L, n, d2, 20, 85).tolist() == [20, 37, 20]
    assert sd.split_depth_reference(L, n, (1, 1, 1), 20, 0)["K"] == 2
    want = _check(eng, L, n, (1, 1, 1), 20, 85, expect=(3, 1))
    assert want["parent"].tolist() == [0, 1, 1, 2]


# ---- 4. min_core, no core -----------------------------------------------------------------------------------------------------
def test_a_second_core_below_min_core_does_not_split(eng):
    mask = np.zeros((14, 14, 80), dtype=bool)
    mask |= ref.ball(mask.shape, (6, 6, 58), 5) | ref.ball(mask.shape, (6, 6, 65), 3)  # the neck at the tile boundary x = 64
    L, n = ref.label26(mask)
    assert n == 1
    cores = sd.cores(L, n, (1, 1, 1), 9, 0)
    assert np.bincount(ref.label26(cores)[0].ravel())[1:].tolist() == [59, 2]  # the voxels at depth 3 and more of either ball
    _check(eng, L, n, (1, 1, 1), 9, expect=(2, 1))
    _check(eng, L, n, (1, 1, 1), 9, min_core=2, expect=(2, 1))
    _check(eng, L, n, (1, 1, 1), 9, min_core=3, expect=(1, 0))


def test_a_label_thinner_than_the_radius_has_no_core_and_stays_whole(eng):
    L = np.zeros((12, 20, 80), dtype=np.uint32)
    L[2:5, 2:18, 50:78] = 1  # a plate of three planes: m = 4 at spacing 1, 16 with planes 2 apart
    L[6:11, 3:8, 3:8] = L[6:11, 3:8, 9:14] = 2  # a pair of cubes of five voxels a side (m = 9) ...
    L[8, 5, 8] = 2  # ... fused by one voxel
    n = 2
    want = _check(eng, L, n, (1, 1, 1), 5, expect=(3, 1))
    assert want["parent"].tolist() == [0, 1, 2, 2]  # the plate has no core: it keeps its voxels and comes first
    np.testing.assert_array_equal(want["out"] == 1, L == 1)
    _check(eng, L, n, (1, 1, 1), 10, expect=(2, 0))  # nobody has a core
    _check(eng, L, n, (2, 1, 1), 16, expect=(2, 0))  # the plate has one now (m = 16), the cubes none (m = 9)


# ---- 5. cells cut by every face of the volume ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def faces():
    """19 x 21 x 149: a pair of balls of radius 5 cut by each of the six faces, their centres 4 voxels inside it - the outside of
    the volume is background, so the centres lie at depth 5 (m = 25) and the necks are cut in half"""
    Z, Y, X = 19, 21, 149
    mask = np.zeros((Z, Y, X), dtype=bool)
    _pair(mask, (4, 10, 40), (4, 10, 48))
    _pair(mask, (14, 10, 70), (14, 10, 78))
    _pair(mask, (9, 4, 100), (9, 4, 108))
    _pair(mask, (9, 16, 120), (9, 16, 128))
    _pair(mask, (10, 6, 4), (10, 14, 4))
    _pair(mask, (8, 6, 144), (8, 14, 144))
    L, n = ref.label26(mask)
    assert n == 6
    L.setflags(write=False)
    return L, n


@pytest.mark.parametrize("spacing, core_d2, fraction, expect", [((1, 1, 1), 25, 0, (12, 6)), ((1, 1, 1), 26, 0, (6, 0)),
                                                                ((2, 1, 1), 26, 0, (8, 2)), ((1, 1, 1), 0, 90, (12, 6))])
def test_cells_cut_by_every_face_of_the_volume(eng, faces, spacing, core_d2, fraction, expect):
    L, n = faces
    d2 = sd.depth.depth_map(L, n, (1, 1, 1))
    assert sd.depth.depth_rows(L, n, d2)["depth_max_sq"].tolist() == [0] + [25] * 6  # (in the open a ball of radius 5 has 26)
    _check(eng, L, n, spacing, core_d2, fraction, expect=expect)


# ---- 6. a long row ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_row():
    """4 x 9 x 530: rows of more than one sweep of 512 voxels of the x pass, X no multiple of 4 (every second row starts 8 bytes
    past a 16-byte boundary); two blocks fused by a bar along x that runs across x = 512"""
    L = np.zeros((4, 9, 530), dtype=np.uint32)
    L[:, 1:8, 490:510] = 1
    L[:, 1:8, 515:530] = 1
    L[1, 4, 505:520] = 1
    L[2, 2, 3:9] = 1
    L, n = ref.label26(L)
    assert n == 2
    L.setflags(write=False)
    return L, n


def test_a_row_longer_than_a_sweep_of_the_x_pass(eng, long_row):
    L, n = long_row
    want = _check(eng, L, n, (1, 1, 1), 4, expect=(3, 1))
    assert want["out"][1, 4, 505] != want["out"][1, 4, 519]
    _check(eng, L, n, (1, 1, 1), 5, expect=(2, 0))
    _check(eng, L, n, (1, 1, 1), 0, 99, expect=(3, 1))


def test_labels_4_bytes_past_a_16_byte_boundary(eng, long_row):
    """the scalar path of the threshold kernel on every quad"""
    import torch

    L, n = long_row
    host = np.full(L.size + 2, 0x7FFFFFF0, dtype=np.int32)  # guards
    host[1:-1] = L.view(np.int32).ravel()
    buf = torch.from_numpy(host).cuda()
    view = buf[1:-1].view(L.shape)
    assert view.data_ptr() % 16 == 4
    want = sd.split_depth_reference(L, n, (1, 1, 1), 4, 0)
    _assert_same(_run(eng, view, n, (1, 1, 1), 4), want)
    got = buf.cpu().numpy()
    assert got[0] == host[0] and got[-1] == host[-1]


# ---- 7. a dense random mask ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    rng = np.random.default_rng(0)
    L, n = ref.label26(rng.random((24, 40, 96)) < 0.62)
    want = sd.split_depth_reference(L, n, (2, 1, 1), 3, 0)
    assert want["max_cores"] >= 500  # one component with many cores
    L.setflags(write=False)
    return L, n, want


def test_a_dense_random_mask_with_many_cores_in_one_component(eng, dense):
    L, n, want = dense
    got = _run(eng, _dev(L), n, (2, 1, 1), 3)
    _assert_same(got, want)
    assert ((got["out"] != 0) == (L != 0)).all() and got["K"] >= n
    labels, first = np.unique(got["out"].ravel(), return_index=True)  # the new labels follow the raster order of their first voxels
    assert labels.tolist() == list(range(got["K"] + 1)) and (np.diff(first[1:]) > 0).all()


def test_two_runs_give_identical_bytes(eng, dense):
    L, n, _ = dense
    a, b = _run(eng, _dev(L), n, (2, 1, 1), 3), _run(eng, _dev(L), n, (2, 1, 1), 3)
    assert a["out"].tobytes() == b["out"].tobytes() and a["parent"].tobytes() == b["parent"].tobytes()
    assert (a["K"], a["n_split"]) == (b["K"], b["n_split"])


def test_the_engine_comes_again_with_a_larger_parent_table(eng, dense):
    """the first table has 2 n + 2 rows; the dense component splits into more pieces than that"""
    L, n, want = dense
    assert want["K"] + 1 > 2 * n + 2
    _check(eng, L, n, (1, 1, 1), 2)


# ---- 8. refused arguments -----------------------------------------------------------------------------------------------------
def test_every_error_path_returns_its_code_with_a_message_and_leaves_the_labels(eng, pairs):
    import torch
    from delivr_cfos_amd import _lib

    L, n = pairs
    dev = _dev(L)
    Z, Y, X = L.shape
    wa, wb = torch.full_like(dev, 0x5A5A5A5A), torch.full_like(dev, 0x5A5A5A5A)
    big = torch.empty(2 * L.size + 8, dtype=torch.int32, device="cuda")
    parent = torch.zeros(16, dtype=torch.int32, device="cuda")
    k, s = C.c_uint64(77), C.c_uint64(77)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    lp, ap, bp, pp = p(dev), p(wa), p(wb), p(parent)
    ok = (lp, Z, Y, X, n, 1, 1, 1, 20, 0, 1, ap, bp, C.byref(k), C.byref(s), pp, 16)
    names = ("labels", "Z", "Y", "X", "n", "wz", "wy", "wx", "core_d2", "pct", "min_core", "a", "b", "k", "s", "parent", "cap")

    def with_(**kw):
        assert set(kw) <= set(names)
        return tuple(kw.get(name, v) for name, v in zip(names, ok))

    def refused(args, code):
        assert eng.lib.dlv_cc_split_depth_dev(eng.ctx, *args) == code, args[1:11]
        message = eng.lib.dlv_last_error(eng.ctx).decode()
        assert message.startswith("cc_split_depth:")
        return message

    # before any launch
    for args in [with_(labels=None), with_(a=None), with_(b=None), with_(k=None), with_(s=None), with_(parent=None),
                 with_(Z=0), with_(Y=0), with_(X=-1), with_(wz=0), with_(wy=65), with_(wx=-1), with_(pct=-1), with_(pct=100),
                 with_(core_d2=0, pct=0), with_(min_core=0), with_(min_core=-5),
                 with_(labels=p(dev, 2)), with_(a=p(wa, 1)), with_(b=p(wb, 2)), with_(parent=p(parent, 2)),
                 with_(a=lp), with_(b=lp), with_(b=ap), with_(a=p(big), b=p(big, 4 * L.size - 4)),
                 with_(n=2**32 - 1)]:
        refused(args, _lib.DLV_EINVAL)
    # the reach rule, from the formula alone: w * ceil((dim + 1) / 2) >= 65536 with w = 64 first at dim = 2046
    assert 64 * ((2046 + 2) // 2) == 65536 and 64 * ((2045 + 2) // 2) < 65536
    for axis, dims in (("z", {"Z": 2046, "Y": 1, "X": 1, "wz": 64}), ("y", {"Z": 1, "Y": 2046, "X": 1, "wy": 64}),
                       ("x", {"Z": 1, "Y": 1, "X": 2046, "wx": 64})):
        assert f"axis {axis}" in refused(with_(**dims), _lib.DLV_EUNSUP)
    assert "2^32" in refused(with_(Z=2048, Y=2048, X=1025), _lib.DLV_EUNSUP)  # ... and a volume above 2^32 voxels
    assert (k.value, s.value) == (77, 77)
    for t in (wa, wb):  # nothing was launched
        assert bool((t == 0x5A5A5A5A).all())
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), L)
    # after the seed pass: a label above n in the volume; after the numbering: a parent table that is too small
    for args in [with_(n=2), with_(cap=0), with_(cap=6)]:  # K = 6 pieces need 7 rows
        refused(args, _lib.DLV_EINVAL)
    assert k.value == 6  # the capacity error reports K, so that the caller can come again
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), L)  # nothing was rewritten
    assert eng.lib.dlv_cc_split_depth_dev(eng.ctx, *with_(cap=7)) == 0
    want = sd.split_depth_reference(L, n, (1, 1, 1), 20, 0)
    assert (k.value, s.value) == (want["K"], want["n_split"])
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), want["out"])
    np.testing.assert_array_equal(parent.cpu().numpy().view(np.uint32)[:7], want["parent"])
    # one voxel short of the reach rule runs
    line = torch.ones((1, 1, 2045), dtype=torch.int32, device="cuda")
    K, par, n_split = eng.cc_split_depth(line, 1, (1, 1, 64), 64 * 64)
    assert (K, n_split, par.tolist()) == (1, 0, [0, 1]) and bool((line == 1).all())
    # the engine
    sp = (1, 1, 1)
    for args in ((dev.cpu(), n, sp, 20), (L, n, sp, 20), (dev.to(torch.int64), n, sp, 20), (dev.reshape(-1), n, sp, 20),
                 (dev.transpose(1, 2), n, sp, 20), (dev[:0], n, sp, 20), (dev, -1, sp, 20), (dev, n, (1, 1), 20), (dev, n, (0, 1, 1), 20),
                 (dev, n, (1, 1.0, 1), 20), (dev, n, (1, 65, 1), 20), (dev, n, 3, 20), (dev, n, sp), (dev, n, sp, 0, 0), (dev, n, sp, -1),
                 (dev, n, sp, 2**32), (dev, n, sp, 2.0), (dev, n, sp, True), (dev, n, sp, 0, 100), (dev, n, sp, 0, -1), (dev, n, sp, 0, 50.0),
                 (dev, n, sp, 0, True), (dev, n, sp, 20, 0, 0), (dev, n, sp, 20, 0, True)):
        with pytest.raises(ValueError, match="cc_split_depth"):
            eng.cc_split_depth(*args)


# ---- 9. count_blobs end to end ------------------------------------------------------------------------------------------------
STD_KEYS = {"voxel_counts", "bounding_boxes", "centroids"}
NEW_KEYS = {"split_parent", "split_siblings", "split_core_d2", "split_fraction", "split_spacing"}


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


SPACING = (2, 1, 1)
KEYS = {"split_radius": 4.2, "split_fraction": 60, "depth_spacing": list(SPACING)}  # core_d2 = ceil(17.64) = 18
CORE_D2, FRACTION = 18, 60


@pytest.fixture(scope="module")
def brain():
    """24 x 40 x 70: specks, and two fused pairs of balls that split; the specks (m <= 4) are thinner than the radius"""
    rng = np.random.default_rng(11)
    mask = rng.random((24, 40, 70)) < 0.02
    _pair(mask, (8, 10, 20), (8, 10, 28))
    _pair(mask, (14, 28, 40), (14, 28, 48))
    mask = mask.astype(np.uint8)
    L, n = ref.label26(mask)
    want = sd.split_depth_reference(L, n, SPACING, CORE_D2, FRACTION)
    assert want["n_split"] == 2 and want["K"] == n + 2 and want["M"] == 4
    for a in (mask, L, want["out"], want["parent"]):
        a.setflags(write=False)
    return mask, L, n, want


def _expect_files(eng, post, shape, labels, K, parent, n_before, extra_keys=()):
    """label file, pickle and CSV of a run against the existing paths on the labels the reference gives"""
    from delivr_cfos_amd.hostlogic import cells_csv_bytes, finish_split

    on_disk = np.load(os.path.join(post, f"brain-{K}-cc3d.npy"))
    assert on_disk.dtype == (np.uint16 if K < 2**16 else np.uint32)
    np.testing.assert_array_equal(on_disk, labels)
    want_stats = eng.cc_stats(_dev(labels), K)
    stats = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(stats) == STD_KEYS | NEW_KEYS | set(extra_keys)  # (no split_depth: that is the erosion depth)
    for key in STD_KEYS:
        assert stats[key].dtype == want_stats[key].dtype
        np.testing.assert_array_equal(stats[key], want_stats[key], err_msg=key)
    for key, value in finish_split(parent, n_before).items():
        assert stats[key].dtype == np.uint32
        np.testing.assert_array_equal(stats[key], value, err_msg=key)
    assert (stats["split_core_d2"], stats["split_fraction"], stats["split_spacing"]) == (CORE_D2, FRACTION, SPACING)
    assert _read(post, f"{shape}_brain.csv") == cells_csv_bytes(want_stats, K)
    return stats


def test_count_blobs_writes_what_the_split_labels_give(eng, tmp_path, brain, capsys):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, L, n, want = brain
    path_in = _brain_on_disk(tmp_path, mask)
    stack = (1, 1) + mask.shape
    post = str(tmp_path / "post")
    K = count_blobs(_settings(path_in, post, **KEYS), path_in, 0, "brain", stack, engine=eng)
    assert K == want["K"]
    assert sorted(os.listdir(post)) == sorted([f"{mask.shape}_brain.csv", f"brain-{K}-cc3d.npy", "brain-stats.pickle"])
    stats = _expect_files(eng, post, mask.shape, want["out"], K, want["parent"], n)
    assert sorted(stats["split_siblings"].tolist())[-4:] == [2, 2, 2, 2]
    assert count_blobs.last_split == {"core_d2": CORE_D2, "fraction": FRACTION, "spacing": SPACING, "min_core": 1, "n_before": n,
                                      "n_after": K, "components_split": 2}
    assert "split_s" in count_blobs.last_timings and count_blobs.last_filter is None and count_blobs.last_depth is None
    assert (f"split of fused cells (radius 4.2: core_d2 18, fraction 60 %, spacing [2, 1, 1], min_core 1): 2 of {n} components split, "
            f"{K} cells") in capsys.readouterr().out
    # a second call finds the cache and does not split again
    before = {name: _read(post, name) for name in os.listdir(post)}
    assert count_blobs(_settings(path_in, post, **KEYS), path_in, 0, "brain", stack, engine=eng) == K
    assert count_blobs.last_split is None and "split_s" not in count_blobs.last_timings
    assert "the cached labelling is reused as it is, it is not split" in capsys.readouterr().out
    assert {name: _read(post, name) for name in os.listdir(post)} == before


def test_count_blobs_without_the_keys_writes_what_it_wrote_before(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import cells_csv_bytes

    mask, L, n, _ = brain
    path_in = _brain_on_disk(tmp_path, mask)
    stack = (1, 1) + mask.shape
    names = sorted([f"{mask.shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle"])
    posts = [str(tmp_path / name) for name in ("absent", "none")]
    for post, mi in zip(posts, ({}, {"split_radius": None, "split_fraction": None})):
        assert count_blobs(_settings(path_in, post, **mi), path_in, 0, "brain", stack, engine=eng) == n
        assert count_blobs.last_split is None and "split_s" not in count_blobs.last_timings
        assert sorted(os.listdir(post)) == names
    for name in names:
        assert _read(posts[0], name) == _read(posts[1], name), name
    # ... which is the labelling as it was, measured by the paths that were there
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
    got = count_blobs(_settings(path_in, post, size_filter=True, **KEYS), path_in, 0, "brain", (1, 1) + mask.shape, lo, hi, engine=eng)
    assert got == K
    _expect_files(eng, post, mask.shape, labels, K, parent, n)
    assert count_blobs.last_filter["n_before"] == want["K"] and count_blobs.last_filter["n_kept"] == K
    assert count_blobs.last_split["n_after"] == want["K"]


def test_count_blobs_with_depth_stats_measures_the_split_labels(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import DEPTH_KEYS, cell_depth_csv_text, finish_depth

    mask, L, n, want = brain
    path_in = _brain_on_disk(tmp_path, mask)
    post = str(tmp_path / "post")
    K = count_blobs(_settings(path_in, post, depth_stats=True, **KEYS), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng)
    stats = _expect_files(eng, post, mask.shape, want["out"], K, want["parent"], n, DEPTH_KEYS)
    d2, rows = sd.depth.depth_reference(want["out"], K, SPACING)  # the pieces bound each other: a piece is shallower than its parent
    depth_ref = finish_depth(rows, stats["voxel_counts"], mask.shape, SPACING)
    for key in DEPTH_KEYS:
        np.testing.assert_array_equal(np.asarray(stats[key]), np.asarray(depth_ref[key]), err_msg=key)
    whole = sd.depth.depth_rows(L, n, sd.depth.depth_map(L, n, SPACING))["depth_max_sq"]
    cut = np.flatnonzero(stats["split_siblings"] == 2)
    assert len(cut) == 4 and (stats["depth_max_sq"][cut] <= whole[stats["split_parent"][cut]]).all()
    depth_ref["voxel_counts"] = stats["voxel_counts"]
    assert _read(os.path.join(post, "cell_depth"), "brain.csv").decode() == cell_depth_csv_text(depth_ref, K)
    assert count_blobs.last_depth == {"n": K, "spacing": SPACING}


def test_split_fused_together_with_split_radius_is_refused_before_any_file_is_written(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask = brain[0]
    path_in = _brain_on_disk(tmp_path, mask)
    post = str(tmp_path / "post")
    with pytest.raises(ValueError, match="split_fused.*split_radius"):
        count_blobs(_settings(path_in, post, split_fused=2, **KEYS), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng)
    assert not os.path.exists(post) and count_blobs.last_split is None


def test_a_mask_above_the_budget_is_refused_before_any_file_is_written(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask = brain[0]
    path_in = _brain_on_disk(tmp_path, mask)
    post = str(tmp_path / "post")
    os.makedirs(post)
    open(os.path.join(post, "kept.txt"), "w").close()
    with pytest.raises(MemoryError, match=r"split_radius.*8 more bytes.*slab-streamed.*hbm_budget_gb"):
        count_blobs(_settings(path_in, post, hbm_budget_gb=1e-4, **KEYS), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng)
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
    settings = _settings(path_in, post, **KEYS)
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
    assert len({str(c) for c in caught}) == 1 and "split_radius" in str(caught[0]) and "torch.distributed" in str(caught[0])
    assert not os.path.exists(post)
