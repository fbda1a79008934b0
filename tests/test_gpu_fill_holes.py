"""Exact hole filling of the cell mask on the device (dlv_fill_holes_u8_dev / HipEngine.fill_holes), the filled voxels per label
(dlv_cc_count_marked_dev / HipEngine.cc_count_marked) and settings["mi355x"]["fill_holes"] in count_blobs.

The reference of every case is scipy.ndimage.binary_fill_holes (tests/helpers/fill_reference.py, pinned on the host by
tests/test_fill_holes_cpu.py).  Integer work only: every comparison is exact equality of the whole mask after the call - the hole
voxels hold fill_value, every other byte is what it was - and of voxels_filled and holes."""
import importlib.util
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("fill_reference")


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(eng, mask, fill_value=2, voxels=None):
    """fill `mask` (bool, or uint8 as it is) on the device and compare everything with the reference -> (voxels_filled, holes)"""
    host = np.ascontiguousarray(mask, dtype=np.uint8)
    dev = _dev(host)
    got = eng.fill_holes(dev, fill_value)
    _, want_voxels, want_holes = ref.fill_reference(host)
    np.testing.assert_array_equal(dev.cpu().numpy(), ref.expected_bytes(host, fill_value))
    assert got == (want_voxels, want_holes)
    if voxels is not None:
        assert got[0] == voxels
    return got


def _tunnel():
    m = ref.three_hollow_balls()
    m[10, 11, 19:21] = False
    return m


def _face_leak():
    m = ref.cube_shell()
    m[4, 4, 7] = False
    return m


def _cup_x0():
    m = np.zeros((9, 9, 9), dtype=bool)
    m[1:7, 1:8, 0:8] = True
    m[2:6, 2:7, 0:7] = False
    return m


HAND_MADE = {  # name: (volume, voxels filled)
    "three hollow balls": (ref.three_hollow_balls, 3269),
    "a tunnel through one wall": (_tunnel, 2344),
    "a leak through a face": (_face_leak, 0),
    "a tunnel that turns over an edge": (lambda: ref.cube_shell(1), 126),
    "the same tunnel, face-connected": (lambda: ref.cube_shell(2), 0),
    "a cup open to z = 0": (lambda: ref.cup(0), 0),
    "a cup open to x = 0": (_cup_x0, 0),
    "a shell inside a shell": (ref.nested, 2679),
}


@pytest.mark.parametrize("name", list(HAND_MADE))
def test_the_hand_made_volumes(eng, name):
    make, voxels = HAND_MADE[name]
    _check(eng, make(), voxels=voxels)


@pytest.mark.parametrize("face", range(6))
def test_a_cup_against_every_face_is_open(eng, face):
    assert _check(eng, ref.cup(face)) == (0, 0)


@pytest.mark.parametrize("X", [96, 83])
def test_rows_of_whole_chunks_and_rows_with_a_remainder(eng, X):
    """X = 96: every row is six 16-byte chunks and starts on a 16-byte boundary; X = 83: a remainder, and rows at every alignment"""
    assert _check(eng, ref.three_hollow_balls(X), voxels=3269) == (3269, 3)


@pytest.mark.parametrize("shape, p, seed, voxels", [((17, 21, 37), 0.7, 3, 1300), ((17, 21, 37), 0.8, 4, 1645),
                                                     ((16, 16, 64), 0.7, 3, None), ((16, 16, 64), 0.8, 4, None)])
def test_dense_random_masks(eng, shape, p, seed, voxels):
    """hundreds of holes of one and two voxels, gaps that chain across rows and planes"""
    got = _check(eng, ref.dense_random(shape, p, seed), voxels=voxels)
    assert got[1] > 400


def test_random_hollow_balls_most_of_which_leak(eng):
    """1920 rows: two scan groups; about 3000 gaps, most of them joined to the outside through a knocked-out voxel"""
    mask = ref.random_hollow_balls()
    got = _check(eng, mask)
    assert got[0] > 1000 and ref.fill_by_gaps(mask)[3] > 2 * got[1]


def test_more_rows_than_workgroups(eng):
    """(34, 250, 35): 8500 rows for the 8192 workgroups of a launch - the rows are walked grid-stride - and nine scan groups"""
    _check(eng, ref.dense_random((34, 250, 35), 0.75, 5))


def test_more_scan_groups_than_threads_of_the_one_block_step(eng):
    """(1030, 1024, 5): 1 054 720 rows are 1030 scan groups of 1024 rows for the 1024 threads of the scan's one-block step, so a
    thread owns two groups (thread 514 the last two, thread 515 and above none) - with the row table scanned in place.  X = 5
    keeps the volume small and puts the rows at every alignment."""
    shape = (1030, 1024, 5)
    groups = -(-shape[0] * shape[1] // 1024)
    assert groups == 1030 > 1024 and -(-groups // 1024) == 2 and groups // 2 == 515
    mask = ref.dense_random(shape, 0.75, 11)
    runs = mask[:, :, 0].astype(np.int64) + (mask[:, :, 1:] & ~mask[:, :, :-1]).sum(axis=2)
    assert np.maximum(runs - 1, 0).sum() == 528289  # the gaps of its rows (a row's foreground runs - 1): what the scan adds up
    assert _check(eng, mask, voxels=342241) == (342241, 200850)


def test_checkerboards(eng):
    # (y + x) even in every plane: X / 2 gaps in every row, every one open along z: nothing is filled, and the call returns
    assert _check(eng, ref.checkerboard(planes=False)) == (0, 0)
    # (z + y + x) even: the same rows, but every inner background voxel is enclosed by its six face neighbours
    assert _check(eng, ref.checkerboard()) == (6076, 6076)
    for planes in (False, True):  # inside a solid box wall everything is filled
        mask = ref.boxed_checkerboard(planes=planes)
        dev = _dev(mask.astype(np.uint8))
        got = eng.fill_holes(dev)
        assert (dev != 0).all() and got[0] == int((~mask).sum())
        _check(eng, mask)


@pytest.mark.parametrize("shape", [(1, 1, 64), (64, 1, 1), (1, 64, 1), (3, 4, 5)])
def test_empty_full_and_flat_volumes(eng, shape):
    assert _check(eng, np.zeros(shape, dtype=bool)) == (0, 0)
    assert _check(eng, np.ones(shape, dtype=bool)) == (0, 0)
    gapped = np.ones(shape, dtype=bool)
    gapped.ravel()[1::3] = False  # in a row, a column or a pile every gap is open to the faces beside it
    got = _check(eng, gapped)
    assert got == ((0, 0) if 1 in shape else (2, 2))


def test_rows_of_65536_voxels_and_the_refusal_above(eng):
    import torch

    from delivr_cfos_amd._lib import DLV_EUNSUP

    mask = np.zeros((1, 2, 65536), dtype=np.uint8)
    mask[0, 0, 0] = mask[0, 0, 65535] = 1  # one gap [1, 65534]: a cup against the z faces
    assert _check(eng, mask) == (0, 0)
    wide = torch.zeros((1, 1, 65537), dtype=torch.uint8, device="cuda")
    wide[0, 0, 5] = wide[0, 0, 9] = 1
    before = wide.clone()
    with pytest.raises(Exception) as exc:
        eng.fill_holes(wide)
    assert getattr(exc.value, "code", None) == DLV_EUNSUP and torch.equal(wide, before)


def test_every_non_zero_byte_is_foreground(eng):
    shells = ref.three_hollow_balls()
    assert _check(eng, shells.astype(np.uint8) * 255, voxels=3269) == (3269, 3)
    mixed = shells.astype(np.uint8)
    mixed[:, ::2] *= 255
    assert set(np.unique(mixed)) == {0, 1, 255}
    assert _check(eng, mixed, voxels=3269) == (3269, 3)


def test_a_mask_that_holds_the_fill_value_is_refused_untouched(eng):
    import ctypes as C

    from delivr_cfos_amd._lib import DLV_EINVAL

    mask = ref.three_hollow_balls().astype(np.uint8)
    mask[20, 22, 82] = 2  # the last byte of the volume, in the remainder of its row
    dev = _dev(mask)
    with pytest.raises(Exception, match="already holds fill_value 2") as exc:
        eng.fill_holes(dev, 2)
    assert getattr(exc.value, "code", None) == DLV_EINVAL
    np.testing.assert_array_equal(dev.cpu().numpy(), mask)
    assert _check(eng, mask, fill_value=3, voxels=3269) == (3269, 3)  # the same mask with another value: filled
    # the other refusals of the entry point, the mask untouched
    voxels, holes = C.c_uint64(77), C.c_uint64(77)
    ptr = C.c_void_p(dev.data_ptr())
    for args in ((ptr, 21, 23, 83, 0), (ptr, 0, 23, 83, 2), (ptr, 21, 23, -1, 2), (None, 21, 23, 83, 2)):
        assert eng.lib.dlv_fill_holes_u8_dev(eng.ctx, *args, C.byref(voxels), C.byref(holes)) == DLV_EINVAL
    assert eng.lib.dlv_fill_holes_u8_dev(eng.ctx, ptr, 21, 23, 83, 2, None, C.byref(holes)) == DLV_EINVAL
    eng.sync()
    np.testing.assert_array_equal(dev.cpu().numpy(), mask)
    assert (voxels.value, holes.value) == (77, 77)
    for bad in (0, 256, True, 2.0):
        with pytest.raises(ValueError, match="fill_value"):
            eng.fill_holes(dev, bad)
    with pytest.raises(ValueError, match="uint8"):
        eng.fill_holes(dev.to(dtype=__import__("torch").int32))


def test_a_mask_one_byte_past_a_16_byte_boundary(eng):
    import torch

    mask = ref.three_hollow_balls(96).astype(np.uint8)
    host = np.full(mask.size + 2, 0x5A, dtype=np.uint8)  # guards
    host[1:-1] = mask.ravel()
    buf = torch.from_numpy(host).cuda()
    view = buf[1:-1].view(mask.shape)
    assert view.data_ptr() % 16 == 1
    assert eng.fill_holes(view) == (3269, 3)
    got = buf.cpu().numpy()
    assert got[0] == 0x5A and got[-1] == 0x5A
    np.testing.assert_array_equal(got[1:-1].reshape(mask.shape), ref.expected_bytes(mask, 2))


# ---- the filled voxels per label ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nested", "random hollow balls", "dense"])
def test_cc_count_marked_against_bincount(eng, name):
    import torch

    mask = {"nested": ref.nested, "random hollow balls": ref.random_hollow_balls,
            "dense": lambda: ref.dense_random((17, 21, 37), 0.7, 3)}[name]()
    bytes_ = ref.expected_bytes(mask.astype(np.uint8), 2)
    labels, n = ref.label26(bytes_)
    if name == "random hollow balls":  # some cells removed, as the size filter does: their filled voxels carry label 0
        labels = np.where(labels % 5 == 0, 0, labels).astype(np.uint32)
    want = np.bincount(labels[bytes_ == 2], minlength=n + 1)
    assert want[1:].sum() > 0
    ldev, mdev = _dev(labels.view(np.int32)), _dev(bytes_)
    got = eng.cc_count_marked(ldev, mdev, n, 2)
    assert got.dtype == torch.int32 and got.shape == (n + 1,) and got.device == ldev.device
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want)
    np.testing.assert_array_equal(eng.cc_count_marked(ldev, mdev, n, 1).cpu().numpy().view(np.uint32),
                                  np.bincount(labels[bytes_ == 1], minlength=n + 1))
    # labels above n are not counted; a mask that starts off a 4-byte boundary takes the byte loads
    few = max(n // 2, 1)
    np.testing.assert_array_equal(eng.cc_count_marked(ldev, mdev, few, 2).cpu().numpy().view(np.uint32), want[:few + 1])
    buf = torch.zeros(bytes_.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = mdev.ravel()
    np.testing.assert_array_equal(eng.cc_count_marked(ldev, buf[1:].view(bytes_.shape), n, 2).cpu().numpy().view(np.uint32), want)
    with pytest.raises(ValueError, match="mask of shape"):
        eng.cc_count_marked(ldev, mdev[:-1], n, 2)


# ---- count_blobs end to end -----------------------------------------------------------------------------------------------------
STD_KEYS = {"voxel_counts", "bounding_boxes", "centroids"}


def _brain_on_disk(root, mask):
    d = root / "in" / "brain"
    os.makedirs(d / "binary_segmentations")
    np.save(str(d / "binary_segmentations" / "binaries.npy"), np.ascontiguousarray(mask, dtype=np.uint8))
    return str(root / "in")


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
    """(40, 48, 190): the random hollow balls, and the shell inside a shell beside them"""
    mask = np.zeros((40, 48, 190), dtype=bool)
    mask[:, :, :150] = ref.random_hollow_balls()
    mask[8:33, 12:37, 150:190] = ref.nested()
    filled, voxels, holes = ref.fill_reference(mask)
    labels, n = ref.label26(filled)
    assert ref.label26(mask)[1] > n  # a cell is swallowed
    for a in (mask, filled, labels):
        a.setflags(write=False)
    return mask, filled, voxels, holes, labels, n


@pytest.mark.parametrize("label_file", ["dense", "runs"])
def test_count_blobs_writes_what_the_filled_mask_gives(eng, tmp_path, brain, capsys, label_file):
    from delivr_cfos_amd import label_runs
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import cell_holes_csv_text

    mask, filled, voxels, holes, labels, n = brain
    stack = (1, 1) + mask.shape
    extra = {} if label_file == "dense" else {"label_file": "runs"}
    # a run without the key on the mask scipy filled ...
    plain_in, plain_post = _brain_on_disk(tmp_path / "plain", filled), str(tmp_path / "plain" / "post")
    assert count_blobs(_settings(plain_in, plain_post, **extra), plain_in, 0, "brain", stack, engine=eng) == n
    # ... and a run with the key on the mask as it is
    path_in, post = _brain_on_disk(tmp_path / "keyed", mask), str(tmp_path / "keyed" / "post")
    assert count_blobs(_settings(path_in, post, fill_holes=True, **extra), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_fill == {"holes": holes, "voxels_filled": voxels, "n_after": n}
    assert "fill_holes_s" in count_blobs.last_timings and "hole_voxels_s" in count_blobs.last_timings
    assert f"fill of holes: {holes} holes filled, {voxels} voxels added, {n} components after the fill" in capsys.readouterr().out
    label_name = f"brain-{n}-cc3d.npy" if label_file == "dense" else label_runs.runs_name("brain", n)
    csv = f"{mask.shape}_brain.csv"
    assert sorted(os.listdir(post)) == sorted([csv, label_name, "brain-stats.pickle", "cell_holes"])
    assert sorted(os.listdir(plain_post)) == sorted([csv, label_name, "brain-stats.pickle"])
    assert _read(post, label_name) == _read(plain_post, label_name) and _read(post, csv) == _read(plain_post, csv)
    if label_file == "dense":
        np.testing.assert_array_equal(np.load(os.path.join(post, label_name)), labels)
    else:
        np.testing.assert_array_equal(label_runs.decode_runs(label_runs.load_runs(os.path.join(post, label_name))), labels)
    stats, plain = pickle.loads(_read(post, "brain-stats.pickle")), pickle.loads(_read(plain_post, "brain-stats.pickle"))
    assert set(plain) == STD_KEYS and set(stats) == STD_KEYS | {"hole_voxels", "holes_filled"}
    for key in STD_KEYS:
        assert stats[key].dtype == plain[key].dtype
        np.testing.assert_array_equal(stats[key], plain[key], err_msg=key)
    want = np.bincount(labels[filled & ~mask], minlength=n + 1)
    assert stats["hole_voxels"].dtype == np.uint32 and stats["holes_filled"] == holes and want.sum() == voxels
    np.testing.assert_array_equal(stats["hole_voxels"], want)
    assert _read(os.path.join(post, "cell_holes"), "brain.csv").decode() == cell_holes_csv_text(stats, n)
    # binaries.npy is step 2's file: not rewritten
    np.testing.assert_array_equal(np.load(os.path.join(path_in, "brain", "binary_segmentations", "binaries.npy")), mask.astype(np.uint8))
    # a second call finds the cached labelling and fills nothing
    before = {name: _read(post, name) for name in os.listdir(post) if name != "cell_holes"}
    assert count_blobs(_settings(path_in, post, fill_holes=True, **extra), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_fill is None and "fill_holes_s" not in count_blobs.last_timings
    assert "fill of holes: the cached labelling is reused as it is, its holes are not filled" in capsys.readouterr().out
    assert {name: _read(post, name) for name in os.listdir(post) if name != "cell_holes"} == before


def test_count_blobs_filters_after_the_fill(eng, tmp_path, brain):
    """the size filter sees the filled sizes; hole_voxels follows the kept cells, the filled voxels of the removed ones are dropped"""
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, filled, voxels, holes, labels, n = brain
    sizes = np.bincount(labels.ravel(), minlength=n + 1)
    added = np.bincount(labels[filled & ~mask], minlength=n + 1)
    lo = int(np.sort(sizes[1:][added[1:] > 0])[1])  # removes the smallest filled cell, keeps the others
    keep = sizes >= lo
    keep[0] = False
    assert (added[1:] > 0)[~keep[1:]].any() and (added[1:] > 0)[keep[1:]].any()
    path_in, post = _brain_on_disk(tmp_path, mask), str(tmp_path / "post")
    K = count_blobs(_settings(path_in, post, fill_holes=True, size_filter=True), path_in, 0, "brain", (1, 1) + mask.shape, lo, -1, engine=eng)
    assert K == int(keep.sum())
    stats = pickle.loads(_read(post, "brain-stats.pickle"))
    np.testing.assert_array_equal(stats["voxel_counts"][1:], sizes[keep])
    np.testing.assert_array_equal(stats["hole_voxels"], np.concatenate([[0], added[keep]]))
    assert stats["holes_filled"] == holes


def test_count_blobs_split_keeps_a_filled_cell_whole(eng, tmp_path):
    """a ball of radius 6 with a cavity of radius 3 off its centre: eroded twice, the hollow ball leaves three cores and is cut
    into three cells; filled first, it leaves one (tests/test_fill_holes_cpu.py shows both on the split's own reference)"""
    from delivr_cfos_amd.count_blobs import count_blobs

    mask = np.zeros((15, 15, 40), dtype=bool)
    mask[:, :, :15] = ref.ball((15, 15, 15), (7, 7, 7), 6) & ~ref.ball((15, 15, 15), (7, 8, 8), 3)
    mask[:, :, 20:35] = ref.ball((15, 15, 15), (7, 7, 7), 5)  # a solid cell beside it
    path_in = _brain_on_disk(tmp_path, mask)
    stack = (1, 1) + mask.shape
    hollow, whole = str(tmp_path / "hollow"), str(tmp_path / "whole")
    assert count_blobs(_settings(path_in, hollow, split_fused=2), path_in, 0, "brain", stack, engine=eng) == 4
    assert count_blobs.last_split["components_split"] == 1 and count_blobs.last_fill is None
    assert count_blobs(_settings(path_in, whole, split_fused=2, fill_holes=True), path_in, 0, "brain", stack, engine=eng) == 2
    assert count_blobs.last_split["components_split"] == 0 and count_blobs.last_fill == {"holes": 1, "voxels_filled": 123, "n_after": 2}
    stats = pickle.loads(_read(whole, "brain-stats.pickle"))
    assert stats["split_parent"].tolist() == [0, 1, 2] and stats["hole_voxels"].tolist() == [0, 123, 0]
    assert pickle.loads(_read(hollow, "brain-stats.pickle"))["split_parent"].tolist() == [0, 1, 2, 1, 1]


def test_count_blobs_without_the_key_writes_what_it_wrote_before(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import cells_csv_bytes

    mask = brain[0]
    labels, n = ref.label26(mask)
    path_in = _brain_on_disk(tmp_path, mask)
    stack = (1, 1) + mask.shape
    names = sorted([f"{mask.shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle"])
    posts = [str(tmp_path / name) for name in ("absent", "false")]
    for post, mi in zip(posts, ({}, {"fill_holes": False})):
        assert count_blobs(_settings(path_in, post, **mi), path_in, 0, "brain", stack, engine=eng) == n
        assert count_blobs.last_fill is None and "fill_holes_s" not in count_blobs.last_timings
        assert "hole_voxels_s" not in count_blobs.last_timings
        assert sorted(os.listdir(post)) == names
    for name in names:
        assert _read(posts[0], name) == _read(posts[1], name), name
    # ... and that is what the labelling of the unfilled mask gives, through the paths that were there before
    np.testing.assert_array_equal(np.load(os.path.join(posts[0], f"brain-{n}-cc3d.npy")), labels)
    stats = pickle.loads(_read(posts[0], "brain-stats.pickle"))
    assert set(stats) == STD_KEYS
    want_stats = eng.cc_stats(_dev(labels.view(np.int32)), n)
    for key in STD_KEYS:
        np.testing.assert_array_equal(stats[key], want_stats[key], err_msg=key)
    assert _read(posts[0], f"{mask.shape}_brain.csv") == cells_csv_bytes(want_stats, n)


def test_a_mask_above_the_budget_is_refused_before_any_file_is_written(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask = brain[0]
    path_in = _brain_on_disk(tmp_path, mask)
    post = str(tmp_path / "post")
    os.makedirs(post)
    open(os.path.join(post, "kept.txt"), "w").close()
    with pytest.raises(MemoryError, match=r"fill_holes.*slab-streamed labelling does not fill holes.*hbm_budget_gb"):
        count_blobs(_settings(path_in, post, fill_holes=True, hbm_budget_gb=1e-4), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng)
    assert os.listdir(post) == ["kept.txt"] and count_blobs.last_fill is None
