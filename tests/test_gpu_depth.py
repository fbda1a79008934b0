"""Per-cell depth on the device (dlv_cc_depth_dev / HipEngine.cc_depth; settings["mi355x"]["depth_stats"] in count_blobs).

The reference of every case is scipy, one label at a time (tests/helpers/depth_reference.py, pinned on hand-made cases in
tests/test_depth_cpu.py): the whole D2 map and the three per-label arrays are integers - equality, no tolerance."""
import ctypes as C
import importlib.util
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAW_KEYS = ("depth_max_sq", "depth_sum_sq", "depth_peak_index")
SPACINGS = ((1, 1, 1), (3, 1, 1), (37, 10, 10), (1, 2, 64))


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("depth_reference")


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def _dev(labels):
    import torch

    return torch.from_numpy(np.ascontiguousarray(labels).view(np.int32).copy()).cuda()


def _map_of(got):
    return got["depth_map"].cpu().numpy().view(np.uint32)


def _assert_same(got: dict, want_map, want_rows):
    """the map and the rows of HipEngine.cc_depth(..., return_map=True) against the reference"""
    assert list(got) == list(RAW_KEYS) + ["depth_map"]
    d2 = _map_of(got)
    assert d2.shape == want_map.shape
    np.testing.assert_array_equal(d2, want_map, err_msg="depth_map")
    for k in RAW_KEYS:
        assert got[k].dtype == want_rows[k].dtype and got[k].shape == want_rows[k].shape, k
        np.testing.assert_array_equal(got[k], want_rows[k], err_msg=k)


def _check(eng, labels, n, spacing):
    dev = _dev(labels)
    got = eng.cc_depth(dev, n, spacing, return_map=True)
    _assert_same(got, *ref.depth_reference(labels, n, spacing))
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), labels)  # the labels are not written
    return got


def _touching_cells(eng, shape, density, seed):
    """a random mask labelled by ccl26; every fifth x-column of each component goes to a second label l + n: touching cells
    -> (labels, n of the labelling: the labels present are 1..2n)"""
    import torch

    rng = np.random.default_rng(seed)
    mask = (rng.random(shape) < density).astype(np.uint8)
    lab, n = eng.ccl26(torch.from_numpy(mask).cuda())
    labels = lab.cpu().numpy().view(np.uint32).copy()
    cols = np.zeros(shape, dtype=bool)
    cols[..., ::5] = True
    labels[cols & (labels > 0)] += np.uint32(n)
    return labels, n


# ---- 1. random masks with touching cells ---------------------------------------------------------------------------------------
# (9, 13, 67): an odd X above 64 voxels; (17, 9, 8); one plane; X < 4, a row shorter than a quad; a y axis longer than X
@pytest.mark.parametrize("density", [0.3, 0.6, 0.9])
@pytest.mark.parametrize("shape", [(9, 13, 67), (17, 9, 8), (1, 9, 9), (5, 1, 3), (3, 70, 5)])
def test_random_masks_with_touching_cells(eng, shape, density):
    labels, n = _touching_cells(eng, shape, density, seed=int(density * 10) + sum(shape))
    assert n >= 1 and int(labels.max()) > n  # both halves are there
    for spacing in SPACINGS:
        got = _check(eng, labels, 2 * n, spacing)
        assert got["depth_max_sq"][0] == 0 and got["depth_sum_sq"][0] == 0 and got["depth_peak_index"][0] == ref.NO_PEAK


# ---- 2. one solid block: long walks in every pass -------------------------------------------------------------------------------
@pytest.mark.parametrize("inset", [0, 1])
def test_one_solid_block(eng, inset):
    labels = np.zeros((40, 40, 70), dtype=np.uint32)
    labels[inset:40 - inset, inset:40 - inset, inset:70 - inset] = 1  # inset 0: every face is a face of the volume
    got = _check(eng, labels, 1, (1, 1, 1))
    assert got["depth_max_sq"][1] == (20 - inset) ** 2
    assert got["depth_peak_index"][1] == (19 * 40 + 19) * 70 + 19
    _check(eng, labels, 1, (2, 1, 3))


def test_rows_wider_than_a_sweep_of_the_x_pass(eng):
    labels = np.zeros((2, 3, 1100), dtype=np.uint32)  # a sweep is 512 voxels: runs across x = 256, 512, 768 and 1024
    labels[:, :, 3:1097] = 1
    labels[1, 1, 500:530] = 2
    labels[0, 2, 1020:1100] = 3
    labels[1, 0, 255:257] = 0
    _check(eng, labels, 3, (1, 1, 1))
    _check(eng, np.ascontiguousarray(labels[:, :, :1027]), 3, (1, 2, 5))  # odd X: three rows in four are not 16-byte aligned


def test_cells_at_linear_indices_past_2_to_31(eng):
    """514 x 2048 x 2048: plane 512 starts at linear index 2^31.  Three boxes, built in HBM (26 GB with the two scratch volumes): one
    in the first corner, one across index 2^31 that is cut by the last z face and the last x face, and the last voxel of the
    volume.  A box's depths depend on its size and on the faces of the volume it touches only, so each is compared with the
    reference on a small volume that shows the box the same faces."""
    import torch

    Z, Y, X = 514, 2048, 2048
    dev = torch.zeros((Z, Y, X), dtype=torch.int32, device="cuda")
    dev[0:3, 0:4, 0:5] = 1
    dev[511:514, 1000:1005, 2040:2048] = 2  # its middle plane, the deepest, is plane 512
    dev[513, 2047, 2047] = 3
    got = eng.cc_depth(dev, 3, (2, 1, 1), return_map=True)
    d2 = got["depth_map"]
    small = {}
    a = np.zeros((4, 5, 6), dtype=np.uint32)
    a[0:3, 0:4, 0:5] = 1
    small[1] = (ref.depth_map(a, 1, (2, 1, 1))[0:3, 0:4, 0:5], (0, 0, 0))
    b = np.zeros((4, 7, 9), dtype=np.uint32)
    b[1:4, 1:6, 1:9] = 1
    small[2] = (ref.depth_map(b, 1, (2, 1, 1))[1:4, 1:6, 1:9], (511, 1000, 2040))
    small[3] = (np.full((1, 1, 1), 1, dtype=np.uint32), (513, 2047, 2047))
    total = 0
    for l, (want, (z0, y0, x0)) in small.items():
        dz, dy, dx = want.shape
        np.testing.assert_array_equal(d2[z0:z0 + dz, y0:y0 + dy, x0:x0 + dx].cpu().numpy().view(np.uint32), want, err_msg=f"cell {l}")
        assert got["depth_max_sq"][l] == want.max() and got["depth_sum_sq"][l] == want.sum()
        pz, py, px = (int(v) for v in np.unravel_index(int(np.argmax(want)), want.shape))  # (the first in raster order)
        assert got["depth_peak_index"][l] == ((z0 + pz) * Y + y0 + py) * X + x0 + px
        total += int(np.count_nonzero(want))
    assert int(got["depth_peak_index"][2]) > 2**31 and int(got["depth_peak_index"][3]) == Z * Y * X - 1
    assert int(torch.count_nonzero(d2)) == total  # nothing else is written but zeros
    assert int(torch.count_nonzero(dev)) == total


# ---- 3. labels above n -------------------------------------------------------------------------------------------------------------
def test_labels_above_n_are_not_measured_and_bound_their_neighbours(eng):
    labels, n = _touching_cells(eng, (9, 13, 67), 0.6, seed=3)
    got = _check(eng, labels, n, (1, 1, 1))  # n is half the labels present
    d2 = _map_of(got)
    assert not d2[labels > n].any() and d2[(labels >= 1) & (labels <= n)].min() >= 1
    whole, _ = ref.depth_reference(np.where(labels > n, labels - n, labels).astype(np.uint32), n)
    assert (d2 < whole).any()  # the upper half bounds the lower one: without it the cells are deeper
    top = labels.copy()
    top[labels > n] = 0xFFFFFFFF  # the largest uint32 is a label above every n as well
    _check(eng, top, n, (3, 1, 1))


# ---- 4. empty and small ------------------------------------------------------------------------------------------------------------
def test_empty_and_small(eng):
    labels, n = _touching_cells(eng, (9, 13, 67), 0.3, seed=4)
    got = _check(eng, labels, 0, (1, 1, 1))  # n = 0: nothing is measured
    assert not _map_of(got).any() and {k: got[k].tolist() for k in RAW_KEYS} == {"depth_max_sq": [0], "depth_sum_sq": [0],
                                                                               "depth_peak_index": [ref.NO_PEAK]}
    empty = np.zeros((5, 6, 7), dtype=np.uint32)
    got = _check(eng, empty, 3, (1, 1, 1))
    assert not _map_of(got).any() and got["depth_peak_index"].tolist() == [ref.NO_PEAK] * 4 and not got["depth_sum_sq"].any()
    one = np.ones((1, 1, 1), dtype=np.uint32)
    got = _check(eng, one, 1, (64, 64, 64))
    assert got["depth_max_sq"].tolist() == [0, 4096] and got["depth_peak_index"].tolist() == [ref.NO_PEAK, 0]
    assert "depth_map" not in eng.cc_depth(_dev(one), 1)


# ---- 5. the first voxel in raster order wins a tie ---------------------------------------------------------------------------------
def test_tie_order(eng):
    labels = np.zeros((3, 5, 9), dtype=np.uint32)
    labels[0:3, 1:4, 1:8] = 1  # five voxels of depth 4 along x
    labels[0, 0, 0] = labels[2, 4, 8] = 2  # two voxels of depth 1, the first and the last of the volume
    got = _check(eng, labels, 2, (1, 1, 1))
    assert (_map_of(got) == 4).sum() == 5
    assert got["depth_peak_index"].tolist() == [ref.NO_PEAK, (1 * 5 + 2) * 9 + 2, 0]


# ---- 6. scratch and determinism: the raw ABI -----------------------------------------------------------------------------------------
def _raw_call(eng, lp, shape, n, spacing, ap, bp, rows=None):
    rows = n + 1 if rows is None else rows
    out = {"depth_max_sq": np.full(rows, 7, np.uint32), "depth_sum_sq": np.full(rows, 7, np.uint64), "depth_peak_index": np.full(rows, 7, np.uint64)}
    rc = eng.lib.dlv_cc_depth_dev(eng.ctx, lp, *shape, n, *spacing, ap, bp, *(a.ctypes.data_as(C.c_void_p) for a in out.values()))
    return rc, out


def test_garbage_in_the_scratch_volumes_and_two_calls(eng):
    import torch

    labels, n = _touching_cells(eng, (9, 13, 67), 0.6, seed=6)
    want_map, want_rows = ref.depth_reference(labels, 2 * n, (37, 10, 10))
    dev = _dev(labels)
    maps = []
    for _ in range(2):
        a = torch.full(labels.shape, -1, dtype=torch.int32, device="cuda")  # 0xFF in every byte
        b = torch.full(labels.shape, -1, dtype=torch.int32, device="cuda")
        rc, out = _raw_call(eng, C.c_void_p(dev.data_ptr()), labels.shape, 2 * n, (37, 10, 10), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()))
        assert rc == 0
        maps.append((a.cpu().numpy().view(np.uint32), out))
        np.testing.assert_array_equal(maps[-1][0], want_map)  # fully written: no byte of the garbage is left
        for k in RAW_KEYS:
            np.testing.assert_array_equal(out[k], want_rows[k], err_msg=k)
    np.testing.assert_array_equal(maps[0][0], maps[1][0])
    for k in RAW_KEYS:
        np.testing.assert_array_equal(maps[0][1][k], maps[1][1][k])
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), labels)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(eng):
    import torch
    from delivr_cfos_amd import _lib

    labels, n = _touching_cells(eng, (9, 13, 67), 0.6, seed=7)
    n *= 2
    shape, nvox = labels.shape, labels.size
    dev = _dev(labels)
    buf = torch.full((2 * nvox + 8,), 0x55555555, dtype=torch.int32, device="cuda")
    a, b = buf[:nvox], buf[nvox + 4:2 * nvox + 4]
    lp, ap, bp = (C.c_void_p(t.data_ptr()) for t in (dev, a, b))
    one = (1, 1, 1)

    def refused(code, *args, rows=None):
        rc, out = _raw_call(eng, *args, rows=rows)
        msg = eng.lib.dlv_last_error(eng.ctx).decode()
        assert rc == code, (rc, msg)
        assert msg.startswith("cc_depth"), msg
        assert all((v == 7).all() for v in out.values())  # nothing written on the host
        np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), labels)
        assert bool((buf == 0x55555555).all())  # nor into the scratch
        return msg

    for args in ((None, shape, n, one, ap, bp), (lp, shape, n, one, None, bp), (lp, shape, n, one, ap, None)):
        assert "NULL" in refused(_lib.DLV_EINVAL, *args)
    for bad in ((0, 13, 67), (9, 0, 67), (9, 13, 0), (-1, 13, 67)):
        refused(_lib.DLV_EINVAL, lp, bad, n, one, ap, bp)
    for spacing in ((0, 1, 1), (1, 65, 1), (1, 1, 0), (65, 1, 1), (1, 1, -3)):
        assert "spacing" in refused(_lib.DLV_EINVAL, lp, shape, n, spacing, ap, bp)
    refused(_lib.DLV_EINVAL, lp, shape, 2**32 - 1, one, ap, bp, rows=4)
    assert "overlaps" in refused(_lib.DLV_EINVAL, lp, shape, n, one, lp, bp)  # work_a is the labels
    assert "overlaps" in refused(_lib.DLV_EINVAL, lp, shape, n, one, ap, lp)
    assert "overlaps" in refused(_lib.DLV_EINVAL, lp, shape, n, one, ap, C.c_void_p(a.data_ptr() + 4 * (nvox - 1)))  # work_b in work_a's last voxel
    assert "overlaps" in refused(_lib.DLV_EINVAL, lp, shape, n, one, ap, C.c_void_p(dev.data_ptr() + 4 * (nvox - 1)))
    for args in ((C.c_void_p(dev.data_ptr() + 2), shape, n, one, ap, bp), (lp, shape, n, one, C.c_void_p(a.data_ptr() + 1), bp),
                 (lp, shape, n, one, ap, C.c_void_p(b.data_ptr() + 2))):
        assert "aligned" in refused(_lib.DLV_EINVAL, *args)
    # 64 * ceil((2050 + 1) / 2) = 64 * 1026 >= 65536: a squared distance would not fit uint32 (the buffers hold 2050 voxels)
    assert nvox >= 2050
    assert "axis x" in refused(_lib.DLV_EUNSUP, lp, (1, 1, 2050), 1, (1, 1, 64), ap, bp)
    assert "axis y" in refused(_lib.DLV_EUNSUP, lp, (1, 2050, 1), 1, (1, 64, 1), ap, bp)
    assert "axis z" in refused(_lib.DLV_EUNSUP, lp, (2050, 1, 1), 1, (64, 1, 1), ap, bp)
    assert "2^32" in refused(_lib.DLV_EUNSUP, lp, (1024, 2048, 2049), 1, one, ap, bp)  # (refused before anything is read)
    rc, out = _raw_call(eng, lp, (1, 1, 2046), 0, (1, 1, 64), ap, bp)  # 64 * 1024 = 65536 is refused too, 64 * 1023 is not
    assert rc == _lib.DLV_EUNSUP
    rc, out = _raw_call(eng, lp, (1, 1, 2045), 0, (1, 1, 64), ap, bp)
    assert rc == 0 and not bool(a[:2045].any())
    # the call still works
    rc, out = _raw_call(eng, lp, shape, n, one, ap, bp)
    want_map, want_rows = ref.depth_reference(labels, n)
    assert rc == 0
    np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32).reshape(shape), want_map)
    for k in RAW_KEYS:
        np.testing.assert_array_equal(out[k], want_rows[k], err_msg=k)
    # the engine
    for bad in ((1, 1), (1, 1, 1, 1), (0, 1, 1), (1, 1, 65), (1.0, 1, 1), (True, 1, 1), 1):
        with pytest.raises(ValueError, match="spacing"):
            eng.cc_depth(dev, n, bad)
    with pytest.raises(ValueError):
        eng.cc_depth(dev, -1)
    with pytest.raises(ValueError):
        eng.cc_depth(dev.cpu(), n)
    with pytest.raises(ValueError):
        eng.cc_depth(labels, n)
    with pytest.raises(ValueError):
        eng.cc_depth(dev.to(torch.int64), n)
    with pytest.raises(ValueError):
        eng.cc_depth(dev.transpose(1, 2), n)  # (not contiguous)
    with pytest.raises(_lib.DelivrHipError, match="axis x"):
        eng.cc_depth(torch.zeros((1, 1, 2050), dtype=torch.int32, device="cuda"), 1, (1, 1, 64))


# ---- 8. count_blobs end to end -------------------------------------------------------------------------------------------------------
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


def _check_outputs(post, shape, n, spacing, other_keys=frozenset(), other_entries=(), runs=False):
    """pickle, table and last_depth of a run with the key against the reference on the label file the run wrote"""
    from delivr_cfos_amd import label_runs
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import DEPTH_KEYS, cell_depth_csv_text, finish_depth

    label_file = label_runs.runs_name("brain", n) if runs else f"brain-{n}-cc3d.npy"
    path = os.path.join(post, label_file)
    labels = (label_runs.load_labels(path) if runs else np.load(path)).astype(np.uint32)
    counts = np.bincount(labels.ravel(), minlength=n + 1).astype(np.uint32)
    want = finish_depth(ref.depth_reference(labels, n, spacing)[1], counts, shape, spacing)
    stats = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(stats) == STD_KEYS | set(DEPTH_KEYS) | set(other_keys)
    for k in DEPTH_KEYS:
        if k == "depth_spacing":
            assert stats[k] == tuple(spacing) and type(stats[k]) is tuple
            continue
        assert stats[k].dtype == want[k].dtype and stats[k].shape == want[k].shape, k
        np.testing.assert_array_equal(stats[k], want[k], err_msg=k)
    np.testing.assert_array_equal(stats["voxel_counts"], counts)
    assert _read(post, os.path.join("cell_depth", "brain.csv")).decode() == cell_depth_csv_text({**want, "voxel_counts": counts}, n)
    assert os.listdir(os.path.join(post, "cell_depth")) == ["brain.csv"]
    assert sorted(os.listdir(post)) == sorted([f"{shape}_brain.csv", label_file, "brain-stats.pickle", "cell_depth", *other_entries])
    assert count_blobs.last_depth == {"n": n, "spacing": tuple(spacing)}
    # the deepest voxel lies inside its cell
    present = counts[1:] > 0
    peaks = stats["depth_peak"][1:][present]
    np.testing.assert_array_equal(labels[peaks[:, 0], peaks[:, 1], peaks[:, 2]], np.flatnonzero(present) + 1)
    return stats


@pytest.fixture(scope="module")
def brain():
    rng = np.random.default_rng(11)
    mask = (rng.random((24, 40, 72)) < 0.05).astype(np.uint8)
    mask[4:11, 10:18, 20:33] = 1
    mask[6:9, 13:16, 24:28] = 0  # a cavity in the large cell
    mask[15:17, 30, 5:40] = 1
    mask[14:22, 2:9, 50:57] = 1  # two blocks joined by a neck: fused cells
    mask[17:19, 5:7, 57:60] = 1
    mask[14:22, 2:9, 60:67] = 1
    mask[0:3, 36:40, 68:72] = 1  # cut by three faces of the volume
    mask.setflags(write=False)
    return mask


def test_count_blobs_with_the_key_and_without(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    path_in = _brain_on_disk(tmp_path, brain)
    shape = brain.shape
    stack = (1, 1) + shape
    on = str(tmp_path / "on")
    n = count_blobs(_settings(path_in, on, depth_stats=True, depth_spacing=[3, 1, 1]), path_in, 0, "brain", stack, engine=eng)
    stats_on = _check_outputs(on, shape, n, (3, 1, 1))
    assert "depth_s" in count_blobs.last_timings and count_blobs.last_shape is None
    # without the key: what a run without it writes, twice the same, and no table
    off, off2 = str(tmp_path / "off"), str(tmp_path / "off2")
    assert count_blobs(_settings(path_in, off), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_depth is None and "depth_s" not in count_blobs.last_timings
    assert count_blobs(_settings(path_in, off2, depth_stats=False), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_depth is None
    names = sorted([f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle"])
    assert sorted(os.listdir(off)) == names and sorted(os.listdir(off2)) == names  # (no cell_depth folder)
    for name in names:
        assert _read(off, name) == _read(off2, name), name
    stats_off = pickle.loads(_read(off, "brain-stats.pickle"))
    assert set(stats_off) == STD_KEYS
    assert _read(on, f"brain-{n}-cc3d.npy") == _read(off, f"brain-{n}-cc3d.npy")
    assert _read(on, f"{shape}_brain.csv") == _read(off, f"{shape}_brain.csv")
    for k in STD_KEYS:
        assert stats_on[k].dtype == stats_off[k].dtype
        np.testing.assert_array_equal(stats_on[k], stats_off[k])
    # the default spacing
    default = str(tmp_path / "default")
    assert count_blobs(_settings(path_in, default, depth_stats=True), path_in, 0, "brain", stack, engine=eng) == n
    _check_outputs(default, shape, n, (1, 1, 1))


def test_count_blobs_measures_the_final_labels_after_fill_and_split(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import SHAPE_KEYS

    path_in = _brain_on_disk(tmp_path, brain)
    stack = (1, 1) + brain.shape
    plain, post = str(tmp_path / "plain"), str(tmp_path / "post")
    n0 = count_blobs(_settings(path_in, plain, depth_stats=True), path_in, 0, "brain", stack, engine=eng)
    before = _check_outputs(plain, brain.shape, n0, (1, 1, 1))
    n = count_blobs(_settings(path_in, post, depth_stats=True, depth_spacing=[2, 1, 1], split_fused=2, fill_holes=True, shape_stats=True),
                    path_in, 0, "brain", stack, engine=eng)
    assert count_blobs.last_split["components_split"] >= 1 and count_blobs.last_fill["holes"] >= 1 and n > n0
    others = {"split_parent", "split_siblings", "split_depth", "hole_voxels", "holes_filled"} | set(SHAPE_KEYS)
    stats = _check_outputs(post, brain.shape, n, (2, 1, 1), others, ["cell_shape", "cell_holes"])
    # the voxel in the middle of the cavity belongs to a cell now, and is the deepest of its row
    final = np.load(os.path.join(post, f"brain-{n}-cc3d.npy"))
    cell = int(final[7, 14, 26])
    assert cell > 0 and np.load(os.path.join(plain, f"brain-{n0}-cc3d.npy"))[7, 14, 26] == 0
    assert stats["depth_max_sq"][cell] > before["depth_max_sq"][1:].min() and stats["hole_voxels"][cell] > 0


def test_count_blobs_with_run_length_labels_and_a_cached_rerun_with_another_spacing(eng, tmp_path, brain):
    from delivr_cfos_amd import label_runs
    from delivr_cfos_amd.count_blobs import count_blobs

    path_in = _brain_on_disk(tmp_path, brain)
    stack = (1, 1) + brain.shape
    post = str(tmp_path / "post")
    n = count_blobs(_settings(path_in, post, depth_stats=True, label_file="runs"), path_in, 0, "brain", stack, engine=eng)
    first = _check_outputs(post, brain.shape, n, (1, 1, 1), runs=True)
    runs_bytes = _read(post, label_runs.runs_name("brain", n))
    # the same spacing again: the cached pickle is complete, nothing is measured
    pickle_bytes = _read(post, "brain-stats.pickle")
    assert count_blobs(_settings(path_in, post, depth_stats=True, label_file="runs"), path_in, 0, "brain", stack, engine=eng) == n
    assert _read(post, "brain-stats.pickle") == pickle_bytes and "depth_s" not in count_blobs.last_timings
    assert count_blobs.last_depth == {"n": n, "spacing": (1, 1, 1)}
    # another spacing: measured again on the decoded runs
    assert count_blobs(_settings(path_in, post, depth_stats=True, depth_spacing=[37, 10, 10], label_file="runs"), path_in, 0, "brain", stack,
                       engine=eng) == n
    assert "depth_s" in count_blobs.last_timings
    second = _check_outputs(post, brain.shape, n, (37, 10, 10), runs=True)
    assert (second["depth_max_sq"][1:] >= 100 * first["depth_max_sq"][1:]).all() and _read(post, label_runs.runs_name("brain", n)) == runs_bytes
    # a dense cached labelling is measured too, and a budget without room for the two scratch volumes refuses
    dense = str(tmp_path / "dense")
    assert count_blobs(_settings(path_in, dense), path_in, 0, "brain", stack, engine=eng) == n
    with pytest.raises(MemoryError, match=r"depth_stats.*cached labels.*hbm_budget_gb"):
        count_blobs(_settings(path_in, dense, depth_stats=True, hbm_budget_gb=brain.size * 11 / 2**30), path_in, 0, "brain", stack, engine=eng)
    assert not os.path.exists(os.path.join(dense, "cell_depth"))
    assert count_blobs(_settings(path_in, dense, depth_stats=True, depth_spacing=[1, 2, 64]), path_in, 0, "brain", stack, engine=eng) == n
    _check_outputs(dense, brain.shape, n, (1, 2, 64))
