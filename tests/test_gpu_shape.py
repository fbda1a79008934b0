"""Per-cell shape accumulators on the device (dlv_cc_shape_dev / HipEngine.cc_shape; settings["mi355x"]["shape_stats"] in
count_blobs).

The reference of every case is numpy (_oracle): the labels padded by one voxel of 0, the six shifted views compared for the exposed
faces and the surface voxels, sums and moments accumulated with np.add.at into uint64 from absolute coordinates.  The five raw
arrays are integers - equality, no tolerance.  The derived values are checked where they are made: covariances against
fractions.Fraction on the integer sums within 4 np.spacing (four roundings: numerator, n^2, division, + 1/12), the principal-axis
variances against eigvalsh of that covariance within 1e-12 of the largest (Weyl's bound plus LAPACK's backward error for a 3 x 3
matrix is a small multiple of 2.2e-16 |C|: about two orders of margin)."""
import ctypes as C
import importlib.util
import os
import pickle
import threading
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAW_KEYS = ("shape_counts", "shape_sums", "shape_moments", "shape_faces", "shape_surface_voxels")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # zz, yy, xx, zy, zx, yx


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _oracle(labels: np.ndarray, n: int, keep=None, z_abs0: int = 0) -> dict:
    """the ABI's rows 0..n for the buffer `labels`: the planes keep = (first, planes) measured, the others neighbours only"""
    first, planes = keep or (0, labels.shape[0])
    pad = np.pad(labels.astype(np.int64), 1, constant_values=0)
    core = pad[1:-1, 1:-1, 1:-1]
    views = [(pad[:-2, 1:-1, 1:-1], pad[2:, 1:-1, 1:-1]), (pad[1:-1, :-2, 1:-1], pad[1:-1, 2:, 1:-1]),
             (pad[1:-1, 1:-1, :-2], pad[1:-1, 1:-1, 2:])]
    exposed = [(lo != core).astype(np.uint64) + (hi != core).astype(np.uint64) for lo, hi in views]
    sel = np.zeros(labels.shape, dtype=bool)
    sel[first:first + planes] = (labels[first:first + planes] >= 1) & (labels[first:first + planes] <= n)
    lab = labels[sel].astype(np.int64)
    zyx = np.nonzero(sel)
    c = [zyx[0].astype(np.uint64) + np.uint64(z_abs0), zyx[1].astype(np.uint64), zyx[2].astype(np.uint64)]
    out = {"shape_counts": np.bincount(lab, minlength=n + 1).astype(np.uint32), "shape_sums": np.zeros((n + 1, 3), np.uint64),
           "shape_moments": np.zeros((n + 1, 6), np.uint64), "shape_faces": np.zeros((n + 1, 3), np.uint64),
           "shape_surface_voxels": np.zeros(n + 1, np.uint32)}
    for a in range(3):
        np.add.at(out["shape_sums"][:, a], lab, c[a])
        np.add.at(out["shape_faces"][:, a], lab, exposed[a][sel])
    for j, (a, b) in enumerate(PAIRS):
        np.add.at(out["shape_moments"][:, j], lab, c[a] * c[b])
    np.add.at(out["shape_surface_voxels"], lab, ((exposed[0] + exposed[1] + exposed[2])[sel] > 0).astype(np.uint32))
    return out


def _assert_same(got: dict, ref: dict, keys=RAW_KEYS):
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


def _dev(labels):
    import torch

    return torch.from_numpy(np.ascontiguousarray(labels).view(np.int32).copy()).cuda()


def _random_labels(shape, n, density, seed):
    """arbitrary labels 1..n (cc_shape does not ask for connected ones): runs along x, so that lanes share labels"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, n + 1, size=shape, dtype=np.uint32)
    lab[..., 1::2] = lab[..., ::2][..., :lab[..., 1::2].shape[-1]]  # pairs along x
    lab[rng.random(shape) >= density] = 0
    return lab


# ---- 1. odd geometry, both alignments --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd(eng):
    """19 x 21 x 139 (x no multiple of 4: a row of the labels starts on a 16-byte boundary every fourth row only): random blobs"""
    rng = np.random.default_rng(5)
    mask = (rng.random((19, 21, 139)) < 0.12).astype(np.uint8)
    mask[3:9, 4:11, 20:60] |= (rng.random((6, 7, 40)) < 0.8).astype(np.uint8)  # a large ragged cell with holes
    labels, n = _label(eng, mask)
    assert n > 100
    ref = _oracle(labels, n)
    assert ref["shape_counts"].max() > 500 and (ref["shape_surface_voxels"][1:] < ref["shape_counts"][1:]).any()
    for a in (labels, *ref.values()):
        a.setflags(write=False)
    return labels, n, ref


def test_odd_geometry_random_blobs(eng, odd):
    labels, n, ref = odd
    dev = _dev(labels)
    assert dev.data_ptr() % 16 == 0
    got = eng.cc_shape(dev, n)
    assert list(got) == list(RAW_KEYS)
    _assert_same(got, ref)
    assert not any(np.any(got[k][0]) for k in RAW_KEYS)  # the background is not measured
    np.testing.assert_array_equal(got["shape_counts"][1:], np.bincount(labels.ravel(), minlength=n + 1)[1:])
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), labels)


def test_odd_geometry_labels_4_bytes_past_a_16_byte_boundary(eng, odd):
    import torch

    labels, n, ref = odd
    host = np.full(labels.size + 2, 0x7FFFFFF0, dtype=np.int32)  # guards: a label far above n
    host[1:-1] = labels.view(np.int32).ravel()
    buf = torch.from_numpy(host).cuda()
    view = buf[1:-1].view(labels.shape)
    assert view.data_ptr() % 16 == 4
    _assert_same(eng.cc_shape(view, n), ref)
    np.testing.assert_array_equal(buf.cpu().numpy(), host)


# ---- 2. flat volumes: every face out of the volume is exposed ---------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 21, 139), (19, 1, 139), (1, 1, 70), (3, 2, 1)])
def test_flat_volumes(eng, shape):
    labels = _random_labels(shape, 7, 0.6, seed=sum(shape))
    ref = _oracle(labels, 7)
    for axis in range(3):
        if shape[axis] == 1:  # both faces along a flat axis are exposed, for every voxel
            np.testing.assert_array_equal(ref["shape_faces"][:, axis], 2 * ref["shape_counts"].astype(np.uint64))
    _assert_same(eng.cc_shape(_dev(labels), 7), ref)


# ---- 3. rows wider than one sweep --------------------------------------------------------------------------------------
def test_wide_rows_cells_across_the_sweep_boundary_and_the_last_quad(eng):
    import torch

    X = 2049 + 7  # one sweep is 256 threads x 8 voxels = 2048
    labels = _random_labels((3, 4, X), 9, 0.05, seed=2)
    labels[:, :, 2040:] = 0
    labels[1, 1:3, 2040:2053] = 10  # across the sweep boundary at x = 2048
    labels[1, 2, 2050:X] = 11       # ... to the last voxel of the row, through its last quad
    labels[2, 3, X - 1] = 12
    labels[0, 0, 1020:1030] = 13    # across the two quads of the threads' halves (x = 1024)
    ref = _oracle(labels, 13)
    _assert_same(eng.cc_shape(_dev(labels), 13), ref)
    host = np.zeros(labels.size + 4, dtype=np.int32)
    host[1:-3] = labels.view(np.int32).ravel()
    view = torch.from_numpy(host).cuda()[1:-3].view(labels.shape)  # no row on a 16-byte boundary: every quad element by element
    assert view.data_ptr() % 16 == 4
    _assert_same(eng.cc_shape(view, 13), ref)
    odd_x = np.ascontiguousarray(labels[:, :, :2051])  # the last quad holds three voxels
    _assert_same(eng.cc_shape(_dev(odd_x), 13), _oracle(odd_x, 13))


# ---- 4. coordinates up to 65535: products at and above 2^31 ------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 65536), (1, 65536, 2)])
def test_large_coordinates_in_the_buffer(eng, shape):
    labels = np.zeros(shape, dtype=np.uint32)
    if shape[2] == 65536:
        labels[0, :, 65000:] = 1
        labels[0, 1, 65530:] = 2
        labels[0, 0, 46340:46345] = 3  # x^2 around 2^31
    else:
        labels[0, 65000:, :] = 1
        labels[0, 65530:, 1] = 2
        labels[0, 46340:46345, 0] = 3
    labels[0, 0, 0] = 4
    ref = _oracle(labels, 4)
    assert int(ref["shape_moments"][2].max()) >= 6 * 65530**2 and int(ref["shape_moments"][1].max()) > 2**40
    _assert_same(eng.cc_shape(_dev(labels), 4), ref)


def test_large_absolute_z(eng):
    labels = _random_labels((4, 5, 70), 6, 0.5, seed=9)
    labels[3, 4, 60:70] = 6
    z0 = 65536 - 4
    ref = _oracle(labels, 6, z_abs0=z0)
    assert int(ref["shape_moments"][6, 0]) >= 10 * 65535**2
    _assert_same(eng.cc_shape(_dev(labels), 6, z_abs0=z0), ref)
    _assert_same(eng.cc_shape(_dev(labels), 6, keep=(1, 2), z_abs0=z0), _oracle(labels, 6, keep=(1, 2), z_abs0=z0))


# ---- 5. many lanes with one label; more than 2^16 labels ---------------------------------------------------------------
def test_a_plane_filling_component_beside_small_ones(eng):
    labels = np.zeros((6, 40, 300), dtype=np.uint32)
    labels[2:4] = 1  # two full planes: every lane of every wave adds to the same row, the inside exposes nothing
    labels[3, 10:14, 100:140] = 0  # a pit in its top plane
    labels[3, 11, 110:120] = 2  # ... with a cell in it, face to face with the component below
    specks = _random_labels((1, 40, 300), 40, 0.03, seed=4)[0]
    labels[0] = np.where(specks > 0, specks + 2, 0)
    labels[5, ::2, ::2] = 43
    n = 43
    ref = _oracle(labels, n)
    assert ref["shape_counts"][1] == 2 * 40 * 300 - 160 and ref["shape_surface_voxels"][1] == ref["shape_counts"][1]
    _assert_same(eng.cc_shape(_dev(labels), n), ref)
    thick = np.zeros((5, 40, 300), dtype=np.uint32)
    thick[:] = 1  # a full block: only the volume's boundary is exposed
    got = eng.cc_shape(_dev(thick), 1)
    _assert_same(got, _oracle(thick, 1))
    assert got["shape_faces"][1].tolist() == [2 * 40 * 300, 2 * 5 * 300, 2 * 5 * 40]
    assert got["shape_surface_voxels"][1] == 5 * 40 * 300 - 3 * 38 * 298


def test_more_than_2_to_16_labels_of_one_voxel(eng):
    shape = (64, 96, 144)
    labels = np.zeros(shape, dtype=np.uint32)
    n = 32 * 48 * 48
    labels[::2, ::2, ::3] = np.arange(1, n + 1, dtype=np.uint32).reshape(32, 48, 48)  # a lattice without touching voxels
    assert n > 65536
    got = eng.cc_shape(_dev(labels), n)
    _assert_same(got, _oracle(labels, n))
    assert (got["shape_counts"][1:] == 1).all() and (got["shape_faces"][1:] == 2).all() and (got["shape_surface_voxels"][1:] == 1).all()


# ---- 6. labels above n, empty and full masks ---------------------------------------------------------------------------
def test_labels_above_n_are_not_accumulated_and_expose_their_neighbours(eng, odd):
    labels, n, ref = odd
    few = 40
    got = eng.cc_shape(_dev(labels), few)
    _assert_same(got, _oracle(labels, few))
    _assert_same(got, {k: v[:few + 1] for k, v in ref.items()})  # the rows 0..few are those of the whole table
    pair = np.zeros((2, 3, 9), dtype=np.uint32)
    pair[0, 1, 2:6] = 1
    pair[0, 1, 6:8] = 2  # above n = 1: not a row of the result, and not "the same label" either
    pair[1, 1, 2:6] = 5
    got = eng.cc_shape(_dev(pair), 1)
    assert got["shape_counts"].tolist() == [0, 4] and got["shape_faces"][1].tolist() == [8, 8, 2]
    _assert_same(got, _oracle(pair, 1))


def test_empty_and_full_masks(eng):
    empty = np.zeros((9, 10, 11), dtype=np.uint32)
    got = eng.cc_shape(_dev(empty), 0)
    assert {k: v.shape for k, v in got.items()} == {"shape_counts": (1,), "shape_sums": (1, 3), "shape_moments": (1, 6),
                                                    "shape_faces": (1, 3), "shape_surface_voxels": (1,)}
    assert not any(v.any() for v in got.values())
    got = eng.cc_shape(_dev(empty), 3)
    assert not any(v.any() for v in got.values()) and got["shape_moments"].shape == (4, 6)
    full = np.ones((9, 10, 11), dtype=np.uint32)
    got = eng.cc_shape(_dev(full), 1)
    _assert_same(got, _oracle(full, 1))
    assert got["shape_faces"][1].tolist() == [2 * 110, 2 * 99, 2 * 90] and got["shape_counts"][1] == 990


# ---- 7. slabs add up ----------------------------------------------------------------------------------------------------
def _slab_volume():
    """24 x 20 x 70 with cells across the cuts at z = 8, 12 and 16"""
    rng = np.random.default_rng(13)
    m = (rng.random((24, 20, 70)) < 0.04).astype(np.uint8)
    m[:, 8:13, 28:40] = 0
    m[5:18, 10, 30:36] = 1   # through every cut
    m[11:13, 4:7, 50:60] = 1  # across z = 12 only
    m[7:9, 15, 5:9] = 1
    m[15:17, 16:19, 60:64] = 1
    return m


@pytest.mark.parametrize("cuts", [(0, 12, 24), (0, 8, 16, 24)])
def test_slabs_with_halo_planes_merge_to_the_whole_volume(eng, cuts):
    from delivr_cfos_amd.hostlogic import merge_shape

    labels, n = _label(eng, _slab_volume())
    assert all(labels[c - 1, 10, 30] == labels[c, 10, 30] != 0 for c in cuts[1:-1])
    dev = _dev(labels)
    whole = eng.cc_shape(dev, n)
    _assert_same(whole, _oracle(labels, n))
    parts, bare = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        e_lo, e_hi = max(lo - 1, 0), min(hi + 1, 24)
        ext = dev[e_lo:e_hi].contiguous()
        parts.append(eng.cc_shape(ext, n, keep=(lo - e_lo, hi - lo), z_abs0=e_lo))
        _assert_same(parts[-1], _oracle(labels[e_lo:e_hi], n, keep=(lo - e_lo, hi - lo), z_abs0=e_lo))
        bare.append(eng.cc_shape(dev[lo:hi].contiguous(), n, z_abs0=lo))
    assert all((p["shape_counts"][1:] == 0).any() for p in parts)  # every slab lacks some labels
    _assert_same(merge_shape(parts), whole)
    _assert_same(merge_shape([parts[-1], None] + parts[:-1]), whole)
    # the test can fail: without the halo planes the faces across the cuts count as exposed (everything else still adds up)
    lone = merge_shape(bare)
    _assert_same(lone, whole, ("shape_counts", "shape_sums", "shape_moments"))
    assert (lone["shape_faces"][:, 0] > whole["shape_faces"][:, 0]).any()
    np.testing.assert_array_equal(lone["shape_faces"][:, 1:], whole["shape_faces"][:, 1:])


# ---- 8. refused arguments -------------------------------------------------------------------------------------------------
def test_refused_arguments(eng, odd):
    import torch
    from delivr_cfos_amd import _lib

    labels, n, ref = odd
    dev = _dev(labels)
    out = {"c": np.zeros(n + 1, np.uint32), "s": np.zeros((n + 1, 3), np.uint64), "m": np.zeros((n + 1, 6), np.uint64),
           "f": np.zeros((n + 1, 3), np.uint64), "v": np.zeros(n + 1, np.uint32)}
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in out.values()]
    lp = C.c_void_p(dev.data_ptr())
    call = eng.lib.dlv_cc_shape_dev
    Z, Y, X = labels.shape
    inval = [
        (None, Z, Y, X, 0, Z, 0, n, *ptrs), (lp, Z, Y, X, 0, Z, 0, n, *ptrs[:4], None), (lp, Z, Y, X, 0, Z, 0, n, None, *ptrs[1:]),
        (lp, 0, Y, X, 0, Z, 0, n, *ptrs), (lp, Z, 0, X, 0, Z, 0, n, *ptrs), (lp, Z, Y, 0, 0, Z, 0, n, *ptrs),
        (lp, Z, Y, X, 0, 0, 0, n, *ptrs), (lp, Z, Y, X, -1, 2, 0, n, *ptrs), (lp, Z, Y, X, 1, Z, 0, n, *ptrs),
        (lp, Z, Y, X, Z, 1, 0, n, *ptrs), (lp, Z, Y, X, 0, Z, -1, n, *ptrs), (lp, Z, Y, X, 0, Z, 0, 2**32 - 1, *ptrs),
        (C.c_void_p(dev.data_ptr() + 2), Z, Y, X, 0, Z, 0, n, *ptrs),
    ]
    for args in inval:
        assert call(eng.ctx, *args) == _lib.DLV_EINVAL, args[:8]
    # (refused before anything is read: the sizes need no buffer behind them)
    for args in ((lp, Z, Y, X, 0, Z, 65536 - Z + 1, n, *ptrs), (lp, 1, 65537, 1, 0, 1, 0, n, *ptrs), (lp, 1, 1, 65537, 0, 1, 0, n, *ptrs),
                 (lp, 65537, 1, 1, 0, 1, 0, n, *ptrs)):
        assert call(eng.ctx, *args) == _lib.DLV_EUNSUP, args[:8]
    assert "uint16" in eng.lib.dlv_last_error(eng.ctx).decode()
    assert not any(a.any() for a in out.values())  # refused: nothing written
    assert call(eng.ctx, lp, Z, Y, X, 0, Z, 0, n, *ptrs) == 0
    _assert_same(dict(zip(RAW_KEYS, out.values())), ref)
    # the engine
    with pytest.raises(ValueError):
        eng.cc_shape(dev.cpu(), n)
    with pytest.raises(ValueError):
        eng.cc_shape(labels, n)
    with pytest.raises(ValueError):
        eng.cc_shape(dev.view(torch.float32), n)
    with pytest.raises(ValueError):
        eng.cc_shape(dev.to(torch.int64), n)
    with pytest.raises(ValueError):
        eng.cc_shape(dev.reshape(-1), n)
    with pytest.raises(ValueError):
        eng.cc_shape(dev.transpose(1, 2), n)  # (not contiguous)
    with pytest.raises(ValueError):
        eng.cc_shape(dev[:0], n)
    for keep in ((-1, 2), (0, 0), (0, Z + 1), (Z, 1), (5, Z - 4)):
        with pytest.raises(ValueError, match="keep"):
            eng.cc_shape(dev, n, keep=keep)
    with pytest.raises(ValueError):
        eng.cc_shape(dev, -1)
    with pytest.raises(ValueError):
        eng.cc_shape(dev, n, z_abs0=-1)
    with pytest.raises(_lib.DelivrHipError):
        eng.cc_shape(dev, n, z_abs0=65536 - Z + 1)


# ---- 9. derived values on the GPU path ----------------------------------------------------------------------------------
def test_derived_values_from_the_device_accumulators(eng, odd):
    from delivr_cfos_amd.hostlogic import finish_shape

    labels, n, ref = odd
    z0 = 40000  # (large coordinates: the products need the exact path)
    got = eng.cc_shape(_dev(labels), n, z_abs0=z0)
    _assert_same(got, _oracle(labels, n, z_abs0=z0))
    out = finish_shape(got, np.bincount(labels.ravel(), minlength=n + 1))
    cov = np.zeros((n + 1, 6))
    for l in range(1, n + 1):
        k = int(got["shape_counts"][l])
        S, M = [int(v) for v in got["shape_sums"][l]], [int(v) for v in got["shape_moments"][l]]
        for j, (a, b) in enumerate(PAIRS):
            exact = Fraction(k * M[j] - S[a] * S[b], k * k) + (Fraction(1, 12) if a == b else 0)
            cov[l, j] = float(exact)
            assert abs(Fraction(float(out["shape_covariance"][l, j])) - exact) <= 4 * Fraction(float(np.spacing(abs(float(exact))))), (l, j)
    mat = np.empty((n + 1, 3, 3))
    for j, (a, b) in enumerate(PAIRS):
        mat[:, a, b] = mat[:, b, a] = cov[:, j]
    axes = np.linalg.eigvalsh(mat)[:, ::-1]
    assert (np.abs(out["shape_axes"] - axes) <= 1e-12 * axes[:, :1]).all()
    np.testing.assert_allclose(out["shape_elongation"][1:], np.sqrt(axes[1:, 0] / axes[1:, 2]), rtol=1e-11, atol=0)
    area = got["shape_faces"][1:].sum(axis=1).astype(np.float64)
    np.testing.assert_allclose(out["shape_sphericity"][1:], np.pi ** (1 / 3) * (6.0 * got["shape_counts"][1:]) ** (2 / 3) / area, rtol=1e-14,
                               atol=0)
    assert (out["shape_elongation"][1:] >= 1).all() and (out["shape_sphericity"][1:] <= 0.81).all()


# ---- 10. count_blobs end to end -------------------------------------------------------------------------------------------
STD_KEYS = {"voxel_counts", "bounding_boxes", "centroids"}


def _brain_on_disk(tmp_path, mask, raw=None):
    d = tmp_path / "in" / "brain"
    os.makedirs(d / "binary_segmentations")
    np.save(str(d / "binary_segmentations" / "binaries.npy"), mask)
    if raw is not None:
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


def _check_outputs(post, shape, n, other_keys=frozenset(), other_entries=()):
    """pickle, table and last_shape of a run with the switch on against numpy on the label file the run wrote"""
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import SHAPE_KEYS, cell_shape_csv_text, finish_shape

    labels = np.load(os.path.join(post, f"brain-{n}-cc3d.npy")).astype(np.uint32)
    counts = np.bincount(labels.ravel(), minlength=n + 1).astype(np.uint32)
    ref = finish_shape(_oracle(labels, n), counts)
    ref["voxel_counts"] = counts
    stats = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(stats) == STD_KEYS | set(SHAPE_KEYS) | set(other_keys)
    _assert_same(stats, ref, SHAPE_KEYS + ("voxel_counts",))
    assert _read(post, os.path.join("cell_shape", "brain.csv")).decode() == cell_shape_csv_text(ref, n)
    assert os.listdir(os.path.join(post, "cell_shape")) == ["brain.csv"]
    assert sorted(os.listdir(post)) == sorted([f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle", "cell_shape", *other_entries])
    assert count_blobs.last_shape == {"n": n}
    return stats


@pytest.fixture(scope="module")
def brain():
    rng = np.random.default_rng(11)
    mask = (rng.random((24, 40, 70)) < 0.06).astype(np.uint8)
    mask[4:9, 10:16, 20:31] = 1
    mask[15:17, 30, 5:40] = 1
    raw = rng.integers(1, 65536, size=(32, 48, 96), dtype=np.uint16)
    mask.setflags(write=False)
    raw.setflags(write=False)
    return mask, raw


def test_count_blobs_switch_on_adds_keys_and_table_and_off_changes_nothing(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, _ = brain
    path_in = _brain_on_disk(tmp_path, mask)  # (no raw volume anywhere: none is opened)
    shape = mask.shape
    stack = (1, 1) + shape
    on = str(tmp_path / "on")
    n = count_blobs(_settings(path_in, on, shape_stats=True), path_in, 0, "brain", stack, engine=eng)
    stats_on = _check_outputs(on, shape, n)
    assert "shape_s" in count_blobs.last_timings and count_blobs.last_intensity is None
    off, off2 = str(tmp_path / "off"), str(tmp_path / "off2")
    assert count_blobs(_settings(path_in, off), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_shape is None and "shape_s" not in count_blobs.last_timings
    assert count_blobs(_settings(path_in, off2, shape_stats=False), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_shape is None
    names = sorted([f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle"])
    assert sorted(os.listdir(off)) == names and sorted(os.listdir(off2)) == names  # (no cell_shape folder)
    for name in names:
        assert _read(off, name) == _read(off2, name), name
    stats_off = pickle.loads(_read(off, "brain-stats.pickle"))
    assert set(stats_off) == STD_KEYS
    assert _read(on, f"brain-{n}-cc3d.npy") == _read(off, f"brain-{n}-cc3d.npy")
    assert _read(on, f"{shape}_brain.csv") == _read(off, f"{shape}_brain.csv")
    for k in STD_KEYS:
        assert stats_on[k].dtype == stats_off[k].dtype
        np.testing.assert_array_equal(stats_on[k], stats_off[k])


def test_count_blobs_with_the_size_filter_measures_the_filtered_labels(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, _ = brain
    path_in = _brain_on_disk(tmp_path, mask)
    post = str(tmp_path / "post")
    n = count_blobs(_settings(path_in, post, shape_stats=True, size_filter=True), path_in, 0, "brain", (1, 1) + mask.shape, 2, 40, engine=eng)
    assert count_blobs.last_filter["n_kept"] == n and 1 < n < count_blobs.last_filter["n_before"]
    stats = _check_outputs(post, mask.shape, n)
    assert stats["voxel_counts"][1:].min() >= 2 and stats["voxel_counts"][1:].max() <= 40


def test_count_blobs_with_intensity_and_shell_statistics_as_well(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import INTENSITY_KEYS, SHELL_KEYS

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, raw)
    stack = (1, 1) + mask.shape
    both, base = str(tmp_path / "both"), str(tmp_path / "base")
    others = set(INTENSITY_KEYS) | {"intensity_mean"} | set(SHELL_KEYS) | {"shell_radius"}
    n = count_blobs(_settings(path_in, both, shape_stats=True, intensity_stats=True, background_shell=2), path_in, 0, "brain", stack, engine=eng)
    stats = _check_outputs(both, mask.shape, n, others, ["cell_intensity"])
    assert count_blobs.last_intensity["shell_radius"] == 2
    assert count_blobs(_settings(path_in, base, intensity_stats=True, background_shell=2), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_shape is None
    plain = pickle.loads(_read(base, "brain-stats.pickle"))
    assert set(plain) == STD_KEYS | others
    for k in plain:
        np.testing.assert_array_equal(stats[k], plain[k], err_msg=k)
    assert _read(both, os.path.join("cell_intensity", "brain.csv")) == _read(base, os.path.join("cell_intensity", "brain.csv"))


def test_count_blobs_on_cached_labels_completes_a_cached_pickle(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, _ = brain
    path_in = _brain_on_disk(tmp_path, mask)
    post = str(tmp_path / "post")
    stack = (1, 1) + mask.shape
    n = count_blobs(_settings(path_in, post), path_in, 0, "brain", stack, engine=eng)
    label_bytes, csv_bytes = _read(post, f"brain-{n}-cc3d.npy"), _read(post, f"{mask.shape}_brain.csv")
    before = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(before) == STD_KEYS
    with pytest.raises(MemoryError, match=r"shape_stats.*cached labels.*hbm_budget_gb"):  # cached labels above the budget
        count_blobs(_settings(path_in, post, shape_stats=True, hbm_budget_gb=1e-4), path_in, 0, "brain", stack, engine=eng)
    assert pickle.loads(_read(post, "brain-stats.pickle")).keys() == before.keys() and not os.path.exists(os.path.join(post, "cell_shape"))
    assert count_blobs(_settings(path_in, post, shape_stats=True), path_in, 0, "brain", stack, engine=eng) == n
    stats = _check_outputs(post, mask.shape, n)
    for k in STD_KEYS:
        assert stats[k].dtype == before[k].dtype
        np.testing.assert_array_equal(stats[k], before[k])
    assert _read(post, f"brain-{n}-cc3d.npy") == label_bytes and _read(post, f"{mask.shape}_brain.csv") == csv_bytes
    # a third run finds the keys in the cached pickle: nothing is measured again
    pickle_bytes = _read(post, "brain-stats.pickle")
    assert count_blobs(_settings(path_in, post, shape_stats=True), path_in, 0, "brain", stack, engine=eng) == n
    assert _read(post, "brain-stats.pickle") == pickle_bytes and "shape_s" not in count_blobs.last_timings
    assert count_blobs.last_shape == {"n": n}
    # cached labels without a cached pickle
    os.remove(os.path.join(post, "brain-stats.pickle"))
    assert count_blobs(_settings(path_in, post, shape_stats=True), path_in, 0, "brain", stack, engine=eng) == n
    _check_outputs(post, mask.shape, n)


def test_a_mask_that_would_be_slab_streamed_is_refused_before_any_file_is_written(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, _ = brain
    path_in = _brain_on_disk(tmp_path, mask)
    post = str(tmp_path / "post")
    os.makedirs(post)
    open(os.path.join(post, "kept.txt"), "w").close()
    with pytest.raises(MemoryError, match=r"shape_stats.*slab-streamed.*hbm_budget_gb"):
        count_blobs(_settings(path_in, post, shape_stats=True, hbm_budget_gb=1e-4), path_in, 0, "brain", (1, 1) + mask.shape, engine=eng)
    assert os.listdir(post) == ["kept.txt"] and count_blobs.last_shape is None


# ---- 11. sharded ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_count_blobs_under_torch_distributed_equals_the_single_engine_result(eng, tmp_path, monkeypatch, world):
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import SHAPE_KEYS

    ranks = _helper("thread_ranks")
    m = _slab_volume()
    path_in = _brain_on_disk(tmp_path, m)
    stack = (1, 1) + m.shape
    single = str(tmp_path / "single")
    n = count_blobs(_settings(path_in, single, shape_stats=True), path_in, 0, "brain", stack, engine=eng)
    ref = _check_outputs(single, m.shape, n)
    fake = ranks.ThreadRanks(world)
    fake.patch(monkeypatch, dist)
    for filtered in (False, True):
        post = str(tmp_path / f"sharded{int(filtered)}")
        settings = _settings(path_in, post, shape_stats=True, size_filter=filtered)
        results = ranks.run_thread_ranks(fake, lambda rank, e: count_blobs(settings, path_in, 0, "brain", stack, 2, 30, engine=e))
        k = results[0]
        assert results == [k] * world and (k < n if filtered else k == n)
        stats = _check_outputs(post, m.shape, k)  # rank 0's pickle and table against numpy on the written labels
        if not filtered:
            for key in STD_KEYS | set(SHAPE_KEYS):
                np.testing.assert_array_equal(stats[key], ref[key], err_msg=key)
            for name in (f"{m.shape}_brain.csv", os.path.join("cell_shape", "brain.csv")):
                assert _read(post, name) == _read(single, name), name


def test_more_ranks_than_planes_raise_the_same_error_on_every_rank(eng, tmp_path, monkeypatch):
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs

    ranks = _helper("thread_ranks")
    m = np.ascontiguousarray(_slab_volume()[:2])
    path_in = _brain_on_disk(tmp_path, m)
    post = str(tmp_path / "post")
    fake = ranks.ThreadRanks(3)  # 2 planes over 3 ranks: rank 0's slab is empty
    fake.patch(monkeypatch, dist)
    settings = _settings(path_in, post, shape_stats=True)
    caught = [None] * 3

    def rank_main(rank):
        fake.bind(rank)
        try:
            count_blobs(settings, path_in, 0, "brain", (1, 1) + m.shape, engine=eng)  # (refused before the engine is used)
        except BaseException as exc:  # noqa: BLE001
            caught[rank] = exc

    ts = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not any(t.is_alive() for t in ts)  # nobody waits in a collective
    assert all(type(c) is ValueError for c in caught), caught
    assert len({str(c) for c in caught}) == 1 and "slabs of 0" in str(caught[0]) and "shape_stats" in str(caught[0])
    assert not os.path.exists(post)
