"""Per-cell background shells on the device (dlv_cc_shell_dev / HipEngine.cc_shell; settings["mi355x"]["background_shell"] in
count_blobs).

The reference is numpy, here: the iterated expansion E_0 = L, E_{k+1} = E_k where that is not 0, else the smallest non-zero E_k
among the 26 neighbours - 27 shifted views of the volume padded with 0xFFFFFFFF, 0 taken as 0xFFFFFFFF - and S = E_r where
L == 0 and raw != 0.  The statistics of S are the reduceat reduction of tests/test_gpu_intensity.py (copied).  One tiny case pins
the iterated reference itself to the direct formula "smallest label at the minimal Chebyshev distance <= r".  Everything compared
is an integer - equality; the two float columns are float64 equality with the same numpy expression on the integer results.

The kernel's tile is 8 x 8 x 64 voxels (z, y, x): the shapes below span two tiles and a remainder on every axis where the
case is about the tiling."""
import ctypes as C
import importlib.util
import itertools
import os
import pickle
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TZ, TY, TX = 8, 8, 64  # cc_shell.hip's tile
NONE = np.uint32(0xFFFFFFFF)
KEYS = ("intensity_sum", "intensity_sumsq", "intensity_min", "intensity_max")
SHELL_KEYS = ("shell_voxels", "shell_sum", "shell_sumsq", "shell_min", "shell_max", "shell_mean", "contrast")


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the reference -------------------------------------------------------------------------------------------------------
def _expand(labels: np.ndarray, r: int) -> np.ndarray:
    """E_r: r synchronous steps, each from the previous volume alone"""
    E = labels.astype(np.uint32)
    Z, Y, X = E.shape
    for _ in range(r):
        P = np.pad(np.where(E == 0, NONE, E), 1, constant_values=NONE)
        m = np.full(E.shape, NONE, dtype=np.uint32)
        for dz, dy, dx in itertools.product(range(3), repeat=3):
            np.minimum(m, P[dz:dz + Z, dy:dy + Y, dx:dx + X], out=m)
        E = np.where(E != 0, E, np.where(m == NONE, 0, m)).astype(np.uint32)
    return E


def _shell(labels: np.ndarray, raw, r: int) -> np.ndarray:
    """S; raw None: no raw condition"""
    keep = labels == 0
    if raw is not None:
        keep &= raw != 0
    return np.where(keep, _expand(labels, r), 0).astype(np.uint32)


def _expand_direct(labels: np.ndarray, r: int) -> np.ndarray:
    """the direct formula, voxel by voxel: the smallest label in the first Chebyshev ball of radius 1..r that holds one"""
    Z, Y, X = labels.shape
    out = labels.astype(np.uint32).copy()
    for z, y, x in itertools.product(range(Z), range(Y), range(X)):
        if labels[z, y, x]:
            continue
        for d in range(1, r + 1):
            ball = labels[max(z - d, 0):z + d + 1, max(y - d, 0):y + d + 1, max(x - d, 0):x + d + 1]
            if ball.any():
                out[z, y, x] = ball[ball != 0].min()
                break
    return out


def _reference(labels: np.ndarray, raw: np.ndarray, n: int) -> dict:
    """(tests/test_gpu_intensity.py) the ABI's rows 0..n: absent labels - and row 0 - read 0, 0, 0xFFFF, 0"""
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


def _shell_counts(S: np.ndarray, n: int) -> np.ndarray:
    return np.bincount(S.ravel(), minlength=n + 1)[:n + 1].astype(np.uint32)


def _finished_shell(labels, raw, n, r):
    """what count_blobs stores for the shells, from numpy alone"""
    S = _shell(labels, raw, r)
    ref = _reference(S, raw, n)
    counts = _shell_counts(S, n)
    counts[0] = 0
    has = counts > 0
    cells = np.zeros(n + 1, dtype=np.float64)
    cell_counts = np.bincount(labels.ravel(), minlength=n + 1)
    cell_sums = _reference(labels, raw, n)["intensity_sum"]
    present = cell_counts > 0
    present[0] = False
    cells[present] = cell_sums[present].astype(np.float64) / cell_counts[present]
    mean, contrast = np.zeros(n + 1, dtype=np.float64), np.zeros(n + 1, dtype=np.float64)
    mean[has] = ref["intensity_sum"][has].astype(np.float64) / counts[has].astype(np.float64)
    contrast[has] = cells[has] / mean[has]
    lo = ref["intensity_min"].copy()
    lo[~has] = 0
    return {"shell_voxels": counts, "shell_sum": ref["intensity_sum"], "shell_sumsq": ref["intensity_sumsq"], "shell_min": lo,
            "shell_max": ref["intensity_max"], "shell_mean": mean, "contrast": contrast}


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


def _dev(a):
    import torch

    a = np.array(a, order="C")  # (a writable copy: the fixtures are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _check_shell_and_statistics(eng, labels, raw, n, r, S=None):
    """cc_shell against the reference volume, and cc_intensity + cc_counts of the device's shell against numpy's of the reference's"""
    S = _shell(labels, raw, r) if S is None else S
    lab_dev, raw_dev = _dev(labels), _dev(raw)
    shell_dev = eng.cc_shell(lab_dev, r, raw_dev)
    import torch

    assert shell_dev.dtype == torch.int32 and tuple(shell_dev.shape) == labels.shape and shell_dev.is_contiguous()
    np.testing.assert_array_equal(_host(shell_dev), S)
    view = raw[:labels.shape[0], :labels.shape[1], :labels.shape[2]]
    _assert_same(eng.cc_intensity(shell_dev, raw_dev, n), _reference(S, view, n))
    np.testing.assert_array_equal(_host(eng.cc_counts(shell_dev, n))[1:], _shell_counts(S, n)[1:])
    np.testing.assert_array_equal(_host(lab_dev), labels)  # inputs untouched
    np.testing.assert_array_equal(raw_dev.cpu().numpy(), raw)
    return S


# ---- 0. the reference itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_tiny_volume_iterated_reference_equals_the_direct_formula_and_the_device(eng, r):
    rng = np.random.default_rng(21)
    labels = np.zeros((9, 14, 19), dtype=np.uint32)
    spots = rng.permutation(labels.size)[:12]
    labels.ravel()[spots] = rng.permutation(12) + 1  # twelve single voxels, labels in no raster order
    labels[4:6, 6:8, 9:12] = 13
    E = _expand(labels, r)
    np.testing.assert_array_equal(E, _expand_direct(labels, r))
    assert (E != 0).sum() > (_expand(labels, r - 1) != 0).sum() if r > 1 else (E != 0).sum() > 13 + 5
    raw = rng.integers(0, 4, size=labels.shape, dtype=np.uint16)  # a quarter of the tissue is "outside"
    S = _check_shell_and_statistics(eng, labels, raw, 13, r)
    np.testing.assert_array_equal(S, np.where((labels == 0) & (raw != 0), E, 0))
    np.testing.assert_array_equal(_host(eng.cc_shell(_dev(labels), r)), np.where(labels == 0, E, 0))


# ---- 1. / 2. odd geometry, padded raw, both alignments ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd(eng):
    """33 x 67 x 131 labels (x no multiple of 4; two x tiles and 3 voxels) of the intensity tests' pitch-4 box mask under a
    48 x 80 x 144 raw volume with zeros (a tenth of it, and the whole surroundings of three cells) and 65535s"""
    import torch

    rng = np.random.default_rng(5)
    shape = (33, 67, 131)
    mask = np.zeros(shape, dtype=np.uint8)
    for z in range(0, shape[0], 4):
        for y in range(0, shape[1], 4):
            ext = rng.integers(1, 4, size=(len(range(0, shape[2], 4)), 3))
            for (dz, dy, dx), x in zip(ext, range(0, shape[2], 4)):
                mask[z:z + dz, y:y + dy, x:x + dx] = 1
    lab, n = eng.ccl26(torch.from_numpy(mask).cuda())
    labels = lab.cpu().numpy().view(np.uint32)
    assert n == 9 * 17 * 33
    raw = rng.integers(1, 65536, size=(48, 80, 144), dtype=np.uint16)
    raw[rng.random(raw.shape) < 0.1] = 0
    raw[rng.random(raw.shape) < 0.01] = 65535
    dark = [int(labels[z, y, x]) for z, y, x in ((0, 0, 0), (16, 32, 64), (32, 64, 128))]
    for z, y, x in ((0, 0, 0), (16, 32, 64), (32, 64, 128)):  # (nothing but "outside" within 4 voxels of these cells' corners)
        raw[max(z - 4, 0):z + 8, max(y - 4, 0):y + 8, max(x - 4, 0):x + 8] = 0
    for a in (labels, raw):
        a.setflags(write=False)
    return labels, n, raw, dark


@pytest.mark.parametrize("r", [1, 2, 3])
def test_odd_geometry_padded_raw(eng, odd, r):
    labels, n, raw, dark = odd
    view = raw[:33, :67, :131]
    E = _expand(labels, r)
    S = _shell(labels, view, r)
    # the reference itself shows what the case is about: voxels lost to raw == 0, raw 0 and 65535 inside the reach of the
    # cells, ties between two cells, cells without a shell
    reach = (labels == 0) & (E != 0)
    assert (reach & (view == 0)).any() and (S[reach & (view == 0)] == 0).all() and (reach & (view == 65535) & (S != 0)).any()
    P = np.pad(np.where(labels == 0, NONE, labels), 1, constant_values=NONE)
    lo, hi = np.full(labels.shape, NONE, dtype=np.uint32), np.zeros(labels.shape, dtype=np.uint32)
    for dz, dy, dx in itertools.product(range(3), repeat=3):
        nb = P[dz:dz + 33, dy:dy + 67, dx:dx + 131]
        np.minimum(lo, nb, out=lo)
        np.maximum(hi, np.where(nb == NONE, 0, nb), out=hi)
    ties = (labels == 0) & (lo != NONE) & (hi != lo)  # two different cells at distance 1
    assert ties.any() and (E[ties] == lo[ties]).all()
    counts = _shell_counts(S, n)
    assert all(counts[d] == 0 for d in dark) and (counts[1:] > 0).sum() > n // 2
    assert not S[labels != 0].any()  # voxels of any cell are never shell
    _check_shell_and_statistics(eng, labels, raw, n, r, S)
    # raw=None: the expanded labels, less the cells
    np.testing.assert_array_equal(_host(eng.cc_shell(_dev(labels), r)), np.where(labels == 0, E, 0))


@pytest.mark.parametrize("r", [1, 3])
def test_odd_geometry_labels_4_bytes_and_raw_2_bytes_past_a_16_byte_boundary(eng, odd, r):
    import torch

    labels, n, raw, _ = odd
    lab_host = np.ones(labels.size + 2, dtype=np.int32)  # guards: label 1 - read as a neighbour, it would win wherever it reaches
    lab_host[1:-1] = labels.view(np.int32).ravel()
    raw_host = np.full(raw.size + 2, 0xABCD, dtype=np.uint16)
    raw_host[1:-1] = raw.ravel()
    lab_buf, raw_buf = torch.from_numpy(lab_host).cuda(), torch.from_numpy(raw_host).cuda()
    lab_view, raw_view = lab_buf[1:-1].view(labels.shape), raw_buf[1:-1].view(raw.shape)
    assert lab_view.data_ptr() % 16 == 4 and raw_view.data_ptr() % 16 == 2
    S = _shell(labels, raw[:33, :67, :131], r)
    shell = eng.cc_shell(lab_view, r, raw_view)
    np.testing.assert_array_equal(_host(shell), S)
    _assert_same(eng.cc_intensity(shell, raw_view, n), _reference(S, raw[:33, :67, :131], n))
    np.testing.assert_array_equal(lab_buf.cpu().numpy(), lab_host)  # guards and payload untouched
    np.testing.assert_array_equal(raw_buf.cpu().numpy(), raw_host)
    # the C entry point with misaligned OUTPUT volumes between guards
    nvox = labels.size
    out = torch.full((2 * nvox + 5,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    shell_view, scratch_view = out[1:1 + nvox], out[nvox + 2:2 * nvox + 2]
    assert shell_view.data_ptr() % 16 == 4 and scratch_view.data_ptr() % 16 in (4, 12)
    rc = eng.lib.dlv_cc_shell_dev(eng.ctx, C.c_void_p(lab_view.data_ptr()), C.c_void_p(raw_view.data_ptr()), 33, 67, 131, 144, 80 * 144, r,
                                  C.c_void_p(shell_view.data_ptr()), C.c_void_p(scratch_view.data_ptr()))
    assert rc == 0
    eng.sync()
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[1:1 + nvox].view(np.uint32).reshape(labels.shape), S)
    assert (got[[0, nvox + 1, 2 * nvox + 2, 2 * nvox + 3, 2 * nvox + 4]] == 0x5A5A5A5A).all()


# ---- 3. tile seams and faces ---------------------------------------------------------------------------------------------
def _seam_cells():
    """19 x 21 x 139: two tiles and a remainder on every axis.  Single voxels on every corner, edge and face of the volume, on
    both sides of every tile boundary in x, y and z and at tile corners (the shell of (7, 7, 63) lies in eight tiles); pairs 2, 3
    and 4 voxels apart; two boxes with a one-voxel gap between their faces.  Labels in no raster order."""
    Z, Y, X = 2 * TZ + 3, 2 * TY + 5, 2 * TX + 11
    zs, ys, xs = (0, Z // 2, Z - 1), (0, Y // 2, Y - 1), (0, X // 2, X - 1)
    pts = [p for p in itertools.product(zs, ys, xs) if p != (Z // 2, Y // 2, X // 2)]  # 8 corners, 12 edges, 6 faces
    pts += [(4, 3, TX - 1), (4, 12, TX), (12, 3, 2 * TX - 1), (12, 12, 2 * TX)]             # x boundaries
    pts += [(4, TY - 1, 20), (4, TY, 30), (4, 2 * TY - 1, 40), (4, 2 * TY, 50)]             # y boundaries
    pts += [(TZ - 1, 18, 20), (TZ, 18, 30), (2 * TZ - 1, 18, 40), (2 * TZ, 18, 50)]         # z boundaries
    pts += [(TZ - 1, TY - 1, TX - 1), (2 * TZ, 2 * TY, 2 * TX)]                             # tile corners
    pts += [(12, 5, 20), (12, 5, 22), (12, 5, 30), (12, 5, 33), (12, 5, 40), (12, 5, 44)]   # 2, 3, 4 apart
    assert len(set(pts)) == len(pts)
    a = np.array(pts)
    d = np.abs(a[:, None, :] - a[None, :, :]).max(axis=2)
    assert d[~np.eye(len(pts), dtype=bool)].min() >= 2  # no two cells touch, not even diagonally
    labels = np.zeros((Z, Y, X), dtype=np.uint32)
    order = np.random.default_rng(3).permutation(len(pts) + 2) + 1
    for (z, y, x), l in zip(pts, order):
        labels[z, y, x] = l
    assert not labels[2:4, 11:15, 89:98].any() and not labels[1:5, 11:15, 89:98].any()
    labels[2:4, 12:14, 90:93] = order[-2]
    labels[2:4, 12:14, 94:97] = order[-1]  # the gap: x = 93
    return labels, len(pts) + 2


@pytest.mark.parametrize("r", [1, 2, 3])
def test_tile_seams_faces_and_meeting_shells(eng, r):
    labels, n = _seam_cells()
    rng = np.random.default_rng(r)
    raw = rng.integers(0, 5, size=labels.shape, dtype=np.uint16) * 13107  # 0 (a fifth of the voxels) .. 52428
    raw[rng.random(raw.shape) < 0.05] = 65535
    S = _check_shell_and_statistics(eng, labels, raw, n, r)
    E = _host(eng.cc_shell(_dev(labels), r))
    np.testing.assert_array_equal(E, np.where(labels == 0, _expand(labels, r), 0))
    a, b = int(labels[2, 12, 90]), int(labels[2, 12, 94])
    assert set(E[2:4, 12:14, 93].ravel()) == {min(a, b)}  # the one-voxel gap goes to the smaller label
    if r == 2:
        row = E[12, 5]
        l = [int(labels[12, 5, x]) for x in (20, 22, 30, 33, 40, 44)]
        assert row[21] == min(l[0], l[1])                                        # 2 apart: the shells meet in a tie
        assert (row[31], row[32]) == (l[2], l[3])                                # 3 apart: they meet without a tie
        assert (row[41], row[42], row[43]) == (l[4], min(l[4], l[5]), l[5])      # 4 apart: they tie in the middle
        assert row[35] != 0 and row[36] == 0 and row[37] == 0 and row[38] != 0   # ... and stay apart from the next pair
    # the shell of the cell at the tile corner lies in eight tiles
    c = int(labels[TZ - 1, TY - 1, TX - 1])
    zz, yy, xx = np.nonzero(E == c)
    assert len({(z // TZ, y // TY, x // TX) for z, y, x in zip(zz, yy, xx)}) == 8
    assert r > 1 or len(zz) == 26  # (further out other cells compete)
    assert S.any()


@pytest.mark.parametrize("shape", [(1, 21, 139), (19, 1, 139), (1, 1, 70), (3, 2, 1)])
def test_flat_volumes(eng, shape):
    rng = np.random.default_rng(sum(shape))
    labels = np.zeros(shape, dtype=np.uint32)
    picks = rng.permutation(labels.size)[:max(labels.size // 60, 1)]
    labels.ravel()[picks] = rng.permutation(len(picks)) + 1
    raw = rng.integers(0, 3, size=shape, dtype=np.uint16)
    for r in (1, 2, 5):
        _check_shell_and_statistics(eng, labels, raw, len(picks), r)


# ---- 4. more than 2^16 labels --------------------------------------------------------------------------------------------
def test_more_than_2_to_16_labels_the_smallest_label_wins_every_tie(eng):
    shape = (8, 200, 360)
    n = 4 * 100 * 180
    assert n > 70000
    labels = np.zeros(shape, dtype=np.uint32)
    labels[::2, ::2, ::2] = np.random.default_rng(8).permutation(n).reshape(4, 100, 180) + 1  # every background voxel is a tie
    raw = np.random.default_rng(9).integers(0, 65536, size=shape, dtype=np.uint16)
    S = _check_shell_and_statistics(eng, labels, raw, n, 1)
    assert int(S.max()) > 65536 and len(np.unique(S)) > 40000


# ---- 5. one large component beside small ones ------------------------------------------------------------------------------
def test_one_plane_filling_component_beside_small_ones(eng):
    rng = np.random.default_rng(10)
    shape = (24, 40, 150)
    labels = np.zeros(shape, dtype=np.uint32)
    labels[10:13] = 7  # a slab through the whole volume: its shell is the three planes on either side, less what smaller labels take
    specks = [(1, 5, 5), (5, 20, 70), (17, 8, 140), (22, 30, 10), (20, 39, 149), (6, 0, 0)]
    for l, p in zip((1, 2, 3, 9, 10, 11), specks):
        labels[p] = l
    raw = rng.integers(1, 65536, size=shape, dtype=np.uint16)
    S = _check_shell_and_statistics(eng, labels, raw, 11, 3)
    counts = _shell_counts(S, 11)
    assert (S[13:16] != 0).all() and (S[7:10] != 0).all()
    others = int((S[7:10] != 7).sum() + (S[13:16] != 7).sum())  # what nearer specks, or smaller labels at the same distance, take
    assert 0 < others < 400 and int(counts[7]) == 6 * 40 * 150 - others > 2**15


# ---- 6. empty and full mask: the output is written whatever it held ---------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2, 3])
def test_empty_and_full_mask_overwrite_an_output_that_held_garbage(eng, r):
    import torch

    shape = (2 * TZ + 1, 2 * TY + 3, 2 * TX + 5)
    raw = _dev(np.full(shape, 9, dtype=np.uint16))
    for fill in (0, 4):
        labels = torch.full(shape, fill, dtype=torch.int32, device="cuda")
        shell = torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        scratch = torch.full(shape, 0x3C3C3C3C, dtype=torch.int32, device="cuda")
        rc = eng.lib.dlv_cc_shell_dev(eng.ctx, C.c_void_p(labels.data_ptr()), C.c_void_p(raw.data_ptr()), *shape, shape[2], shape[1] * shape[2],
                                      r, C.c_void_p(shell.data_ptr()), C.c_void_p(scratch.data_ptr()) if r > 1 else None)
        assert rc == 0
        eng.sync()
        assert not shell.any().item(), fill
        assert (labels == fill).all().item()
        assert not eng.cc_shell(labels, r, raw).any().item()
    # the same allocation again, now with something in it, then empty again
    one = torch.zeros(shape, dtype=torch.int32, device="cuda")
    one[TZ, TY, TX] = 1
    args = (*shape, shape[2], shape[1] * shape[2], r, C.c_void_p(shell.data_ptr()), C.c_void_p(scratch.data_ptr()))
    assert eng.lib.dlv_cc_shell_dev(eng.ctx, C.c_void_p(one.data_ptr()), C.c_void_p(raw.data_ptr()), *args) == 0
    eng.sync()
    assert int((shell == 1).sum()) == (2 * r + 1) ** 3 - 1
    none = torch.zeros_like(one)
    assert eng.lib.dlv_cc_shell_dev(eng.ctx, C.c_void_p(none.data_ptr()), C.c_void_p(raw.data_ptr()), *args) == 0
    eng.sync()
    assert not shell.any().item()


# ---- 7. slabs ------------------------------------------------------------------------------------------------------------
def _slab_volume():
    rng = np.random.default_rng(14)
    shape = (24, 40, 72)
    labels = np.zeros(shape, dtype=np.uint32)
    picks = np.flatnonzero(rng.random(labels.size) < 0.004)
    labels.ravel()[picks] = rng.permutation(len(picks)) + 1
    labels[5:19, 20, 30] = len(picks) + 1  # a cell through every seam
    raw = rng.integers(0, 4, size=shape, dtype=np.uint16)
    return labels, len(picks) + 1, raw


@pytest.mark.parametrize("cuts", [(0, 12, 24), (0, 8, 16, 24)])
def test_slabs_extended_by_r_planes_and_trimmed_concatenate_to_the_whole_volume(eng, cuts):
    r = 3
    labels, n, raw = _slab_volume()
    lab_dev, raw_dev = _dev(labels), _dev(raw)
    whole = _host(eng.cc_shell(lab_dev, r, raw_dev))
    np.testing.assert_array_equal(whole, _shell(labels, raw, r))
    pieces = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        a, b = max(lo - r, 0), min(hi + r, 24)
        pieces.append(_host(eng.cc_shell(lab_dev[a:b], r, raw_dev[a:b]))[lo - a:lo - a + hi - lo])
    np.testing.assert_array_equal(np.concatenate(pieces), whole)
    # (without the extension the seams differ: the extension is what makes it exact)
    bare = np.concatenate([_host(eng.cc_shell(lab_dev[lo:hi], r, raw_dev[lo:hi])) for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert (bare != whole).any()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def test_refused_arguments(eng):
    import torch
    from delivr_cfos_amd import _lib

    labels, n, raw = _slab_volume()
    lab_dev, raw_dev = _dev(labels), _dev(raw)
    for bad in (0, 17, -1, True, 2.0, "3", None):
        with pytest.raises(ValueError, match="radius"):
            eng.cc_shell(lab_dev, bad, raw_dev)
    for small in (raw[:23], raw[:, :39], raw[:, :, :71]):
        with pytest.raises(ValueError, match="smaller"):
            eng.cc_shell(lab_dev, 2, _dev(small))
    with pytest.raises(ValueError):
        eng.cc_shell(lab_dev, 2, raw_dev.view(torch.uint8))
    with pytest.raises(ValueError):
        eng.cc_shell(lab_dev.view(torch.float32), 2, raw_dev)
    with pytest.raises(ValueError):
        eng.cc_shell(lab_dev.reshape(-1), 2, raw_dev)
    with pytest.raises(ValueError):
        eng.cc_shell(lab_dev.transpose(1, 2), 2, None)  # (not contiguous)
    with pytest.raises(ValueError):
        eng.cc_shell(lab_dev, 2, raw_dev.transpose(1, 2))
    with pytest.raises(ValueError):
        eng.cc_shell(lab_dev.cpu(), 2, raw_dev)
    with pytest.raises(ValueError):
        eng.cc_shell(lab_dev, 2, raw_dev.cpu())
    # the C entry point
    nvox = labels.size
    buf = torch.full((3 * nvox,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    lp, rp = C.c_void_p(lab_dev.data_ptr()), C.c_void_p(raw_dev.data_ptr())
    at = lambda off: C.c_void_p(buf.data_ptr() + 4 * off)  # noqa: E731
    call, err = eng.lib.dlv_cc_shell_dev, lambda: eng.lib.dlv_last_error(eng.ctx).decode()  # noqa: E731
    geom = (24, 40, 72, 72, 40 * 72)
    refused = [
        ((lp, rp, *geom, 0, at(0), at(nvox)), "radius"), ((lp, rp, *geom, 17, at(0), at(nvox)), "radius"),
        ((lp, rp, *geom, 2, at(0), None), "scratch_dev"), ((lp, rp, *geom, 2, None, at(nvox)), "shell_dev"),
        ((None, rp, *geom, 2, at(0), at(nvox)), "labels_dev"),
        ((lp, rp, 24, 0, 72, 72, 40 * 72, 2, at(0), at(nvox)), "empty"),
        ((lp, rp, 24, 40, 72, 71, 40 * 72, 2, at(0), at(nvox)), "pitches"), ((lp, rp, 24, 40, 72, 72, 40 * 72 - 1, 2, at(0), at(nvox)), "pitches"),
        ((lp, C.c_void_p(raw_dev.data_ptr() + 1), *geom, 2, at(0), at(nvox)), "aligned"),
        ((lp, rp, *geom, 2, C.c_void_p(buf.data_ptr() + 2), at(nvox)), "aligned"),
        # aliasing: the message names the argument
        ((lp, rp, *geom, 2, lp, at(nvox)), "shell_dev overlaps labels_dev"),
        ((lp, rp, *geom, 2, at(0), lp), "scratch_dev overlaps labels_dev"),
        ((lp, rp, *geom, 2, at(0), at(0)), "scratch_dev overlaps shell_dev"),
        ((lp, rp, *geom, 2, at(0), at(nvox - 1)), "scratch_dev overlaps shell_dev"),  # by one voxel
        ((at(1), rp, *geom, 1, at(nvox), None), "shell_dev overlaps labels_dev"),     # the labels' last voxel is the shell's first
    ]
    for args, word in refused:
        assert call(eng.ctx, *args) == _lib.DLV_EINVAL, word
        assert word in err(), (word, err())
    eng.sync()
    assert (buf == 0x5A5A5A5A).all().item()  # refused: nothing written
    # ... and what is allowed: volumes that touch without overlapping, a NULL scratch with radius 1, a NULL raw
    assert call(eng.ctx, lp, rp, *geom, 2, at(0), at(nvox)) == 0
    assert call(eng.ctx, lp, None, 24, 40, 72, 0, 0, 1, at(2 * nvox), None) == 0
    eng.sync()
    got = buf.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got[:nvox].reshape(labels.shape), _shell(labels, raw, 2))
    np.testing.assert_array_equal(got[2 * nvox:].reshape(labels.shape), _shell(labels, None, 1))


# ---- 9. count_blobs end to end -----------------------------------------------------------------------------------------------
STD_KEYS = {"voxel_counts", "bounding_boxes", "centroids"}
INTENSITY_KEYS = set(KEYS) | {"intensity_mean"}
ALL_KEYS = STD_KEYS | INTENSITY_KEYS | set(SHELL_KEYS) | {"shell_radius"}


def _brain_on_disk(tmp_path, mask, raw):
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


def _check_outputs(post, shape, raw, n, r):
    """pickle, table and last_intensity of a run with the key on against numpy on the label file the run wrote and the raw file"""
    from delivr_cfos_amd.count_blobs import count_blobs

    labels = np.load(os.path.join(post, f"brain-{n}-cc3d.npy")).astype(np.uint32)
    view = raw[:shape[0], :shape[1], :shape[2]]
    ref = _finished_shell(labels, view, n, r)
    stats = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(stats) == ALL_KEYS
    assert stats["shell_radius"] == r and type(stats["shell_radius"]) is int
    _assert_same(stats, ref, SHELL_KEYS)
    assert [stats[k].dtype for k in SHELL_KEYS] == [np.uint32, np.uint64, np.uint64, np.uint16, np.uint16, np.float64, np.float64]
    assert all(len(stats[k]) == n + 1 and stats[k][0] == 0 for k in SHELL_KEYS)
    has = stats["shell_voxels"] > 0
    np.testing.assert_array_equal(stats["shell_mean"][has], stats["shell_sum"][has].astype(np.float64) / stats["shell_voxels"][has].astype(np.float64))
    np.testing.assert_array_equal(stats["contrast"][has], stats["intensity_mean"][has] / stats["shell_mean"][has])
    assert not stats["shell_mean"][~has].any() and not stats["contrast"][~has].any() and has.any() and (stats["shell_mean"][has] > 0).all()
    lines = _read(post, os.path.join("cell_intensity", "brain.csv")).decode().splitlines()
    assert lines[0] == "Blob,Size,Min,Max,Sum,SumSq,Mean,ShellSize,ShellMin,ShellMax,ShellSum,ShellSumSq,ShellMean,Contrast" and len(lines) == n + 1
    for i in (1, n // 2, n):
        assert lines[i] == (f"{i},{int(stats['voxel_counts'][i])},{int(stats['intensity_min'][i])},{int(stats['intensity_max'][i])},"
                            f"{int(stats['intensity_sum'][i])},{int(stats['intensity_sumsq'][i])},{float(stats['intensity_mean'][i])!r},"
                            f"{int(ref['shell_voxels'][i])},{int(ref['shell_min'][i])},{int(ref['shell_max'][i])},{int(ref['shell_sum'][i])},"
                            f"{int(ref['shell_sumsq'][i])},{float(ref['shell_mean'][i])!r},{float(ref['contrast'][i])!r}")
    assert sorted(os.listdir(post)) == sorted([f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle", "cell_intensity"])
    assert count_blobs.last_intensity["n"] == n and count_blobs.last_intensity["shell_radius"] == r
    return stats, labels


@pytest.fixture(scope="module")
def brain():
    rng = np.random.default_rng(12)
    mask = (rng.random((40, 64, 72)) < 0.02).astype(np.uint8)
    raw = rng.integers(0, 65536, size=(48, 64, 96), dtype=np.uint16)
    raw[rng.random(raw.shape) < 0.2] = 0
    mask.setflags(write=False)
    raw.setflags(write=False)
    return mask, raw


def test_count_blobs_key_on_adds_keys_and_columns_and_key_off_changes_nothing(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, raw)
    stack = (1, 1) + mask.shape
    on = str(tmp_path / "on")
    n = count_blobs(_settings(path_in, on, intensity_stats=True, background_shell=2), path_in, 0, "brain", stack, engine=eng)
    stats_on, _ = _check_outputs(on, mask.shape, raw, n, 2)
    # off: absent, 0 and false - with intensity_stats on every file is byte for byte that of a run without the key
    base = str(tmp_path / "base")
    assert count_blobs(_settings(path_in, base, intensity_stats=True), path_in, 0, "brain", stack, engine=eng) == n
    assert set(count_blobs.last_intensity) == {"n", "raw_file"}
    names = [f"{mask.shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle", os.path.join("cell_intensity", "brain.csv")]
    for tag, value in (("zero", 0), ("false", False)):
        off = str(tmp_path / tag)
        assert count_blobs(_settings(path_in, off, intensity_stats=True, background_shell=value), path_in, 0, "brain", stack, engine=eng) == n
        assert set(count_blobs.last_intensity) == {"n", "raw_file"}
        assert sorted(os.listdir(off)) == sorted(os.listdir(base)) and os.listdir(os.path.join(off, "cell_intensity")) == ["brain.csv"]
        for name in names:
            assert _read(off, name) == _read(base, name), name
    stats_off = pickle.loads(_read(base, "brain-stats.pickle"))
    assert set(stats_off) == STD_KEYS | INTENSITY_KEYS and not any(k.startswith("shell") or k == "contrast" for k in stats_off)
    # ... and the key changes nothing else: labels, the reference's CSV, the other entries, the first seven columns
    for name in names[:2]:
        assert _read(on, name) == _read(base, name), name
    for k in stats_off:
        assert stats_on[k].dtype == stats_off[k].dtype
        np.testing.assert_array_equal(stats_on[k], stats_off[k])
    plain = _read(base, names[3]).decode().splitlines()
    assert [l.split(",")[:7] for l in _read(on, names[3]).decode().splitlines()] == [l.split(",") for l in plain]
    # without intensity_stats: ValueError before any file exists
    none = str(tmp_path / "none")
    with pytest.raises(ValueError, match="intensity_stats"):
        count_blobs(_settings(path_in, none, background_shell=2), path_in, 0, "brain", stack, engine=eng)
    with pytest.raises(ValueError, match="background_shell"):
        count_blobs(_settings(path_in, none, intensity_stats=True, background_shell=17), path_in, 0, "brain", stack, engine=eng)
    assert not os.path.exists(none)


def test_count_blobs_with_the_size_filter_takes_the_shell_on_the_filtered_labels(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, raw)
    post, plain = str(tmp_path / "post"), str(tmp_path / "plain")
    stack = (1, 1) + mask.shape
    n = count_blobs(_settings(path_in, post, intensity_stats=True, background_shell=2, size_filter=True), path_in, 0, "brain", stack, 2, 20,
                    engine=eng)
    assert count_blobs.last_filter["n_kept"] == n and 1 < n < count_blobs.last_filter["n_before"]
    _, kept = _check_outputs(post, mask.shape, raw, n, 2)
    # a removed component's voxels are plain background: some are shell of a neighbour
    n_all = count_blobs(_settings(path_in, plain), path_in, 0, "brain", stack, engine=eng)
    removed = (np.load(os.path.join(plain, f"brain-{n_all}-cc3d.npy")) != 0) & (kept == 0)
    assert removed.any() and (_shell(kept, raw[:40, :64, :72], 2)[removed] != 0).any()


def test_count_blobs_on_cached_labels_completes_a_cached_pickle(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, raw)
    post = str(tmp_path / "post")
    stack = (1, 1) + mask.shape
    n = count_blobs(_settings(path_in, post, intensity_stats=True), path_in, 0, "brain", stack, engine=eng)
    label_bytes = _read(post, f"brain-{n}-cc3d.npy")
    before = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(before) == STD_KEYS | INTENSITY_KEYS
    before["note"] = "kept"  # an entry of the user's
    with open(os.path.join(post, "brain-stats.pickle"), "wb") as fh:
        pickle.dump(before, fh)
    # a cached pickle without the shell keys, then one with another radius: both measured again and rewritten
    for r in (3, 1):
        assert count_blobs(_settings(path_in, post, intensity_stats=True, background_shell=r), path_in, 0, "brain", stack, engine=eng) == n
        assert "intensity_s" in count_blobs.last_timings
        stats = pickle.loads(_read(post, "brain-stats.pickle"))
        assert stats.pop("note") == "kept"
        with open(os.path.join(post, "brain-stats.pickle"), "wb") as fh:
            pickle.dump(stats, fh)
        _check_outputs(post, mask.shape, raw, n, r)
        for k in STD_KEYS | INTENSITY_KEYS:
            assert stats[k].dtype == before[k].dtype
            np.testing.assert_array_equal(stats[k], before[k])
        stats["note"] = "kept"
        with open(os.path.join(post, "brain-stats.pickle"), "wb") as fh:
            pickle.dump(stats, fh)
    assert _read(post, f"brain-{n}-cc3d.npy") == label_bytes
    # the same radius again: complete - nothing is measured, the pickle keeps its bytes
    pickle_bytes = _read(post, "brain-stats.pickle")
    assert count_blobs(_settings(path_in, post, intensity_stats=True, background_shell=1), path_in, 0, "brain", stack, engine=eng) == n
    assert _read(post, "brain-stats.pickle") == pickle_bytes and "intensity_s" not in count_blobs.last_timings
    assert count_blobs.last_intensity["shell_radius"] == 1
    # a cached pickle without any intensity key: cells and shells from one pass
    with open(os.path.join(post, "brain-stats.pickle"), "wb") as fh:
        pickle.dump({k: before[k] for k in STD_KEYS}, fh)
    assert count_blobs(_settings(path_in, post, intensity_stats=True, background_shell=2), path_in, 0, "brain", stack, engine=eng) == n
    _check_outputs(post, mask.shape, raw, n, 2)


def test_budget_refusals_write_no_file(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.streaming import ccl_bytes_per_voxel

    mask, raw = brain
    path_in = _brain_on_disk(tmp_path, mask, raw)
    post = str(tmp_path / "post")
    os.makedirs(post)
    open(os.path.join(post, "kept.txt"), "w").close()
    stack = (1, 1) + mask.shape
    per_voxel = ccl_bytes_per_voxel() + 2
    gb = lambda bpv: mask.size * bpv / 2**30  # noqa: E731
    # enough for the cells' statistics, not for the shell volume (radius 1: 4 bytes more) / the scratch volume (radius 2: 8 more)
    for r, budget in ((1, gb(per_voxel + 3)), (2, gb(per_voxel + 7))):
        with pytest.raises(MemoryError, match=r"background_shell.*hbm_budget_gb"):
            count_blobs(_settings(path_in, post, intensity_stats=True, background_shell=r, hbm_budget_gb=budget), path_in, 0, "brain", stack, engine=eng)
        assert os.listdir(post) == ["kept.txt"]
    # a budget under which the mask would be slab-streamed: refused like intensity_stats itself
    with pytest.raises(MemoryError, match=r"slab-streamed"):
        count_blobs(_settings(path_in, post, intensity_stats=True, background_shell=2, hbm_budget_gb=1e-4), path_in, 0, "brain", stack, engine=eng)
    assert os.listdir(post) == ["kept.txt"] and count_blobs.last_intensity is None
    # ... and the budgets that just fit do run (radius 1 in the room radius 2 lacks)
    out = str(tmp_path / "fits")
    n = count_blobs(_settings(path_in, out, intensity_stats=True, background_shell=1, hbm_budget_gb=gb(per_voxel + 7)), path_in, 0, "brain", stack,
                    engine=eng)
    _check_outputs(out, mask.shape, raw, n, 1)


# ---- 10. sharded -----------------------------------------------------------------------------------------------------------
def _sharded_volume():
    """45 x 40 x 56 (the size-filter tests' volume): components across the seams of two and three even slabs"""
    rng = np.random.default_rng(13)
    m = (rng.random((45, 40, 56)) < 0.02).astype(np.uint8)
    m[:, 18:23, 28:33] = 0
    m[10:24, 20, 30] = 1
    m[29:31, 20, 30] = 1
    raw = rng.integers(0, 4, size=(48, 48, 64), dtype=np.uint16) * 9000
    return m, raw


@pytest.mark.parametrize("world", [2, 3])
def test_count_blobs_under_torch_distributed_equals_the_single_engine_result(eng, tmp_path, monkeypatch, world):
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs

    ranks = _helper("thread_ranks")
    m, raw = _sharded_volume()
    path_in = _brain_on_disk(tmp_path, m, raw)
    stack = (1, 1) + m.shape
    single = str(tmp_path / "single")
    n = count_blobs(_settings(path_in, single, intensity_stats=True, background_shell=3), path_in, 0, "brain", stack, engine=eng)
    ref, _ = _check_outputs(single, m.shape, raw, n, 3)
    fake = ranks.ThreadRanks(world)
    fake.patch(monkeypatch, dist)
    post = str(tmp_path / "sharded")
    settings = _settings(path_in, post, intensity_stats=True, background_shell=3)
    results = ranks.run_thread_ranks(fake, lambda rank, e: count_blobs(settings, path_in, 0, "brain", stack, engine=e))  # (joins with a time limit)
    assert results == [n] * world
    stats, _ = _check_outputs(post, m.shape, raw, n, 3)
    for key in ALL_KEYS - {"shell_radius"}:
        np.testing.assert_array_equal(stats[key], ref[key], err_msg=key)
    for name in (f"{m.shape}_brain.csv", os.path.join("cell_intensity", "brain.csv")):
        assert _read(post, name) == _read(single, name), name


def test_slabs_thinner_than_the_radius_raise_the_same_error_on_every_rank(eng, tmp_path, monkeypatch):
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs

    ranks = _helper("thread_ranks")
    m, raw = _sharded_volume()
    path_in = _brain_on_disk(tmp_path, m, raw)
    post = str(tmp_path / "post")
    fake = ranks.ThreadRanks(3)  # slabs of 15 planes under a radius of 16
    fake.patch(monkeypatch, dist)
    settings = _settings(path_in, post, intensity_stats=True, background_shell=16)
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
    assert len({str(c) for c in caught}) == 1 and "slabs of 15" in str(caught[0]) and "background_shell" in str(caught[0])
    assert not os.path.exists(post)
