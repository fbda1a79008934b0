"""The neighbour table of a label volume on the device (dlv_cc_neighbours_count_dev / dlv_cc_neighbours_dev,
HipEngine.cc_neighbours; settings["mi355x"]["neighbour_stats"] in count_blobs).

The reference of every case is tests/helpers/neighbour_reference.py - every offset of the full box, both signs, none of the kernel's
prunings -, pinned against an all-voxel-pairs brute force in tests/test_neighbours_cpu.py.  Pairs and gaps are integers: equality,
no tolerance.

A workgroup owns a tile of 8 x 8 x 32 voxels (csrc/cc_neighbours.hip) and stages up to 8 more planes behind it and up to 8 rows /
voxels on either side: the shapes cover one tile and several with an odd remainder on every axis, the hand-made pairs every tile
boundary."""
import ctypes as C
import importlib.util
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = (8, 8, 32)  # NTZ, NTY, NTX of csrc/cc_neighbours.hip
# per spacing: squared radii with a reach of 0 on an axis, of 1, of 8, and in between (the reach is floor(sqrt(R2) / w), at most 8)
CASES = (((1, 1, 1), (1, 3, 64)),           # reaches 1, 1 (the corners too), 8
         ((3, 1, 1), (8, 64)),              # (0, 2, 2), (2, 8, 8)
         ((37, 10, 10), (100, 1569, 6400)),  # (0, 1, 1), (1, 3, 3), (2, 8, 8)
         ((1, 2, 64), (1, 16, 64)))         # (1, 0, 0), (4, 2, 0), (8, 4, 0)


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("neighbour_reference")


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def _dev(labels):
    import torch

    return torch.from_numpy(np.ascontiguousarray(labels).view(np.int32).copy()).cuda()


def _check(eng, labels, n, spacing, radius_sq):
    """HipEngine.cc_neighbours against the reference; the labels are not written -> the reference's {(a, b): gap2}"""
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    dev = _dev(labels)
    got = eng.cc_neighbours(dev, n, spacing, radius_sq)
    want = ref.neighbour_table(labels, n, spacing, radius_sq)
    ref.assert_table_equal(got, want)
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), labels)
    return want


def _touching_cells(eng, shape, density, seed):
    """a random mask labelled by ccl26; every fifth x-column of each component goes to a second label l + n: touching cells
    (the construction of tests/test_gpu_depth.py) -> (labels, n of the labelling: the labels present are 1..2n)"""
    import torch

    rng = np.random.default_rng(seed)
    mask = (rng.random(shape) < density).astype(np.uint8)
    lab, n = eng.ccl26(torch.from_numpy(mask).cuda())
    labels = lab.cpu().numpy().view(np.uint32).copy()
    cols = np.zeros(shape, dtype=bool)
    cols[..., ::5] = True
    labels[cols & (labels > 0)] += np.uint32(n)
    return labels, n


# ---- 1. random masks ---------------------------------------------------------------------------------------------------------------
# (9, 13, 67): an odd X above two tiles; (17, 9, 8): three tiles in z; one plane; a row shorter than a quad; a y axis longer than X;
# (19, 21, 141): more than two tiles with an odd remainder on every axis.  With a reach of 8 the small ones are shorter than the reach.
SHAPES = [(9, 13, 67), (17, 9, 8), (1, 9, 9), (5, 1, 3), (3, 70, 5), (19, 21, 141)]


# seeds for which the reference alone finds at least two components, a pair, and (but for the 15 voxels of (5, 1, 3)) a pair at every
# spacing's largest radius and one exactly at a radius
SPARSE_SEEDS = {(9, 13, 67): 1, (17, 9, 8): 1, (1, 9, 9): 7, (5, 1, 3): 9, (3, 70, 5): 1, (19, 21, 141): 1}


@pytest.mark.parametrize("shape", SHAPES)
def test_sparse_random_masks(eng, shape):
    """density 0.03 - 0.05: separate cells with background between them"""
    labels, n = _touching_cells(eng, shape, 0.05 if np.prod(shape) < 2000 else 0.03, seed=SPARSE_SEEDS[shape])
    assert n >= 2
    n *= 2
    pairs, at_radius = 0, 0
    for spacing, radii in CASES:
        for radius_sq in radii:
            want = _check(eng, labels, n, spacing, radius_sq)
            pairs += len(want)
            at_radius += sum(g == radius_sq for g in want.values())
    assert pairs > 0
    assert at_radius > 0 or shape == (5, 1, 3)  # a pair exactly at the radius: included


@pytest.mark.parametrize("density", [0.3, 0.6])
@pytest.mark.parametrize("shape", SHAPES[:5])
def test_dense_random_masks_with_touching_cells(eng, shape, density):
    labels, n = _touching_cells(eng, shape, density, seed=2 if shape == (5, 1, 3) else 1)  # (seeds with a touching pair in the reference)
    assert n >= 1 and int(labels.max()) > n  # both halves are there
    touching = 0
    for spacing, radii in CASES:
        for radius_sq in radii:
            want = _check(eng, labels, 2 * n, spacing, radius_sq)
            touching += sum(g == min(spacing) ** 2 for g in want.values())
            # with n of the labelling alone the second halves are labels above n: they contribute nothing and block nothing
            if radius_sq == radii[-1]:
                _check(eng, labels, n, spacing, radius_sq)
    assert touching > 0  # two halves of a component share a face


# ---- 2. hand-made boundary cases ---------------------------------------------------------------------------------------------------
def _two_voxels(shape, v, u):
    lab = np.zeros(shape, dtype=np.uint32)
    lab[v], lab[u] = 1, 2
    return lab


def test_a_pair_exactly_at_the_radius_and_one_step_further(eng):
    shape = (12, 20, 40)
    for spacing, radius_sq, v, u, further in (((1, 1, 1), 9, (2, 2, 2), (2, 2, 5), (2, 2, 6)),
                                              ((1, 1, 1), 64, (1, 3, 4), (9, 3, 4), (10, 3, 4)),
                                              ((1, 1, 1), 29, (4, 9, 20), (6, 12, 16), (6, 12, 15)),  # 4 + 9 + 16
                                              ((37, 10, 10), 1569, (3, 5, 5), (4, 6, 4), (4, 6, 3)),  # 1369 + 100 + 100
                                              ((3, 1, 1), 64, (2, 10, 10), (4, 15, 11), (4, 16, 11)),  # 36 + 25 + 1 = 62, 36 + 36 + 1 = 73
                                              ((1, 2, 64), 64, (0, 6, 7), (0, 10, 7), (0, 10, 8))):  # no reach along x
        w = np.array(spacing)
        d2 = int((((np.array(u) - np.array(v)) * w) ** 2).sum())
        assert d2 <= radius_sq < int((((np.array(further) - np.array(v)) * w) ** 2).sum())
        assert _check(eng, _two_voxels(shape, v, u), 2, spacing, radius_sq) == {(1, 2): d2}
        assert _check(eng, _two_voxels(shape, u, v), 2, spacing, radius_sq) == {(1, 2): d2}  # the later voxel holds the smaller label
        assert _check(eng, _two_voxels(shape, v, further), 2, spacing, radius_sq) == {}
    assert _check(eng, _two_voxels(shape, (2, 2, 2), (2, 2, 5)), 2, (1, 1, 1), 8) == {}  # 9 > 8


def test_pairs_across_every_tile_boundary(eng):
    tz, ty, tx = TILE
    shape = (2 * tz + 1, 2 * ty + 1, 2 * tx + 6)
    last = (tz - 1, ty - 1, tx - 1)  # the last voxel of the first tile
    cases = [((1, 0, 0), 1), ((0, 1, 0), 1), ((0, 0, 1), 1), ((1, 1, 1), 3),  # across a face in z, y, x; across the corner
             ((1, -1, 0), 2), ((1, 0, -1), 2), ((0, 1, -1), 2), ((1, -1, -1), 3), ((1, 1, -1), 3), ((1, -1, 1), 3)]
    for step, d2 in cases:
        # ... from the last voxel of a tile, or ending on the first voxel of the next one
        v = tuple(l if s >= 0 else l + 1 for l, s in zip(last, step))
        u = tuple(a + s for a, s in zip(v, step))
        assert _check(eng, _two_voxels(shape, v, u), 2, (1, 1, 1), 3) == {(1, 2): d2}, step
        assert _check(eng, _two_voxels(shape, u, v), 2, (1, 1, 1), 3) == {(1, 2): d2}, step
    # far apart, the pair's box covering the corner where eight tiles meet: the halo in all three directions
    v, u = (tz - 3, ty - 2, tx - 3), (tz + 1, ty + 2, tx + 2)
    assert _check(eng, _two_voxels(shape, v, u), 2, (1, 1, 1), 57) == {(1, 2): 16 + 16 + 25}
    assert _check(eng, _two_voxels(shape, v, u), 2, (1, 1, 1), 56) == {}
    # from the first voxel of the second tile to the first of the third, eight voxels along each axis in turn (the whole halo)
    for axis in range(3):
        v = [2, 3, 5]
        v[axis] = 2 * TILE[axis] - 8
        u = list(v)
        u[axis] += 8
        assert _check(eng, _two_voxels(shape, tuple(v), tuple(u)), 2, (1, 1, 1), 64) == {(1, 2): 64}, axis


def test_pairs_found_only_through_a_negative_dy_or_dx_with_a_positive_dz(eng):
    shape = (10, 20, 45)
    for v, u in (((3, 9, 40), (5, 6, 36)), ((3, 9, 20), (4, 2, 20)), ((0, 0, 44), (8, 0, 44)), ((2, 12, 36), (3, 12, 29)),
                 ((7, 8, 32), (8, 7, 31)), ((1, 19, 44), (2, 13, 40))):
        d2 = int(((np.array(u) - np.array(v)) ** 2).sum())
        assert 0 < d2 <= 65
        assert _check(eng, _two_voxels(shape, v, u), 2, (1, 1, 1), 65) == {(1, 2): d2}
    # a cell whose only voxel near the other lies behind and below it: rods that cross at a distance
    lab = np.zeros(shape, dtype=np.uint32)
    lab[2, 15, 5:40] = 1
    lab[4:9, 11, 38] = 2
    assert _check(eng, lab, 2, (1, 1, 1), 64) == {(1, 2): 4 + 16}
    assert _check(eng, lab, 2, (3, 1, 1), 64) == {(1, 2): 36 + 16}


def test_cells_on_the_faces_and_corners_of_the_volume(eng):
    shape = (6, 9, 8)
    lab = np.zeros(shape, dtype=np.uint32)
    corners = [(z, y, x) for z in (0, 5) for y in (0, 8) for x in (0, 7)]
    for i, c in enumerate(corners, 1):
        lab[c] = i
    lab[3, 4, 0], lab[0, 4, 4], lab[3, 0, 4], lab[5, 4, 3], lab[2, 8, 4], lab[3, 5, 7] = 9, 10, 11, 12, 13, 14  # one on every face
    want = _check(eng, lab, 14, (1, 1, 1), 64)
    assert want[(1, 2)] == 49 and want[(1, 5)] == 25 and want[(1, 3)] == 64 and (1, 8) not in want and len(want) > 20
    _check(eng, lab, 14, (2, 1, 1), 70)
    # a volume of one voxel, and of one row
    assert _check(eng, np.ones((1, 1, 1), np.uint32), 1, (1, 1, 1), 64) == {}
    assert _check(eng, np.array([[[1, 0, 0, 2, 2, 3]]], np.uint32), 3, (1, 1, 1), 9) == {(1, 2): 9, (2, 3): 1}


def test_a_label_above_n_between_two_cells_is_ignored(eng):
    lab = np.zeros((5, 12, 40), dtype=np.uint32)
    lab[2, 5, 10:13] = 1
    lab[2, 5, 13:17] = 7  # between the two, touching both
    lab[2, 5, 17:20] = 2
    lab[3, 5, 10:20] = 0xFFFFFFFF  # and the largest uint32 beside them
    assert _check(eng, lab, 2, (1, 1, 1), 25) == {(1, 2): 25}
    assert _check(eng, lab, 2, (1, 1, 1), 24) == {}
    assert _check(eng, lab, 7, (1, 1, 1), 25) == {(1, 2): 25, (1, 7): 1, (2, 7): 1}
    assert _check(eng, lab, 1, (1, 1, 1), 25) == {}
    assert _check(eng, lab, 0, (1, 1, 1), 25) == {}


# ---- 3. skew ---------------------------------------------------------------------------------------------------------------------------
def test_one_large_cell_surrounded_by_many_small_ones(eng):
    """one hot partner, and many keys out of one tile"""
    lab = np.zeros((20, 24, 70), dtype=np.uint32)
    lab[6:14, 6:18, 10:60] = 1
    n = 1
    for z in range(2, 20, 3):
        for y in range(1, 24, 3):
            for x in range(3, 70, 3):
                if lab[z, y, x] == 0 and not lab[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].any():
                    n += 1
                    lab[z, y, x] = n
    assert n > 300
    want = _check(eng, lab, n, (1, 1, 1), 9)
    assert sum(1 for a, _ in want if a == 1) > 100 and len(want) > 1000
    _check(eng, lab, n, (2, 1, 3), 36)


def test_cells_without_a_pair(eng):
    lab = np.zeros((12, 30, 70), dtype=np.uint32)
    lab[1, 1, 1], lab[10, 28, 68], lab[1, 28, 30] = 1, 2, 3
    dev = _dev(lab)
    got = eng.cc_neighbours(dev, 3, (1, 1, 1), 64)
    assert got["segments"] == 0 and all(got[k].shape == (0,) and got[k].dtype == np.uint32 for k in ("a", "b", "gap_sq"))
    ref.assert_table_equal(got, {})
    assert ref.neighbour_table(lab, 3, (1, 1, 1), 64) == {}


# ---- 4. the C entries called directly ----------------------------------------------------------------------------------------------
def _count(eng, lp, shape, n, spacing, r2, out=True):
    s = C.c_uint64(7)
    rc = eng.lib.dlv_cc_neighbours_count_dev(eng.ctx, lp, *shape, n, *spacing, r2, C.byref(s) if out else None)
    return rc, s.value


def _table(eng, lp, shape, n, spacing, r2, S, tp, cap, kp, gp, out_cap, out=True):
    p = C.c_uint64(7)
    rc = eng.lib.dlv_cc_neighbours_dev(eng.ctx, lp, *shape, n, *spacing, r2, S, tp, cap, kp, gp, out_cap, C.byref(p) if out else None)
    return rc, p.value


def _pairs_of(keys, gaps, P):
    k = keys[:P].cpu().numpy().view(np.uint64)
    g = gaps[:P].cpu().numpy().view(np.uint32)
    return {(int(v >> np.uint64(32)), int(v & np.uint64(0xFFFFFFFF))): int(d) for v, d in zip(k, g)}


def test_the_smallest_legal_table_and_refused_arguments(eng):
    import torch
    from delivr_cfos_amd import _lib

    labels, n = _touching_cells(eng, (9, 13, 67), 0.3, seed=8)
    n *= 2
    shape, one, r2 = labels.shape, (1, 1, 1), 9
    want = ref.neighbour_table(labels, n, one, r2)
    assert len(want) > 8
    dev = _dev(labels)
    lp = C.c_void_p(dev.data_ptr())
    rc, S = _count(eng, lp, shape, n, one, r2)
    assert rc == 0 and S >= len(want)
    bound = min(S, n * (n - 1) // 2)
    cap = 1 << (2 * bound - 1).bit_length()
    FILL = 0x55555555
    buf = torch.full((4 * cap + 8 + 2 * bound + 2 + bound + 2,), FILL, dtype=torch.int32, device="cuda")
    table, keys, gaps = buf[:4 * cap], buf[4 * cap + 4:4 * cap + 4 + 2 * bound], buf[4 * cap + 8 + 2 * bound:4 * cap + 8 + 3 * bound]
    assert table.data_ptr() % 16 == 0 and keys.data_ptr() % 8 == 0
    tp, kp, gp = (C.c_void_p(t.data_ptr()) for t in (table, keys, gaps))
    good = (lp, shape, n, one, r2, S, tp, cap, kp, gp, bound)

    # the smallest legal table holds the same pairs, and so does a larger one with S overstated
    rc, P = _table(eng, *good)
    assert rc == 0 and P == len(want) and _pairs_of(keys.view(torch.int64), gaps, P) == want
    assert bool((gaps[P:] == FILL).all()) and bool((buf[4 * cap:4 * cap + 4] == FILL).all())  # nothing beyond the P entries
    big = torch.full((8 * cap,), -1, dtype=torch.int32, device="cuda")  # (garbage in the table: the call clears it)
    rc, P2 = _table(eng, lp, shape, n, one, r2, S, C.c_void_p(big.data_ptr()), 2 * cap, kp, gp, bound)
    assert rc == 0 and P2 == P and _pairs_of(keys.view(torch.int64), gaps, P) == want
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), labels)
    buf.fill_(FILL)

    def refused(code, *args, word=None, out=True):
        rc, P = _table(eng, *args, out=out)
        msg = eng.lib.dlv_last_error(eng.ctx).decode()
        assert rc == code, (rc, msg)
        assert P == 7  # not written
        assert bool((buf == FILL).all())  # nor the table, nor the outputs
        if word is not None:
            assert msg.startswith("cc_neighbours") and word in msg, msg
        return msg

    def but(**kw):
        names = ("lp", "shape", "n", "spacing", "r2", "S", "tp", "cap", "kp", "gp", "out_cap")
        return tuple(kw.get(k, v) for k, v in zip(names, good))

    E, U = _lib.DLV_EINVAL, _lib.DLV_EUNSUP
    for null in ("lp", "tp", "kp", "gp"):
        refused(E, *but(**{null: None}))
    refused(E, *good, out=False)
    refused(E, *but(lp=C.c_void_p(dev.data_ptr() + 2)), word="aligned")
    refused(E, *but(tp=C.c_void_p(table.data_ptr() + 8)), word="aligned")
    refused(E, *but(kp=C.c_void_p(keys.data_ptr() + 4)), word="aligned")
    refused(E, *but(gp=C.c_void_p(gaps.data_ptr() + 2)), word="aligned")
    for bad in ((0, 13, 67), (9, 0, 67), (9, 13, 0), (-1, 13, 67)):
        refused(E, *but(shape=bad), word="empty volume")
    for spacing in ((0, 1, 1), (1, 65, 1), (1, 1, 0), (65, 1, 1), (1, 1, -3)):
        refused(E, *but(spacing=spacing), word="spacing")
    refused(E, *but(r2=0), word="r2")
    refused(E, *but(n=2**32 - 1), word="uint32 labels")
    refused(E, *but(cap=cap // 2), word="power of two")
    refused(E, *but(cap=cap + 1), word="power of two")
    refused(E, *but(cap=0), word="power of two")
    refused(E, *but(out_cap=bound - 1), word="outputs")
    # the reach rule names the axis, the reach and the limit
    assert "axis z" in refused(U, *but(r2=81), word="reaches 9 voxels")
    assert "axis y" in refused(U, *but(r2=81, spacing=(2, 1, 2)), word="at most 8")
    assert "axis x" in refused(U, *but(r2=6400, spacing=(37, 10, 8)), word="reaches 10 voxels")
    refused(U, *but(r2=2**40), word="axis z")
    # beyond the launch grid, beyond the 32-bit x arithmetic (refused before anything is read)
    refused(E, *but(shape=(65536 * 8, 1, 1)), word="launch grid")
    refused(E, *but(shape=(1, 65536 * 8, 1)), word="launch grid")
    refused(U, *but(shape=(1, 1, 2**30 + 1)), word="X =")
    # the count refuses the same
    for args, code in (((None, shape, n, one, r2), E), ((C.c_void_p(dev.data_ptr() + 2), shape, n, one, r2), E), ((lp, (9, 0, 67), n, one, r2), E),
                       ((lp, shape, n, (1, 65, 1), r2), E), ((lp, shape, n, one, 0), E), ((lp, shape, 2**32 - 1, one, r2), E),
                       ((lp, shape, n, one, 81), U), ((lp, (65536 * 8, 1, 1), n, one, r2), E), ((lp, (1, 1, 2**30 + 1), n, one, r2), U)):
        rc, s = _count(eng, *args)
        assert rc == code and s == 7, (args, rc, eng.lib.dlv_last_error(eng.ctx).decode())
    assert _count(eng, lp, shape, n, one, r2, out=False)[0] == E
    # S = 0: nothing is launched, the smallest table there is will do; n < 2: no pair whatever the segments
    rc, P = _table(eng, *but(S=0, cap=1, out_cap=0))
    assert rc == 0 and P == 0 and bool((buf == FILL).all())
    rc, P = _table(eng, *but(n=1, cap=1, out_cap=0))
    assert rc == 0 and P == 0 and bool((buf == FILL).all())
    assert _count(eng, lp, shape, 1, one, r2) == (0, 0)
    # segments understated: the probes and the writes stay inside the table and the outputs, and the error names the table
    rc, P = _table(eng, *but(S=1, cap=2, out_cap=1))
    msg = eng.lib.dlv_last_error(eng.ctx).decode()
    assert rc == _lib.DLV_ESTATE and P == 7 and "pair table of 2 slots" in msg, (rc, msg)
    assert bool((buf[8:4 * cap + 4] == FILL).all()) and bool((keys[2:] == FILL).all()) and bool((gaps[1:] == FILL).all())
    buf.fill_(FILL)
    # the calls still work
    assert _count(eng, lp, shape, n, one, r2) == (0, S)
    rc, P = _table(eng, *good)
    assert rc == 0 and _pairs_of(keys.view(torch.int64), gaps, P) == want
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), labels)


def test_the_engine_refuses(eng):
    import torch

    labels, n = _touching_cells(eng, (9, 13, 67), 0.3, seed=8)
    dev = _dev(labels)
    for bad in ((1, 1), (1, 1, 1, 1), (0, 1, 1), (1, 1, 65), (1.0, 1, 1), (True, 1, 1), 1):
        with pytest.raises(ValueError, match="spacing"):
            eng.cc_neighbours(dev, n, bad, 4)
    for bad in (0, -4, 1.5, True, None, "4"):
        with pytest.raises(ValueError, match="radius_sq"):
            eng.cc_neighbours(dev, n, (1, 1, 1), bad)
    with pytest.raises(ValueError, match=r"radius_sq = 81.*reaches 9 voxels along z.*at most 8"):
        eng.cc_neighbours(dev, n, (1, 1, 1), 81)
    with pytest.raises(ValueError, match=r"reaches 9 voxels along x"):
        eng.cc_neighbours(dev, n, (37, 10, 9), 6600)
    with pytest.raises(ValueError):
        eng.cc_neighbours(dev, -1, (1, 1, 1), 4)
    with pytest.raises(ValueError):
        eng.cc_neighbours(dev.cpu(), n, (1, 1, 1), 4)
    with pytest.raises(ValueError):
        eng.cc_neighbours(labels, n, (1, 1, 1), 4)
    with pytest.raises(ValueError):
        eng.cc_neighbours(dev.to(torch.int64), n, (1, 1, 1), 4)
    with pytest.raises(ValueError):
        eng.cc_neighbours(dev.transpose(1, 2), n, (1, 1, 1), 4)  # (not contiguous)
    with pytest.raises(MemoryError, match=r"cc_neighbours needs a pair table of \d+ slots.*outputs of \d+ pairs.*hbm_budget_gb"):
        eng.cc_neighbours(dev, 2 * n, (1, 1, 1), 9, settings={"mi355x": {"hbm_budget_gb": 1e-8}})
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), labels)
    ref.assert_table_equal(eng.cc_neighbours(dev, 2 * n, (1, 1, 1), 9), ref.neighbour_table(labels, 2 * n, (1, 1, 1), 9))


# ---- 5. count_blobs end to end -----------------------------------------------------------------------------------------------------
STD_KEYS = {"voxel_counts", "bounding_boxes", "centroids"}
SPLIT_KEYS = {"split_parent", "split_siblings", "split_depth"}


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
    rng = np.random.default_rng(11)
    mask = (rng.random((24, 40, 72)) < 0.03).astype(np.uint8)
    mask[4:11, 10:18, 20:33] = 1
    mask[15:17, 30, 5:40] = 1
    mask[14:22, 2:9, 50:57] = 1  # two blocks joined by a neck: fused cells, siblings that touch after the split
    mask[17:19, 5:7, 57:60] = 1
    mask[14:22, 2:9, 60:67] = 1
    mask[0:3, 36:40, 68:72] = 1  # cut by three faces of the volume
    mask.setflags(write=False)
    return mask


def _check_outputs(post, shape, n, radius_sq, spacing, other_keys=frozenset(), other_entries=()):
    """pickle, both tables and last_neighbours of a run with the key against the reference on the label file the run wrote"""
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import NEIGHBOUR_KEYS, cell_neighbours_csv_text, cell_pairs_csv_text, neighbour_summary

    labels = np.load(os.path.join(post, f"brain-{n}-cc3d.npy")).astype(np.uint32)
    counts = np.bincount(labels.ravel(), minlength=n + 1).astype(np.uint32)
    pairs, gaps = ref.as_arrays(ref.neighbour_table(labels, n, spacing, radius_sq))
    want = {"neighbour_pairs": pairs, "neighbour_gap_sq": gaps, **neighbour_summary(pairs, gaps, n)}
    stats = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(stats) == STD_KEYS | set(NEIGHBOUR_KEYS) | set(other_keys)
    assert stats["neighbour_radius_sq"] == radius_sq and type(stats["neighbour_radius_sq"]) is int
    assert stats["neighbour_spacing"] == tuple(spacing) and type(stats["neighbour_spacing"]) is tuple
    for k, v in want.items():
        assert stats[k].dtype == np.uint32 and stats[k].shape == v.shape, k
        np.testing.assert_array_equal(stats[k], v, err_msg=k)
    assert all(stats[k].shape == (n + 1,) and stats[k][0] == 0 for k in ("neighbour_count", "nearest_gap_sq", "nearest_cell", "cluster_id", "cluster_size"))
    np.testing.assert_array_equal(stats["voxel_counts"], counts)
    assert _read(post, os.path.join("cell_neighbours", "brain.csv")).decode() == cell_neighbours_csv_text({**want, "voxel_counts": counts}, n)
    assert _read(post, os.path.join("cell_pairs", "brain.csv")).decode() == cell_pairs_csv_text(want)
    assert os.listdir(os.path.join(post, "cell_neighbours")) == ["brain.csv"] and os.listdir(os.path.join(post, "cell_pairs")) == ["brain.csv"]
    assert sorted(os.listdir(post)) == sorted([f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle", "cell_neighbours",
                                               "cell_pairs", *other_entries])
    sizes, ids = want["cluster_size"][1:], want["cluster_id"][1:]
    assert count_blobs.last_neighbours == {"n": n, "radius_sq": radius_sq, "spacing": tuple(spacing), "pairs": len(gaps),
                                           "clusters": len(set(ids[sizes >= 2].tolist())),
                                           "cells_without_neighbour": int((want["neighbour_count"][1:] == 0).sum())}
    assert len(gaps) > 0
    return stats


def test_count_blobs_with_the_key_and_without(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    path_in = _brain_on_disk(tmp_path, brain)
    shape = brain.shape
    stack = (1, 1) + shape
    on = str(tmp_path / "on")
    keys = dict(neighbour_stats=4.5, depth_spacing=[3, 1, 1], split_fused=2)  # R2 = floor(20.25) = 20: reaches 1, 4, 4
    n = count_blobs(_settings(path_in, on, **keys), path_in, 0, "brain", stack, engine=eng)
    assert count_blobs.last_split["components_split"] >= 1
    stats_on = _check_outputs(on, shape, n, 20, (3, 1, 1), SPLIT_KEYS)
    assert (stats_on["neighbour_gap_sq"] == 1).any()  # siblings of a split cell still touch
    assert (stats_on["neighbour_count"][1:] == 0).any() and (stats_on["cluster_size"] >= 3).any()  # lone cells, and a cluster worth the name
    assert "neighbours_s" in count_blobs.last_timings and count_blobs.last_depth is None
    # the same settings again: the cached pickle is complete, nothing is measured
    pickle_bytes = _read(on, "brain-stats.pickle")
    assert count_blobs(_settings(path_in, on, **keys), path_in, 0, "brain", stack, engine=eng) == n
    assert _read(on, "brain-stats.pickle") == pickle_bytes and "neighbours_s" not in count_blobs.last_timings
    _check_outputs(on, shape, n, 20, (3, 1, 1), SPLIT_KEYS)
    # another radius: measured again, on the cached labels
    assert count_blobs(_settings(path_in, on, neighbour_stats=2, depth_spacing=[3, 1, 1]), path_in, 0, "brain", stack, engine=eng) == n
    assert "neighbours_s" in count_blobs.last_timings
    _check_outputs(on, shape, n, 4, (3, 1, 1), SPLIT_KEYS)
    # without the key: no folder, no key in the pickle, every other file byte for byte what the run with the key wrote
    off, off0 = str(tmp_path / "off"), str(tmp_path / "off0")
    assert count_blobs(_settings(path_in, off, split_fused=2), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_neighbours is None and "neighbours_s" not in count_blobs.last_timings
    assert count_blobs(_settings(path_in, off0, split_fused=2, neighbour_stats=0), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_neighbours is None
    names = sorted([f"{shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle"])
    assert sorted(os.listdir(off)) == names and sorted(os.listdir(off0)) == names  # (no cell_neighbours, no cell_pairs)
    for name in names:
        assert _read(off, name) == _read(off0, name), name
    stats_off = pickle.loads(_read(off, "brain-stats.pickle"))
    assert set(stats_off) == STD_KEYS | SPLIT_KEYS
    for name in (f"brain-{n}-cc3d.npy", f"{shape}_brain.csv"):
        assert _read(on, name) == _read(off, name), name
    for k in STD_KEYS | (SPLIT_KEYS - {"split_depth"}):
        assert stats_on[k].dtype == stats_off[k].dtype
        np.testing.assert_array_equal(stats_on[k], stats_off[k])
    # a mask that would need the slab-streamed path is refused before anything is written
    fresh = str(tmp_path / "fresh")
    with pytest.raises(MemoryError, match=r"neighbour_stats.*slab-streamed labelling does not measure"):
        count_blobs(_settings(path_in, fresh, neighbour_stats=4, hbm_budget_gb=brain.size * 4 / 2**30), path_in, 0, "brain", stack, engine=eng)
    assert os.listdir(fresh) == []
