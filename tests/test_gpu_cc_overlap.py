"""The overlap table of two label volumes on the device (dlv_cc_overlap_count_dev / dlv_cc_overlap_dev, HipEngine.cc_overlap) and
compare_cells on top of it.

The reference of every case is tests/helpers/overlap_reference.py - a dictionary filled voxel by voxel, the summary and the per-cell
columns in plain Python, pinned on the host by tests/test_compare_cells_cpu.py - never the device's own output.  Integer work only:
every comparison is exact equality.  Every test asserts the property of its input that it is there for.

The kernels walk rows with one wave per row in sweeps of 512 voxels (csrc/cc_overlap.hip): a lane takes the quads [4l, 4l + 4) and
[256 + 4l, 256 + 4l + 4) of a sweep, a sweep of one pair goes to the wave's carry and any other one through the leader loop, and a
launch has at most 8192 workgroups (OVERLAP_MAX_WG)."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from delivr_cfos_amd import compare_cells as cc
from delivr_cfos_amd import label_runs as lr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_WORKGROUPS = 8192  # OVERLAP_MAX_WG of csrc/cc_overlap.hip
QUAD, HALF, SWEEP = 4, 256, 512  # voxels of a quad, of the lanes' first quads, of a sweep
BIG = 2**32 - 2  # the largest label


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("overlap_reference")


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


def _check(eng, a, b, n_a, n_b):
    """the device's table of (a, b) equals the dictionary loop's -> (pairs, segments) of the reference"""
    pairs, segments = ref.table(a, b, n_a, n_b)
    ref.assert_table_equal(eng.cc_overlap(_dev(a), n_a, _dev(b), n_b), pairs, segments)
    return pairs, segments


# ---- 1. boundaries of the sweep layout -----------------------------------------------------------------------------------------
EDGES = (QUAD, 2 * QUAD, HALF, HALF + QUAD, SWEEP, SWEEP + HALF, 2 * SWEEP, 4 * SWEEP)  # quad, half-sweep and sweep edges


@pytest.fixture(scope="module")
def boundaries():
    rng = np.random.default_rng(11)
    Z, Y, X = 3, 5, 2051
    a = np.zeros((Z * Y, X), dtype=np.uint32)
    b = np.zeros((Z * Y, X), dtype=np.uint32)
    a[0, 10:50], b[0, 60:90] = 1, 1          # row 0: both volumes hold labels, no voxel holds two
    a[1], b[1] = 3, 4                        # row 1: one pair from end to end
    a[2], b[2] = 1, 1 + (np.arange(X) & 1)   # row 2: A constant, B alternates every voxel
    a[3], b[3] = 1 + (np.arange(X) & 1), 2   # row 3: B constant, A alternates
    for k, x in enumerate(EDGES):            # rows 4-7: segments that end at, begin at and straddle every edge
        a[4, x - 2:x], b[4, x - 2:x] = 10 + k, 20 + k
        a[5, x:x + 2], b[5, x:x + 2] = 10 + k, 20 + k
        a[6, x - 2:x + 2], b[6, x - 2:x + 2] = 10 + k, 20 + k
        a[7, x - 2:x + 2], b[7, x - 2:x], b[7, x:x + 2] = 10 + k, 20 + k, 30 + k  # ... and two segments that meet at the edge
    a[8, 0], b[8, 0], a[8, X - 1], b[8, X - 1] = 5, 6, 7, 8  # row 8: the first and the last voxel of a row
    a[9, 0], b[9, 0] = 7, 8                  # (the pair (7, 8) again, at the start of the next row: a segment ends with its row)
    a[9, 4:100] = 40                         # row 9: one pair in every other lane, another pair in the lanes between them
    b[9, 4:100] = 50 + ((np.arange(4, 100) // QUAD) & 1)
    for r in range(10, Z * Y):               # rows 10-14: random stretches of both, labels above n and the largest label among them
        for v in (a, b):
            x = int(rng.integers(0, 6))
            while x < X:
                n = int(rng.integers(1, 10))
                v[r, x:x + n] = BIG if rng.random() < 0.02 else rng.integers(1, 70041)
                x += n + int(rng.integers(0, 3))
    a, b = a.reshape(Z, Y, X), b.reshape(Z, Y, X)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def test_boundaries_of_the_sweep_layout(eng, boundaries):
    import torch

    a, b = boundaries
    X = a.shape[2]
    n_a = n_b = 70000
    rows = [ref.table(a.reshape(-1, 1, X)[r:r + 1], b.reshape(-1, 1, X)[r:r + 1], n_a, n_b) for r in range(15)]
    # what the input is there for
    assert X % 4 == 3 and X > 4 * SWEEP  # the rows' alignment changes from row to row; more than four sweeps, the last one partial
    assert rows[0] == ({}, 0) and rows[1] == ({(3, 4): X}, 1)
    assert rows[2] == ({(1, 1): 1026, (1, 2): 1025}, X) and rows[3] == ({(1, 2): 1026, (2, 2): 1025}, X)
    assert rows[4][1] == rows[5][1] == rows[6][1] == len(EDGES) and rows[7][1] == 2 * len(EDGES)
    assert rows[4][0] == rows[5][0] == {(10 + k, 20 + k): 2 for k in range(len(EDGES))}
    assert rows[8] == ({(5, 6): 1, (7, 8): 1}, 2) and rows[9][0][(7, 8)] == 1
    assert rows[9] == ({(7, 8): 1, (40, 50): 48, (40, 51): 48}, 1 + 24)  # 24 quads of alternating pairs
    assert all(len(rows[r][0]) > 100 for r in range(10, 15))
    assert (a > n_a).sum() > 20 and (b > n_b).sum() > 20 and ((a != 0) & (b == 0)).sum() > 100
    pairs, segments = _check(eng, a, b, n_a, n_b)
    assert segments == sum(r[1] for r in rows) and pairs[(7, 8)] == 2
    # the same from buffers that start 4 and 12 bytes past a 16-byte boundary
    views = []
    for v, lead in ((a, 1), (b, 3)):
        host = np.full(v.size + 4, 0x7FFFFFF0, dtype=np.int32)
        host[lead:lead + v.size] = v.view(np.int32).ravel()
        buf = torch.from_numpy(host).cuda()
        views.append(buf[lead:lead + v.size].view(v.shape))
        assert views[-1].data_ptr() % 16 == 4 * lead
    ref.assert_table_equal(eng.cc_overlap(views[0], n_a, views[1], n_b), pairs, segments)


# ---- 2. what takes part ---------------------------------------------------------------------------------------------------------
def test_what_takes_part(eng):
    rng = np.random.default_rng(3)
    shape = (2, 3, 70)
    a = rng.integers(0, 9, size=shape).astype(np.uint32)
    b = rng.integers(0, 7, size=shape).astype(np.uint32)
    pairs, _ = _check(eng, a, b, 5, 4)  # the labels 6..8 of A and 5, 6 of B lie above n
    assert (a > 5).sum() > 50 and (b > 4).sum() > 50 and (a == 0).sum() > 20 and (b == 0).sum() > 20
    assert max(k[0] for k in pairs) == 5 and max(k[1] for k in pairs) == 4 and len(pairs) == 20
    assert sum(pairs.values()) == int(((a >= 1) & (a <= 5) & (b >= 1) & (b <= 4)).sum())
    assert _check(eng, a, b, 0, 4) == ({}, 0)
    # the largest label in both: the key with all high bits, beside the value that stands for no voxel
    a2, b2 = a.copy(), b.copy()
    a2[0, 0, :9], b2[0, 0, 3:12], b2[0, 0, 0] = BIG, BIG, 3
    a2[1, 2, 60:], b2[1, 2, 60:] = BIG + 1, BIG + 1
    pairs, _ = _check(eng, a2, b2, BIG, BIG)
    assert pairs[(BIG, BIG)] == 6 and not any(BIG + 1 in k for k in pairs) and (BIG, 3) in pairs
    got = eng.cc_overlap(_dev(a2), BIG, _dev(b2), BIG)
    assert (int(got["a"][-1]) << 32 | int(got["b"][-1])) == 0xFFFFFFFEFFFFFFFE
    # one label against 70 000
    a3 = rng.choice(np.array([0, 1, 2], dtype=np.uint32), size=(4, 50, 700), p=[0.1, 0.8, 0.1])  # (1, and 2 above n_a)
    b3 = np.arange(a3.size, dtype=np.uint32).reshape(a3.shape) % 70000 + 1
    pairs, segments = _check(eng, a3, b3, 1, 70000)
    assert int(b3.max()) == 70000 and (a3 == 2).sum() > 10000 and {k[0] for k in pairs} == {1} and len(pairs) > 40000
    assert min(segments, 1 * 70000) == 70000 > len(pairs)  # the table is sized by n_a * n_b here


# ---- 3. many distinct pairs -----------------------------------------------------------------------------------------------------
def test_many_distinct_pairs(eng):
    rng = np.random.default_rng(5)
    shape = (8, 64, 512)
    vols = []
    for _ in range(2):
        v = rng.integers(1, 5001, size=shape).astype(np.uint32)
        v[rng.random(shape) >= 0.6] = 0
        vols.append(v)
    a, b = vols
    pairs, segments = _check(eng, a, b, 5000, 5000)
    assert len(pairs) >= 50000 and segments >= len(pairs)  # probing and compaction: tens of thousands of slots
    assert abs(float((a != 0).mean()) - 0.6) < 0.01 and abs(float((b != 0).mean()) - 0.6) < 0.01
    assert int(a.max()) == int(b.max()) == 5000


# ---- 4. one heavy slot ----------------------------------------------------------------------------------------------------------
def test_one_heavy_slot(eng):
    rng = np.random.default_rng(9)
    shape = (16, 256, 512)
    a = np.ones(shape, dtype=np.uint32)
    b = np.ones(shape, dtype=np.uint32)
    b[rng.random(shape) < 0.001] = 0
    b[7] = 2
    # (the reference of two million voxels in numpy: the dictionary loop states the same on the smaller cases)
    want = {(1, 1): int((b == 1).sum()), (1, 2): int((b == 2).sum())}
    key = b.reshape(-1, shape[2])
    segments = int((key != 0).sum() - ((key[:, 1:] == key[:, :-1]) & (key[:, 1:] != 0)).sum())
    head = ref.table(a[6:8, :8], b[6:8, :8], 1, 2)
    assert head[0] == {(1, 1): int((b[6, :8] == 1).sum()), (1, 2): 8 * 512}
    assert len(want) <= 2 and want[(1, 1)] > 10**6 and (b == 0).sum() > 1000
    got = eng.cc_overlap(_dev(a), 1, _dev(b), 2)
    ref.assert_table_equal(got, want, segments)
    ref.assert_table_equal(cc.overlap_table_np(a, b, 1, 2), want, segments)


# ---- 5. more rows than workgroups -----------------------------------------------------------------------------------------------
def test_more_rows_than_workgroups(eng):
    """(40, 320, 8): 12 800 rows for the 8192 workgroups (OVERLAP_MAX_WG) of a launch - the rows are walked grid-stride"""
    rng = np.random.default_rng(13)
    shape = (40, 320, 8)
    a = (rng.integers(1, 300, size=shape) * (rng.random(shape) < 0.3)).astype(np.uint32)
    b = (rng.integers(1, 300, size=shape) * (rng.random(shape) < 0.3)).astype(np.uint32)
    a[20:, :, 2:6] = a[20:, :, 2:3]  # (stretches of one label in the rows of the second lap)
    assert shape[0] * shape[1] == 12800 > MAX_WORKGROUPS
    pairs, segments = _check(eng, a, b, 299, 299)
    late = ref.table(a[30:], b[30:], 299, 299)[0]  # rows beyond the first 8192
    assert len(pairs) > 5000 and len(late) > 1000 and segments < sum(pairs.values())


# ---- 6. nothing in common -------------------------------------------------------------------------------------------------------
def test_disjoint_foregrounds(eng):
    a = np.zeros((5, 9, 130), dtype=np.uint32)
    b = np.zeros_like(a)
    a[:, :, ::2], b[:, :, 1::2] = 3, 4
    assert (a != 0).sum() > 0 and (b != 0).sum() > 0 and not ((a != 0) & (b != 0)).any()
    got = eng.cc_overlap(_dev(a), 3, _dev(b), 4)
    ref.assert_table_equal(got, {}, 0)
    assert got["a"].dtype == np.uint32 and got["b"].dtype == np.uint32 and got["voxels"].dtype == np.uint64 and got["segments"] == 0
    assert len(got["a"]) == len(got["b"]) == len(got["voxels"]) == 0
    ref.assert_table_equal(eng.cc_overlap(_dev(a), 0, _dev(a), 0), {}, 0)  # no label at all


# ---- 7. refusals: checked on the host, nothing is launched ----------------------------------------------------------------------
def test_abi_refusals_write_nothing(eng):
    import torch

    from delivr_cfos_amd._lib import DLV_EINVAL

    Z, Y, X, n, S = 2, 3, 16, 5, 10  # min(S, n * n) = 10: a table of >= 20 slots, outputs of >= 10 entries
    a = torch.ones((Z, Y, X), dtype=torch.int32, device="cuda")
    b = torch.ones((Z, Y, X), dtype=torch.int32, device="cuda")
    sentinel = 0x0123456789ABCDEF
    table = torch.full((2 * 64 + 2,), sentinel, dtype=torch.int64, device="cuda")
    keys = torch.full((16,), sentinel, dtype=torch.int64, device="cuda")
    voxels = torch.full((16,), sentinel, dtype=torch.int64, device="cuda")
    assert table.data_ptr() % 16 == 0 and keys.data_ptr() % 8 == 0
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    good = dict(a=ptr(a), b=ptr(b), Z=Z, Y=Y, X=X, n_a=n, n_b=n, S=S, table=ptr(table), cap=32, keys=ptr(keys), voxels=ptr(voxels), out_cap=10)

    def table_call(**change):
        k = dict(good, **change)
        n_pairs = C.c_uint64(77)
        rc = eng.lib.dlv_cc_overlap_dev(eng.ctx, k["a"], k["b"], k["Z"], k["Y"], k["X"], k["n_a"], k["n_b"], k["S"], k["table"], k["cap"],
                                        k["keys"], k["voxels"], k["out_cap"], None if k.get("no_result") else C.byref(n_pairs))
        assert n_pairs.value == 77
        return rc

    def count_call(**change):
        k = dict(good, **change)
        s = C.c_uint64(77)
        rc = eng.lib.dlv_cc_overlap_count_dev(eng.ctx, k["a"], k["b"], k["Z"], k["Y"], k["X"], k["n_a"], k["n_b"],
                                              None if k.get("no_result") else C.byref(s))
        assert s.value == 77
        return rc

    refused = [dict(cap=48), dict(cap=0), dict(cap=16), dict(cap=31), dict(out_cap=9), dict(out_cap=0),  # the table and the outputs
               dict(a=None), dict(b=None), dict(table=None), dict(keys=None), dict(voxels=None), dict(no_result=True),  # NULL pointers
               dict(Z=0), dict(Y=0), dict(X=0), dict(X=-3), dict(n_a=BIG + 1), dict(n_b=2**40),  # dimensions, label counts
               dict(a=ptr(a, 2)), dict(table=ptr(table, 8)), dict(keys=ptr(keys, 4)), dict(voxels=ptr(voxels, 2))]  # alignment
    for change in refused:
        assert table_call(**change) == DLV_EINVAL, change
        if not {"cap", "out_cap", "table", "keys", "voxels"} & set(change):
            assert count_call(**change) == DLV_EINVAL, change
    assert table_call(cap=48) == DLV_EINVAL and "power of two" in eng.lib.dlv_last_error(eng.ctx).decode()
    eng.sync()
    for t in (table, keys, voxels):
        assert (t.cpu().numpy() == sentinel).all()
    assert bool((a == 1).all()) and bool((b == 1).all())
    # S = 0 is a valid call that launches nothing and writes nothing
    n_pairs = C.c_uint64(77)
    assert eng.lib.dlv_cc_overlap_dev(eng.ctx, good["a"], good["b"], Z, Y, X, n, n, 0, good["table"], 1, good["keys"], good["voxels"], 0,
                                      C.byref(n_pairs)) == 0 and n_pairs.value == 0
    eng.sync()
    assert (table.cpu().numpy() == sentinel).all()
    # ... and the accepted call on the same buffers: one pair of Z * Y * X voxels in Z * Y segments
    s = C.c_uint64()
    assert eng.lib.dlv_cc_overlap_count_dev(eng.ctx, good["a"], good["b"], Z, Y, X, n, n, C.byref(s)) == 0 and s.value == Z * Y
    assert eng.lib.dlv_cc_overlap_dev(eng.ctx, good["a"], good["b"], Z, Y, X, n, n, s.value, good["table"], 16, good["keys"], good["voxels"], 6,
                                      C.byref(n_pairs)) == 0 and n_pairs.value == 1
    assert keys.cpu().numpy()[:2].tolist() == [(1 << 32) | 1, sentinel] and voxels.cpu().numpy()[:2].tolist() == [Z * Y * X, sentinel]
    assert (table.cpu().numpy()[32:] == sentinel).all()  # 16 slots were cleared, nothing beyond them
    # the engine's own checks
    with pytest.raises(ValueError, match="labels_b of shape"):
        eng.cc_overlap(a, n, b[:, :, :8].contiguous(), n)
    with pytest.raises(ValueError, match="contiguous"):
        eng.cc_overlap(a[:, :, ::2], n, b[:, :, ::2], n)
    with pytest.raises(ValueError, match="contiguous"):
        eng.cc_overlap(a[:, :, :8].contiguous(), n, b[:, :, ::2], n)
    with pytest.raises(ValueError, match="3-D tensor of torch.int32"):
        eng.cc_overlap(a.to(torch.int64), n, b, n)
    with pytest.raises(MemoryError, match=r"DLV_ENOMEM.*pair table of 16 slots"):
        eng.cc_overlap(a, n, b, n, settings={"mi355x": {"hbm_budget_gb": 1e-8}})


# ---- 8. end to end: three kinds of source, one answer ----------------------------------------------------------------------------
def _ball(mask, c, r):
    z, y, x = np.ogrid[-r:r + 1, -r:r + 1, -r:r + 1]
    mask[c[0] - r:c[0] + r + 1, c[1] - r:c[1] + r + 1, c[2] - r:c[2] + r + 1] |= (z * z + y * y + x * x <= r * r).astype(np.uint8)


def two_masks():
    """(48, 96, 100): the reference mask, balls of radius 2-4 on a grid of pitch 12; the prediction, made from it: moved by
    (0, 1, 1), a tenth of the balls dropped, as many added in the gaps, cut in two by an empty plane, bridged to a neighbour"""
    rng = np.random.default_rng(21)
    shape = (48, 96, 100)
    ref_mask = np.zeros(shape, dtype=np.uint8)
    balls = [((6 + 12 * iz, 6 + 12 * iy, 6 + 12 * ix), int(rng.integers(2, 5)), (ix + 3 * iy + 5 * iz) % 10)
             for iz in range(4) for iy in range(8) for ix in range(8)]
    for c, r, _ in balls:
        _ball(ref_mask, c, r)
    pred = np.zeros_like(ref_mask)
    pred[:, 1:, 1:] = ref_mask[:, :-1, :-1]
    for (cz, cy, cx), r, kind in balls:
        cy, cx = cy + 1, cx + 1
        if kind == 0:  # dropped
            pred[cz - r:cz + r + 1, cy - r:cy + r + 1, cx - r:cx + r + 1] = 0
        elif kind == 1 and cz + 8 < shape[0] and cy + 8 < shape[1] and cx + 8 < shape[2]:  # added, in the gap between eight balls
            _ball(pred, (cz + 6, cy + 5, cx + 5), 2)
        elif kind == 2:  # cut in two
            pred[cz - r:cz + r + 1, cy, cx - r:cx + r + 1] = 0
        elif kind == 3 and cx + 12 < shape[2]:  # bridged to the next ball along x
            pred[cz, cy, cx:cx + 13] = 1
    return pred, ref_mask


@pytest.fixture(scope="module")
def end_to_end(eng, tmp_path_factory):
    import torch

    pred, ref_mask = two_masks()
    d = tmp_path_factory.mktemp("compare")
    out = {"masks": (str(d / "pred.npy"), str(d / "annotation.npy"))}
    np.save(out["masks"][0], pred)
    np.save(out["masks"][1], ref_mask)
    labels = []
    for mask in (pred, ref_mask):
        dev, n = eng.ccl26(torch.from_numpy(mask).cuda())
        labels.append((_host(dev).copy(), n))
    (la, n_a), (lb, n_b) = labels
    assert 0 < n_a < 65536 and 0 < n_b < 65536
    out["dense"] = (str(d / f"pred-{n_a}-cc3d.npy"), str(d / "annotation_labels.npy"))  # (n from the name; n found on the device)
    np.save(out["dense"][0], la.astype(np.uint16))
    np.save(out["dense"][1], lb.astype(np.uint16))
    out["runs"] = (str(d / f"pred-{n_a}-cc3d.runs"), str(d / f"annotation-{n_b}-cc3d.runs"))
    lr.save_runs(out["runs"][0], lr.encode_runs(la), n_a)
    lr.save_runs(out["runs"][1], lr.encode_runs(lb), n_b)
    pairs, _ = ref.table(la, lb, n_a, n_b)
    counts = ref.counts(la, n_a), ref.counts(lb, n_b)
    out.update(labels=labels, pairs=pairs, counts=counts, dir=d)
    return out


def _files(folder):
    got = {}
    for f in sorted(os.listdir(folder)):
        with open(os.path.join(folder, f), "rb") as fh:
            got[f] = fh.read()
    return got


@pytest.mark.parametrize("min_iou", [0.0, 0.5])
def test_three_kinds_of_source_give_one_answer(eng, end_to_end, tmp_path, min_iou):
    e = end_to_end
    want = ref.match(e["pairs"], *e["counts"], min_iou)
    s0, s = ref.match(e["pairs"], *e["counts"], 0.0)["summary"], want["summary"]
    # what the masks are there for (asserted on the reference's result)
    assert s0["false_pred"] > 0 and s0["missed_ref"] > 0 and s0["merges"] > 0 and s0["splits"] > 0
    assert ref.match(e["pairs"], *e["counts"], 0.5)["summary"]["true_pred"] < s0["true_pred"]
    want_files = {k: v.encode() for k, v in ref.files(want, "crop").items()}
    for kind in ("masks", "dense", "runs"):
        folder = str(tmp_path / kind)
        got = cc.compare_cells(*e[kind], out_dir=folder, name="crop", min_iou=min_iou, engine=eng)
        ref.assert_match_equal(got, want)
        assert _files(folder) == want_files, kind
    # arrays and tensors in HBM as sources, and no files without out_dir
    (la, n_a), (lb, n_b) = e["labels"]
    got = cc.compare_cells((_dev(la), n_a), lb, min_iou=min_iou, engine=eng)
    ref.assert_match_equal(got, want)
    assert s["min_iou"] == min_iou and s["n_pred"] == n_a and s["n_ref"] == n_b


def test_the_command_line_prints_the_same_summary(end_to_end, tmp_path):
    e = end_to_end
    want = ref.match(e["pairs"], *e["counts"], 0.25)
    r = subprocess.run([sys.executable, "-m", "delivr_cfos_amd.compare_cells", *e["masks"], "--out", str(tmp_path / "cli"), "--name", "crop",
                        "--min-iou", "0.25"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == want["summary"] and lines[0] == json.dumps(want["summary"])
    assert _files(str(tmp_path / "cli")) == {k: v.encode() for k, v in ref.files(want, "crop").items()}


def test_sources_that_do_not_fit_are_refused(eng, end_to_end):
    e = end_to_end
    (la, n_a), _ = e["labels"]
    with pytest.raises(ValueError, match=r"prediction has shape \(48, 96, 100\), the reference \(47, 96, 100\)"):
        cc.compare_cells(e["masks"][0], la[1:], engine=eng)
    with pytest.raises(ValueError, match="below 2\\^32 - 1"):
        cc.open_labels(np.full((1, 2, 3), 2**32 - 1, dtype=np.uint32), eng)
    labels, n = cc.open_labels(np.full((1, 2, 3), BIG, dtype=np.uint32), eng)  # (the largest label is found on the device)
    assert n == BIG and labels.dtype.is_signed and int(labels[0, 0, 0]) == BIG - 2**32
    labels, n = cc.open_labels(la.astype(np.uint16), eng)
    assert n == n_a and np.array_equal(_host(labels), la)
