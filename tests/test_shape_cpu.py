"""Host side of settings["mi355x"]["shape_stats"] (hostlogic.shape_stats_enabled / merge_shape / finish_shape /
cell_shape_csv_text): no device.  The accumulators come from numpy on small hand-built label volumes, or - for cells no volume of
this test could hold - from the closed sums over boxes in Python integers.  Integers are compared for equality; covariances with
fractions.Fraction on the integer sums, within 4 np.spacing of the value: the path has four roundings (the numerator, n^2, the
division and the + 1/12)."""
from fractions import Fraction

import numpy as np
import pytest

from delivr_cfos_amd.hostlogic import (SHAPE_KEYS, SHAPE_RAW_KEYS, cell_shape_csv_text, finish_shape, merge_shape, shape_stats_enabled)

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # zz, yy, xx, zy, zx, yx


def _accumulate(labels: np.ndarray, n: int, planes=None, z_abs0: int = 0) -> dict:
    """HipEngine.cc_shape's answer from numpy: the planes [planes[0], planes[1]) of `labels` measured, the rest neighbours only"""
    lo, hi = planes or (0, labels.shape[0])
    pad = np.pad(labels.astype(np.int64), 1, constant_values=-1)  # (outside the buffer: differs from every label)
    core = pad[1:-1, 1:-1, 1:-1]
    exposed = [(np.roll(pad, 1, a)[1:-1, 1:-1, 1:-1] != core).astype(np.uint64) + (np.roll(pad, -1, a)[1:-1, 1:-1, 1:-1] != core)
               for a in range(3)]
    sel = np.zeros(labels.shape, dtype=bool)
    sel[lo:hi] = (labels[lo:hi] >= 1) & (labels[lo:hi] <= n)
    lab = labels[sel].astype(np.int64)
    c = [v[sel].astype(np.uint64) for v in np.indices(labels.shape)]
    c[0] = c[0] + np.uint64(z_abs0)
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


def _volume():
    """label 1: a single voxel, 2: a 3 x 3 x 3 cube, 3: a 1 x 1 x 5 rod along x, 4: an L of three voxels in the plane z = 9"""
    v = np.zeros((11, 9, 12), dtype=np.uint32)
    v[0, 0, 0] = 1
    v[2:5, 3:6, 4:7] = 2
    v[7, 1, 2:7] = 3
    v[9, 5, 5] = v[9, 6, 5] = v[9, 6, 6] = 4
    return v


def _box_sums(boxes):
    """(counts, sums[3], moments[6]) in Python integers of the cell made of the disjoint boxes [(z0, z1, y0, y1, x0, x1), ...)"""
    n, S, M = 0, [0] * 3, [0] * 6
    for box in boxes:
        ext = [(box[2 * a], box[2 * a + 1]) for a in range(3)]
        cnt = [hi - lo for lo, hi in ext]
        s1 = [sum(range(lo, hi)) for lo, hi in ext]
        s2 = [sum(v * v for v in range(lo, hi)) for lo, hi in ext]
        vox = cnt[0] * cnt[1] * cnt[2]
        n += vox
        for a in range(3):
            S[a] += s1[a] * vox // cnt[a]
        for j, (a, b) in enumerate(PAIRS):
            M[j] += s2[a] * vox // cnt[a] if a == b else s1[a] * s1[b] * vox // (cnt[a] * cnt[b])
    return n, S, M


def _merged_from(cells):
    """finish_shape's input for cells given as (n, S, M): label i + 1 = cells[i]; faces are not the subject (6 per voxel)"""
    rows = len(cells) + 1
    out = {"shape_counts": np.zeros(rows, np.uint32), "shape_sums": np.zeros((rows, 3), np.uint64),
           "shape_moments": np.zeros((rows, 6), np.uint64), "shape_faces": np.zeros((rows, 3), np.uint64),
           "shape_surface_voxels": np.zeros(rows, np.uint32)}
    for i, (n, S, M) in enumerate(cells, 1):
        assert n < 2**32 and max(M) < 2**64
        out["shape_counts"][i] = n
        out["shape_sums"][i] = S
        out["shape_moments"][i] = M
        out["shape_faces"][i] = 2 * n
        out["shape_surface_voxels"][i] = n
    return out


def _assert_covariance(got_row, n, S, M):
    for j, (a, b) in enumerate(PAIRS):
        exact = Fraction(n * M[j] - S[a] * S[b], n * n) + (Fraction(1, 12) if a == b else 0)
        tol = 4 * Fraction(float(np.spacing(abs(float(exact)))))
        assert abs(Fraction(float(got_row[j])) - exact) <= tol, (j, float(got_row[j]), float(exact))


def test_shape_stats_enabled_only_for_a_truthy_key():
    for off in (None, {}, {"mi355x": None}, {"mi355x": {}}, {"mi355x": {"shape_stats": False}}, {"mi355x": {"shape_stats": 0}},
                {"mi355x": {"intensity_stats": True}}):
        assert shape_stats_enabled(off) is False
    for on in (True, 1, "yes"):
        assert shape_stats_enabled({"mi355x": {"shape_stats": on}}) is True


def test_key_names():
    assert SHAPE_RAW_KEYS == ("shape_counts", "shape_sums", "shape_moments", "shape_faces", "shape_surface_voxels")
    assert set(SHAPE_KEYS) == {"shape_sums", "shape_moments", "shape_faces", "shape_surface_voxels", "shape_covariance", "shape_axes",
                               "shape_elongation", "shape_sphericity"}


def test_merge_shape_adds_split_parts_and_raises_the_two_errors():
    v = _volume()
    whole = _accumulate(v, 4)
    # cuts through the cube (z = 3) and ahead of the L: each part measures its own planes and sees the whole volume as neighbours
    parts = [_accumulate(v, 4, planes=p) for p in ((0, 3), (3, 9), (9, 11))]
    assert all((p["shape_counts"][1:] == 0).any() for p in parts)
    for order in (parts, [parts[2], None, parts[0], parts[1]]):
        merged = merge_shape(order)
        assert list(merged) == list(SHAPE_RAW_KEYS)
        for k in SHAPE_RAW_KEYS:
            assert merged[k].dtype == whole[k].dtype and merged[k].shape == whole[k].shape, k
            np.testing.assert_array_equal(merged[k], whole[k], err_msg=k)
    with pytest.raises(ValueError, match="no slab"):
        merge_shape([None, None])
    with pytest.raises(ValueError, match="no slab"):
        merge_shape([])
    short = {k: a[:-1] for k, a in parts[1].items()}
    with pytest.raises(ValueError, match="same labels"):
        merge_shape([parts[0], short])


def test_finish_shape_dtypes_shapes_and_row_0():
    v = _volume()
    raw = _accumulate(v, 4)
    counts = np.bincount(v.ravel(), minlength=5).astype(np.uint32)  # (row 0: the background's count, as cc_stats gives it)
    out = finish_shape(raw, counts)
    assert tuple(out) == SHAPE_KEYS
    expect = {"shape_sums": (np.uint64, (5, 3)), "shape_moments": (np.uint64, (5, 6)), "shape_faces": (np.uint64, (5, 3)),
              "shape_surface_voxels": (np.uint32, (5,)), "shape_covariance": (np.float64, (5, 6)), "shape_axes": (np.float64, (5, 3)),
              "shape_elongation": (np.float64, (5,)), "shape_sphericity": (np.float64, (5,))}
    for k, (dt, shape) in expect.items():
        assert out[k].dtype == dt and out[k].shape == shape, k
        assert not np.any(out[k][0]), k
    for k in ("shape_sums", "shape_moments", "shape_faces", "shape_surface_voxels"):
        np.testing.assert_array_equal(out[k], raw[k], err_msg=k)
    assert (out["shape_elongation"][1:] >= 1).all() and np.isfinite(out["shape_elongation"]).all()
    assert (np.diff(out["shape_axes"], axis=1) <= 0).all() and (out["shape_axes"] >= 0).all()
    again = _accumulate(v, 4)  # the input is not modified
    for k in SHAPE_RAW_KEYS:
        np.testing.assert_array_equal(raw[k], again[k], err_msg=k)


def test_finish_shape_raises_on_a_count_mismatch_and_names_the_first_label():
    v = _volume()
    raw = _accumulate(v, 4)
    counts = np.bincount(v.ravel(), minlength=5).astype(np.uint32)
    counts[3] += 1
    counts[4] += 1
    with pytest.raises(RuntimeError, match="first label 3"):
        finish_shape(raw, counts)
    with pytest.raises(RuntimeError):
        finish_shape(raw, counts[:4])


def test_known_values_single_voxel_cube_rod():
    v = _volume()
    out = finish_shape(_accumulate(v, 4), np.bincount(v.ravel(), minlength=5))
    twelfth = 1.0 / 12.0
    # 1: a single voxel
    assert out["shape_covariance"][1].tolist() == [twelfth] * 3 + [0.0] * 3
    assert out["shape_faces"][1].tolist() == [2, 2, 2] and out["shape_surface_voxels"][1] == 1
    assert out["shape_elongation"][1] == 1.0
    assert out["shape_sphericity"][1] == pytest.approx((np.pi / 6) ** (1 / 3), rel=1e-15)
    # 2: a 3 x 3 x 3 cube: variance of {-1, 0, 1} is 2/3
    np.testing.assert_allclose(out["shape_axes"][2], [2 / 3 + twelfth] * 3, rtol=1e-14, atol=0)
    assert out["shape_covariance"][2, 3:].tolist() == [0.0] * 3
    assert out["shape_faces"][2].tolist() == [18, 18, 18] and out["shape_surface_voxels"][2] == 26
    assert out["shape_sphericity"][2] == pytest.approx((np.pi / 6) ** (1 / 3), rel=1e-15)
    # 3: a rod of 5 along x: variance of {-2..2} is 2
    np.testing.assert_allclose(out["shape_axes"][3], [2 + twelfth, twelfth, twelfth], rtol=1e-14, atol=0)
    assert out["shape_elongation"][3] == pytest.approx(5.0, rel=1e-15)
    assert out["shape_faces"][3].tolist() == [10, 10, 2] and out["shape_surface_voxels"][3] == 5
    assert out["shape_covariance"][3].tolist() == [twelfth, twelfth, 2 + twelfth, 0.0, 0.0, 0.0]
    # 4: the L: (5,5), (6,5), (6,6) in (y, x): cov_yy = cov_xx = 2/9, cov_yx = 1/9, nothing along z
    np.testing.assert_allclose(out["shape_covariance"][4], [twelfth, 2 / 9 + twelfth, 2 / 9 + twelfth, 0.0, 0.0, 1 / 9], rtol=4e-16, atol=0)
    assert out["shape_faces"][4].tolist() == [6, 4, 4] and out["shape_surface_voxels"][4] == 3
    np.testing.assert_allclose(out["shape_axes"][4], [1 / 3 + twelfth, 1 / 9 + twelfth, twelfth], rtol=1e-14, atol=0)


def test_covariance_against_fractions_small_large_and_beyond_int64():
    v = _volume()
    raw = _accumulate(v, 4, z_abs0=65536 - 11)  # the hand-built cells at the far end of the z range
    small = finish_shape(raw, raw["shape_counts"])
    for l in range(1, 5):
        _assert_covariance(small["shape_covariance"][l], int(raw["shape_counts"][l]), [int(s) for s in raw["shape_sums"][l]],
                           [int(m) for m in raw["shape_moments"][l]])
    cells = [
        _box_sums([(65491, 65536, 65491, 65536, 65491, 65536)]),  # 91 125 voxels at the far corner: n * S_ab is above 2^64
        _box_sums([(65000, 65040, 65100, 65130, 65400, 65536), (65040, 65100, 65130, 65200, 65300, 65400)]),  # skewed: off-diagonals
        _box_sums([(0, 3, 0, 5, 0, 65536), (3, 4, 5, 6, 0, 7)]),  # a thin slab along the whole x range
        _box_sums([(65520, 65536, 0, 2048, 0, 65536)]),  # 2^31 voxels: n^2 * extent^2 is far above 2^63 - the Python-integer path
        _box_sums([(0, 16, 0, 1024, 0, 65536), (16, 32, 1024, 2048, 0, 32768)]),  # ... with off-diagonals
        _box_sums([(7, 8, 9, 10, 65535, 65536)]),  # a single voxel at the end of the x range
    ]
    assert cells[0][0] * cells[0][2][0] > 2**64 and cells[3][0] == 2**31
    merged = _merged_from(cells)
    out = finish_shape(merged, merged["shape_counts"])
    for l, (n, S, M) in enumerate(cells, 1):
        _assert_covariance(out["shape_covariance"][l], n, S, M)
    assert out["shape_covariance"][6].tolist() == [1 / 12] * 3 + [0.0] * 3
    assert (out["shape_covariance"][1, 3:] == 0).all() and (np.abs(out["shape_covariance"][2, 3:]) > 1).all()
    assert (np.abs(out["shape_covariance"][5, 3:5]) > 1).all()


def test_finish_shape_is_quick_for_half_a_million_labels():
    import time

    rng = np.random.default_rng(3)
    n = 500_000
    lo = rng.integers(0, 65000, size=(n, 3))
    ext = rng.integers(1, 12, size=(n, 3))
    cells = {"shape_counts": np.zeros(n + 1, np.uint32), "shape_sums": np.zeros((n + 1, 3), np.uint64),
             "shape_moments": np.zeros((n + 1, 6), np.uint64), "shape_faces": np.zeros((n + 1, 3), np.uint64),
             "shape_surface_voxels": np.zeros(n + 1, np.uint32)}
    vox = ext.prod(axis=1)
    s1 = ext * lo + ext * (ext - 1) // 2  # sum of lo .. lo + ext - 1
    s2 = ext * lo * lo + lo * ext * (ext - 1) + (ext - 1) * ext * (2 * ext - 1) // 6
    cells["shape_counts"][1:] = vox
    for a in range(3):
        cells["shape_sums"][1:, a] = s1[:, a] * (vox // ext[:, a])
    for j, (a, b) in enumerate(PAIRS):
        cells["shape_moments"][1:, j] = s2[:, a] * (vox // ext[:, a]) if a == b else s1[:, a] * s1[:, b] * (vox // (ext[:, a] * ext[:, b]))
    cells["shape_faces"][1:] = 2 * (vox[:, None] // ext)
    t0 = time.perf_counter()
    out = finish_shape(cells, cells["shape_counts"])
    took = time.perf_counter() - t0
    # boxes: the covariance is diagonal, (ext^2 - 1) / 12 + 1 / 12 per axis
    np.testing.assert_allclose(out["shape_covariance"][1:, :3], ext * ext / 12.0, rtol=1e-9, atol=0)
    assert not out["shape_covariance"][1:, 3:].any()
    np.testing.assert_allclose(out["shape_axes"][1:], np.sort(ext * ext / 12.0, axis=1)[:, ::-1], rtol=1e-9, atol=0)
    assert took < 5.0, took  # (well under a second of exact arithmetic plus eigvalsh on an idle core; generous for a loaded one)


def test_cell_shape_csv_text():
    v = _volume()
    stats = finish_shape(_accumulate(v, 4), np.bincount(v.ravel(), minlength=5))
    stats["voxel_counts"] = np.bincount(v.ravel(), minlength=5).astype(np.uint32)
    text = cell_shape_csv_text(stats, 4)
    lines = text.split("\n")
    assert text.endswith("\n") and lines[-1] == "" and len(lines) == 6
    assert lines[0] == "Blob,Size,FacesZ,FacesY,FacesX,SurfaceVoxels,VarMajor,VarMid,VarMinor,Elongation,Sphericity"
    t = 1 / 12
    assert lines[1] == f"1,1,2,2,2,1,{t!r},{t!r},{t!r},1.0,{float(stats['shape_sphericity'][1])!r}"
    for i, line in enumerate(lines[1:5], 1):
        f = line.split(",")
        assert f[:6] == [str(i), str(stats["voxel_counts"][i]), *(str(int(x)) for x in stats["shape_faces"][i]),
                         str(stats["shape_surface_voxels"][i])]
        assert f[6:] == [repr(float(x)) for x in (*stats["shape_axes"][i], stats["shape_elongation"][i], stats["shape_sphericity"][i])]
        assert [float(x) for x in f[6:9]] == stats["shape_axes"][i].tolist()  # (repr round-trips)
    assert cell_shape_csv_text(stats, 2) == "\n".join(lines[:3]) + "\n"
    assert cell_shape_csv_text(stats, 0) == lines[0] + "\n"
    with pytest.raises(ValueError, match="shorter"):
        cell_shape_csv_text(stats, 5)
