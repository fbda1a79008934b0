"""tests/helpers/finalize_reference.py without a GPU: the reference of tests/test_gpu_finalize_kernels.py equals orc.finalize where
both are defined, its erosion is scipy's, its slab semantics are the ones parallel.finalize_owned relies on, and the inputs the GPU
cases are built from meet their conditions (no voxel near a threshold, the erosion keeps and removes a share of every case)."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import delivr_oracle as orc


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fr = _helper("finalize_reference")
FAMILIES = fr.all_cases()


@pytest.mark.parametrize("tag", ["oneblock", "blocks"])
def test_reference_equals_the_oracle_on_the_golden(golden_dir, tag):
    """both variants of ref_finalize.npz: finalize_reference with the block size orc.zblock_planes derives from buf_size gives the
    reference's own binaries"""
    g = np.load(os.path.join(golden_dir, "ref_finalize.npz"), allow_pickle=False)
    shape = tuple(int(v) for v in g["stack_shape"][2:])
    buf = int(g[f"{tag}_buf"])
    axis, nb = orc.zblock_planes(shape, buf)
    assert axis == "z" and (nb < shape[0]) == (tag == "blocks")
    mask, _ = fr.finalize_reference(g["mean"], None, g["raw"], shape, 0.5, 30, nb)
    np.testing.assert_array_equal(mask, g[f"{tag}_binaries"])
    np.testing.assert_array_equal(mask, orc.finalize(g["mean"], None, g["raw"], shape, 0.5, 30, buf_size=buf))


@pytest.mark.parametrize("nb", [1, 3, 4, 7, 11, 12, 40])
@pytest.mark.parametrize("threshold,with_cnt", [(0.5, True), (0.3, True), (0.9, False)])
def test_reference_equals_the_oracle_on_padded_random_inputs(nb, threshold, with_cnt):
    """z_abs0 = 0: the blocks of finalize_reference are orc.finalize's for the buf_size that yields the same block size, on padded
    buffers with a count map, x / 0 and 0 / 0 included"""
    Z, Y, X, Yp, Xp = 11, 6, 9, 8, 12
    rng = np.random.default_rng(nb)
    acc = rng.normal(0, 3, size=(Z, Yp, Xp)).astype(np.float32)
    cnt = rng.integers(0, 5, size=(Z, Yp, Xp)).astype(np.uint8)
    acc[rng.random(acc.shape) < 0.1] = 0.0
    raw = (rng.integers(1, 65536, size=(Z, Yp, Xp)) * (rng.random((Z, Yp, Xp)) > 0.03)).astype(np.uint16)
    buf = nb * Y * X + (Y * X) // 2
    assert orc.zblock_planes((Z, Y, X), buf) == ("z", min(nb, Z))
    for r in (0, 1, 2):
        mask, sig = fr.finalize_reference(acc, cnt if with_cnt else None, raw, (Z, Y, X), threshold, r, nb)
        if r == 0:
            want = orc.finalize(acc, cnt if with_cnt else None, np.ones_like(raw), (Z, Y, X), threshold, 1, buf_size=buf) * (raw[:Z, :Y, :X] > 0)
        else:
            want = orc.finalize(acc, cnt if with_cnt else None, raw, (Z, Y, X), threshold, r, buf_size=buf)
        np.testing.assert_array_equal(mask, want)
        assert mask.any() and sig.shape == (Z, Y, X)
        if with_cnt:
            assert np.isnan(sig).any() and np.isinf(fr.mean32(acc, cnt, (Z, Y, X))).any()


@pytest.mark.parametrize("radius", [1, 2, 30, 31, 32, 57, 253])
def test_scipy_erosion_equals_the_l1_distance_form(radius):
    """the radii of the GPU cases on small random volumes, a (3, 5, 300) row volume among them so that 253 has voxels on both sides"""
    rng = np.random.default_rng(radius)
    for shape, nzero in (((9, 11, 13), 5), ((3, 5, 300), 3), ((70, 5, 8), 5), ((3, 5, 8200), 40)):
        m = np.ones(shape, dtype=np.uint8)
        m.ravel()[rng.choice(m.size, size=nzero, replace=False)] = 0
        np.testing.assert_array_equal(orc.erode_l1(m, radius), orc.l1_distance_keep(m, radius))


def test_radius_0_means_no_erosion_unlike_scipy_iterations_0():
    """scipy's binary_erosion(iterations=0) repeats until nothing changes - with a zero in the volume nothing is left - so it is not
    the reference of radius 0; orc.l1_distance_keep returns the mask itself, and eroded_keep takes that one"""
    rng = np.random.default_rng(5)
    m = (rng.random((4, 6, 9)) > 0.05).astype(np.uint8)
    assert 0 < (m == 0).sum() < m.size // 4
    assert not orc.erode_l1(m, 0).any()
    np.testing.assert_array_equal(orc.l1_distance_keep(m, 0), m)
    raw = (m * 7).astype(np.uint16)
    for zblock in (0, 1, 3):
        np.testing.assert_array_equal(fr.eroded_keep(raw, m.shape, 0, zblock), m)
    assert np.array_equal(fr.eroded_keep(raw, m.shape, 1, 0), orc.erode_l1(m, 1)) and not np.array_equal(orc.erode_l1(m, 1), m)


def test_zblocks_sit_at_absolute_multiples():
    assert fr.zblocks(25, 10, 20) == [(0, 10), (10, 20), (20, 25)]
    assert fr.zblocks(4, 10, 21) == [(0, 4)]
    assert fr.zblocks(12, 10, 29) == [(0, 1), (1, 11), (11, 12)]
    assert fr.zblocks(7, 0, 29) == [(0, 7)] and fr.zblocks(5, 9, 0) == [(0, 5)] and fr.zblocks(3, 1, 4) == [(0, 1), (1, 2), (2, 3)]


@pytest.mark.parametrize("nb", [2, 3, 5, 16])
def test_owned_planes_of_a_slab_with_margin_equal_the_whole_volume(nb):
    """what parallel.finalize_owned relies on: a slab that carries `radius` planes of margin inside the z-blocks of its owned planes
    (cut as finalize_owned cuts it) gives, on the owned planes, the whole-volume result - for blocks smaller than, equal to and
    larger than the radius (3)"""
    Z, Y, X, r = 40, 5, 8, 3
    c = fr.case("whole", (Z, Y, X), r, zblock=nb)
    whole = fr.build(c)
    raw_fg = whole.raw > 0
    assert 0.05 <= fr.shares(whole.keep, raw_fg)[1] <= 0.95
    for lo, hi in ((0, 7), (7, 19), (19, 20), (20, 33), (33, 40), (9, 10), (10, 15)):
        elo = max(lo - r, (lo // nb) * nb)
        ehi = min(hi + r, min(((hi - 1) // nb + 1) * nb, Z))
        mask, sig = fr.finalize_reference(whole.acc[elo:ehi], whole.cnt[elo:ehi], whole.raw[elo:ehi], (ehi - elo, Y, X), 0.5, r, nb, elo)
        np.testing.assert_array_equal(mask[lo - elo:hi - elo], whole.mask[lo:hi], err_msg=f"owned [{lo}, {hi}) of slab [{elo}, {ehi})")
        np.testing.assert_array_equal(sig[lo - elo:hi - elo], whole.sig[lo:hi])
    # the margin is needed: without it the planes next to a cut inside a block differ somewhere
    differs = False
    for lo in range(1, Z):
        if lo % nb:
            mask, _ = fr.finalize_reference(whole.acc[lo:], whole.cnt[lo:], whole.raw[lo:], (Z - lo, Y, X), 0.5, r, nb, lo)
            differs |= not np.array_equal(mask, whole.mask[lo:])
    assert differs


def test_ulp_distance():
    a = np.array([0.5, 1.0, 0.0, 0.25], dtype=np.float32)
    np.testing.assert_array_equal(fr.ulp_distance(a, a.astype(np.float64)), 0)
    np.testing.assert_array_equal(fr.ulp_distance(np.nextafter(a, np.float32(2)), a.astype(np.float64)), 1)
    assert fr.ulp_distance(np.array([1.0], np.float32), np.array([1.0 - 2.0 ** -24]))[0] == 1  # one float32 step below 1


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_inputs_of_every_gpu_case_meet_their_conditions(family):
    """no voxel's sigmoid within 1e-6 of a threshold (after redrawing, nothing masked out); the reference alone keeps at least 5 % and
    removes at least 5 % of the foreground (build asserts it) unless the case is a declared all-or-nothing one; the sums differ
    on every plane; the counts are 1..8; the zeros are few"""
    for c in FAMILIES[family]:
        inp = fr.build(c)
        Z, Y, X = c.shape
        acc, raw = inp.acc[:, :Y, :X], inp.raw[:, :Y, :X]
        cnt = inp.cnt[:, :Y, :X] if inp.cnt is not None else None
        assert not fr.in_band(acc, cnt).any(), c.name
        assert np.isfinite(acc).all() and (cnt is None or (1 <= cnt.min() and cnt.max() <= 8)), c.name
        assert all(not np.array_equal(acc[i], acc[j]) for i in range(Z) for j in range(i)), c.name
        assert (raw == 0).sum() <= max(1, raw.size // 4), c.name
        if c.pad != (0, 0):
            assert np.isnan(inp.acc).sum() == inp.acc.size - acc.size
        if not c.exempt:
            kept, removed = fr.shares(inp.keep, raw > 0)
            assert kept >= 0.05 and removed >= 0.05, (c.name, kept, removed)
        assert inp.mask.shape == c.shape and inp.sig.shape == c.shape


def test_exemptions_are_the_all_or_nothing_cases_only():
    """a case is exempt from the kept / removed shares only where the reference cannot give both: single-zero rows of X = 57 at
    radius 56 / 57 (nothing of such a row is kept), radius 0 (nothing is removed), and stacks or slabs whose largest distance
    does not exceed their radius - and every exempt case does miss a share"""
    n = 0
    for family, cs in FAMILIES.items():
        for c in cs:
            if c.exempt:
                Z, Y, X = c.shape
                rows = c.zeros.startswith("rows") and X == 57 and c.radius in (56, 57)
                assert rows or c.radius == 0 or (Z - 1) + (Y - 1) + (X - 1) <= c.radius, (family, c.name)
                kept, removed = fr.shares(fr.build(c).keep, fr.build(c).raw[:, :Y, :X] > 0)
                assert kept < 0.05 or removed < 0.05, (family, c.name, kept, removed)
                n += 1
    assert n < sum(len(cs) for cs in FAMILIES.values()) // 4


def test_expected_launch_records_cover_every_kernel_and_branch():
    """the records the GPU cases assert (expected_ran restates the dispatch; the GPU module compares it with dlv_diag_finalize_ran
    field by field) cover every instantiation, both values of every alignment condition and a zphase != 0"""
    records = [fr.expected_ran(c) for cs in FAMILIES.values() for c in cs]
    assert fr.coverage(records) == set()
    assert fr.coverage(records[:3]) != set()
    names = [(f, c.name) for f, cs in FAMILIES.items() for c in cs]
    assert len(names) == len(set(names))
