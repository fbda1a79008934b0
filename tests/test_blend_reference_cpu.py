"""tests/helpers/blend_reference.py (the expectation of tests/test_gpu_blend_exact.py) against the oracle's own sliding-window
loop, and the conditions its volumes must meet for those tests to mean something: no GPU."""
import importlib.util
import os

import numpy as np
import pytest


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("blend_reference")
GEOS = sorted(ref.GEOMETRIES)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in GEOS:
        shape, roi, ov = ref.GEOMETRIES[name]
        vol = ref.volume(shape)
        out[name] = (vol, roi, ov) + ref.expected(vol, roi, ov)
    return out


@pytest.mark.parametrize("name", GEOS)
def test_helper_restates_the_oracle_loop(cases, name):
    """the oracle's window loop with a predictor that answers 3.0 everywhere: acc and cnt equal the count formula exactly, and
    with the Gaussian importance map the weighted sums equal the helper's float64 sums up to the float32 products of the loop"""
    from oracle import delivr_oracle as orc

    vol, roi, ov, act, skp, wins, wmax = cases[name]
    const3 = lambda x: np.full(x.shape, 3.0, np.float32)  # noqa: E731
    acc = np.zeros(vol.shape, dtype=np.float32)
    cnt = np.zeros(vol.shape, dtype=np.uint8)
    info = orc.sliding_window_pass(vol, roi, const3, acc, cnt, ov, None, sw_batch_size=1, fp16=False)
    assert info["n_windows"] == len(wins) and info["n_skipped"] == int((wmax <= 0).sum())
    assert np.array_equal(acc, ref.constant_acc(act, skp, 3))
    assert np.array_equal(cnt, ref.constant_cnt(act, skp))
    # flips change nothing in a constant
    acc2 = np.zeros(vol.shape, dtype=np.float32)
    orc.sliding_window_pass(vol, roi, const3, acc2, None, ov, 3, sw_batch_size=1, fp16=False)
    assert np.array_equal(acc2, acc)

    imp = orc.gaussian_importance_map(roi, 0.125)
    w_act, w_skp = ref.expected_weighted(vol, roi, ov, imp)
    gacc = np.zeros(vol.shape, dtype=np.float64)
    gws = np.zeros(vol.shape, dtype=np.float64)
    orc.sliding_window_pass(vol, roi, const3, gacc, gws, ov, None, sw_batch_size=1, fp16=False, importance=imp)
    # the loop adds the float32 map in float64: the helper's terms in another association (at most 18 of them)
    np.testing.assert_allclose(gws, w_act + w_skp, rtol=1e-14, atol=0)
    # ... and float32 products map * logit: one rounding (2^-24 relative) per term
    assert np.all(np.abs(gacc - (3.0 * w_act - 1000.0 * w_skp)) <= (2.0 ** -24 + 1e-14) * (3.0 * w_act + 1000.0 * w_skp))
    assert float(imp.min()) > 1e-12 and float(imp.min()) * 4 > np.finfo(np.float32).tiny  # no term is subnormal


@pytest.mark.parametrize("name", GEOS)
def test_volumes_meet_the_coverage_conditions(cases, name):
    """conditions on the inputs: enough windows of either kind, enough voxels that only active windows cover (where the Gaussian
    test compares bits), enough voxels covered by both kinds (where a -1000 and a logit meet in one sum)"""
    vol, roi, ov, act, skp, wins, wmax = cases[name]
    share = float((wmax <= 0).mean())
    assert 0.25 <= share <= 0.60, share
    assert act.min() >= 0 and (act + skp).min() >= 1  # every voxel is covered
    assert float(((act > 0) & (skp == 0)).mean()) >= 0.25
    assert float(((act > 0) & (skp > 0)).mean()) >= 0.05


def test_window_counts_of_the_table(cases):
    n = {k: (len(c[5]), int((c[6] <= 0).sum())) for k, c in cases.items()}
    assert n["A"] == (12, 4) and n["B"] == (72, 36), n
    vol, roi, ov, act, skp, wins, wmax = cases["B"]
    assert int((act + skp).max()) == 18
    for k in (0, 1):  # a clamped last window along z and y (x: 70 = 5 intervals + a window, the last start is regular)
        st = np.unique(wins[:, k])
        assert st[-1] + roi[k] == vol.shape[k] and st[-1] - st[-2] < st[1] - st[0]
    assert np.any(wins[:, 2] % 8) and vol.shape[2] % 4  # general window maxima, scalar fill
    st = np.unique(cases["D"][5][:, 2])
    assert len(st) == 7 and st[1] == 6 and st[-1] - st[-2] < 6
    vol, roi, ov, act, skp, wins, wmax = cases["E"]
    assert not np.any(wins[:, 2] % 8) and vol.shape[2] % 8 == 0 and roi[2] % 8 == 0  # cell maxima, 16-byte fill


@pytest.mark.parametrize("name", GEOS)
def test_sums_stay_exact_in_float32(cases, name):
    """the largest accumulator of the GPU rows: repeat 5, and four passes onto a pre-fill of at most 2^16"""
    vol, roi, ov, act, skp, wins, wmax = cases[name]
    worst = np.abs(3 * act - 1000 * skp).max()
    assert 5 * worst < 2 ** 24 and 4 * worst + 2 ** 16 < 2 ** 24
    assert 5 * int((act + skp).max()) <= 255


def test_threshold_and_window_range_restrict_the_counts(cases):
    vol, roi, ov, act, skp, wins, wmax = cases["B"]
    thr = int(np.sort(wmax[wmax > 0])[len(wmax[wmax > 0]) // 2])
    a2, s2, _, _ = ref.expected(vol, roi, ov, skip_threshold=thr)
    assert np.array_equal(a2 + s2, act + skp) and s2.sum() > skp.sum() and a2.sum() > 0
    a3, s3, _, _ = ref.expected(vol, roi, ov, win_range=(3, len(wins) - 2))
    rest = ref.expected(vol, roi, ov, win_range=(0, 3)), ref.expected(vol, roi, ov, win_range=(len(wins) - 2, len(wins)))
    assert np.array_equal(a3 + rest[0][0] + rest[1][0], act) and np.array_equal(s3 + rest[0][1] + rest[1][1], skp)
