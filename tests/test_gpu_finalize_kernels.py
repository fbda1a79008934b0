"""Every kernel and branch of the finalize pass (csrc/finalize.hip) alone against scipy: the fused x/y distance at its chunk-count
boundaries, at small and ragged rows and at the reach of its 64-bit windows; the separate x and y passes, switched and unswitched,
and the log-step x kernel; the one-sweep and the two-sweep z decision in both instantiations over stack depths, z-blocks and slab
phases; padded planes with zeros or poison in the padding; the decision at +-0, x / 0 and 0 / 0; the values of `prob`; and the
stores at both ends of `out`.

The reference is tests/helpers/finalize_reference.py (scipy's binary_erosion per z-block at absolute multiples of the block size,
the float32 decision of orc.finalize), which tests/test_finalize_reference_cpu.py checks without a GPU.  Masks are compared for
equality over the whole volume; no voxel is masked out of a comparison, because the inputs hold no voxel whose sigmoid lies within
1e-6 of a threshold.  The sums differ on every plane, so a z kernel that pairs a distance plane with the sums of another plane
cannot pass.  Every case first asserts, through HipEngine.finalize_ran() (dlv_diag_finalize_ran: recorded at the launch sites of
finalize_impl), that it ran the path it is named for - all ten fields against finalize_reference.expected_ran - and, before it looks
at the device, that the reference alone keeps at least 5 % and removes at least 5 % of the foreground (all-or-nothing cases
excepted: finalize_reference.build).

`prob` against the fp64 sigmoid of the float32 mean, rounded to float32: the largest distance measured on an MI355X over the cases
of test_prob_values is 2 units in the last place of the result (PROB_ULP_MEASURED; expf, the add and the divide each round
once); the test asserts twice that, 4, and never less than 2."""
import ctypes as C
import importlib.util
import os
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROB_ULP_MEASURED = 2  # on an MI355X, over the cases of test_prob_values (1 or 2 in every one of them)
PROB_ULP_BOUND = max(2, 2 * PROB_ULP_MEASURED)


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fr = _helper("finalize_reference")
FAMILIES = fr.all_cases()
USED = set()  # the families some test of this module walks (test_asserted_launch_records_cover_every_kernel_and_branch)


def _family(name):
    USED.add(name)
    return FAMILIES[name]


def _by_name(name):
    return {c.name: c for c in _family(name)}


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


@contextmanager
def _switches(eng, names):
    for n in names:
        eng.diag_set(n, 1)
    try:
        yield
    finally:
        for n in names:
            eng.diag_set(n, 0)


def _upload(eng, inp):
    acc, raw = eng.to_device(inp.acc), eng.to_device(inp.raw)
    cnt = eng.to_device(inp.cnt) if inp.cnt is not None else None
    assert acc.data_ptr() % 16 == 0 and raw.data_ptr() % 16 == 0
    return acc, cnt, raw


def _run(eng, c, inp=None, want_prob=False, out=None):
    """one case on the device -> (mask, prob or None, launch record); the record is held to expected_ran(c) first"""
    inp = inp if inp is not None else fr.build(c)
    Z, Y, X = c.shape
    if not c.exempt:  # the reference alone, before the device is looked at
        kept, removed = fr.shares(inp.keep, inp.raw[:, :Y, :X] > 0)
        assert kept >= 0.05 and removed >= 0.05, (c.name, kept, removed)
    acc, cnt, raw = _upload(eng, inp)
    with _switches(eng, c.switches):
        if c.z_abs0 is None:
            res = eng.finalize(acc, cnt, raw, c.shape, c.threshold, c.radius, c.zblock, want_prob=want_prob, out=out)
        else:
            assert out is None
            res = eng.finalize_slab(acc, cnt, raw, c.z_abs0, (Y, X), c.threshold, c.radius, c.zblock, want_prob=want_prob)
    ran = eng.finalize_ran()
    assert ran == fr.expected_ran(c), (c.name, ran, fr.expected_ran(c))
    mask, prob = res if want_prob else (res, None)
    return mask.cpu().numpy(), (prob.cpu().numpy() if want_prob else None), ran


def _check(eng, c, want=None, inp=None):
    """the case's mask equals the reference over the whole volume; `want`: the fields of the launch record the case is named for"""
    inp = inp if inp is not None else fr.build(c)
    mask, _, ran = _run(eng, c, inp)
    for k, v in (want or {}).items():
        assert ran[k] == v, (c.name, k, ran)
    np.testing.assert_array_equal(mask, inp.mask, err_msg=f"{c.name} {ran}")
    return ran


# ---- x/y distance, fused ------------------------------------------------------------------------------------------------------
XY_CHUNK_WANT = {
    2048: dict(xy_form=0, nc=1, raw_vec=1, dist_vec=1), 2049: dict(xy_form=0, nc=2, raw_vec=0, dist_vec=0),
    4096: dict(xy_form=0, nc=2, raw_vec=1, dist_vec=1), 4097: dict(xy_form=0, nc=4, raw_vec=0, dist_vec=0),
    8192: dict(xy_form=0, nc=4, raw_vec=1, dist_vec=1), 8193: dict(xy_form=1, nc=0, y_v=1),
    2056: dict(xy_form=0, nc=2, raw_vec=1, dist_vec=1), 4104: dict(xy_form=0, nc=4, raw_vec=1, dist_vec=1),
    4099: dict(xy_form=0, nc=4, raw_vec=0, dist_vec=0),
}


@pytest.mark.parametrize("c", _family("xy_chunks"), ids=lambda c: c.name)
def test_fused_xy_at_the_chunk_count_boundaries(eng, c):
    """erode_xy_kernel<1 / 2 / 4> on either side of 256 and 512 chunks per row, vector and ragged; 8193 leaves the fused kernel.
    Smallest shape: (2, 3, X) - two planes, a first, an inner and a last row."""
    _check(eng, c, XY_CHUNK_WANT[c.shape[2]])


@pytest.mark.parametrize("c", _family("xy_small"), ids=lambda c: c.name)
def test_fused_xy_on_small_rows(eng, c):
    """rows of three chunks, of a chunk and a ragged one, of exactly one chunk, of less than one, of one voxel"""
    _check(eng, c, dict(xy_form=0, nc=1, dist_vec=int(c.shape[2] % 8 == 0)))


@pytest.mark.parametrize("c", _family("xy_rows"), ids=lambda c: c.name)
def test_fused_xy_double_buffer_and_prefetch(eng, c):
    """Y = 1 (no backward scan, nothing to prefetch), 2, 3 and 6 rows through the double-buffered mask and the prefetched rows, with
    the vector (X = 24) and the voxel-by-voxel (X = 13) backward scan"""
    _check(eng, c, dict(xy_form=0, nc=1))


def test_fused_xy_padded_rows_that_break_one_alignment_each(eng):
    """X = 16 in rows of 19: the raw rows are unaligned, the distances are not.  X = 13 in rows of 16: aligned raw rows with a
    ragged last chunk, voxel-by-voxel stores."""
    cases = _by_name("xy_padding")
    _check(eng, cases["X16_Xp19"], dict(xy_form=0, raw_vec=0, dist_vec=1))
    _check(eng, cases["X13_Xp16"], dict(xy_form=0, raw_vec=1, dist_vec=0))


@pytest.mark.parametrize("X", fr.WINDOW_X)
def test_reach_of_the_64_bit_windows(eng, X):
    """rows with one zero each - at x = 0, 7, 8, 63, 64, X - 8, X - 1 - at radius 56 (cap 57: the farthest the windows of
    erode_xy_kernel and erode_x_bits_kernel see) and 57 (the log-step kernel takes over), over row lengths of every chunk phase.
    The x distance is the binding one: alone (one row per plane, one plane per z-block), behind the y scan (a zero-free second
    row) and behind the z scan (a zero-free second plane), fused and through the separate passes; radius 56 and 57 take the
    two-sweep z kernel, <4> or <1> by X % 4."""
    cs = [c for c in _family("windows") if c.shape[2] == X]
    assert len(cs) == 9
    for c in cs:
        form = 2 if c.radius == 57 else 1 if c.switches else 0
        _check(eng, c, dict(xy_form=form, z_form=1, z_v=4 if X % 4 == 0 else 1, nblk=c.shape[0] // c.zblock))


# ---- separate passes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _family("split"), ids=lambda c: c.name)
def test_separate_x_and_y_passes(eng, c):
    """erode_x_bits_kernel + erode_y_kernel<4> (X = 24, 8200) / <1> (X = 13, 8193): under "erode_xy_split" at small rows, and
    unswitched beyond 8192 voxels per row"""
    X = c.shape[2]
    _check(eng, c, dict(xy_form=1, nc=0, y_v=4 if X % 4 == 0 else 1, raw_vec=int(X % 8 == 0), dist_vec=int(X % 8 == 0)))


@pytest.mark.parametrize("c", _family("logstep"), ids=lambda c: c.name)
def test_log_step_x_kernel_beyond_cap_57(eng, c):
    """erode_x_kernel at radius 57 (the first it takes), 100 and 253 (the largest) with single zeros far apart, so that voxels lie
    beyond the radius; X = 301 runs erode_y_kernel<1> and erode_z_final_kernel<1>"""
    v = 4 if c.shape[2] % 4 == 0 else 1
    _check(eng, c, dict(xy_form=2, y_v=v, z_form=1, z_v=v, raw_vec=0, dist_vec=0))


# ---- z decision ---------------------------------------------------------------------------------------------------------------
def _z_want(c):
    two = c.radius > 31 or "erode_z_two_sweeps" in c.switches
    return dict(z_form=int(two), z_v=4 if c.shape[2] % 4 == 0 else 1)


@pytest.mark.parametrize("X", [8, 7])
@pytest.mark.parametrize("radius,switches", fr.Z_RADII, ids=[f"r{r}{'_two_sweeps' if sw else ''}" for r, sw in fr.Z_RADII])
def test_z_decision_over_stack_depths(eng, X, radius, switches):
    """erode_z_shift_kernel<4 / 1> at radius 0, 1, 30 and 31 (the last it takes), erode_z_final_kernel<4 / 1> at 32 and, switched, at
    1 and 30, on stacks of 1, 2, 3 and 5 planes (fewer than, and one more than, the pipeline's four), of radius, radius + 1 and
    2 * radius + 3 planes and of 150.  Planes of 5 x 8 / 5 x 7 with few zeros: z is the binding direction."""
    tag = f"X{X}_r{radius}{'_two' if switches else ''}_Z"
    cs = [c for c in _family("z_depth") if c.name.startswith(tag)]
    assert [c.shape[0] for c in cs] == fr.z_depths(radius)
    for c in cs:
        _check(eng, c, dict(_z_want(c), nblk=1, zphase=0))


@pytest.mark.parametrize("X", [8, 7])
@pytest.mark.parametrize("radius,switches", [(3, ()), (30, ()), (32, ()), (3, fr.TWO)], ids=["r3", "r30", "r32", "r3_two_sweeps"])
def test_z_decision_over_zblocks(eng, X, radius, switches):
    """z-blocks of 1, 2, radius - 1, radius, radius + 1 planes, of a non-divisor of Z and of more than Z planes"""
    tag = f"X{X}_r{radius}{'_two' if switches else ''}_zb"
    cs = [c for c in _family("z_blocks") if c.name.startswith(tag)]
    Z = 2 * radius + 3
    assert [c.zblock for c in cs] == fr.z_blocks_of(radius, Z) and any(Z % c.zblock for c in cs) and cs[-1].zblock > Z
    for c in cs:
        _check(eng, c, dict(_z_want(c), nblk=-(-Z // min(c.zblock, Z)), zphase=0))


@pytest.mark.parametrize("X", [8, 7])
@pytest.mark.parametrize("zblock,radius", [(b, r) for b, r, _ in fr.SLABS])
def test_finalize_slab_at_every_phase(eng, X, zblock, radius):
    """finalize_slab against finalize_reference(..., z_abs0) on every plane of the slab: z_abs0 % zblock = 0, 1 and zblock - 1,
    slabs shorter than a block, slabs that begin and end inside one; one sweep and two sweeps"""
    cs = [c for c in _family("z_slabs") if c.name.startswith(f"X{X}_r{radius}_") and c.zblock == zblock]
    assert {c.z_abs0 % zblock for c in cs} >= {0, 1, zblock - 1}
    assert any(c.shape[0] < zblock for c in cs)
    for c in cs:
        blocks = fr.zblocks(c.shape[0], zblock, c.z_abs0)
        _check(eng, c, dict(_z_want(c), nblk=(c.z_abs0 % zblock + c.shape[0] + zblock - 1) // zblock, zphase=c.z_abs0 % zblock))
        assert len(blocks) <= (c.z_abs0 % zblock + c.shape[0] + zblock - 1) // zblock


@pytest.mark.parametrize("c", _family("acc_unaligned"), ids=lambda c: c.name)
def test_z_shift_kernel_with_rows_of_sums_off_the_16_byte_grid(eng, c):
    """X % 4 == 0 in rows of Xp = 10 (Xp % 4 != 0): erode_z_shift_kernel<4> reads its sums one by one; Xp = 12 beside it: 16-byte
    loads"""
    _check(eng, c, dict(z_form=0, z_v=4, acc_vec=int(c.pad[1] % 4 == 0)))


# ---- padding ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _family("padding"), ids=lambda c: c.name)
def test_padding_is_never_read_into_the_result(eng, c):
    """Yp > Y and Xp > X with the padding of raw once all zero and once all 65535, the padding of the sums NaN and of the counts 0:
    the two results are identical and equal the reference, through the fused, the separate and the log-step x/y kernels and both
    z kernels"""
    zero, poison = fr.build(c, 0), fr.build(c, 65535)
    Z, Y, X = c.shape
    assert (zero.raw[:, Y:] == 0).all() and (zero.raw[:, :, X:] == 0).all() and (poison.raw[:, Y:] == 65535).all() and (poison.raw[:, :, X:] == 65535).all()
    assert np.isnan(zero.acc[:, Y:]).all() and np.isnan(zero.acc[:, :, X:]).all()
    np.testing.assert_array_equal(zero.mask, poison.mask)
    m0, _, _ = _run(eng, c, zero)
    m1, _, _ = _run(eng, c, poison)
    np.testing.assert_array_equal(m0, zero.mask)
    np.testing.assert_array_equal(m1, m0)


# ---- decision -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _family("decision"), ids=lambda c: c.name)
def test_decision_thresholds_and_planted_voxels(eng, c):
    """thresholds 0.5, 0.3 and 0.9 with and without a count map, through the decision code of all four z instantiations; planted on
    voxels the erosion keeps: sums of +0 and -0 (foreground at 0.5: the comparison is >=), 0 / 0 (background), x / 0 (foreground
    for x > 0, background for x < 0) and +-1000 (what skipped windows contribute)"""
    inp, where = fr.plant_decision(c, fr.build(c))
    mask, _, _ = _run(eng, c, inp)
    np.testing.assert_array_equal(mask, inp.mask)
    if c.threshold == 0.5:
        for p, (_, _, fg_cnt, fg_mean) in zip(where, fr.PLANTED):
            assert inp.keep[p] == 1 and mask[p] == int(fg_cnt if c.cnt else fg_mean), (p, mask[p])


# ---- prob ---------------------------------------------------------------------------------------------------------------------
def _finalize_raw(eng, c, acc, cnt, raw, out, prob):
    Z, Y, X = c.shape
    Yp, Xp = int(acc.shape[-2]), int(acc.shape[-1])
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    eng._enter()
    with _switches(eng, c.switches):
        eng._check(eng.lib.dlv_finalize_dev(eng.ctx, ptr(acc), ptr(cnt), ptr(raw), Yp, Xp, Z, Y, X, float(c.threshold), c.radius, c.zblock,
                                            ptr(out), ptr(prob)))
    eng._leave()


def test_prob_values(eng, capsys):
    """`prob` is written for every voxel, eroded or not (the buffer is prefilled with 7, which no sigmoid is), is NaN where the mean
    is NaN, and elsewhere lies within PROB_ULP_BOUND units in the last place of the fp64 sigmoid of the float32 mean rounded to
    float32 - over the decision cases at threshold 0.5 (all four z instantiations, with and without a count map, the planted
    +-0, x / 0, 0 / 0 and +-1000 included), a padded case and a slab.  The largest distance is printed before it is asserted."""
    import torch

    worst = 0
    cs = [c for c in _family("decision") if c.threshold == 0.5] + [_by_name("padding")["X16_Xp19"], _by_name("padding")["X24_Xp27_two"]]
    for c in cs:
        inp, _ = fr.plant_decision(c, fr.build(c))
        acc, cnt, raw = _upload(eng, inp)
        out = torch.full(c.shape, 0xAB, dtype=torch.uint8, device=eng.device)
        prob = torch.full(c.shape, 7.0, dtype=torch.float32, device=eng.device)
        _finalize_raw(eng, c, acc, cnt, raw, out, prob)
        assert eng.finalize_ran() == fr.expected_ran(c)
        np.testing.assert_array_equal(out.cpu().numpy(), inp.mask)
        got = prob.cpu().numpy()
        assert (got != 7.0).all(), c.name
        assert (inp.keep == 0).any() and (inp.mask == 0).any()
        nan = np.isnan(inp.sig)
        assert nan.any() == (c.cnt and True)
        np.testing.assert_array_equal(np.isnan(got), nan, err_msg=c.name)
        assert ((got[~nan] >= 0) & (got[~nan] <= 1)).all()
        d = int(fr.ulp_distance(got[~nan], inp.sig[~nan]).max())
        worst = max(worst, d)
        with capsys.disabled():
            print(f"\nprob {c.name}: largest distance {d} ulp")
        assert d <= PROB_ULP_BOUND, (c.name, d)
    slab = next(c for c in _family("z_slabs") if c.z_abs0 % c.zblock == 1 and not c.exempt)
    mask, prob, _ = _run(eng, slab, want_prob=True)
    inp = fr.build(slab)
    np.testing.assert_array_equal(mask, inp.mask)
    d = int(fr.ulp_distance(prob, inp.sig).max())
    worst = max(worst, d)
    with capsys.disabled():
        print(f"\nprob {slab.name}: largest distance {d} ulp; over all cases {worst} ulp (bound {PROB_ULP_BOUND})")
    assert worst <= PROB_ULP_BOUND


# ---- stores stay inside -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _family("guards"), ids=lambda c: c.name)
def test_stores_stay_inside_out(eng, c):
    """out = planes 1 .. Z of a (Z + 2, Y, X) tensor filled with 0xAB: both guard planes are untouched, the planes between equal
    the reference - voxel-by-voxel stores (X = 13), 4-byte stores (X = 16) and the widest rows of erode_xy_kernel<2> (X = 2056)"""
    import torch

    Z, Y, X = c.shape
    buf = torch.full((Z + 2, Y, X), 0xAB, dtype=torch.uint8, device=eng.device)
    mask, _, _ = _run(eng, c, out=buf[1:Z + 1])
    host = buf.cpu().numpy()
    assert (host[0] == 0xAB).all() and (host[Z + 1] == 0xAB).all()
    np.testing.assert_array_equal(host[1:Z + 1], fr.build(c).mask)
    np.testing.assert_array_equal(mask, fr.build(c).mask)


# ---- coverage -----------------------------------------------------------------------------------------------------------------
def test_asserted_launch_records_cover_every_kernel_and_branch(eng):
    """Every case of the table is walked by a test above, and every one of them holds its launch record to expected_ran, so the
    union of those records is what this module asserts: erode_xy_kernel<1 / 2 / 4>, both separate x kernels with erode_y_kernel<4>
    and <1>, both z kernels in both instantiations, both values of raw_vec, dist_vec and acc_vec, and a zphase != 0.  The radius-32
    cases pin the erode_iters <= 31 branch: they must report the two-sweep kernel unswitched, radius 31 the one-sweep kernel."""
    assert USED == set(FAMILIES)
    records = [fr.expected_ran(c) for cs in FAMILIES.values() for c in cs]
    assert fr.coverage(records) == set()
    for X in (8, 7):
        for r, form in ((31, 0), (32, 1)):
            c = next(c for c in FAMILIES["z_depth"] if c.name == f"X{X}_r{r}_Z{2 * r + 3}")
            assert not c.switches and _check(eng, c)["z_form"] == form
