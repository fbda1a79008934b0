"""Putting logits into the accumulator, checked per voxel.

1. Whole passes with a checkpoint whose final conv has weight 0 and bias c: every forwarded voxel has the logit c exactly in every
   format, so a pass leaves small integers in acc and cnt - independent of summation order - that are compared BIT FOR BIT with
   the numpy restatement of the window list (tests/helpers/blend_reference.py, pinned against the oracle's loop in
   tests/test_blend_reference_cpu.py).  A window written one voxel off under a flip, added twice at a clamped edge, dropped
   between two lanes or counted in the wrong shard changes an integer somewhere.  Rows: formats and flips, with and without the
   count map, batch sizes and pipeline lanes, repeat and accumulation into pre-filled buffers, a skip threshold, a shard of the
   window list on a slab, the sharded pass with its seam exchange, and the Gaussian blend (bitwise acc == 4 wsum with bias 4
   where only active windows reach; the map itself against the oracle's within the tolerances of the libm / torch erf).
2. The BLEND instantiation of final_conv_kernel alone through the layer hook (dlv_debug_layer16 with an accumulator): three
   disjoint windows at odd places of a pre-filled accumulator, every flip, constant and weighted, against
   oracle/layer_ref.py::final_logits in float64 with a derived bound; every voxel outside the windows bitwise untouched."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("blend_reference")
DEFAULT_LANES = 3  # (common.h: lanes_wanted)


# ---------------------------------------------------------------------------------------------------
# engines and cases
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    import torch
    from oracle import delivr_oracle as orc

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    n = orc.build_unet(seed=0)
    orc.randomize_affine(n, seed=1)
    return n


def _const_sd(net, bias):
    """the network with a final conv of weight 0 and bias `bias`: every logit is `bias`"""
    import torch

    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    sd["final_conv.weight"] = torch.zeros_like(sd["final_conv.weight"])
    sd["final_conv.bias"] = torch.full_like(sd["final_conv.bias"], float(bias))
    return sd


def _engine(sd):
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    e.load_state_dict({"state_dict": sd})
    return e


@pytest.fixture(scope="module")
def eng3(net):
    e = _engine(_const_sd(net, 3.0))
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng4(net):
    e = _engine(_const_sd(net, 4.0))
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng(net):
    """the network as it is (section 3 runs its final conv)"""
    e = _engine(net.state_dict())
    yield e
    e.close()


class Case:
    def __init__(self, name):
        import torch

        self.name = name
        self.shape, self.roi, self.overlap = ref.GEOMETRIES[name]
        self.vol = ref.volume(self.shape)
        self.act, self.skp, self.wins, self.wmax = ref.expected(self.vol, self.roi, self.overlap)
        self.v = torch.from_numpy(self.vol).cuda()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name)
        return made[name]

    return get


def _zeros(shape, dtype):
    import torch

    return torch.zeros(tuple(shape), dtype=dtype, device="cuda")


def _same(got, want, what):
    """bit for bit (integers in float32: no -0.0, no NaN), with the first differing voxel in the message"""
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, g.shape, want.dtype, want.shape)
    if not np.array_equal(g, want):
        bad = np.argwhere(g != want)
        at = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} voxels differ, first at {at}: got {g[at]}, expected {want[at]}")


def _pass(e, c, precision, flip=None, with_cnt=True, sw_batch=0, repeat=1, thr=0, bias=3):
    """one constant-blend pass into zeroed buffers, and the four assertions of a row"""
    import torch

    act, skp = (c.act, c.skp) if thr == 0 else ref.expected(c.vol, c.roi, c.overlap, skip_threshold=thr)[:2]
    acc = _zeros(c.shape, torch.float32)
    cnt = _zeros(c.shape, torch.uint8) if with_cnt else None
    p = e.make_sw_params(c.shape, c.roi, c.overlap, flip, thr, precision, sw_batch=sw_batch, repeat=repeat)
    st = e.sw_infer(p, c.v, acc, cnt)
    e.sync()
    what = f"{c.name} {precision} flip {flip} cnt {with_cnt} batch {sw_batch} repeat {repeat} thr {thr}"
    assert (st["n_windows"], st["n_skipped"]) == (len(c.wins), int((c.wmax <= thr).sum())), (what, st)
    assert np.array_equal(e.window_max(p, c.v), c.wmax), what
    _same(acc, ref.constant_acc(act, skp, bias, repeat), what + ": acc")
    if with_cnt:
        _same(cnt, ref.constant_cnt(act, skp, repeat), what + ": cnt")
    return st


# ---------------------------------------------------------------------------------------------------
# 2. whole passes, bit-exact
# ---------------------------------------------------------------------------------------------------
# fp32: gather_f32_kernel + blend_add_kernel (which also counts); 16-bit: final_conv_kernel<P, true> plain, the count by
# fill_add_kernel(value 0) on the lane's stream.  Skipped windows with a count map: the scalar loop of fill_add_kernel.
# Window maxima: cell path on E (x boundaries on the 8-voxel grid), general path on A - D.
# "bf16" is the mixed default (fp16 at level 0, bf16 below), "bf16_all" bf16 proper.
FORMAT_ROWS = (
    [(g, "fp32", None) for g in "ABCDE"] + [("B", "fp32", 2), ("C", "fp32", 3), ("D", "fp32", 4)]
    + [("A", "fp16", 2), ("C", "bf16_all", 3), ("D", "bf16", 4), ("E", "fp16", None), ("E", "bf16_all", 4), ("A", "bf16", None)]
    + [("B", fmt, flip) for fmt in ("fp16", "bf16_all") for flip in (None, 2, 3, 4)] + [("B", "bf16", 3), ("C", "fp16", 4)]
)


@pytest.mark.parametrize("geo,precision,flip", FORMAT_ROWS, ids=[f"{g}-{f}-flip{d}" for g, f, d in FORMAT_ROWS])
def test_constant_pass_formats_and_flips(eng3, cases, geo, precision, flip):
    _pass(eng3, cases(geo), precision, flip)


# without a count map the skipped fill takes its 16-byte branch where w, Xp and x0 are multiples of 4 (A: x starts 0, 12, 24; D:
# x starts 0, 6, .. - mixed within one launch; E: all of them) and the scalar loop elsewhere (B: Xp = 70, C: w = 21)
NOCNT_ROWS = [("E", "fp16", None), ("E", "fp32", 2), ("E", "bf16", 3), ("A", "bf16_all", 2), ("B", "fp16", 4), ("C", "fp32", None),
              ("D", "fp16", 3)]


@pytest.mark.parametrize("geo,precision,flip", NOCNT_ROWS, ids=[f"{g}-{f}-flip{d}" for g, f, d in NOCNT_ROWS])
def test_constant_pass_without_count_map(eng3, cases, geo, precision, flip):
    _pass(eng3, cases(geo), precision, flip, with_cnt=False)


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("sw_batch,lanes", [(1, 1), (1, 3), (3, 3), (3, 1), (0, 2)])
def test_constant_pass_batches_and_lanes(eng3, cases, sw_batch, lanes, precision):
    """sw_batch 1 on B: 36 forwards, up to 5 per colour class, rotating over the lanes; the count of each batch on its lane"""
    c = cases("B")
    try:
        eng3.set_lanes(lanes)
        st = _pass(eng3, c, precision, 2, sw_batch=sw_batch)
        _pass(eng3, c, precision, None, with_cnt=False, sw_batch=sw_batch)
    finally:
        eng3.set_lanes(DEFAULT_LANES)
    if sw_batch == 1:
        assert st["n_forward_launches"] == st["n_windows"] - st["n_skipped"]


@pytest.mark.parametrize("precision", ["fp16", "bf16_all", "fp32"])
def test_constant_pass_repeat(eng3, cases, precision):
    _pass(eng3, cases("B"), precision, 3, repeat=5)
    _pass(eng3, cases("E"), precision, None, with_cnt=False, repeat=5)


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("geo", ["B", "E"])
def test_four_passes_accumulate_onto_a_prefill(eng3, cases, geo, precision):
    """flip None, 2, 3, 4 into the same buffers, which start from integers of the test's choosing: four times the single
    expectation plus the pre-fill"""
    import torch

    c = cases(geo)
    rng = np.random.default_rng(5)
    acc0 = rng.integers(-30000, 30000, c.shape).astype(np.float32)
    cnt0 = rng.integers(0, 100, c.shape).astype(np.uint8)
    assert 4 * int((c.act + c.skp).max()) + 99 <= 255
    acc = torch.from_numpy(acc0).cuda()
    cnt = torch.from_numpy(cnt0).cuda()
    for flip in (None, 2, 3, 4):
        eng3.sw_infer(eng3.make_sw_params(c.shape, c.roi, c.overlap, flip, 0, precision), c.v, acc, cnt)
    eng3.sync()
    want = 4 * ref.constant_acc(c.act, c.skp, 3).astype(np.int64) + acc0.astype(np.int64)
    assert np.abs(want).max() < 2 ** 24
    _same(acc, want.astype(np.float32), f"{geo} {precision}: acc")
    _same(cnt, (4 * (c.act + c.skp) + cnt0).astype(np.uint8), f"{geo} {precision}: cnt")
    # ... and without the count map (the 16-byte fill on E) onto the same pre-fill
    acc = torch.from_numpy(acc0).cuda()
    for flip in (None, 2, 3, 4):
        eng3.sw_infer(eng3.make_sw_params(c.shape, c.roi, c.overlap, flip, 0, precision), c.v, acc)
    eng3.sync()
    _same(acc, want.astype(np.float32), f"{geo} {precision}: acc without cnt")


@pytest.mark.parametrize("geo,precision", [("B", "fp16"), ("B", "fp32"), ("E", "bf16")])
def test_constant_pass_skip_threshold(eng3, cases, geo, precision):
    """a threshold from the middle of the non-zero window maxima: windows with signal are skipped too"""
    c = cases(geo)
    live = np.sort(c.wmax[c.wmax > 0])
    thr = int(live[len(live) // 2])
    n_skip = int((c.wmax <= thr).sum())
    assert int((c.wmax <= 0).sum()) < n_skip < len(c.wmax)
    _pass(eng3, c, precision, 3, thr=thr)
    _pass(eng3, c, precision, None, with_cnt=False, thr=thr)


@pytest.mark.parametrize("geo,precision", [("B", "fp16"), ("B", "fp32"), ("E", "fp16"), ("C", "bf16_all")])
def test_constant_pass_shard_on_a_slab(eng3, cases, geo, precision):
    """windows [3, n - 2) on exactly the planes they touch: the helper restricted to those windows"""
    import torch

    c = cases(geo)
    d = c.roi[0]
    lo, hi = 3, len(c.wins) - 2
    z0 = int(c.wins[lo:hi, 0].min())
    z1 = int(c.wins[lo:hi, 0].max()) + d
    act, skp, _, _ = ref.expected(c.vol, c.roi, c.overlap, win_range=(lo, hi))
    assert act[:z0].sum() + skp[:z0].sum() + act[z1:].sum() + skp[z1:].sum() == 0
    slab_shape = (z1 - z0,) + tuple(c.shape[1:])
    vs = c.v[z0:z1].contiguous()
    for flip, with_cnt in ((2, True), (None, False)):
        acc = _zeros(slab_shape, torch.float32)
        cnt = _zeros(slab_shape, torch.uint8) if with_cnt else None
        q = eng3.make_sw_params(c.shape, c.roi, c.overlap, flip, 0, precision, win_range=(lo, hi), slab=(z0, z1 - z0))
        st = eng3.sw_infer(q, vs, acc, cnt)
        eng3.sync()
        assert (st["n_windows"], st["n_skipped"]) == (hi - lo, int((c.wmax[lo:hi] <= 0).sum())), st
        assert np.array_equal(eng3.window_max(q, vs), c.wmax[lo:hi])
        _same(acc, ref.constant_acc(act, skp, 3)[z0:z1], f"{geo} {precision} flip {flip}: acc")
        if with_cnt:
            _same(cnt, ref.constant_cnt(act, skp)[z0:z1], f"{geo} {precision} flip {flip}: cnt")


# ---- the sharded pass -------------------------------------------------------------------------------
def _sharded_case():
    """the volume of test_c_abi_sharded_pass_on_slabs_equals_the_single_device_pass"""
    from delivr_cfos_amd.synth import synth_volume_np

    shape, roi = (160, 64, 64), (32, 32, 32)
    vol = synth_volume_np(shape, seed=31, dense=True)
    vol[:, :12] = 0
    vol[70:110, 20:40, 30:50] = 0
    vol[100:] = 0
    return shape, roi, vol


def _sharded_run(sd, params_kw, gaussian):
    """three ranks on device 0, the weighted plan, every rank on its slab -> (plan, slabs, accs, cnts or wsums, stats, wmax)"""
    import torch
    from delivr_cfos_amd.engine import HipComm

    shape, roi, vol = _sharded_case()
    world, er, nb = 3, 7, 24
    comm = HipComm([0] * world)
    try:
        e0 = comm.engines[0]
        e0.load_state_dict({"state_dict": sd})
        comm.bcast_weights(0)
        v = e0.to_device(vol)
        p = e0.make_sw_params(shape, roi, 0.5, params_kw.get("flip"), 0, params_kw["precision"], blend="gaussian" if gaussian else "constant")
        wmax = e0.window_max(p, v)
        plan = comm.make_plan(p, np.where(wmax > 0, 1.0, 0.02).astype(np.float32))
        slabs, vols, accs, seconds = [], [], [], []
        for r in range(world):
            lo, hi = plan.slab(r, shape[0], er, nb)
            slabs.append((lo, hi - lo))
            vols.append(v[lo:hi].clone())
            accs.append(_zeros((hi - lo,) + shape[1:], torch.float32))
            seconds.append(_zeros((hi - lo,) + shape[1:], torch.float32 if gaussian else torch.uint8))
        if gaussian:
            stats = comm.sw_infer_sharded(p, plan, slabs, vols, accs, wsums=seconds)
        else:
            stats = comm.sw_infer_sharded(p, plan, slabs, vols, accs, seconds)
        torch.cuda.synchronize()
        out_a = [a.cpu().numpy() for a in accs]
        out_s = [s.cpu().numpy() for s in seconds]
    finally:
        comm.close()
    return shape, roi, vol, plan, slabs, out_a, out_s, stats, wmax


def test_sharded_constant_blend_equals_the_count_formula(net):
    """on the planes a rank owns, after the seam exchange: acc and cnt equal the numpy expectation exactly (integers: the seam's
    other association of the same terms changes nothing)"""
    shape, roi, vol, plan, slabs, accs, cnts, stats, wmax = _sharded_run(_const_sd(net, 3.0), {"precision": "fp16"}, False)
    act, skp, wins, wm = ref.expected(vol, roi, 0.5)
    assert np.array_equal(wmax, wm)
    assert sum(s["n_windows"] for s in stats) == len(wins) and sum(s["n_skipped"] for s in stats) == int((wm <= 0).sum())
    assert 0 < int((wm <= 0).sum()) < len(wins)
    want_a, want_c = ref.constant_acc(act, skp, 3), ref.constant_cnt(act, skp)
    covered, seams = 0, 0
    for r in range(3):
        olo, ohi = plan.z_owned[r]
        if ohi <= olo:
            continue
        lo = slabs[r][0]
        assert np.array_equal(accs[r][olo - lo:ohi - lo], want_a[olo:ohi]), r
        assert np.array_equal(cnts[r][olo - lo:ohi - lo], want_c[olo:ohi]), r
        covered += ohi - olo
        seams += len(plan.recvs(r))
    assert covered == shape[0] and seams >= 2


# ---- Gaussian blend -----------------------------------------------------------------------------------
def _check_gaussian(acc, ws, w_act, w_skp, act, skp, what):
    """acc, ws: float32 numpy.  Bitwise: with every logit 4 = 2^2 each term of acc is 4 x the term of wsum, and scaling by a power
    of two commutes with every rounding (no term is subnormal: the map's floor is ~5e-11), so acc == 4 wsum where only active
    windows reach, in whatever order and with or without FMA contraction.  Against the oracle's map (torch erf; the library's is
    libm's): the project's tolerances for this map."""
    only_act = (act > 0) & (skp == 0)
    assert float(only_act.mean()) >= 0.2
    assert np.array_equal(acc[only_act], 4.0 * ws[only_act]), (what, int((acc[only_act] != 4.0 * ws[only_act]).sum()))
    w_all = w_act + w_skp
    want = 4.0 * w_act - 1000.0 * w_skp
    mag = 4.0 * w_act + 1000.0 * w_skp
    core = w_all > 0.05
    print(f"RESULT gaussian {what}: max |wsum - W| / W {float((np.abs(ws - w_all) / w_all).max()):.3e} (core "
          f"{float((np.abs(ws - w_all) / w_all)[core].max()):.3e}), max |acc - want| / (4 W_act + 1000 W_skp) "
          f"{float((np.abs(acc - want) / mag).max()):.3e} (core {float((np.abs(acc - want) / mag)[core].max()):.3e}), "
          f"max |acc - want| / |want| {float((np.abs(acc - want) / np.maximum(np.abs(want), 1e-300)).max()):.3e}")
    np.testing.assert_allclose(ws, w_all, rtol=1e-3, atol=1e-9)
    np.testing.assert_allclose(ws[core], w_all[core], rtol=1e-5)
    np.testing.assert_allclose(acc, want, rtol=1e-3, atol=1e-9)
    # The 1e-5 of the core presupposes a sum dominated by the map's large entries.  acc weighs a skipped window's entries 250 x
    # more than an active one's, so "wsum > 0.05" does not say that of acc: on B the host arithmetic alone (glibc erff against
    # torch's erf, no GPU involved) differs by 1.7e-5 of |acc| at voxels where wsum > 0.05 but the -1000 W_skp part is made of
    # tail entries.  The same 1e-5 therefore holds where EACH part is a core sum (or absent), relative to the parts' magnitudes.
    parts_core = ((w_act > 0.05) | (act == 0)) & ((w_skp > 0.05) | (skp == 0))
    assert float(parts_core.mean()) >= 0.1
    assert np.all(np.abs(acc - want)[parts_core] <= 1e-5 * mag[parts_core]), float((np.abs(acc - want) / mag)[parts_core].max())


@pytest.mark.parametrize("flip", [None, 3])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("geo", ["A", "B"])
def test_gaussian_pass_bitwise_and_vs_oracle_map(eng4, cases, geo, precision, flip):
    import torch
    from oracle import delivr_oracle as orc

    c = cases(geo)
    imp = orc.gaussian_importance_map(c.roi, 0.125)
    w_act, w_skp = ref.expected_weighted(c.vol, c.roi, c.overlap, imp)
    acc = _zeros(c.shape, torch.float32)
    ws = _zeros(c.shape, torch.float32)
    p = eng4.make_sw_params(c.shape, c.roi, c.overlap, flip, 0, precision, sw_batch=3, blend="gaussian", sigma_scale=0.125, wsum=ws)
    st = eng4.sw_infer(p, c.v, acc)
    eng4.sync()
    assert (st["n_windows"], st["n_skipped"]) == (len(c.wins), int((c.wmax <= 0).sum()))
    _check_gaussian(acc.cpu().numpy(), ws.cpu().numpy(), w_act, w_skp, c.act, c.skp, f"{geo} {precision} flip {flip}")


def test_sharded_gaussian_blend_bitwise_and_vs_oracle_map(net):
    from oracle import delivr_oracle as orc

    shape, roi, vol, plan, slabs, accs, wss, stats, wmax = _sharded_run(_const_sd(net, 4.0), {"precision": "fp16"}, True)
    act, skp, wins, wm = ref.expected(vol, roi, 0.5)
    w_act, w_skp = ref.expected_weighted(vol, roi, 0.5, orc.gaussian_importance_map(roi, 0.125))
    assert sum(s["n_windows"] for s in stats) == len(wins) and sum(s["n_skipped"] for s in stats) == int((wm <= 0).sum())
    acc = np.zeros(shape, dtype=np.float32)
    ws = np.zeros(shape, dtype=np.float32)
    covered = 0
    for r in range(3):
        olo, ohi = plan.z_owned[r]
        if ohi <= olo:
            continue
        lo = slabs[r][0]
        acc[olo:ohi] = accs[r][olo - lo:ohi - lo]
        ws[olo:ohi] = wss[r][olo - lo:ohi - lo]
        covered += ohi - olo
    assert covered == shape[0]
    _check_gaussian(acc, ws, w_act, w_skp, act, skp, "sharded fp16")


# ---------------------------------------------------------------------------------------------------
# 3. final_conv_kernel<P, true> alone
# ---------------------------------------------------------------------------------------------------
F_SHAPE = (20, 72, 104)                      # 149760 voxels: more than the 131072-voxel grid stride, which neither W nor W H divides
F_ACC = (44, 150, 109)
F_STARTS = np.array([(0, 0, 0), (24, 1, 5), (3, 77, 2)])
F_SCALE = 3.0
F_BMIN = 1e-4


def _rnd(fmt):
    return (lambda t: t.half().float()) if fmt == "fp16" else (lambda t: t.bfloat16().float())


@pytest.fixture(scope="module")
def final_ref(net):
    """per format: inputs and the float64 reference of test_final_conv_vs_fp64 (same seed, same shape), computed once"""
    import torch
    from oracle import layer_ref as lr

    made = {}

    def get(fmt):
        if fmt not in made:
            g = torch.Generator().manual_seed(11)
            x = _rnd(fmt)(torch.randn((3, 32) + F_SHAPE, generator=g) * 1.5)
            ss = torch.stack([0.5 + 1.5 * torch.rand((3, 32), generator=g), 2 * torch.rand((3, 32), generator=g) - 1], dim=-1).contiguous()
            fc = net.final_conv
            r = lr.final_logits(x, ss, fc.weight.detach(), fc.bias.detach(), fmt)
            w = fc.weight.detach().double().reshape(1, 32, 1, 1, 1)
            # the bound of test_final_conv_vs_fp64: per channel the activation's error, then a 32-term fp32 sum
            bound = (w.abs() * 2.0 ** -20 * (1 + r["y"].abs())).sum(dim=1) + 32 * 2.0 ** -24 * (w * r["m"]).abs().sum(dim=1)
            made[fmt] = (x.cuda(), ss.cuda(), r["logits"].numpy(), bound.numpy())
        return made[fmt]

    return get


@pytest.fixture(scope="module")
def final_fill():
    """the pre-fill of acc and wsum and the weighted rows' factors: U(0.01, 1) with a few entries at 1e-6, so that the floor
    (bmin = 1e-4) engages - factors of the test's choosing, not the pass's map"""
    rng = np.random.default_rng(17)
    acc0 = rng.standard_normal(F_ACC).astype(np.float32) * 5
    ws0 = rng.random(F_ACC).astype(np.float32) * 3
    D, H, W = F_SHAPE
    bw = rng.uniform(0.01, 1.0, D + H + W).astype(np.float32)
    bw[[2, D - 1, D + 7, D + H - 1, D + H, D + H + 50]] = 1e-6
    for k in range(3):
        lo = (0, D, D + H)[k]
        assert not np.array_equal(bw[lo:lo + F_SHAPE[k]], bw[lo:lo + F_SHAPE[k]][::-1])  # orientation matters
    return acc0, ws0, bw


def test_final_blend_windows_are_disjoint_and_unaligned():
    assert np.prod(F_SHAPE) > 131072 and 131072 % F_SHAPE[2] and 131072 % (F_SHAPE[1] * F_SHAPE[2])
    seen = np.zeros(F_ACC, dtype=np.int32)
    for z, y, x in F_STARTS:
        seen[z:z + F_SHAPE[0], y:y + F_SHAPE[1], x:x + F_SHAPE[2]] += 1
    assert seen.max() == 1 and int(seen.sum()) == 3 * int(np.prod(F_SHAPE))
    assert F_ACC[2] % 4 and F_SHAPE[2] % 4 == 0 and any(int(s[2]) % 4 for s in F_STARTS) and any(int(s[1]) % 4 for s in F_STARTS)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("flip", [None, 2, 3, 4])
@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_final_conv_blend_vs_fp64(eng, final_ref, final_fill, fmt, flip, weighted):
    """acc0 + 3 g L with window voxel (z, y, x) of the flipped forward at the un-flipped place, g = max(bz by bx, bmin) at the
    VOLUME-orientation coordinate (plain: g = 1).  Bound: 3 g x (the plain final conv's bound) + 2^-22 (|acc0| + |3 g L|) - the
    two products of the factors, the scale, the product with the logit and the add, five fp32 roundings of 2^-24 each, rounded up
    to 2^-22 of the magnitudes; wsum: 2^-22 (|wsum0| + 3 g)."""
    import torch

    x, ss, L, lbound = final_ref(fmt)
    acc0, ws0, bw = final_fill
    D, H, W = F_SHAPE
    acc = torch.from_numpy(acc0).cuda()
    ws = torch.from_numpy(ws0).cuda() if weighted else None
    kw = dict(bw=torch.from_numpy(bw).cuda(), bmin=F_BMIN, wsum=ws) if weighted else {}
    rep = eng.debug_layer16(0, "final", 0, x, ss, flip_dim=flip, precision="fp16" if fmt == "fp16" else "bf16", acc=acc, starts=F_STARTS,
                            scale=F_SCALE, **kw)
    eng.sync()
    assert rep["norm_passes"] == 0, rep  # (the final conv activates on load)
    if weighted:
        b = bw.astype(np.float64)
        g = np.maximum(b[:D, None, None] * b[None, D:D + H, None] * b[None, None, D + H:], F_BMIN)
        assert 0.001 < float((g == F_BMIN).mean()) < 0.5  # the floor engages, and not everywhere
    else:
        g = np.ones(F_SHAPE)
    got = acc.cpu().numpy()
    want = acc0.astype(np.float64)
    bound = np.zeros(F_ACC)
    inside = np.zeros(F_ACC, dtype=bool)
    want_ws = ws0.astype(np.float64)
    bound_ws = np.zeros(F_ACC)
    for n, (z, y, xs) in enumerate(F_STARTS):
        sl = np.s_[z:z + D, y:y + H, xs:xs + W]
        Lf, bf = (L[n], lbound[n]) if flip is None else (np.flip(L[n], axis=flip - 2), np.flip(lbound[n], axis=flip - 2))
        term = F_SCALE * g * Lf
        bound[sl] = F_SCALE * g * bf + 2.0 ** -22 * (np.abs(acc0[sl]) + np.abs(term))
        want[sl] += term
        inside[sl] = True
        bound_ws[sl] = 2.0 ** -22 * (np.abs(ws0[sl]) + F_SCALE * g)
        want_ws[sl] += F_SCALE * g
    # outside the three windows: bitwise untouched
    assert np.array_equal(got[~inside].view(np.uint32), acc0[~inside].view(np.uint32))
    err = np.abs(got - want)
    ratio = np.where(inside, err / np.where(inside, bound, 1.0), 0.0)
    at = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))
    n_at = next(n for n, (z, y, xs) in enumerate(F_STARTS) if inside[at] and z <= at[0] < z + D and y <= at[1] < y + H and xs <= at[2] < xs + W)
    rel = tuple(int(a - s) for a, s in zip(at, F_STARTS[n_at]))
    what = f"{fmt} flip {flip} {'weighted' if weighted else 'plain'}"
    line = f"RESULT final blend {what}: acc worst |err| / bound {float(ratio.max()):.3f} in window {n_at} at {rel}, max |err| {float(err.max()):.3e}"
    worst_ws = 0.0
    if weighted:
        got_ws = ws.cpu().numpy()
        assert np.array_equal(got_ws[~inside].view(np.uint32), ws0[~inside].view(np.uint32))
        r_ws = np.where(inside, np.abs(got_ws - want_ws) / np.where(inside, bound_ws, 1.0), 0.0)
        worst_ws = float(r_ws.max())
        at_ws = tuple(int(v) for v in np.unravel_index(int(r_ws.argmax()), r_ws.shape))
        line += f"; wsum worst |err| / bound {worst_ws:.3f} at {at_ws}"
    print(line)
    assert float(ratio.max()) <= 1.0, line
    assert worst_ws <= 1.0, line


def test_final_conv_blend_refuses_bad_arguments(eng, final_ref, final_fill):
    import torch
    from delivr_cfos_amd._lib import DelivrHipError

    x, ss, _L, _b = final_ref("fp16")
    acc0, _ws0, bw = final_fill
    acc = torch.from_numpy(acc0).cuda()
    with pytest.raises(DelivrHipError):
        eng.debug_layer16(0, "final", 0, x, ss, flip_dim=5, precision="fp16", acc=acc, starts=F_STARTS, scale=F_SCALE)
    with pytest.raises(DelivrHipError):
        eng.debug_layer16(0, "final", 0, x, ss, precision="fp16", acc=acc, starts=F_STARTS, scale=float("inf"))
    with pytest.raises(DelivrHipError):  # the weight sums belong to the weighted blend
        eng.debug_layer16(0, "final", 0, x, ss, precision="fp16", acc=acc, starts=F_STARTS, wsum=torch.zeros_like(acc))
    for n, k, v in ((1, 2, 6), (2, 1, 79), (0, 2, -1), (0, 1, -1)):  # 6 + 104 > 109, 79 + 72 > 150: the hook's check of the planes
        bad = F_STARTS.copy()
        bad[n, k] = v
        with pytest.raises(DelivrHipError):
            eng.debug_layer16(0, "final", 0, x, ss, precision="fp16", acc=acc, starts=bad)
    bad = F_STARTS.copy()
    bad[1, 0] += 1  # 25 + 20 > 44 planes: only the caller knows how many there are
    with pytest.raises(ValueError):
        eng.debug_layer16(0, "final", 0, x, ss, precision="fp16", acc=acc, starts=bad)
    eng.sync()
    assert np.array_equal(acc.cpu().numpy().view(np.uint32), acc0.view(np.uint32))  # nothing was written
