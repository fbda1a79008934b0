"""Every instantiation of the register-resident-weights conv (conv_zreg_kernel.h), both upconv kernels of the folded UpCat
conv (upconv.hip) and the MFMA stem, each run on its own through the layer hook (dlv_debug_layer16) and compared with the
float64 references of oracle/layer_ref.py on the same 16-bit-rounded operands.

The hook reports which kernel ran, so each row of ZREG_ROWS proves that the instantiation it names was the one compared
(tests/test_layer_ref_cpu.py fails when conv_zreg.h declares an instantiation without a row).  Every row runs B = 3 windows
with their own data and their own per-(sample, channel) scale/shift, on a ragged shape (D not a multiple of 16, W not a
multiple of 32, H not a multiple of 8-row tiles), and checks the global maximum AND the mean error of every (sample,
channel): a mistake confined to one sample, one channel or one face of the window is not diluted by the rest."""
import os
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = {"fp16": (0.01, 1e-3), "bf16": (0.06, 6e-3)}  # max abs error, mean abs error per (sample, channel): the conv-block tolerances
SCALE_TOL = 1e-3  # relative error of the InstanceNorm scale (one lost partial of 64 moves the variance by ~1.5 %)

# inst: the z-reg instantiation the hook must report; op: "conv" (block li on c1 [+ c2] channels) or "folded" (block 16 from
# a fine skip tensor and an activated coarse one); act: the first input is raw and carries a scale/shift; upconv: the
# upconv kernel the folded conv must run
Row = namedtuple("Row", "inst op li c1 c2 shape act upconv")
_T8, _T16 = (33, 20, 72), (72, 32, 112)
_BASE = [
    ("c32_t8_a0", "conv", 1, 32, 0, _T8, False, None),
    ("c32_t8_a1", "conv", 17, 32, 0, _T8, True, None),
    ("c32_t16_a0", "conv", 1, 32, 0, _T16, False, None),
    ("c32_t16_a0", "conv", 17, 32, 0, (64, 64, 128), False, None),
    ("c32_t16_a1", "conv", 17, 32, 0, _T16, True, None),
    ("c64_t8_a0", "conv", 5, 64, 0, _T8, False, None),       # 64 -> 64: two output-channel blocks
    ("c64_t8_a0", "conv", 16, 32, 32, _T8, False, None),     # 32 + 32 concatenation
    ("c64_t8_a1", "conv", 16, 32, 32, _T8, True, None),      # the raw 32 of a 32 + 32 concatenation activated on load
    ("c32_t16_add", "folded", 16, 32, 32, (64, 64, 128), False, "upconv2m"),
    ("c32_t8_add", "folded", 16, 32, 32, (64, 48, 128), False, "upconv2m"),
    ("c32_t16_add", "folded", 16, 32, 32, (72, 64, 80), False, "upconv2"),    # coarse width 40: one tile per workgroup
    ("c32_t8_add", "folded", 16, 32, 32, (36, 52, 72), False, "upconv2"),     # coarse 18 x 26 x 36
    ("c32_t16_adda1", "folded", 16, 32, 32, (64, 64, 128), True, "upconv2m"),
    ("c32_t8_adda1", "folded", 16, 32, 32, (64, 48, 128), True, "upconv2m"),
    ("c32_t16_adda1", "folded", 16, 32, 32, (72, 64, 80), True, "upconv2"),
    ("c32_t8_adda1", "folded", 16, 32, 32, (36, 52, 72), True, "upconv2"),
]
ZREG_ROWS = [Row(f"{prefix}_{b[0]}", *b[1:]) for prefix in ("f16", "bf16") for b in _BASE]


def _fmt_of(row):
    return "fp16" if row.inst.startswith("f16_") else "bf16"


def _rnd(fmt):
    return (lambda t: t.half().float()) if fmt == "fp16" else (lambda t: t.bfloat16().float())


@pytest.fixture(scope="module")
def net():
    import torch

    from oracle import delivr_oracle as orc

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    n = orc.build_unet(seed=0)
    orc.randomize_affine(n, seed=1)
    return n


@pytest.fixture(scope="module")
def eng(net):
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    e.load_state_dict({"state_dict": net.state_dict()})
    yield e
    e.close()


def _block(net, li):
    from delivr_cfos_amd.engine import CONV_BLOCKS

    mod = net
    for part in CONV_BLOCKS[li].split("."):
        mod = getattr(mod, part)
    return mod


def _ss(g, B, C):
    """a scale/shift of its own for every (sample, channel): scale U(0.5, 2), shift U(-1, 1) - as float2 [B][C]"""
    import torch

    return torch.stack([0.5 + 1.5 * torch.rand((B, C), generator=g), 2 * torch.rand((B, C), generator=g) - 1], dim=-1).contiguous()


def _region(idx, shape, tyt):
    """where a voxel (z, y, x) of a window sits relative to the kernels' structure"""
    z, y, x = idx
    D, H, W = shape
    faces = sum(c == 0 or c == n - 1 for c, n in zip(idx, shape))
    if faces:
        return {1: "face", 2: "edge", 3: "corner"}[faces] + f" at {idx}"
    if y % tyt in (0, tyt - 1) or x % 32 in (0, 31):
        return f"tile seam at {idx}"
    if z % 16 in (0, 15):
        return f"z-chunk boundary at {idx}"
    return f"interior at {idx}"


def _check_final(out, ref, fmt, shape, tyt, what):
    """global max AND mean |error| of every (sample, channel); returns the max error"""
    tmax, tmean = TOL[fmt]
    err = (out.double() - ref).abs()
    mx = float(err.max())
    per = err.mean(dim=(2, 3, 4))
    n, c = np.unravel_index(int(per.argmax()), per.shape)
    flat = int(err.argmax())
    nb, cb, *zyx = np.unravel_index(flat, err.shape)
    where = f"{what}: max |err| {mx:.3e} at sample {nb} channel {cb}, {_region(tuple(int(v) for v in zyx), shape, tyt)}; " \
            f"worst mean |err| {float(per.max()):.3e} at sample {n} channel {c}"
    print(where)
    assert mx < tmax, where
    assert float(per.max()) < tmean, where
    return mx


def _check_scale(ss_gpu, ref, raw_scale, what, tol=SCALE_TOL):
    """kind 3: the scale applies to the STORED raw tensor (raw_scale times the conv's): scale * raw_scale = fp64 scale"""
    sc = ss_gpu[..., 0].double() * raw_scale
    rel = ((sc - ref["scale"]) / ref["scale"]).abs()
    n, c = np.unravel_index(int(rel.argmax()), rel.shape)
    msg = f"{what}: scale rel err {float(rel.max()):.3e} at sample {n} channel {c}"
    print(msg)
    assert float(rel.max()) < tol, msg
    return float(rel.max())


def _inputs(row, B, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    D, H, W = row.shape
    x1 = torch.randn((B, row.c1, D, H, W), generator=g)
    ss = _ss(g, B, row.c1) if row.act else None
    if row.op == "folded":  # an activated coarse tensor: Mish output range
        x2 = torch.nn.functional.mish(torch.randn((B, 32, D // 2, H // 2, W // 2), generator=g))
    else:
        x2 = torch.randn((B, row.c2, D, H, W), generator=g) if row.c2 else None
    return x1, ss, x2


def _reference(net, row, fmt, x1, ss, x2):
    from oracle import layer_ref as lr

    blk = _block(net, row.li)
    N = blk.adn.N
    if row.op == "folded":
        dc = net.upcat_1.upsample.deconv
        return lr.folded_upcat(x1, x2, blk.conv.weight.detach(), blk.conv.bias.detach(), dc.weight.detach(), dc.bias.detach(),
                               N.weight.detach(), N.bias.detach(), fmt, ss_skip=ss)
    return lr.conv_block(x1, blk.conv.weight.detach(), blk.conv.bias.detach(), N.weight.detach(), N.bias.detach(), fmt, ss1=ss, x2=x2)


def _switch_values(row):
    # the activating instantiations run where the dispatcher lets block li activate its first input (fuse_layers bit li);
    # the default (bit 17 only) otherwise
    return {"fuse_layers": (1 << 17) | ((1 << row.li) if row.act else 0)}


def _switches(eng, row):
    for name, value in _switch_values(row).items():
        eng.diag_set(name, value)


_LEVEL = (0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0)


def _planned(row, fmt, B):
    """what the plan (csrc/layer_plan.h through dlv_diag_plan) says of block row.li on row.shape under the row's switches: the
    z-reg instantiation and the upconv kernel in the words of the hook's report.  The plan is of a whole forward: the window
    whose level of block li has the row's shape."""
    from delivr_cfos_amd.engine import layer_plan

    window = tuple(n << _LEVEL[row.li] for n in row.shape)
    plan = layer_plan(window, _switch_values(row), precision="fp16" if fmt == "fp16" else "bf16_all", batch=B)
    c = plan["conv"][row.li]
    inst = None
    if c["kernel"] == "ZREG":
        # (the plan is of a forward, where the first input of block li is raw; a row that hands the hook a final tensor leaves the
        # conv nothing to activate: plan_conv with raw1 = false)
        act = bool(c["act_on_load"]) and row.act
        assert bool(c["act_on_load"]) or not row.act, c
        suffix = ("adda1" if act else "add") if c["folded"] else ("a1" if act else "a0")
        inst = f"{'f16' if fmt == 'fp16' else 'bf16'}_c{c['cin']}_t{c['tile_rows']}_{suffix}"
    upconv = [l.split("_")[0] for l, _, _ in plan["labels"] if l.startswith("upconv2")]
    assert len(upconv) == (1 if plan["conv"][16]["folded"] else 0), plan["labels"]  # (a forward's one upconv launch belongs to block 16)
    return inst, bool(c["folded"]), upconv[0] if c["folded"] else None


def _run(eng, row, fmt, kind, x1, ss, x2):
    return eng.debug_layer16(kind, row.op, row.li, x1.cuda(), None if ss is None else ss.cuda(), None if x2 is None else x2.cuda(),
                             precision=fmt)


def _rnd_in(fmt, x1, ss, x2):
    r = _rnd(fmt)
    return r(x1), ss, None if x2 is None else r(x2)


@pytest.mark.parametrize("row", ZREG_ROWS, ids=[f"{r.inst}-{r.op}{r.li}-{'x'.join(map(str, r.shape))}" for r in ZREG_ROWS])
def test_zreg_instantiation_vs_fp64(eng, net, row):
    fmt = _fmt_of(row)
    B = 3
    x1, ss, x2 = _rnd_in(fmt, *_inputs(row, B, seed=hash((row.li, row.shape, row.act)) % 10000))
    ref = _reference(net, row, fmt, x1, ss, x2)
    _switches(eng, row)
    try:
        out, rep = _run(eng, row, fmt, 0, x1, ss, x2)
        ssg, rep3 = _run(eng, row, fmt, 3, x1, ss, x2)
    finally:
        eng.diag_set("fuse_layers", 1 << 17)
    assert rep["zreg"] == row.inst and rep3["zreg"] == row.inst, (rep, row.inst)
    assert rep["upconv"] == row.upconv, rep
    # ... and it is what the plan says of this shape under these switches: instantiation (format, Cin, tile rows, activation
    # on load, addend) and an upconv launch exactly where the plan folds
    p_inst, p_folded, p_upconv = _planned(row, fmt, B)
    assert p_inst == rep["zreg"], (p_inst, rep)
    assert p_folded == (rep["upconv"] is not None) == (row.op == "folded"), (p_folded, rep)
    assert p_upconv == rep["upconv"], (p_upconv, rep)
    tyt = 16 if "_t16_" in row.inst else 8
    what = f"{row.inst} {row.op} block {row.li} {row.shape}"
    mx = _check_final(out.cpu(), ref["out"], fmt, row.shape, tyt, what)
    se = _check_scale(ssg.cpu(), ref, rep3["raw_scale"], what)
    print(f"RESULT {what}: max {mx:.3e} scale {se:.3e}")


# ---------------------------------------------------------------------------------------------------
# a whole forward runs the launches its plan lists
# ---------------------------------------------------------------------------------------------------
# 16 x 48 x 64: 8-row z-reg tiles at level 0; 16 x 128 x 64: the smallest window with 16-row tiles; 24 x 40 x 72: odd levels
# (12 x 20 x 36 -> 6 x 10 x 18 -> 3 x 5 x 9): replicate padding and the pool-then-normalise path
@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("window", [(16, 48, 64), (16, 128, 64), (24, 40, 72)], ids=lambda w: "x".join(map(str, w)))
def test_forward_launches_the_labels_of_its_plan(eng, window, fmt):
    import torch

    from delivr_cfos_amd.engine import layer_plan

    plan = layer_plan(window, {}, precision=fmt)
    assert plan["conv"][1]["tile_rows"] == (16 if window == (16, 128, 64) else 8) and plan["conv"][1]["kernel"] == "ZREG"
    assert any(q["norm_after"] for q in plan["pool"]) == (window == (24, 40, 72))
    vol = torch.randint(1, 60000, window, generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(torch.uint16).cuda()
    acc = torch.zeros(window, dtype=torch.float32, device="cuda")
    eng.prof_reset()
    eng.prof_enable(True)
    try:
        eng.sw_infer(eng.make_sw_params(window, window, 0.5, None, 0, fmt), vol, acc)  # one window
        eng.sync()
        ran = eng.prof_report()
    finally:
        eng.prof_enable(False)
        eng.prof_reset()
    tiler = {"window_max_u16", "skip_fill_f32"}  # (sw_infer.hip's own launches around the forward)
    planned = {l for l, _, _ in plan["labels"]}
    assert set(ran) - tiler == planned, (sorted(set(ran) - tiler - planned), sorted(planned - set(ran)))
    # one pass of one window: as many launches under each label as the plan lists, with its algorithmic FLOPs and bytes
    for label in planned:
        n = sum(1 for l, _, _ in plan["labels"] if l == label)
        assert ran[label]["launches"] == n, (label, ran[label], n)
        assert ran[label]["flops"] == sum(f for l, f, _ in plan["labels"] if l == label), label
        assert ran[label]["bytes"] == sum(b for l, _, b in plan["labels"] if l == label), label
    assert bool(torch.isfinite(acc).all())


# ---------------------------------------------------------------------------------------------------
# the stem: uint16 windows, bias in its statistics, two passes (statistics, then the activating pass)
# ---------------------------------------------------------------------------------------------------
def _stem_ref(net, vol, fmt, flip_dim=None, shift=0):
    from oracle import layer_ref as lr

    blk = _block(net, 0)
    w_scale = (2.0 ** -8 if fmt == "fp16" else 1.0) * 2.0 ** -shift
    return lr.stem(vol, blk.conv.weight.detach(), blk.conv.bias.detach(), blk.adn.N.weight.detach(), blk.adn.N.bias.detach(), fmt,
                   w_scale=w_scale, flip_dim=flip_dim)


def _stem_run(eng, kind, vol, fmt, flip_dim=None):
    import torch

    v = vol.to(torch.int32).to(torch.uint16).cuda()
    return eng.debug_layer16(kind, "stem", vol=v, flip_dim=flip_dim, precision=fmt)


def _stem_vol(seed, B, shape):
    """dense windows over the whole uint16 range (both bytes of the split in use, normalised values O(1)); window 0 saturated
    in a corner"""
    import torch

    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 65536, (B,) + shape, generator=g)
    v[0, :2, :2, :2] = 65535
    return v


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("flip_dim", [None, 2, 4])
def test_stem_vs_fp64(eng, net, fmt, flip_dim):
    shape = (20, 28, 72)  # D not a multiple of the 4-plane chunks x 8, H not of 8 rows, W not of 32 columns
    vol = _stem_vol(5, 3, shape)
    ref = _stem_ref(net, vol, fmt, flip_dim)
    out, rep = _stem_run(eng, 0, vol, fmt, flip_dim)
    ssg, rep3 = _stem_run(eng, 3, vol, fmt, flip_dim)
    raw, rep2 = _stem_run(eng, 2, vol, fmt, flip_dim)
    assert rep["stem"] and rep3["stem"] and rep["zreg"] is None
    what = f"stem {fmt} flip {flip_dim}"
    mx = _check_final(out.cpu(), ref["out"], fmt, shape, 8, what)
    se = _check_scale(ssg.cpu(), ref, rep3["raw_scale"], what)
    # the raw pass: the stored tensor is raw_scale * (conv + bias), rounded once to the format
    from oracle import layer_ref as lr

    sr = lr.stored_raw(ref, rep2["raw_scale"], rep2["drops_bias"])
    # (one rounding to the format, relative; plus fp32 summation, against the channel's spread)
    spread = sr.std(dim=(2, 3, 4))[:, :, None, None, None]
    rel = float(((raw.cpu().double() - sr).abs() / (sr.abs() + 1e-2 * spread)).max())
    print(f"RESULT {what}: max {mx:.3e} scale {se:.3e} raw rel {rel:.3e}")
    assert rel < (2.0 ** -10 if fmt == "fp16" else 2.0 ** -7), rel


# ---------------------------------------------------------------------------------------------------
# invariance: a window's result does not depend on its batch (z segments depend on B) or on the edge-step switch
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", ["f16_c32_t16_a1", "bf16_c32_t8_a0", "f16_c64_t8_a1", "bf16_c32_t16_adda1"])
def test_window_result_independent_of_batch_and_zreg_dbg(eng, net, inst):
    import torch

    row = next(r for r in ZREG_ROWS if r.inst == inst)
    fmt = _fmt_of(row)
    x1, ss, x2 = _rnd_in(fmt, *_inputs(row, 16, seed=77))

    def run(pick):  # the window x[5] inside a batch of the windows `pick`
        a1, s, a2 = (None if t is None else t[pick].contiguous() for t in (x1, ss, x2))
        o, rep = _run(eng, row, fmt, 0, a1, s, a2)
        q, _ = _run(eng, row, fmt, 3, a1, s, a2)
        assert rep["zreg"] == inst, rep
        at = pick.index(5)
        return o[at].cpu(), q[at].cpu()

    _switches(eng, row)
    try:
        res = {1: run([5]), 3: run([0, 5, 2]), 16: run(list(range(16)))}
        eng.diag_set("zreg_dbg", 1)
        try:
            res["dbg"] = run([0, 5, 2])
        finally:
            eng.diag_set("zreg_dbg", 0)
    finally:
        eng.diag_set("fuse_layers", 1 << 17)
    for k in (3, 16, "dbg"):
        assert torch.equal(res[k][0], res[1][0]), (inst, k, float((res[k][0] - res[1][0]).abs().max()))
        assert torch.equal(res[k][1], res[1][1]), (inst, k)


# ---------------------------------------------------------------------------------------------------
# statistics edges: a background window, a variance near eps (with a block shift), DC offsets
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_zero_and_tiny_variance_samples(eng, net, fmt):
    import torch

    row = Row("", "conv", 1, 32, 0, _T8, False, None)
    g = torch.Generator().manual_seed(9)
    x1 = torch.randn((3, 32) + _T8, generator=g)
    x1[1] = 0  # a background window: every raw value 0, variance 0
    # sample 2: raw variance about eps (the weights of block 1 give a raw std of ~0.3 per unit input std)
    x1[2] *= 1e-2
    x1 = _rnd(fmt)(x1)
    ref = _reference(net, row, fmt, x1, None, None)
    print(f"{fmt}: raw variance of sample 2 {float(ref['var'][2].min()):.2e} .. {float(ref['var'][2].max()):.2e} (eps 1e-5)")
    worst = {}
    for shift in (0, 3):
        eng.set_conv_shift(1, shift)
        try:
            out, rep = _run(eng, row, fmt, 0, x1, None, None)
            ssg, rep3 = _run(eng, row, fmt, 3, x1, None, None)
        finally:
            eng.set_conv_shift(1, 0)
        assert rep3["raw_scale"] == 2.0 ** -shift
        what = f"{fmt} block 1 zero / tiny-variance samples, shift {shift}"
        worst[shift] = (_check_final(out.cpu(), ref["out"], fmt, _T8, 8, what), _check_scale(ssg.cpu(), ref, rep3["raw_scale"], what))
    print("RESULT zero/tiny-variance", fmt, worst)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_stem_background_and_saturated_windows(eng, net, fmt):
    """window 0 all zero (background: raw = bias only, variance 0), window 1 nearly constant (variance near eps through
    STEM_SCALE^2), window 2 at 20000 +- 200 with saturated voxels"""
    import torch

    g = torch.Generator().manual_seed(3)
    shape = (20, 28, 72)
    vol = torch.zeros((3,) + shape, dtype=torch.long)
    vol[1] = (torch.rand(shape, generator=g) < 1e-3).long()
    vol[2] = (20000 + 200 * torch.randn(shape, generator=g)).round().long()
    vol[2][torch.rand(shape, generator=g) < 1e-3] = 65535
    ref = _stem_ref(net, vol, fmt)
    out, rep = _stem_run(eng, 0, vol, fmt)
    ssg, rep3 = _stem_run(eng, 3, vol, fmt)
    what = f"stem {fmt} background / near-constant / bright windows"
    _check_final(out.cpu(), ref["out"], fmt, shape, 8, what)
    _check_scale(ssg.cpu(), ref, rep3["raw_scale"], what)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_dc_offset_statistics(eng, net, fmt):
    """fp32 sum / sum-of-squares partials lose precision with the ratio |mean| / std of a channel (E[x^2] - E[x]^2).  Inputs with
    DC offsets of 10, 100 and 1000 times their spread; the ratio each channel's raw output reaches is measured on the float64
    reference.  Channels at ratios <= 100 must meet the scale bound; larger ratios are printed."""
    import torch

    row = Row("", "conv", 1, 32, 0, _T16, False, None)
    lines = []
    worst_le100 = 0.0
    for dc in (10.0, 100.0, 1000.0):
        g = torch.Generator().manual_seed(int(dc))
        x1 = _rnd(fmt)(dc + torch.randn((3, 32) + _T16, generator=g))
        ref = _reference(net, row, fmt, x1, None, None)
        ssg, rep = _run(eng, row, fmt, 3, x1, None, None)
        # the conv bias is not stored by the z-reg conv: the ratio of what the kernel sums
        mean = ref["mean"] - ref["drop"]
        ratio = mean.abs() / ref["var"].sqrt()
        sc = ssg.cpu()[..., 0].double() * rep["raw_scale"]
        rel = ((sc - ref["scale"]) / ref["scale"]).abs()
        for lo, hi in ((0, 10), (10, 100), (100, 300), (300, 1e9)):
            m = (ratio > lo) & (ratio <= hi)
            if m.any():
                lines.append(f"{fmt} dc {dc:g}: ratio ({lo}, {hi:g}] {int(m.sum())} channels, max scale rel err {float(rel[m].max()):.3e}")
        le = ratio <= 100
        if le.any():
            worst_le100 = max(worst_le100, float(rel[le].max()))
    print("\n".join(lines))
    print(f"RESULT dc offsets {fmt}: worst scale rel err at ratio <= 100: {worst_le100:.3e}")
    assert worst_le100 < SCALE_TOL, lines

    # the stem keeps its bias in the statistics: a window of sparse single photons on a dark background puts the bias far above
    # the spread of the raw output; and a bright window (20000 +- 200)
    for name, vol in (("sparse", (torch.rand((2, 24, 32, 64), generator=torch.Generator().manual_seed(1)) < 2e-3).long()),
                      ("bright", (20000 + 200 * torch.randn((2, 24, 32, 64), generator=torch.Generator().manual_seed(2))).round().long())):
        ref = _stem_ref(net, vol, fmt)
        ssg, rep = _stem_run(eng, 3, vol, fmt)
        ratio = ref["mean"].abs() / ref["var"].sqrt()
        rel = ((ssg.cpu()[..., 0].double() * rep["raw_scale"] - ref["scale"]) / ref["scale"]).abs()
        le = ratio <= 100
        print(f"stem {fmt} {name}: ratio max {float(ratio.max()):.1f}, scale rel err at ratio <= 100: "
              f"{float(rel[le].max()) if le.any() else 0:.3e}, above: {float(rel[~le].max()) if (~le).any() else 0:.3e}")
        if le.any():
            assert float(rel[le].max()) < SCALE_TOL, (name, float(rel[le].max()))


# ---------------------------------------------------------------------------------------------------
# large offsets: a window just under the z-reg conv's 2^26-voxel guard, and the guard itself
# ---------------------------------------------------------------------------------------------------
def test_large_window_offsets_and_guard(eng, net):
    import torch
    import torch.nn.functional as F

    from delivr_cfos_amd._lib import DelivrHipError

    fmt = "fp16"
    D, H, W = 63, 1024, 1040
    assert D * H * W < 2 ** 26
    n_big = 32 * 64 * 1024 * 1024
    flat = torch.zeros(n_big, dtype=torch.float32, device="cuda")
    x = flat[: 32 * D * H * W].view(1, 32, D, H, W)
    g = torch.Generator().manual_seed(4)
    # nonzero values in a few planes at the start and at the far end (the largest offsets), in small patches
    slabs = [(slice(0, 2), slice(0, 8), slice(0, 16)), (slice(D - 3, D), slice(H - 8, H), slice(W - 24, W)),
             (slice(30, 32), slice(500, 508), slice(512, 530))]
    for sz, sy, sx in slabs:
        blk = _rnd(fmt)(torch.randn((32, sz.stop - sz.start, sy.stop - sy.start, sx.stop - sx.start), generator=g))
        x[0, :, sz, sy, sx] = blk.cuda()
    raw, rep = eng.debug_layer16(2, "conv", 1, x, precision=fmt)
    assert rep["zreg"] == "f16_c32_t16_a0" and rep["drops_bias"], rep
    ssg, rep3 = eng.debug_layer16(3, "conv", 1, x, precision=fmt)
    cb = _block(net, 1)
    w = cb.conv.weight.detach().half().double()
    s = torch.zeros(32, dtype=torch.float64)
    q = torch.zeros(32, dtype=torch.float64)
    worst = 0.0
    for sz, sy, sx in slabs:  # the reference of a slab: its conv on a crop with 2 voxels of margin (zero padding inside)
        z0, z1 = max(sz.start - 2, 0), min(sz.stop + 2, D)
        y0, y1 = max(sy.start - 2, 0), min(sy.stop + 2, H)
        x0, x1 = max(sx.start - 2, 0), min(sx.stop + 2, W)
        crop = x[0, :, z0:z1, y0:y1, x0:x1].cpu().double()[None]
        ref = F.conv3d(crop, w, padding=1)[0] * rep["raw_scale"]
        got = raw[0, :, z0:z1, y0:y1, x0:x1].cpu().double()
        worst = max(worst, float(((got - ref).abs() / (ref.abs() + 1e-2)).max()))
        s += ref.sum(dim=(1, 2, 3))
        q += (ref ** 2).sum(dim=(1, 2, 3))
        raw[0, :, z0:z1, y0:y1, x0:x1] = 0
    assert worst < 2.0 ** -9, worst
    assert float(raw.abs().max()) == 0.0, "a voxel outside the slabs is not 0"
    # the statistics follow analytically: the zeros add nothing to the sums but count
    nvox = D * H * W
    mean = s / nvox
    var = q / nvox - mean ** 2
    N = cb.adn.N
    scale = N.weight.detach().double() / (var + 1e-5 * rep3["raw_scale"] ** 2).sqrt()
    rel = float(((ssg.cpu()[0, :, 0].double() - scale) / scale).abs().max())
    print(f"RESULT large window {D}x{H}x{W}: raw rel {worst:.3e}, scale rel {rel:.3e}")
    assert rel < SCALE_TOL, rel
    # at 2^26 voxels the z-reg conv refuses: an error, not a result
    xg = flat.view(1, 32, 64, 1024, 1024)
    with pytest.raises(DelivrHipError):
        eng.debug_layer16(2, "conv", 1, xg, precision=fmt)
