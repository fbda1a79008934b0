"""Every kernel of the 16-bit forward that tests/test_gpu_conv_kernels.py does not reach, each run on its own through the layer
hook (dlv_debug_layer16) and compared with the float64 references of oracle/layer_ref.py on the same 16-bit-rounded operands:
conv_deep.hip (all four (TX, NCB) instantiations, also with several items per persistent workgroup), the LDS-weights z-march,
the generic conv (all ten (TX, NCB, WLDS) instantiations), the five transposed-conv kernels (with activation on load and with
UpCat's replicate padding), the InstanceNorm + Mish (+ MaxPool) passes with the two format seams of the mixed mode, and the
final 1x1x1 conv.

Each row names the kernel and the template parameters it must run and asserts them from the hook's report (recorded at the
launch sites); where the row's shape is a level of a window the planner accepts it also asserts agreement with the plan.
Every row runs B = 3 windows with their own data (B = 9 where the row says so) in both formats and prints a RESULT line.
tests/test_layer_ref_cpu.py holds the row tables against the launcher lists of the C++ sources.

Left out: the non-temporal instantiations of the norm passes (they need tensors above 768 MiB).  The blend mode of the final conv
runs alone, per voxel against float64, in tests/test_gpu_blend_exact.py."""
from collections import namedtuple

import numpy as np
import pytest

from test_gpu_conv_kernels import SCALE_TOL, TOL, _LEVEL, _block, _check_final, _check_scale, _rnd, _ss, eng, net  # noqa: F401

pytestmark = pytest.mark.gpu

FMTS = ("fp16", "bf16")
_DEFAULTS = {"no_zmarch": 0, "generic_ncb": 0, "deep_mask": 2, "pool_rows_off": 0}


def _u(fmt):
    """half an ulp, relative: one rounding to the format"""
    return 2.0 ** -11 if fmt == "fp16" else 2.0 ** -8


def _reset(eng):
    for name, value in _DEFAULTS.items():
        eng.diag_set(name, value)


def _sx(shape):
    return "x".join(map(str, shape))


def _plan(window, switches, fmt, B):
    """the plan of a forward over `window`, or None where the planner refuses the window (too small for five levels)"""
    from delivr_cfos_amd._lib import DelivrHipError
    from delivr_cfos_amd.engine import layer_plan

    try:
        return layer_plan(window, switches, precision="fp16" if fmt == "fp16" else "bf16_all", batch=B)
    except DelivrHipError:
        return None


# ---------------------------------------------------------------------------------------------------
# conv blocks: conv_deep.hip, conv_zmarch.hip, conv3_mfma_kernel
# ---------------------------------------------------------------------------------------------------
# family: what the hook must report (a name of _lib.PLAN_CONV_KERNELS); tx / ncb / wlds: the template parameters (z-march: ncb =
# Cout / 32, no tx); items: work items of the deep kernel's launch; sw: switches; raw: the row also checks the stored raw
# tensor (kind 2) at shift 0 and 3; multi: more items than CUs and not a multiple of 8
ConvRow = namedtuple("ConvRow", "family li c1 c2 shape tx ncb wlds items B sw raw multi")


def _c(family, li, c1, c2, shape, tx=0, ncb=0, wlds=False, items=0, B=3, sw=None, raw=False, multi=False):
    return ConvRow(family, li, c1, c2, shape, tx, ncb, wlds, items, B, sw or {}, raw, multi)


_NZ = {"no_zmarch": 1}
_CONV_BASE = [
    # conv_deep.hip: items = (Cout / (16 NCB)) x B x tiles (TX 16: 4 x 8 x 16 voxels, TX 8: 8 x 8 x 8)
    _c("DEEP", 7, 128, 0, (6, 12, 24), 16, 4, items=48, raw=True),            # partial tiles on all three axes
    _c("DEEP", 6, 64, 0, (18, 20, 40), 16, 4, items=270, multi=True),         # 45 tiles x 2 x 3: several items per workgroup
    _c("DEEP", 14, 32, 32, (6, 12, 24), 16, 2, items=24),                     # Cout 32; the concatenation crosses a slab boundary
    _c("DEEP", 12, 64, 64, (4, 8, 16), 16, 2, items=6),                       # grid 6: the plain stride walk
    _c("DEEP", 9, 256, 0, (8, 8, 8), 8, 2, items=24),                         # level 4 of a 128^3 window
    _c("DEEP", 9, 256, 0, (4, 4, 2), 8, 2, items=24),                         # level 4 of a 64 x 64 x 32 window
    _c("DEEP", 9, 256, 0, (10, 12, 12), 8, 4, items=96),
    _c("DEEP", 10, 128, 128, (6, 6, 12), 8, 2, items=24),
    _c("DEEP", 8, 128, 0, (24, 24, 8), 8, 4, items=324, B=9, multi=True),     # 9 tiles x 4 x 9
    # conv_zmarch.hip (at most 32768 voxels, W >= 32, Cin and Cout <= 64)
    _c("ZMARCH", 1, 32, 0, (20, 20, 72), ncb=1, raw=True),
    _c("ZMARCH", 4, 32, 0, (20, 20, 72), ncb=2),
    _c("ZMARCH", 5, 64, 0, (20, 20, 72), ncb=2),
    _c("ZMARCH", 14, 32, 32, (20, 20, 72), ncb=1),
    _c("ZMARCH", 1, 32, 0, (6, 12, 40), ncb=1),                               # one ragged tile
    # the generic conv under the default switches: W < 32 with more than 32768 voxels (level 1 of a 256 x 256 x 32 window)
    _c("GENERIC", 2, 32, 0, (72, 40, 16), 16, 1, raw=True),
    # ... and its other instantiations ("no_zmarch": every layer; "generic_ncb" where the kernel's own choice is another)
    _c("GENERIC", 1, 32, 0, (6, 10, 24), 16, 1, sw=dict(_NZ, generic_ncb=1)),
    _c("GENERIC", 5, 64, 0, (6, 10, 24), 16, 2, sw=dict(_NZ, generic_ncb=2)),
    _c("GENERIC", 7, 128, 0, (6, 10, 24), 16, 4, sw=dict(_NZ, generic_ncb=4)),
    _c("GENERIC", 9, 256, 0, (12, 12, 12), 8, 1, sw=dict(_NZ, generic_ncb=1)),
    _c("GENERIC", 9, 256, 0, (12, 12, 12), 8, 2, sw=dict(_NZ, generic_ncb=2)),
    _c("GENERIC", 9, 256, 0, (12, 12, 12), 8, 4, sw=dict(_NZ, generic_ncb=4)),
    _c("GENERIC", 9, 256, 0, (8, 8, 8), 8, 1, wlds=True, sw=dict(_NZ, generic_ncb=1)),
    _c("GENERIC", 9, 256, 0, (8, 8, 8), 8, 2, wlds=True, sw=dict(_NZ, generic_ncb=2)),
    _c("GENERIC", 7, 128, 0, (4, 6, 24), 16, 2, wlds=True, sw=dict(_NZ, generic_ncb=2)),
    _c("GENERIC", 1, 32, 0, (4, 6, 24), 16, 1, wlds=True, sw=dict(_NZ, generic_ncb=1)),
]
CONV_ROWS = [(fmt, r) for fmt in FMTS for r in _CONV_BASE]


def _conv_id(p):
    fmt, r = p
    return f"{fmt}-{r.family}-b{r.li}-{_sx(r.shape)}-tx{r.tx}-ncb{r.ncb}{'-wlds' if r.wlds else ''}{'-B%d' % r.B if r.B != 3 else ''}"


def _conv_inputs(row, fmt, B, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    r = _rnd(fmt)
    x1 = r(torch.randn((B, row.c1) + row.shape, generator=g))
    x2 = r(torch.randn((B, row.c2) + row.shape, generator=g)) if row.c2 else None
    return x1, x2


def _conv_ref(net, row, fmt, x1, x2, shift=0):
    """shift: the block stores its raw output 2^-shift times smaller - the kernel multiplies with round16(w * 2^-shift) (in fp16
    the smallest weights become subnormal: not the rounded weights scaled), so the reference does the same and its "raw" is then
    in the stored scale"""
    from oracle import layer_ref as lr

    blk = _block(net, row.li)
    N = blk.adn.N
    ws = 2.0 ** -shift
    return lr.conv_block(x1, blk.conv.weight.detach() * ws, blk.conv.bias.detach() * ws, N.weight.detach(), N.bias.detach(), fmt, x2=x2)


def _conv_run(eng, row, fmt, kind, x1, x2):
    return eng.debug_layer16(kind, "conv", row.li, x1.cuda(), None, None if x2 is None else x2.cuda(), precision=fmt)


def _assert_conv_report(rep, row, B):
    assert rep["conv"] == row.family and rep["zreg"] is None, (rep, row)
    if row.family == "ZMARCH":
        assert rep["ncb"] == row.ncb, (rep, row)
        return
    assert (rep["tx"], rep["ncb"]) == (row.tx, row.ncb), (rep, row)
    if row.family == "GENERIC":
        assert rep["wlds"] == row.wlds, (rep, row)
    else:
        assert rep["items"] == row.items, (rep, row)


def _check_raw(raw, ref, rep, fmt, what):
    """kind 2: the stored tensor is the conv [+ bias] in the stored scale (ref: _conv_ref with the block's shift) rounded once to
    the format - relative to |ref| + 1e-2 x the channel's spread, as the stem's raw check"""
    from oracle import layer_ref as lr

    sr = lr.stored_raw(ref, 1.0, rep["drops_bias"])
    spread = sr.std(dim=(2, 3, 4))[:, :, None, None, None]
    rel = float(((raw.double() - sr).abs() / (sr.abs() + 1e-2 * spread)).max())
    print(f"{what}: raw rel {rel:.3e} (drops_bias {rep['drops_bias']}, raw_scale {rep['raw_scale']})")
    assert rel < (2.0 ** -10 if fmt == "fp16" else 2.0 ** -7), (what, rel)
    return rel


@pytest.mark.parametrize("case", CONV_ROWS, ids=_conv_id)
def test_conv_row_vs_fp64(eng, net, case):
    import torch

    fmt, row = case
    B = row.B
    x1, x2 = _conv_inputs(row, fmt, B, seed=row.li * 1000 + sum(row.shape))
    ref = _conv_ref(net, row, fmt, x1, x2)
    raw_rel = {}
    try:
        for name, value in row.sw.items():
            eng.diag_set(name, value)
        out, rep = _conv_run(eng, row, fmt, 0, x1, x2)
        ssg, rep3 = _conv_run(eng, row, fmt, 3, x1, x2)
        if row.raw:
            for shift in (0, 3):
                eng.set_conv_shift(row.li, shift)
                try:
                    raw, rep2 = _conv_run(eng, row, fmt, 2, x1, x2)
                finally:
                    eng.set_conv_shift(row.li, 0)
                assert rep2["raw_scale"] == 2.0 ** -shift and rep2["conv"] == row.family, rep2
                # conv_deep.hip stores no bias (its header); the z-march and the generic kernel add it
                assert rep2["drops_bias"] == (row.family == "DEEP"), rep2
                ref_s = ref if shift == 0 else _conv_ref(net, row, fmt, x1, x2, shift)
                raw_rel[shift] = _check_raw(raw.cpu(), ref_s, rep2, fmt, f"{_conv_id(case)} shift {shift}")
    finally:
        _reset(eng)
    _assert_conv_report(rep, row, B)
    _assert_conv_report(rep3, row, B)
    if row.multi:
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        assert rep["items"] > ncu and rep["items"] % 8 != 0 and rep["grid"] == ncu, (rep, ncu)
    elif row.family == "DEEP":
        assert rep["grid"] == rep["items"], rep  # (one item per workgroup)
    # ... and it is what the plan says of this level of a window
    plan = _plan(tuple(n << _LEVEL[row.li] for n in row.shape), row.sw, fmt, B)
    if plan is not None:
        c = plan["conv"][row.li]
        assert c["kernel"] == row.family, (c, row)
        if row.family == "GENERIC":
            assert (c["tx"], c["ncb"], bool(c["wlds"])) == (row.tx, row.ncb, row.wlds), (c, row)
    what = _conv_id(case)
    mx = _check_final(out.cpu(), ref["out"], fmt, row.shape, 8, what)
    se = _check_scale(ssg.cpu(), ref, rep3["raw_scale"], what)
    print(f"RESULT conv {what}: grid {rep['grid']} items {rep['items']} plan {'checked' if plan else 'n/a'}: max {mx:.3e} scale {se:.3e} raw {raw_rel}")


# ---------------------------------------------------------------------------------------------------
# transposed convs (kind 1: raw output with its bias)
# ---------------------------------------------------------------------------------------------------
# kernel: a name of _lib.PLAN_DECONV_KERNELS; gpw: 64-channel groups per workgroup (DEEP); skip: the skip tensor's shape
# (replicate padding); act: also run with a raw input + scale/shift (activation on load; Cin >= 128: a norm pass first)
DeconvRow = namedtuple("DeconvRow", "kernel j shape sw gpw skip act")
_DECONV_BASE = [
    DeconvRow("DEEP", 0, (8, 8, 8), {}, 1, None, False),
    DeconvRow("DEEP", 0, (3, 4, 5), {}, 1, None, False),        # 60 voxels: not a multiple of 16
    DeconvRow("DEEP", 0, (12, 16, 20), {}, 1, None, False),     # 15 workgroups of 256 voxels
    DeconvRow("DEEP", 0, (13, 16, 20), {}, 2, None, False),     # 17 workgroups: both 64-channel groups in one workgroup
    DeconvRow("DEEP", 1, (6, 6, 4), {}, 1, None, False),
    DeconvRow("DEEP", 1, (16, 16, 16), {}, 1, None, False),
    # 17 x 31 x 4 = 2108 row segments >= 2048; the last segment of a row has 8 voxels, the last wave 4 of its 8 segments
    DeconvRow("REGW", 2, (17, 31, 56), {}, 0, None, True),
    DeconvRow("REGW", 3, (17, 31, 56), {}, 0, None, True),
    DeconvRow("ROWS", 2, (5, 6, 20), {}, 0, None, True),
    DeconvRow("ROWS", 3, (5, 6, 20), {}, 0, None, True),
    DeconvRow("WST", 0, (4, 6, 12), {"deep_mask": 0}, 0, None, True),
    DeconvRow("WST", 1, (5, 6, 20), {"deep_mask": 0}, 0, None, True),
    DeconvRow("PARITY", 0, (3, 5, 7), _NZ, 0, None, False),     # 105 voxels: not a multiple of 32
    DeconvRow("PARITY", 1, (3, 5, 7), _NZ, 0, None, False),
    DeconvRow("PARITY", 2, (3, 5, 7), _NZ, 0, None, False),
    DeconvRow("PARITY", 3, (3, 5, 7), _NZ, 0, None, False),
    DeconvRow("ROWS", 2, (5, 6, 20), {}, 0, (11, 12, 41), True),  # padded along D and W
]
DECONV_ROWS = [(fmt, r, act) for fmt in FMTS for r in _DECONV_BASE for act in ((False, True) if r.act else (False,))]


def _deconv_id(p):
    fmt, r, act = p
    return f"{fmt}-{r.kernel}-j{r.j}-{_sx(r.shape)}{'-pad' if r.skip else ''}{'-act' if act else ''}"


def _deconv_case(eng, net, fmt, row, act, B, seed, pick=None):
    """runs transposed conv row.j through the hook -> (output, report, reference, |x| |w| sum), the last two on the CPU"""
    import torch

    from oracle import layer_ref as lr

    up = getattr(net, f"upcat_{4 - row.j}").upsample.deconv
    g = torch.Generator().manual_seed(seed)
    x = _rnd(fmt)(torch.randn((B, up.in_channels) + row.shape, generator=g))
    ss = _ss(g, B, up.in_channels) if act else None
    if pick is not None:
        x, ss = x[pick].contiguous(), None if ss is None else ss[pick].contiguous()
        out, rep = eng.debug_layer16(1, "conv", row.j, x.cuda(), None if ss is None else ss.cuda(), precision=fmt, skip_shape=row.skip)
        return out, rep, None, None
    ref = lr.deconv(x, up.weight.detach(), up.bias.detach(), fmt, ss=ss)
    r, ab = ref["raw"], ref["abs"]
    if row.skip:
        r, ab = lr.replicate_pad(r, row.skip), lr.replicate_pad(ab, row.skip)
    out, rep = eng.debug_layer16(1, "conv", row.j, x.cuda(), None if ss is None else ss.cuda(), precision=fmt, skip_shape=row.skip)
    return out, rep, r, ab


def _check_deconv(got, r, ab, cin, fmt, act, what):
    """the output is an fp32 sum rounded once: per element 2u |ref| + Cin 2^-23 sum|x||w| + 2^-24 (+ 2u sum|x_act||w| where the
    operand went through a Mish: every staged operand one ulp off); and, so that the loose term hides nothing, per (sample,
    channel) the mean error at most twice the mean rounding error of the reference itself"""
    from oracle import layer_ref as lr

    u = _u(fmt)
    err = (got.double() - r).abs()
    bound = 2 * u * r.abs() + cin * 2.0 ** -23 * ab + 2.0 ** -24 + (2 * u * ab if act else 0.0)
    ratio = err / bound
    worst = float(ratio.max())
    at = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))
    own = (lr.round16(r, fmt) - r).abs().mean(dim=(2, 3, 4))
    mratio = float((err.mean(dim=(2, 3, 4)) / own).max())
    print(f"RESULT deconv {what}: worst |err| / bound {worst:.3f} at {at}, max |err| {float(err.max()):.3e}, "
          f"worst mean |err| / mean rounding error {mratio:.3f}")
    assert worst <= 1.0, (what, worst, at)
    assert mratio <= 2.0, (what, mratio)


@pytest.mark.parametrize("case", DECONV_ROWS, ids=_deconv_id)
def test_deconv_row_vs_fp64(eng, net, case):
    fmt, row, act = case
    B = 3
    cin = getattr(net, f"upcat_{4 - row.j}").upsample.deconv.in_channels
    try:
        for name, value in row.sw.items():
            eng.diag_set(name, value)
        out, rep, r, ab = _deconv_case(eng, net, fmt, row, act, B, seed=row.j * 100 + sum(row.shape) + act)
    finally:
        _reset(eng)
    assert tuple(out.shape) == tuple(r.shape), (out.shape, r.shape)
    assert rep["deconv"] == row.kernel and rep["conv"] is None, (rep, row)
    if row.kernel == "DEEP":
        assert rep["gpw"] == row.gpw, (rep, row)
    assert rep["pad"] == (row.skip is not None), rep
    # activation on load exists for Cin < 128 in the rows / regw kernels; the deep levels get one normalisation pass first
    assert rep["norm_passes"] == (1 if act and cin >= 128 else 0), (rep, cin)
    plan = None if row.skip else _plan(tuple(n << (4 - row.j) for n in row.shape), row.sw, fmt, B)
    if plan is not None and plan["deconv"][row.j]["kernel"] is not None:  # (None: upcat_1 folded, no transposed conv launched)
        assert plan["deconv"][row.j]["kernel"] == row.kernel, (plan["deconv"][row.j], row)
        assert bool(plan["deconv"][row.j]["norm_first"]) == (cin >= 128 or row.kernel == "PARITY"), plan["deconv"][row.j]  # (a forward's input is raw)
    _check_deconv(out.cpu(), r, ab, cin, fmt, act, _deconv_id(case))
    if row.skip:  # the padding is a copy: bit-equal to the edge value, the rest bit-equal to the unpadded run
        import torch

        plain, rep_p, _, _ = _deconv_case(eng, net, fmt, row._replace(skip=None), act, B, seed=row.j * 100 + sum(row.shape) + act)
        assert not rep_p["pad"], rep_p
        D2, H2, W2 = plain.shape[2:]
        assert torch.equal(out[:, :, :D2, :H2, :W2], plain)
        for dim, n in ((2, D2), (3, H2), (4, W2)):
            if out.shape[dim] > n:
                assert torch.equal(out.select(dim, n), out.select(dim, n - 1)), dim


# ---------------------------------------------------------------------------------------------------
# InstanceNorm + Mish (+ MaxPool) passes
# ---------------------------------------------------------------------------------------------------
def _norm_inputs(fmt, B, C, shape, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    x = _rnd(fmt)(torch.randn((B, C) + shape, generator=g) * 1.5)
    return x, _ss(g, B, C)


def _check_act(got, act, y, fmt_out, what):
    """mish_fast's absolute error is |y| 2^-23 (its comment); with the fp32 affine and one rounding to the output format:
    |got - ref| <= u |ref| + 2^-20 (1 + |y|) + 2^-24 per element"""
    err = (got.double() - act).abs()
    bound = _u(fmt_out) * act.abs() + 2.0 ** -20 * (1 + y.abs()) + 2.0 ** -24
    ratio = err / bound
    worst = float(ratio.max())
    at = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))
    print(f"{what}: worst |err| / bound {worst:.3f} at {at}, max |err| {float(err.max()):.3e}")
    assert worst <= 1.0, (what, worst, at)
    return worst


def _pooled_y(y):
    """the pre-activation of the voxel that wins each pooled cell (Mish is not monotone below its minimum: take the winner's)"""
    import torch
    import torch.nn.functional as F

    from oracle import layer_ref as lr

    _, idx = F.max_pool3d(lr.mish(y), 2, return_indices=True)
    return torch.gather(y.flatten(2), 2, idx.flatten(2)).view_as(idx)


# form: "plain" | "pool_wb" | "pool_only" | "seam_pool" (fp16 raw -> bf16 pooled) | "seam_act" (bf16 raw -> fp16 activated)
NORM_ROWS = [(fmt, form, C, shape) for fmt in FMTS for C in (32, 64)
             for form, shape in (("plain", (5, 7, 9)), ("pool_wb", (6, 8, 24)), ("pool_only", (7, 9, 11)))]
NORM_ROWS += [("fp16", "seam_pool", C, (6, 8, 24)) for C in (32, 64)] + [("bf16", "seam_act", C, (6, 8, 24)) for C in (32, 64)]


@pytest.mark.parametrize("fmt,form,C,shape", NORM_ROWS, ids=lambda v: _sx(v) if isinstance(v, tuple) else str(v))
def test_norm_pass_vs_fp64(eng, fmt, form, C, shape):
    import torch

    from oracle import layer_ref as lr

    B = 3
    x, ss = _norm_inputs(fmt, B, C, shape, seed=C + sum(shape))
    pool = form in ("pool_wb", "pool_only", "seam_pool")
    wb = form != "pool_only"
    seam = form.startswith("seam")
    other = "bf16" if fmt == "fp16" else "fp16"
    ref = lr.norm_pool(x, ss, fmt, other if seam else fmt, pool)
    res = eng.debug_layer16(0, "norm", 0, x.cuda(), ss.cuda(), precision=fmt, pool=pool, writeback=wb, seam=seam)
    out, rep = res[0].cpu(), res[-1]
    assert rep["norm"] == {"rows": False, "pooled": pool, "writeback": wb, "nt": False, "seam": seam} and rep["norm_passes"] == 1, rep
    what = f"norm {fmt} {form} C{C} {_sx(shape)}"
    worst = {}
    if wb:
        # what the pooling pass writes back: everything it pools (odd sizes: the last plane / row / column stays raw)
        fmt_wb = other if form == "seam_act" else fmt
        D2, H2, W2 = (2 * (n // 2) if pool else n for n in shape)
        worst["act"] = _check_act(out[:, :, :D2, :H2, :W2], ref["act"][:, :, :D2, :H2, :W2], ref["y"][:, :, :D2, :H2, :W2], fmt_wb, what)
        if pool:
            edge = torch.ones(shape, dtype=torch.bool)
            edge[:D2, :H2, :W2] = False
            assert torch.equal(out[:, :, edge], x[:, :, edge]), f"{what}: voxels outside the pooled region changed"
    else:
        assert torch.equal(out, x), f"{what}: the raw tensor did not come back bit-identical"
    if pool:
        worst["pooled"] = _check_act(res[1].cpu(), ref["pooled_act"], _pooled_y(ref["y"]), other if seam else fmt, what + " pooled")
    print(f"RESULT {what}: worst |err| / bound {worst}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("shape", [(4, 6, 64), (4, 4, 128)], ids=_sx)
@pytest.mark.parametrize("wb", [True, False], ids=["wb", "poolonly"])
def test_full_line_pool_kernel(eng, fmt, C, shape, wb):
    """norm_mish_pool_rows_kernel (W a multiple of 64): against fp64, and bit-identical to the per-voxel kernel"""
    import torch

    from oracle import layer_ref as lr

    x, ss = _norm_inputs(fmt, 3, C, shape, seed=C + sum(shape) + wb)
    ref = lr.norm_pool(x, ss, fmt, fmt, True)
    out, pooled, rep = eng.debug_layer16(0, "norm", 0, x.cuda(), ss.cuda(), precision=fmt, pool=True, writeback=wb)
    assert rep["norm"] == {"rows": True, "pooled": True, "writeback": wb, "nt": False, "seam": False}, rep
    eng.diag_set("pool_rows_off", 1)
    try:
        out_v, pooled_v, rep_v = eng.debug_layer16(0, "norm", 0, x.cuda(), ss.cuda(), precision=fmt, pool=True, writeback=wb)
    finally:
        _reset(eng)
    assert rep_v["norm"]["rows"] is False, rep_v
    assert torch.equal(out, out_v) and torch.equal(pooled, pooled_v)
    what = f"norm rows {fmt} C{C} {_sx(shape)} {'wb' if wb else 'pool only'}"
    if wb:
        w0 = _check_act(out.cpu(), ref["act"], ref["y"], fmt, what)
    else:
        assert torch.equal(out.cpu(), x), what
        w0 = 0.0
    w1 = _check_act(pooled.cpu(), ref["pooled_act"], _pooled_y(ref["y"]), fmt, what + " pooled")
    print(f"RESULT {what}: worst |err| / bound act {w0:.3f} pooled {w1:.3f}")


# ---------------------------------------------------------------------------------------------------
# final 1x1x1 conv: 149760 voxels > the 131072-voxel grid stride, and neither W nor W x H divides it: every carry runs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_final_conv_vs_fp64(eng, net, fmt):
    from oracle import layer_ref as lr

    shape = (20, 72, 104)
    assert np.prod(shape) > 131072 and 131072 % shape[2] and 131072 % (shape[1] * shape[2])
    x, ss = _norm_inputs(fmt, 3, 32, shape, seed=11)
    fc = net.final_conv
    ref = lr.final_logits(x, ss, fc.weight.detach(), fc.bias.detach(), fmt)
    out, rep = eng.debug_layer16(0, "final", 0, x.cuda(), ss.cuda(), precision=fmt)
    assert tuple(out.shape) == (3,) + shape
    w = fc.weight.detach().double().reshape(1, 32, 1, 1, 1)
    # per channel the activation's error (as the norm pass, without the 16-bit store), then a 32-term fp32 sum
    bound = (w.abs() * 2.0 ** -20 * (1 + ref["y"].abs())).sum(dim=1) + 32 * 2.0 ** -24 * (w * ref["m"]).abs().sum(dim=1)
    err = (out.cpu().double() - ref["logits"]).abs()
    ratio = err / bound
    worst = float(ratio.max())
    at = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))
    print(f"RESULT final conv {fmt} {_sx(shape)}: worst |err| / bound {worst:.3f} at {at}, max |err| {float(err.max()):.3e}")
    assert worst <= 1.0, (worst, at)


# ---------------------------------------------------------------------------------------------------
# invariance: the result of a window does not depend on the windows that share its launch
# ---------------------------------------------------------------------------------------------------
_INV_CONV = {
    "deep": (_c("DEEP", 7, 128, 0, (6, 12, 24), 16, 4), {1: 4, 3: 4, 16: 4}),
    "zmarch": (_c("ZMARCH", 1, 32, 0, (20, 20, 72), ncb=1), {1: 1, 3: 1, 16: 1}),
    # the generic conv's cout blocks per workgroup follow B: 32 tiles x 16 windows reach the 512 workgroups NCB 2 asks for
    "generic": (_c("GENERIC", 5, 64, 0, (8, 16, 64), 16, 0, sw=_NZ), {1: 1, 3: 1, 16: 2}),
}


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(_INV_CONV))
def test_conv_window_independent_of_batch(eng, net, name, fmt):
    import torch

    row, ncbs = _INV_CONV[name]
    x1, x2 = _conv_inputs(row, fmt, 16, seed=77)

    def run(pick):
        a1 = x1[pick].contiguous()
        o, rep = _conv_run(eng, row, fmt, 0, a1, None)
        q, _ = _conv_run(eng, row, fmt, 3, a1, None)
        assert rep["conv"] == row.family and rep["ncb"] == ncbs[len(pick)], (rep, len(pick))
        at = pick.index(5)
        return o[at].cpu(), q[at].cpu()

    try:
        for k, v in row.sw.items():
            eng.diag_set(k, v)
        res = {1: run([5]), 3: run([0, 5, 2]), 16: run(list(range(16)))}
    finally:
        _reset(eng)
    for k in (3, 16):
        assert torch.equal(res[k][0], res[1][0]), (name, k, float((res[k][0] - res[1][0]).abs().max()))
        assert torch.equal(res[k][1], res[1][1]), (name, k)


@pytest.mark.parametrize("fmt", FMTS)
def test_regw_deconv_window_independent_of_batch(eng, net, fmt):
    import torch

    row = DeconvRow("REGW", 3, (17, 31, 56), {}, 0, None, True)
    res = {}
    for pick in ([5], [0, 5, 2], list(range(16))):
        out, rep, _, _ = _deconv_case(eng, net, fmt, row, True, 16, seed=78, pick=pick)
        assert rep["deconv"] == "REGW", rep
        res[len(pick)] = out[pick.index(5)].cpu()
    for k in (3, 16):
        assert torch.equal(res[k], res[1]), (k, float((res[k] - res[1]).abs().max()))
