"""The float64 single-layer references of oracle/layer_ref.py (used by tests/test_gpu_conv_kernels.py and
tests/test_gpu_layer_kernels.py) against the oracle U-Net's own layers (orc.build_unet) run in float64, and the coverage tables
of the two GPU files against conv_zreg.h and the launcher lists of conv_deep.hip / unet_bf16.hip."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def net64():
    from oracle import delivr_oracle as orc

    n = orc.build_unet(seed=0)
    orc.randomize_affine(n, seed=1)
    return n.double()


def _close(a, b, tol=1e-10):
    err = float((a - b).abs().max())
    assert err < tol * max(1.0, float(b.abs().max())), err


def test_conv_block_ref_matches_module(net64):
    import torch

    from oracle import layer_ref as lr

    g = torch.Generator().manual_seed(0)
    for blk, c1, c2 in ((net64.conv_0.conv_1, 32, 0), (net64.upcat_2.convs.conv_0, 32, 32)):
        x1 = torch.randn((2, c1, 5, 6, 7), generator=g, dtype=torch.float64)
        x2 = torch.randn((2, c2, 5, 6, 7), generator=g, dtype=torch.float64) if c2 else None
        ref = lr.conv_block(x1, blk.conv.weight, blk.conv.bias, blk.adn.N.weight, blk.adn.N.bias, None, x2=x2)
        with torch.no_grad():
            xin = x1 if x2 is None else torch.cat([x1, x2], dim=1)
            _close(ref["out"], blk(xin))
            _close(ref["raw"], blk.conv(xin))
            _close(ref["raw"] * ref["scale"][:, :, None, None, None] + ref["shift"][:, :, None, None, None], blk.adn.N(blk.conv(xin)))
        # activate-on-load: the consumer sees mish(raw * sc + sh)
        ss = torch.stack([torch.rand((2, c1), generator=g) * 1.5 + 0.5, torch.rand((2, c1), generator=g) * 2 - 1], dim=-1)
        ref_a = lr.conv_block(x1, blk.conv.weight, blk.conv.bias, blk.adn.N.weight, blk.adn.N.bias, None, ss1=ss, x2=x2)
        act = torch.nn.functional.mish(x1 * ss[..., 0, None, None, None].double() + ss[..., 1, None, None, None].double())
        with torch.no_grad():
            _close(ref_a["out"], blk(act if x2 is None else torch.cat([act, x2], dim=1)))


def test_folded_upcat_ref_matches_module(net64):
    import torch

    from oracle import layer_ref as lr

    up = net64.upcat_1
    c0 = up.convs.conv_0
    g = torch.Generator().manual_seed(1)
    skip = torch.randn((2, 32, 6, 8, 10), generator=g, dtype=torch.float64)
    coarse = torch.randn((2, 32, 3, 4, 5), generator=g, dtype=torch.float64)
    ref = lr.folded_upcat(skip, coarse, c0.conv.weight, c0.conv.bias, up.upsample.deconv.weight, up.upsample.deconv.bias,
                          c0.adn.N.weight, c0.adn.N.bias, None)
    with torch.no_grad():
        u = up.upsample(coarse)
        xin = torch.cat([skip, u], dim=1)
        _close(ref["raw"], c0.conv(xin))
        _close(ref["out"], c0(xin))
        # the interior constant: what the conv of u gains from the transposed conv's bias at a voxel whose 27 taps lie inside
        cb = torch.nn.functional.conv3d(torch.ones((1, 32, 3, 3, 3), dtype=torch.float64) * up.upsample.deconv.bias[None, :, None, None, None],
                                        c0.conv.weight[:, 32:])[0, :, 0, 0, 0]
        _close(ref["drop"][0], cb + c0.conv.bias)


@pytest.mark.parametrize("flip_dim", [None, 2, 3, 4])
def test_stem_ref_matches_module(net64, flip_dim):
    import torch

    from oracle import layer_ref as lr

    blk = net64.conv_0.conv_0
    g = torch.Generator().manual_seed(2)
    vol = torch.randint(0, 65536, (2, 5, 6, 7), generator=g)
    ref = lr.stem(vol, blk.conv.weight, blk.conv.bias, blk.adn.N.weight, blk.adn.N.bias, None, w_scale=2.0 ** -8, flip_dim=flip_dim)
    x = vol.double()[:, None]
    if flip_dim is not None:
        x = x.flip(flip_dim)
    with torch.no_grad():
        _close(ref["raw"], blk.conv(x))
        _close(ref["out"], blk(x), 1e-9)


def test_activate_rounds_like_the_kernels():
    """round16 before the affine (the stored raw tensor) and after the Mish (the staged operand)."""
    import torch

    from oracle import layer_ref as lr

    raw = torch.tensor([[[[[1.0 + 2 ** -10]]]]], dtype=torch.float64)
    ss = torch.tensor([[[1.0, 0.0]]])
    a = lr.activate(raw, ss, "bf16")
    assert float(a) == float(torch.nn.functional.mish(torch.tensor(1.0, dtype=torch.float64)).bfloat16())


def test_every_zreg_instantiation_has_a_gpu_test_row():
    """conv_zreg.h's ZR_DECLARE list against the coverage table of tests/test_gpu_conv_kernels.py: a new instantiation
    cannot land without a row that proves it ran and was compared with the float64 reference."""
    import importlib.util

    decl = open(os.path.join(ROOT, "delivr_cfos_amd", "csrc", "conv_zreg.h")).read()
    declared = set(re.findall(r"^ZR_DECLARE\(dlv_zr_([a-z0-9_]+)\);", decl, re.M))
    assert len(declared) == 20, sorted(declared)
    spec = importlib.util.spec_from_file_location("_gck", os.path.join(ROOT, "tests", "test_gpu_conv_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    covered = {r.inst for r in mod.ZREG_ROWS}
    assert declared <= covered, f"no GPU test row for {sorted(declared - covered)}"
    assert covered <= declared, f"rows name instantiations that do not exist: {sorted(covered - declared)}"
    assert {r.upconv for r in mod.ZREG_ROWS if r.upconv} == {"upconv2", "upconv2m"}


# ---------------------------------------------------------------------------------------------------
# the references of tests/test_gpu_layer_kernels.py against the oracle U-Net's own modules
# ---------------------------------------------------------------------------------------------------
def test_deconv_ref_matches_module(net64):
    import torch

    from oracle import layer_ref as lr

    g = torch.Generator().manual_seed(3)
    for up in (net64.upcat_4.upsample.deconv, net64.upcat_1.upsample.deconv):
        x = torch.randn((2, up.in_channels, 3, 4, 5), generator=g, dtype=torch.float64)
        ref = lr.deconv(x, up.weight, up.bias, None)
        with torch.no_grad():
            _close(ref["raw"], up(x))
        assert tuple(ref["raw"].shape) == (2, up.out_channels, 6, 8, 10)
        # the sum of absolute products bounds the bias-free output
        assert bool((ref["abs"] + 1e-12 >= (ref["raw"] - up.bias[None, :, None, None, None]).abs()).all())
        # a raw input: the module sees mish(x * sc + sh)
        ss = torch.stack([torch.rand((2, up.in_channels), generator=g) * 1.5 + 0.5, torch.rand((2, up.in_channels), generator=g) * 2 - 1], dim=-1)
        act = torch.nn.functional.mish(x * ss[..., 0, None, None, None].double() + ss[..., 1, None, None, None].double())
        with torch.no_grad():
            _close(lr.deconv(x, up.weight, up.bias, None, ss=ss)["raw"], up(act))


def test_norm_pool_ref_matches_module(net64):
    import torch

    from oracle import layer_ref as lr

    g = torch.Generator().manual_seed(4)
    raw = torch.randn((2, 32, 7, 9, 11), generator=g, dtype=torch.float64)  # odd sizes: the last plane / row / column is dropped
    ss = torch.stack([torch.rand((2, 32), generator=g) * 1.5 + 0.5, torch.rand((2, 32), generator=g) * 2 - 1], dim=-1)
    ref = lr.norm_pool(raw, ss, None, None, True)
    act = torch.nn.functional.mish(raw * ss[..., 0, None, None, None].double() + ss[..., 1, None, None, None].double())
    _close(ref["out"], act)
    _close(ref["pooled"], net64.down_1.max_pooling(act))
    assert tuple(ref["pooled"].shape) == (2, 32, 3, 4, 5)
    assert "pooled" not in lr.norm_pool(raw, ss, None, None, False)
    # rounding to the output format commutes with the maximum
    r16 = lr.norm_pool(raw, ss, "fp16", "bf16", True)
    assert torch.equal(r16["pooled"], torch.nn.functional.max_pool3d(r16["out"], 2))
    assert torch.equal(r16["out"], r16["out"].bfloat16().double())


def test_replicate_pad_ref_matches_upcat(net64):
    import torch

    from oracle import layer_ref as lr

    up = net64.upcat_2
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 64, 3, 4, 5), generator=g, dtype=torch.float64)
    for skip_shape in ((7, 8, 11), (6, 9, 10), (7, 9, 11), (6, 8, 10)):
        x_e = torch.randn((2, 32) + skip_shape, generator=g, dtype=torch.float64)
        with torch.no_grad():
            u = lr.replicate_pad(up.upsample(x), skip_shape)
            assert tuple(u.shape[2:]) == skip_shape
            _close(up.convs(torch.cat([x_e, u], dim=1)), up(x, x_e))
        # the edge value at the far end
        if skip_shape[0] == 7:
            assert torch.equal(u[:, :, 6], u[:, :, 5])
        if skip_shape[2] == 11:
            assert torch.equal(u[..., 10], u[..., 9])
    with pytest.raises(ValueError):
        lr.replicate_pad(x, (8, 8, 10))


def test_final_logits_ref_matches_module(net64):
    import torch

    from oracle import layer_ref as lr

    g = torch.Generator().manual_seed(6)
    raw = torch.randn((2, 32, 4, 5, 6), generator=g, dtype=torch.float64)
    ss = torch.stack([torch.rand((2, 32), generator=g) * 1.5 + 0.5, torch.rand((2, 32), generator=g) * 2 - 1], dim=-1)
    fc = net64.final_conv
    ref = lr.final_logits(raw, ss, fc.weight, fc.bias, None)
    act = torch.nn.functional.mish(raw * ss[..., 0, None, None, None].double() + ss[..., 1, None, None, None].double())
    with torch.no_grad():
        _close(ref["logits"], fc(act)[:, 0])
    _close(ref["m"], act)


def test_every_layer_kernel_has_a_gpu_test_row():
    """the row tables of tests/test_gpu_layer_kernels.py against the launcher lists of the C++ sources: every conv family and
    transposed-conv kernel of the plan in both formats, every (TX, NCB) of conv_deep.hip's CD_GO list and every (TX, NCB, WLDS)
    launch_generic_ncb can reach"""
    import importlib.util
    import itertools

    spec = importlib.util.spec_from_file_location("_glk", os.path.join(ROOT, "tests", "test_gpu_layer_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    diag = open(os.path.join(ROOT, "include", "delivr_hip_diag.h")).read()
    fmts = {"fp16", "bf16"}
    # plan codes
    conv_codes = set(re.findall(r"^#define DLV_PLAN_(DEEP|ZMARCH|GENERIC)\b", diag, re.M))
    assert conv_codes == {"DEEP", "ZMARCH", "GENERIC"}
    dc_codes = set(re.findall(r"^#define DLV_PLAN_DC_([A-Z]+)\b", diag, re.M))
    assert len(dc_codes) == 5, dc_codes
    for code in conv_codes:
        assert {f for f, r in mod.CONV_ROWS if r.family == code} == fmts, code
    for code in dc_codes:
        assert {f for f, r, _ in mod.DECONV_ROWS if r.kernel == code} == fmts, code
    assert {r.kernel for _, r, _ in mod.DECONV_ROWS} == dc_codes
    # conv_deep.hip: CD_GO(P, TX, NCB)
    deep = open(os.path.join(ROOT, "delivr_cfos_amd", "csrc", "conv_deep.hip")).read()
    go = set(re.findall(r"CD_GO\((PF16|PBf16), (\d+), (\d+)\);", deep))
    assert len(go) == 8, sorted(go)
    want = {("fp16" if p == "PF16" else "bf16", int(tx), int(ncb)) for p, tx, ncb in go}
    have = {(f, r.tx, r.ncb) for f, r in mod.CONV_ROWS if r.family == "DEEP"}
    assert want == have, (sorted(want - have), sorted(have - want))
    # the generic conv: launch_generic_ncb<TX, WLDS> for TX 16 / 8, each reaching launch_generic<NCB, TX, WLDS> for NCB 1, 2 and
    # (without LDS weights) 4
    unet = open(os.path.join(ROOT, "delivr_cfos_amd", "csrc", "unet_bf16.hip")).read()
    reach = set(re.findall(r"launch_generic_ncb<(\d+), (true|false)>\(plan\.ncb", unet))
    assert reach == {("16", "true"), ("8", "true"), ("16", "false"), ("8", "false")}, reach
    body = unet[unet.index("int launch_generic_ncb("):unet.index("// one planned conv")]
    assert re.findall(r"launch_generic<([^,]+), TX, WLDS>", body) == ["1", "2", "WLDS ? 2 : 4"], body
    want = {(f, int(tx), ncb, w == "true") for f in fmts for tx, w in reach for ncb in ((1, 2) if w == "true" else (1, 2, 4))}
    assert len(want) == 20
    have = {(f, r.tx, r.ncb, r.wlds) for f, r in mod.CONV_ROWS if r.family == "GENERIC"}
    assert want == have, (sorted(want - have), sorted(have - want))
    # every row appears once per format
    for rows in (mod.CONV_ROWS, mod.DECONV_ROWS):
        for a, b in itertools.combinations(rows, 2):
            assert a != b, a
