"""bf16 MFMA path vs the oracle: every kernel in isolation (dlv_debug_layer16), the whole
forward, and the fused sliding-window pass.  Tolerances are the bf16 ones stated in DESIGN.md:
activations/weights carry 8 significant bits, accumulation and InstanceNorm statistics are fp32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net():
    from oracle import delivr_oracle as orc

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


def _bf(t):
    return t.bfloat16().float()


def _conv_block(net, li):
    from delivr_cfos_amd.engine import CONV_BLOCKS

    mod = net
    for part in CONV_BLOCKS[li].split("."):
        mod = getattr(mod, part)
    return mod


# (layer, c1, c2, D, H, W); CONV_FAMILY: the conv family the dispatcher (csrc/layer_plan.h) sends each case to under the default
# switches, asserted from the layer hook's report.  W < 32 at these sizes: conv_deep.hip (16-wide and 8-wide tiles, 32 / 64
# output channels per workgroup, concat inputs, ragged tile borders); W >= 32: the z-march up to 32768 voxels, the z-reg conv
# above.  None of them reaches the generic conv (conv3_mfma_kernel): each kernel on its own, with every instantiation, is in
# tests/test_gpu_layer_kernels.py and tests/test_gpu_conv_kernels.py
CONV_CASES = [
    (1, 32, 0, 8, 8, 32),
    (1, 32, 0, 6, 10, 24),      # partial tiles in z, y and x
    (16, 32, 32, 8, 12, 16),    # concat 32+32 -> 32
    (5, 64, 0, 8, 8, 16),       # 64 -> 64
    (4, 32, 0, 4, 6, 8),        # 32 -> 64, W=8 -> 8-wide tiles
    (9, 256, 0, 4, 4, 8),       # 256 -> 256, 8-wide tiles
    (10, 128, 128, 2, 6, 12),   # concat 128+128 -> 128, odd sizes
    (12, 64, 64, 4, 8, 16),
    # W >= 32 and Cout = 32 (ragged tiles, z segments, concat).  Layers of at most 32768 voxels take the LDS-weights
    # z-march (conv_zmarch.hip), larger ones the register-resident-weights conv (conv_zreg_kernel.h, 8-row tiles here)
    (1, 32, 0, 6, 12, 40),
    (17, 32, 0, 40, 16, 64),     # c32_t8
    (16, 32, 32, 9, 8, 32),
    (14, 32, 32, 24, 20, 72),    # c64_t8 (32 + 32)
    # Cout = 64 with W >= 32: two output-channel blocks (z segments, ragged rows)
    (4, 32, 0, 20, 12, 32),
    (5, 64, 0, 33, 24, 64),      # c64_t8
]
CONV_FAMILY = dict(zip(CONV_CASES, ("ZMARCH", "DEEP", "DEEP", "DEEP", "DEEP", "DEEP", "DEEP", "DEEP", "ZMARCH", "ZREG", "ZMARCH", "ZREG", "ZMARCH", "ZREG")))


@pytest.mark.parametrize("li,c1,c2,D,H,W", CONV_CASES)
def test_conv_block_bf16(eng, net, li, c1, c2, D, H, W):
    """Conv3d+InstanceNorm+Mish of one block vs torch fp32 on the SAME bf16-rounded inputs and
    weights: what remains is fp32 summation order + the bf16 rounding of the stored raw / output
    tensors -> max abs error 0.06 on O(1) activations, mean abs error 6e-3."""
    import torch
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(li * 100 + D)
    B = 2
    x1 = _bf(torch.randn((B, c1, D, H, W), generator=g))
    x2 = _bf(torch.randn((B, c2, D, H, W), generator=g)) if c2 else None
    blk = _conv_block(net, li)
    xin = x1 if x2 is None else torch.cat([x1, x2], dim=1)
    with torch.no_grad():
        raw = F.conv3d(xin, _bf(blk.conv.weight), blk.conv.bias, padding=1)
        ref = F.mish(F.instance_norm(raw, weight=blk.adn.N.weight, bias=blk.adn.N.bias, eps=1e-5))
    out, rep = eng.debug_layer16(0, "conv", li, x1.cuda(), None, None if x2 is None else x2.cuda(), precision="bf16")
    assert rep["conv"] == CONV_FAMILY[(li, c1, c2, D, H, W)], rep
    err = (out.cpu() - ref).abs()
    assert err.max() < 0.06, float(err.max())
    assert err.mean() < 6e-3, float(err.mean())


@pytest.mark.parametrize("j,D,H,W", [(0, 2, 2, 4), (1, 3, 4, 5), (2, 4, 8, 8), (3, 8, 8, 16)])
def test_deconv_bf16(eng, net, j, D, H, W):
    import torch
    import torch.nn.functional as F

    up = getattr(net, f"upcat_{4 - j}").upsample.deconv
    g = torch.Generator().manual_seed(j)
    x = _bf(torch.randn((2, up.in_channels, D, H, W), generator=g))
    with torch.no_grad():
        ref = F.conv_transpose3d(x, _bf(up.weight), up.bias, stride=2)
    out, rep = eng.debug_layer16(1, "conv", j, x.cuda(), precision="bf16")
    assert rep["deconv"] == ("DEEP" if j < 2 else "ROWS"), rep
    assert tuple(out.shape) == tuple(ref.shape)
    err = (out.cpu() - ref).abs()
    scale = float(ref.abs().max())
    assert err.max() < 8e-3 * max(scale, 1.0), (float(err.max()), scale)


@pytest.mark.parametrize("fmt", ["bf16_all", "bf16"])  # bf16 at every level / the mixed format (fp16 at level 0: DLV_PREC_BF16)
def test_forward_bf16_vs_oracle(eng, net, golden_dir, fmt):
    """Whole forward, bf16 vs the torch-fp32 oracle logits.  Stated tolerance: relative RMS error of
    the logits <= 5e-2 and sign agreement >= 0.97 with SEEDED RANDOM weights (whose logits have
    std ~0.36 and no margin around 0 - see DESIGN.md 'Precision'); the fp32 path is the IoU>=0.999
    parity mode."""
    import os
    import torch

    g = np.load(os.path.join(golden_dir, "orc_unet.npz"))
    for xk, lk in (("x32", "logits32"), ("x_odd", "logits_odd")):
        x = torch.from_numpy(g[xk].astype(np.float32))[None, None].cuda()
        out = eng.unet_forward(x, fmt).cpu().numpy()[0, 0]
        ref = g[lk]
        rel = float(np.sqrt(np.mean((out - ref) ** 2)) / ref.std())
        agree = float(((out >= 0) == (ref >= 0)).mean())
        print(f"{xk} [{fmt}]: rel rms {rel:.4f} sign agreement {agree:.4f}")
        assert rel < 5e-2, rel
        assert agree > 0.97, agree


@pytest.mark.parametrize("fmt", ["bf16_all", "bf16"])
def test_forward_bf16_batch_independent(eng, golden_dir, fmt):
    import os
    import torch

    g = np.load(os.path.join(golden_dir, "orc_unet.npz"))
    x = torch.from_numpy(g["x32"].astype(np.float32))[None, None].cuda()
    xb = torch.cat([x, x.flip(3), x * 0.25], dim=0).contiguous()
    a = eng.unet_forward(xb, fmt)
    b = eng.unet_forward(x, fmt)
    assert torch.equal(a[0], b[0])  # per-sample statistics, deterministic reductions


@pytest.mark.parametrize("fmt", ["bf16_all", "bf16"])
@pytest.mark.parametrize("flip", [None, 2, 3, 4])
def test_sw_pass_bf16_matches_fp32_engine(eng, golden_dir, flip, fmt):
    """Fused path (stem reads the uint16 volume, final layer blends) vs the fp32 engine pass: same
    windows, same skips, count map identical; blended logits within the bf16 tolerance."""
    import os
    import torch

    vol = np.load(os.path.join(golden_dir, "ref_blend.npz"))["volume"]
    roi = (32, 32, 16)
    v = eng.to_device(vol)
    res = {}
    for prec in ("fp32", fmt):
        acc = torch.zeros(vol.shape, dtype=torch.float32, device="cuda")
        cnt = torch.zeros(vol.shape, dtype=torch.uint8, device="cuda")
        st = eng.sw_infer(eng.make_sw_params(vol.shape, roi, 0.5, flip, 0, prec, sw_batch=5), v, acc, cnt)
        eng.sync()
        res["fp32" if prec == "fp32" else "bf16"] = (acc.cpu().numpy(), cnt.cpu().numpy(), st)
    assert res["fp32"][2] == res["bf16"][2]
    np.testing.assert_array_equal(res["fp32"][1], res["bf16"][1])
    a32, a16 = res["fp32"][0], res["bf16"][0]
    live = a32 > -500
    assert np.abs(a32[~live] - a16[~live]).max() < 0.5  # skipped windows add exactly -1000 in both
    rel = float(np.sqrt(np.mean((a16 - a32)[live] ** 2)) / a32[live].std())
    assert rel < 5e-2, rel
    # repeat=5 equals five passes up to fp32 rounding
    acc5 = torch.zeros(vol.shape, dtype=torch.float32, device="cuda")
    eng.sw_infer(eng.make_sw_params(vol.shape, roi, 0.5, flip, 0, fmt, sw_batch=5, repeat=5), v, acc5)
    eng.sync()
    np.testing.assert_allclose(acc5.cpu().numpy(), 5 * a16, rtol=1e-5, atol=1e-3)


def test_sw_pass_fast_kernels_vs_generic_and_fp32(net):
    """Window 16x32x48 (W >= 32: z-marching convs + MFMA stem, ragged x tiles) against the generic
    kernels (diag switch "no_zmarch") and the fp32 engine."""
    import os
    import torch
    from delivr_cfos_amd.engine import HipEngine
    from delivr_cfos_amd.synth import synth_volume_np

    vol = synth_volume_np((32, 64, 96), seed=11, dense=True)
    vol[:, :, 40:] = 0
    roi = (16, 32, 48)
    out = {}
    for tag, env, prec in (("fast", None, "bf16"), ("generic", "1", "bf16"), ("fp32", None, "fp32")):
        e = HipEngine(0)
        if env:
            e.diag_set("no_zmarch", 1)
        e.load_state_dict({"state_dict": net.state_dict()})
        acc = torch.zeros(vol.shape, dtype=torch.float32, device="cuda")
        st = e.sw_infer(e.make_sw_params(vol.shape, roi, 0.5, 3, 0, prec), e.to_device(vol), acc)
        e.sync()
        out[tag] = (acc.cpu().numpy(), st)
        e.close()
    assert out["fast"][1] == out["generic"][1] == out["fp32"][1]
    assert out["fp32"][1]["n_skipped"] > 0
    ref = out["fp32"][0]
    live = ref > -500
    for tag in ("fast", "generic"):
        a = out[tag][0]
        rel = float(np.sqrt(np.mean((a - ref)[live] ** 2)) / ref[live].std())
        print(tag, "rel rms vs fp32:", rel)
        assert rel < 5e-2, (tag, rel)


# ---------------------------------------------------------------------------------------------------
# IEEE-half variant of the same kernels (precision="fp16"): 11 significant bits instead of 8
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("li,c1,c2,D,H,W", [CONV_CASES[0], CONV_CASES[2], CONV_CASES[5], CONV_CASES[8], CONV_CASES[11], CONV_CASES[12],
                                            CONV_CASES[13]])
def test_conv_block_fp16(eng, net, li, c1, c2, D, H, W):
    """Same check as test_conv_block_bf16 on fp16-rounded inputs/weights: errors shrink by the 3 extra mantissa bits."""
    import torch
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(li * 100 + D)
    x1 = torch.randn((2, c1, D, H, W), generator=g).half().float()
    x2 = torch.randn((2, c2, D, H, W), generator=g).half().float() if c2 else None
    blk = _conv_block(net, li)
    xin = x1 if x2 is None else torch.cat([x1, x2], dim=1)
    with torch.no_grad():
        raw = F.conv3d(xin, blk.conv.weight.half().float(), blk.conv.bias, padding=1)
        ref = F.mish(F.instance_norm(raw, weight=blk.adn.N.weight, bias=blk.adn.N.bias, eps=1e-5))
    out, rep = eng.debug_layer16(0, "conv", li, x1.cuda(), None, None if x2 is None else x2.cuda(), precision="fp16")
    assert rep["conv"] == CONV_FAMILY[(li, c1, c2, D, H, W)], rep
    err = (out.cpu() - ref).abs()
    assert err.max() < 0.01, float(err.max())
    assert err.mean() < 1e-3, float(err.mean())


def test_forward_fp16_vs_oracle(eng, golden_dir):
    """fp16 whole forward vs the torch-fp32 oracle: relative RMS <= 1e-2 (measured ~1e-3), sign agreement >= 0.999."""
    import os
    import torch

    g = np.load(os.path.join(golden_dir, "orc_unet.npz"))
    for xk, lk in (("x32", "logits32"), ("x_odd", "logits_odd")):
        x = torch.from_numpy(g[xk].astype(np.float32))[None, None].cuda()
        out = eng.unet_forward(x, "fp16").cpu().numpy()[0, 0]
        ref = g[lk]
        rel = float(np.sqrt(np.mean((out - ref) ** 2)) / ref.std())
        agree = float(((out >= 0) == (ref >= 0)).mean())
        print(f"fp16 {xk}: rel rms {rel:.5f} sign agreement {agree:.5f}")
        assert rel < 1e-2, rel
        assert agree > 0.999, agree


def test_sw_pass_fp16_matches_fp32_engine(eng, golden_dir):
    """fused fp16 path (MFMA stem with the 2^-8 output scale, z-march convs) vs the fp32 engine on a 16x32x48-window pass."""
    import torch
    from delivr_cfos_amd.synth import synth_volume_np

    vol = synth_volume_np((32, 64, 96), seed=11, dense=True)
    vol[:, :, 40:] = 0
    vol[0, 0, 0] = 65535  # the largest uint16 through the scaled stem
    roi = (16, 32, 48)
    v = eng.to_device(vol)
    res = {}
    for prec in ("fp32", "fp16"):
        acc = torch.zeros(vol.shape, dtype=torch.float32, device="cuda")
        st = eng.sw_infer(eng.make_sw_params(vol.shape, roi, 0.5, 2, 0, prec), v, acc)
        eng.sync()
        res[prec] = (acc.cpu().numpy(), st)
    assert res["fp32"][1] == res["fp16"][1]
    a32, a16 = res["fp32"][0], res["fp16"][0]
    live = a32 > -500
    assert np.isfinite(a16).all()
    rel = float(np.sqrt(np.mean((a16 - a32)[live] ** 2)) / a32[live].std())
    assert rel < 1e-2, rel


# ---------------------------------------------------------------------------------------------------
# the "zm_variant" switch (dlv_diag_set): same torch reference, same tolerance
# ---------------------------------------------------------------------------------------------------
def test_product_library_refuses_the_diagnostic_zmarch_builds(eng):
    """ONE test for all of them: the experimental / stamped / timing-only builds (6, 11, 20, 24, 40, ...) of the z-march conv
    were retired; the library refuses to select them, so no setting can reach a wrong-result kernel."""
    from delivr_cfos_amd._lib import DelivrHipError

    for variant in (3, 4, 6, 11, 12, 13, 20, 24, 30, 40, 41, 45):
        with pytest.raises(DelivrHipError):
            eng.diag_set("zm_variant", variant)
    eng.diag_set("zm_variant", 0)


@pytest.mark.parametrize("variant", [50, 51])
@pytest.mark.parametrize("li,c1,c2,prec", [(1, 32, 0, "fp16"), (16, 32, 32, "fp16"), (1, 32, 0, "bf16"), (16, 32, 32, "bf16")])
def test_zmarch_variants(eng, net, variant, li, c1, c2, prec):
    """Register-resident-weights conv (50 = the default) and the LDS-resident-weights kernel (51) on the
    32->32 / 64->32 conv block on a 40x24x64 window (3 z chunks of 16, an in-plane tile grid of 3x2, ragged z tail):
    against conv3d+InstanceNorm+Mish in fp32 on the same 16-bit-rounded operands."""
    import torch
    import torch.nn.functional as F

    D, H, W = 40, 24, 64
    g = torch.Generator().manual_seed(li * 7 + variant)
    rnd = (lambda t: t.half().float()) if prec == "fp16" else _bf
    x1 = rnd(torch.randn((3, c1, D, H, W), generator=g))
    x2 = rnd(torch.randn((3, c2, D, H, W), generator=g)) if c2 else None
    blk = _conv_block(net, li)
    xin = x1 if x2 is None else torch.cat([x1, x2], dim=1)
    with torch.no_grad():
        raw = F.conv3d(xin, rnd(blk.conv.weight), blk.conv.bias, padding=1)
        ref = F.mish(F.instance_norm(raw, weight=blk.adn.N.weight, bias=blk.adn.N.bias, eps=1e-5))
    try:
        eng.diag_set("zm_variant", variant)
        out = eng.debug_layer16(0, "conv", li, in1=x1.cuda(), in2=None if x2 is None else x2.cuda(), precision=prec)[0].cpu()
    finally:
        eng.diag_set("zm_variant", 0)
    base = eng.debug_layer16(0, "conv", li, in1=x1.cuda(), in2=None if x2 is None else x2.cuda(), precision=prec)[0].cpu()
    err = (out - ref).abs()
    tol_max, tol_mean = (0.01, 1e-3) if prec == "fp16" else (0.06, 6e-3)
    assert err.max() < tol_max, float(err.max())
    assert err.mean() < tol_mean, float(err.mean())
    # the default build carries no conv bias (InstanceNorm removes it), the LDS-weights builds do: the stored raw values
    # round differently
    assert (out - base).abs().max() < 2 * tol_max


def _pass_with_switches(prec, switches, lanes=None, big=False, odd=None):
    """one sliding-window pass on a fresh engine whose kernel-selection switches were set through dlv_diag_set
    (include/delivr_hip_diag.h): 64^3 windows of a 64x96x128 volume (6 windows, z-reg convs at levels 0/1), or two 128^3 windows"""
    import torch
    from delivr_cfos_amd.engine import HipEngine
    from delivr_cfos_amd.synth import synth_volume_np
    from delivr_cfos_amd.weights import random_state_dict

    eng = HipEngine(0)
    try:
        for k, v in switches.items():
            eng.diag_set(k, v)
        if lanes:
            eng.set_lanes(lanes)
        eng.load_state_dict({"state_dict": random_state_dict(0)})
        vol = synth_volume_np((odd[0], odd[1], 3 * odd[2]) if odd else (128, 128, 256) if big else (64, 96, 128), seed=9, dense=True)
        acc = torch.zeros(vol.shape, dtype=torch.float32, device="cuda")
        eng.sw_infer(eng.make_sw_params(vol.shape, odd or ((128, 128, 128) if big else (64, 64, 64)), 0.5, None, 0, prec), eng.to_device(vol), acc)
        eng.sync()
        return acc.cpu().numpy()
    finally:
        eng.close()


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_library_switches_that_pick_other_kernels_give_the_same_pass(prec):
    """Every kernel-selection switch (dlv_diag_set; the library reads none from the environment) selects kernels, never results:
    the activation fused into the z-reg conv's staging (by conv block, "fuse_layers": the default fuses block 17 = upcat_1.conv_1,
    0 = a normalisation pass in front of every conv; by level, "fuse_levels": levels 0 and 1, incl. the 16-row and the addend
    instantiations), edge-step code on every plane ("zreg_dbg"), the LDS-weights z-march instead of the z-reg conv
    ("zreg_mask"), cout blocks of the generic conv ("generic_ncb"), lanes, the pooling pass by pooled voxels instead of by
    full lines ("pool_rows_off"), upcat_1 unfolded ("no_upconv") or folded with the one-tile kernel ("upconv_simple"), the
    generic kernel for the deep levels ("deep_mask" 0)."""
    base = _pass_with_switches(prec, {})
    std = float(base.std())
    # bit-identical: same arithmetic in another order of execution / another code path of the same kernel
    np.testing.assert_array_equal(_pass_with_switches(prec, {}, lanes=1), base, err_msg="lanes")
    for sw in ({"zreg_dbg": 1}, {"generic_ncb": 1}, {"pool_rows_off": 1}):
        np.testing.assert_array_equal(_pass_with_switches(prec, sw), base, err_msg=str(sw))
    # same values up to the rounding of one 16-bit store (activation applied while staging: the activated tensor is never
    # rounded through HBM differently, but the InstanceNorm partial sums are taken over other tiles) / another kernel
    tol = 2e-3 if prec == "fp16" else 2e-2
    for sw in ({"fuse_layers": 0}, {"fuse_layers": 3 << 16}, {"fuse_levels": 1}, {"fuse_levels": 2}, {"fuse_levels": 3}, {"zreg_mask": 0}, {"no_upconv": 1},
               {"upconv_simple": 1}, {"deep_mask": 0}, {"no_upconv": 1, "fuse_levels": 3}, {"no_upconv": 1, "fuse_layers": 0}):
        a = _pass_with_switches(prec, sw)
        rel = float(np.sqrt(np.mean((a - base) ** 2)) / std)
        print(sw, "rel rms vs default:", rel)
        assert rel < tol, (sw, rel)
    with pytest.raises(Exception):
        _pass_with_switches(prec, {"no_such_switch": 1})


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_library_switches_on_windows_with_odd_levels(prec):
    """The same on (67, 93, 70) windows (odd at levels 0, 1 and 3: 33 x 46 x 35, 16 x 23 x 17, 8 x 11 x 8, 4 x 5 x 4): the pooling
    pass of an odd level does not write back (MaxPool3d drops the last plane), a second pass - or the consumers' activation on
    load ("fuse_levels") - makes the skip tensor final, the up-sampled tensor is replicate-padded."""
    odd = (67, 93, 70)
    base = _pass_with_switches(prec, {}, odd=odd)
    std = float(base.std())
    np.testing.assert_array_equal(_pass_with_switches(prec, {}, lanes=1, odd=odd), base, err_msg="lanes")
    for sw in ({"zreg_dbg": 1}, {"generic_ncb": 1}, {"pool_rows_off": 1}):
        np.testing.assert_array_equal(_pass_with_switches(prec, sw, odd=odd), base, err_msg=str(sw))
    tol = 2e-3 if prec == "fp16" else 2e-2
    for sw in ({"fuse_layers": 0}, {"fuse_levels": 1}, {"fuse_levels": 2}, {"fuse_levels": 3}, {"zreg_mask": 0}, {"deep_mask": 0}, {"no_zmarch": 1}):
        a = _pass_with_switches(prec, sw, odd=odd)
        rel = float(np.sqrt(np.mean((a - base) ** 2)) / std)
        print(sw, "rel rms vs default:", rel)
        assert rel < tol, (sw, rel)


# ---------------------------------------------------------------------------------------------------
# upcat_1 folded: transposed conv + first conv = skip-half conv + 8-tap conv of the COARSE tensor (upconv.hip)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16", "bf16_all"])
@pytest.mark.parametrize("roi,shape,kernel", [
    ((64, 64, 64), (64, 64, 160), "upconv2m"),    # coarse 32^3: the persistent kernel; windows that overlap
    ((48, 80, 96), (48, 80, 192), "upconv2m"),    # coarse 24 x 40 x 48: full tiles, not a cube
    ((48, 48, 80), (48, 96, 80), "upconv2_"),     # coarse width 40: not a multiple of the 16-voxel tile -> the one-tile kernel
    ((128, 128, 128), (128, 128, 128), "upconv2m"),
])
def test_folded_upcat_conv_against_the_unfolded_path_and_fp32(net, prec, roi, shape, kernel):
    """The folded path (default) must agree with the unfolded one (diag switch "no_upconv": ConvTranspose kernel + 64-channel conv) to
    the rounding of the 16-bit format, both kernels of the folded path with each other, and each with the fp32 VALU path of
    the library within the tolerance of the other 16-bit tests; the profile labels prove which kernel ran.  The switches are
    read when a context is created."""
    import os

    import torch

    from delivr_cfos_amd.engine import HipEngine
    from delivr_cfos_amd.synth import synth_volume_np

    engs = {}
    try:
        for tag, sw in (("folded", {}), ("simple", {"upconv_simple": 1}), ("unfolded", {"no_upconv": 1})):
            e = HipEngine(0)
            for k, v in sw.items():
                e.diag_set(k, v)
            e.load_state_dict({"state_dict": net.state_dict()})
            engs[tag] = e
    finally:
        pass
    vol = synth_volume_np(shape, seed=13, dense=True)
    dvol = engs["folded"].to_device(vol)
    out, ran = {}, {}
    for tag, p in (("fp32", "fp32"), ("folded", prec), ("simple", prec), ("unfolded", prec)):
        e = engs["folded" if tag == "fp32" else tag]
        acc = torch.zeros(shape, dtype=torch.float32, device="cuda")
        e.prof_reset()
        e.prof_enable(True)
        e.sw_infer(e.make_sw_params(shape, roi, 0.5, None, 0, p), dvol, acc)
        e.sync()
        e.prof_enable(False)
        ran[tag] = [k for k, v in e.prof_report().items() if v["launches"]]
        out[tag] = acc.cpu().numpy()
    for e in engs.values():
        e.close()
    assert any(k.startswith(kernel) for k in ran["folded"]), ran["folded"]
    assert any(k.startswith("upconv2_") for k in ran["simple"]) and not any(k.startswith("upconv2m") for k in ran["simple"]), ran["simple"]
    assert not any(k.startswith("upconv") for k in ran["unfolded"]) and any(k.startswith("deconv2") for k in ran["unfolded"]), ran["unfolded"]
    assert not any(k.endswith("_add") for k in ran["unfolded"]) and any(k.endswith("_add") for k in ran["folded"])
    std = float(out["fp32"].std())
    rel = {t: float(np.sqrt(np.mean((out[t] - out["fp32"]) ** 2)) / std) for t in ("folded", "simple", "unfolded")}
    between = {t: float(np.sqrt(np.mean((out[t] - out["unfolded"]) ** 2)) / std) for t in ("folded", "simple")}
    kernels = float(np.sqrt(np.mean((out["folded"] - out["simple"]) ** 2)) / std)
    print(prec, roi, "vs fp32:", rel, "vs unfolded:", between, "persistent vs one-tile kernel:", kernels)
    tol32, tol16 = (1e-2, 2e-3) if prec == "fp16" else (5e-2, 2e-2)
    for t, r in rel.items():
        assert r < tol32, (t, r)
        assert r < 1.1 * rel["unfolded"] + 1e-4, (t, r, rel["unfolded"])  # folding does not cost accuracy (one rounding less)
    for t, r in between.items():
        assert r < tol16, (t, r)
    assert kernels < tol16 / 4, kernels  # same products, the face correction enters the fp32 sum first instead of last


def test_pooling_pass_by_full_lines_is_bit_identical_at_128():
    """Windows of 128^3: the full-line pooling kernel runs on levels 0 and 1 (W = 128 / 64, two / one 64-voxel segments per row) with
    the non-temporal policy on level 0; the diag switch "pool_rows_off" runs the pooled-voxel-per-thread kernel instead.  Same bits."""
    rows = _pass_with_switches("fp16", {}, big=True)
    voxels = _pass_with_switches("fp16", {"pool_rows_off": 1}, big=True)
    assert np.isfinite(rows).all() and rows.std() > 0
    np.testing.assert_array_equal(rows, voxels)
    # ... and the 16-row activating instantiation of the z-reg conv (the default's upcat_1.conv_1 at these windows) against a
    # normalisation pass + the plain one: the activated value is rounded to 16 bits once either way
    np.testing.assert_array_equal(_pass_with_switches("fp16", {"fuse_layers": 0}, big=True), rows)
