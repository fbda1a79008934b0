"""The float64 single-layer references of oracle/layer_ref.py (used by tests/test_gpu_conv_kernels.py) against the oracle
U-Net's own layers (orc.build_unet) run in float64, and the coverage table of the GPU file against conv_zreg.h."""
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
