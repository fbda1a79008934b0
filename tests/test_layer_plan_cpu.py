"""The kernel each layer of the 16-bit forward runs, as delivr_cfos_amd/csrc/layer_plan.h decides it: dlv_diag_plan is host
arithmetic (what the forward itself consults), so the table of DESIGN section 4 and the rules it follows from are checked here
without a GPU.  tests/test_gpu_conv_kernels.py holds the same plans against what ran."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURES = (32, 32, 64, 128, 256, 32)
LEVEL = (0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0)
# the switch sets of tests/test_gpu_bf16.py (test_library_switches_*), and the default
SWITCH_SETS = [{}, {"zreg_dbg": 1}, {"generic_ncb": 1}, {"pool_rows_off": 1}, {"fuse_layers": 0}, {"fuse_layers": 3 << 16}, {"fuse_levels": 1},
               {"fuse_levels": 2}, {"fuse_levels": 3}, {"zreg_mask": 0}, {"no_upconv": 1}, {"upconv_simple": 1}, {"deep_mask": 0},
               {"no_upconv": 1, "fuse_levels": 3}, {"no_upconv": 1, "fuse_layers": 0}, {"no_zmarch": 1}]


@pytest.fixture(scope="module")
def layer_plan():
    from delivr_cfos_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    from delivr_cfos_amd.engine import layer_plan as lp

    return lp


def _first_input_channels(li):
    """c1 of conv block li: the skip tensor of an UpCat block's first conv, else all of its input"""
    f = FEATURES
    skip = {10: f[3], 12: f[2], 14: f[1], 16: f[0]}
    cin = [1, f[0], f[0], f[1], f[1], f[2], f[2], f[3], f[3], f[4], f[3] + f[4] // 2, f[3], f[2] + f[3] // 2, f[2], f[1] + f[2] // 2, f[1],
           f[0] + f[1], f[5]]
    return skip.get(li, cin[li])


def test_default_plan_of_a_128_window_is_the_table_of_design_section_4(layer_plan):
    p = layer_plan((128, 128, 128))
    kern = [c["kernel"] for c in p["conv"]]
    assert kern[0] == "STEM_MFMA"
    for li in (1, 2, 3, 14, 15, 16, 17):
        assert kern[li] == "ZREG", (li, kern[li])
    for li in (4, 5, 13):
        assert kern[li] == "ZMARCH", (li, kern[li])
    for li in range(6, 13):
        assert kern[li] == "DEEP", (li, kern[li])
    assert [li for li in range(18) if p["conv"][li]["folded"]] == [16]  # upconv + z-reg conv with addend
    assert (p["conv"][16]["cin"], p["conv"][16]["cout"]) == (32, 32)
    assert [li for li in range(18) if p["conv"][li]["act_on_load"]] == [17]
    assert [p["conv"][li]["tile_rows"] for li in (1, 16, 17)] == [16, 16, 16]  # level 0
    assert [p["conv"][li]["tile_rows"] for li in (2, 3, 14, 15)] == [8, 8, 8, 8]  # level 1
    assert [d["kernel"] for d in p["deconv"]] == ["DEEP", "DEEP", "REGW", None]
    assert [q["rows"] for q in p["pool"]] == [1, 1, 0, 0]
    assert [q["writeback"] for q in p["pool"]] == [1, 1, 1, 1] and not any(q["norm_after"] for q in p["pool"])
    labels = [l for l, _, _ in p["labels"]]
    assert labels[0] == "stem_mfma_u16" and labels[-1] == "final_conv_blend"
    assert "upconv2m_f16_c32x32_d64" in labels and "conv3_zreg_f16_c32x32_d128_add" in labels
    assert "conv3_zreg_f16_c32x32_d128_act" in labels
    assert not any(l.startswith("conv3_mfma") for l in labels)
    # the mixed mode: fp16 at level 0, bf16 below, the format changing in the two passes at the seam
    mixed = [l for l, _, _ in layer_plan((128, 128, 128), precision="bf16")["labels"]]
    assert "norm_mish_pool_f16_to_bf16" in mixed and "norm_mish_bf16_to_f16" in mixed
    assert "conv3_zreg_bf16_c32x32_d64" in mixed and "conv3_zreg_f16_c32x32_d128_act" in mixed


def test_no_zmarch_runs_the_generic_kernels_everywhere(layer_plan):
    p = layer_plan((128, 128, 128), {"no_zmarch": 1})
    assert p["conv"][0]["kernel"] == "STEM_VALU"
    assert all(c["kernel"] == "GENERIC" for c in p["conv"][1:])
    assert all(d["kernel"] == "PARITY" for d in p["deconv"])
    assert not any(c["folded"] or c["act_on_load"] for c in p["conv"])
    assert not any(q["norm_after"] for q in p["pool"])


def test_no_upconv_unfolds_upcat_1(layer_plan):
    p = layer_plan((128, 128, 128), {"no_upconv": 1})
    c = p["conv"][16]
    assert (c["kernel"], c["cin"], c["cout"], c["folded"], c["tile_rows"]) == ("ZREG", 64, 32, 0, 8)
    assert p["deconv"][3]["kernel"] == "REGW"
    assert not any(l.startswith("upconv2") for l, _, _ in p["labels"])


@pytest.mark.parametrize("window", [(128, 128, 128), (64, 64, 64), (24, 40, 72)])
@pytest.mark.parametrize("sw", [{}, {"no_zmarch": 1}, {"deep_mask": 0}], ids=str)
def test_only_the_generic_ncb_and_the_cache_policy_follow_the_batch(layer_plan, window, sw):
    """the InstanceNorm partial sums are per tile: a window's result must not depend on its batch.  What may: how many cout
    blocks a workgroup of the generic conv takes (same tiles), the non-temporal policy of a pass (same values) - and with
    them the algorithmic FLOPs / bytes of the labels, which count the whole batch"""
    def shape_of(p):
        for c in p["conv"]:
            c.pop("ncb")
        for q in p["pool"]:
            q.pop("nt")
        p["labels"] = [l for l, _, _ in p["labels"]]
        return p

    one = shape_of(layer_plan(window, sw, batch=1))
    for B in (3, 16):
        assert shape_of(layer_plan(window, sw, batch=B)) == one, B


def test_sweep_of_windows_and_switch_sets(layer_plan):
    from delivr_cfos_amd._lib import DelivrHipError

    sizes = (8, 16, 24, 40, 64, 96, 128)
    n_plans = 0
    for (d, h, w), sw in itertools.product(itertools.product(sizes, repeat=3), SWITCH_SETS):
        supported = min(d, h, w) >= 16 and (d >> 4) * (h >> 4) * (w >> 4) >= 2  # what dlv_unet_forward_dev / dlv_sw_infer_dev accept
        if not supported:
            with pytest.raises(DelivrHipError):
                layer_plan((d, h, w), sw)
            continue
        p = layer_plan((d, h, w), sw)
        n_plans += 1
        what = {}
        for li, c in enumerate(p["conv"][1:], start=1):
            l = LEVEL[li]
            dims = (d >> l, h >> l, w >> l)
            vox = dims[0] * dims[1] * dims[2]
            ctx = ((d, h, w), sw, li, c)
            if c["kernel"] == "ZREG":
                assert dims[2] >= 32 and vox > 32768, ctx
                assert c["tile_rows"] in (8, 16) and (c["tile_rows"] == 8 or c["cin"] == 32), ctx
            if c["act_on_load"]:
                assert c["kernel"] == "ZREG" and _first_input_channels(li) == 32, ctx
            if c["kernel"] == "DEEP":
                assert vox <= 32768, ctx
            if c["folded"]:
                assert li == 16 and c["kernel"] == "ZREG" and p["deconv"][3]["kernel"] is None, ctx
            what[li] = (c["kernel"], c["cin"], c["cout"], dims, c["act_on_load"], c["folded"])
        assert (p["deconv"][3]["kernel"] is None) == bool(p["conv"][16]["folded"])
        # one label per (family, shape): the conv labels of a forward and what they stand for map one to one
        conv_labels = [l for l, _, _ in p["labels"] if l.startswith("conv3_")]
        assert len(conv_labels) == 17, conv_labels
        by_label, by_what = {}, {}
        for li, label in zip(range(1, 18), conv_labels):
            assert by_label.setdefault(label, what[li]) == what[li], ((d, h, w), sw, label)
            assert by_what.setdefault(what[li], label) == label, ((d, h, w), sw, label)
            fam = {"ZREG": "zreg", "DEEP": "deep", "ZMARCH": "zmarch", "GENERIC": "mfma"}[what[li][0]]
            assert label.startswith(f"conv3_{fam}_") and f"_c{what[li][1]}x{what[li][2]}_d{what[li][3][0]}" in label, label
    assert n_plans > 3000


def test_unknown_switch_is_refused(layer_plan):
    from delivr_cfos_amd._lib import DelivrHipError

    with pytest.raises(DelivrHipError):
        layer_plan((64, 64, 64), {"no_such_switch": 1})


def test_zm_variant_takes_0_50_and_51_only(layer_plan):
    """the numbers that selected the retired experiment builds of the z-march conv are refused by the planner as dlv_diag_set
    refuses them; 50 is the default by another name, 51 gives every z-reg layer to the LDS-weights z-march conv"""
    from delivr_cfos_amd._lib import DelivrHipError

    for v in (3, 4, 6, 11, 12, 13, 20, 24, 25, 30, 31, 40, 45, 1, -1, 52):
        with pytest.raises(DelivrHipError):
            layer_plan((128, 128, 128), {"zm_variant": v})
    default = layer_plan((128, 128, 128), {"zm_variant": 0})
    assert default == layer_plan((128, 128, 128))
    assert layer_plan((128, 128, 128), {"zm_variant": 50}) == default
    lds = layer_plan((128, 128, 128), {"zm_variant": 51})
    zreg = [li for li in range(18) if default["conv"][li]["kernel"] == "ZREG"]
    assert zreg == [1, 2, 3, 14, 15, 16, 17]
    for li in range(1, 18):
        assert lds["conv"][li]["kernel"] == ("ZMARCH" if li in zreg else default["conv"][li]["kernel"]), li
    assert not any(c["folded"] or c["act_on_load"] for c in lds["conv"])
    assert any(l.startswith("conv3_zmarch_f16_c64x32_d128") for l, _, _ in lds["labels"])  # (upcat_1 unfolded: 32 + 32 channels)


def test_layer_plan_header_is_plain_host_code():
    """layer_plan.h compiles as C++17 on the host alone: no HIP header, nothing of the context"""
    cxx = shutil.which("clang++") or shutil.which("g++") or ("/opt/rocm/llvm/bin/clang++" if os.path.isfile("/opt/rocm/llvm/bin/clang++") else None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = os.path.join(ROOT, "delivr_cfos_amd", "csrc", "layer_plan.h")
    text = open(src).read()
    assert "hip/" not in text and "common.h" not in text
    subprocess.check_call([cxx, "-x", "c++", "-std=c++17", "-fsyntax-only", "-Wno-pragma-once-outside-header", src])
