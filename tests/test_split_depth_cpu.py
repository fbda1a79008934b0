"""The split of fused cells by Euclidean depth cores (settings["mi355x"]["split_radius"] / ["split_fraction"]): the host side - the
parsers, the options record, the HBM row, the measuring plan, the header - and the numpy reference the GPU tests compare with
(tests/helpers/split_depth_reference.py), pinned on the case the erosion split cannot do: flat cells in a stack whose planes lie far
apart.  No GPU."""
import dataclasses
import importlib.util
import os
import re

import numpy as np
import pytest

from delivr_cfos_amd import hostlogic as hl
from delivr_cfos_amd.hostlogic import (CountOptions, check_hbm_budget, count_options, depth_stats_settings, measuring_plan,
                                       split_depth_settings, split_fused_settings)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sd = _helper("split_depth_reference")
ref = sd.split


def _mi(**keys):
    return {"mi355x": keys}


# ---- the parsers --------------------------------------------------------------------------------------------------------------
def test_absent_keys_switch_nothing_on():
    for off in (None, {}, {"mi355x": None}, _mi(), _mi(split_radius=None, split_fraction=None), _mi(split_fused=2), _mi(depth_stats=True)):
        assert split_depth_settings(off) is None


@pytest.mark.parametrize("radius, core_d2", [(3, 9), (2.5, 7), (0.1, 1), (np.float64(2.5), 7), (np.int64(3), 9), (65535, 65535**2),
                                             (65535.9, 4294954189), (65535.99999, 2**32 - 1)])
def test_core_d2_is_the_square_of_the_radius_rounded_up(radius, core_d2):
    got = split_depth_settings(_mi(split_radius=radius))
    assert got == (core_d2, 0, 1, (1, 1, 1)) and type(got[0]) is int


def test_the_keys_alone_and_together():
    assert split_depth_settings(_mi(split_fraction=60)) == (0, 60, 1, (1, 1, 1))
    assert split_depth_settings(_mi(split_fraction=1)) == (0, 1, 1, (1, 1, 1))
    assert split_depth_settings(_mi(split_fraction=np.int32(99))) == (0, 99, 1, (1, 1, 1))
    got = split_depth_settings(_mi(split_radius=30, split_fraction=60, split_min_core=4, depth_spacing=[37, 10, 10]))
    assert got == (900, 60, 4, (37, 10, 10))
    assert all(type(v) is int for v in got[:3] + got[3])
    assert split_depth_settings(_mi(split_fraction=50, split_fused=0)) == (0, 50, 1, (1, 1, 1))  # (an erosion split that is off)
    assert split_depth_settings(_mi(split_radius=2, split_fused=False, split_min_core=2)) == (4, 0, 2, (1, 1, 1))


@pytest.mark.parametrize("bad", [True, False, 0, -1, 0.0, -2.5, "3", [3], float("nan"), float("inf"), 65536, 65535.999999, 1e30])
def test_a_bad_radius_is_refused(bad):
    with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['split_radius'\]"):
        split_depth_settings(_mi(split_radius=bad))
    with pytest.raises(ValueError, match="split_radius"):
        count_options(_mi(split_radius=bad), -1, -1)


@pytest.mark.parametrize("bad", [True, False, 0, 100, -5, 50.5, "50", [50]])
def test_a_bad_fraction_is_refused(bad):
    with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['split_fraction'\] = .*an integer 1\.\.99"):
        split_depth_settings(_mi(split_fraction=bad))
    with pytest.raises(ValueError, match="split_fraction"):  # (beside a good radius too)
        split_depth_settings(_mi(split_radius=3, split_fraction=bad))


def test_the_spacing_is_that_of_depth_stats():
    for bad in (3, [1, 1], [0, 1, 1], [1, 65, 1], [1.0, 1, 1], [True, 1, 1]):
        with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['depth_spacing'\] = .*three integers 1\.\.64"):
            split_depth_settings(_mi(split_radius=3, depth_spacing=bad))
    # depth_spacing needs somebody who measures with it: depth_stats, or one of the two keys
    assert depth_stats_settings(_mi(split_radius=3, depth_spacing=[2, 1, 1])) is None
    assert depth_stats_settings(_mi(split_fraction=50, depth_spacing=[2, 1, 1])) is None
    with pytest.raises(ValueError, match=r"depth_spacing'\] = \[2, 1, 1\] needs settings\['mi355x'\]\['depth_stats'\]"):
        depth_stats_settings(_mi(depth_spacing=[2, 1, 1]))
    both = count_options(_mi(split_radius=3, depth_stats=True, depth_spacing=[3, 2, 1]), -1, -1)
    assert both.depth == (3, 2, 1) and both.split_depth == (9, 0, 1, (3, 2, 1))


def test_split_min_core_belongs_to_whichever_split_is_on():
    for bad in (0, -1, True, 1.5, "2"):
        with pytest.raises(ValueError, match=r"split_min_core'\] = .*an integer >= 1"):
            split_depth_settings(_mi(split_radius=3, split_min_core=bad))
    assert split_fused_settings(_mi(split_radius=3, split_min_core=2)) is None
    assert split_fused_settings(_mi(split_fraction=50, split_min_core=2)) is None
    assert split_fused_settings(_mi(split_fused=0, split_fraction=50, split_min_core=2)) is None
    for alone in (_mi(split_min_core=2), _mi(split_fused=0, split_min_core=2), _mi(split_fused=False, split_min_core=1)):
        with pytest.raises(ValueError, match="split_min_core.*needs.*split_fused"):  # (the text of before)
            split_fused_settings(alone)
        with pytest.raises(ValueError, match="split_min_core.*needs.*split_fused"):
            count_options(alone, -1, -1)
    assert split_fused_settings(_mi(split_fused=3, split_min_core=4)) == (3, 4)  # (still a 2-tuple)


@pytest.mark.parametrize("other", [{"split_radius": 3}, {"split_fraction": 50}, {"split_radius": 3, "split_fraction": 50}])
def test_the_two_splits_are_alternatives(other):
    named = "split_radius" if "split_radius" in other else "split_fraction"
    with pytest.raises(ValueError, match=rf"split_fused.*{named}|{named}.*split_fused"):
        split_depth_settings(_mi(split_fused=2, **other))
    with pytest.raises(ValueError, match=rf"split_fused.*{named}|{named}.*split_fused"):
        count_options(_mi(split_fused=2, **other), -1, -1)


# ---- the options record -------------------------------------------------------------------------------------------------------
def test_the_options_record():
    names = [f.name for f in dataclasses.fields(CountOptions)]
    assert names[-2:] == ["split_depth", "fill_holes"] and names.index("split") == 5  # (before fill_holes, which stays last)
    assert names[:6] == ["bounds", "intensity", "shell_radius", "quartiles", "shape", "split"]
    assert CountOptions().split_depth is None and CountOptions().split is None
    assert count_options({}, -1, -1) == CountOptions()
    assert count_options(_mi(split_fused=2), -1, -1) == CountOptions(split=(2, 1))  # (split stays (depth, min_core))
    opts = count_options(_mi(split_radius=2.5, split_fraction=70, split_min_core=3, depth_spacing=[37, 10, 10]), -1, -1)
    assert opts == CountOptions(split_depth=(7, 70, 3, (37, 10, 10))) and opts.split is None and opts.depth is None


def test_the_measuring_plan_is_unaffected():
    opts = CountOptions(split_depth=(9, 0, 1, (3, 1, 1)))
    assert measuring_plan(opts, None) == frozenset() == measuring_plan(opts, {"voxel_counts": 0})
    both = CountOptions(split_depth=(9, 0, 1, (3, 1, 1)), depth=(3, 1, 1), shape=True)
    assert measuring_plan(both, None) == measuring_plan(CountOptions(depth=(3, 1, 1), shape=True), None) == {"depth", "shape"}


# ---- the HBM row --------------------------------------------------------------------------------------------------------------
def test_the_hbm_row_and_its_order():
    assert "split_radius" not in hl._HBM_CACHED and "split_fused" not in hl._HBM_CACHED
    at = hl._HBM_FRESH.index("split_fused")
    assert hl._HBM_FRESH[at + 1] == "split_radius"  # where split_fused stands: after what is measured, before the size filter
    assert hl._HBM_FRESH.index("depth_stats") < at and hl._HBM_FRESH.index("size_filter") > at + 1
    vox = 1000
    for opts in (CountOptions(split_depth=(9, 0, 1, (1, 1, 1))), CountOptions(split_depth=(0, 50, 1, (37, 10, 10)))):
        check_hbm_budget(opts, frozenset(), False, 9, vox, vox * 17)  # the mask, its labels and 8 more bytes per voxel fit
        with pytest.raises(MemoryError, match=r"settings\['mi355x'\]\['split_radius'\].* needs 8 more bytes per voxel in HBM beside the mask "
                                              r"and its labels.*slab-streamed labelling does not split.*hbm_budget_gb"):
            check_hbm_budget(opts, frozenset(), False, 9, vox, vox * 17 - 1)
        check_hbm_budget(opts, frozenset(), True, 4, vox, vox * 4)  # cached labels are not split: nothing is asked
    # ... the same need as split_fused
    with pytest.raises(MemoryError, match="split_fused"):
        check_hbm_budget(CountOptions(split=(2, 1)), frozenset(), False, 9, vox, vox * 17 - 1)
    check_hbm_budget(CountOptions(), frozenset(), False, 9, vox, 1)  # without a key nothing is asked


# ---- the header ---------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entry_with_its_definition():
    header = open(os.path.join(ROOT, "include", "delivr_hip.h")).read()
    decl = re.search(r"int dlv_cc_split_depth_dev\(([^;]*)\);", header)
    assert decl, "include/delivr_hip.h does not declare dlv_cc_split_depth_dev"
    args = " ".join(decl.group(1).split())
    assert args == ("dlv_ctx* ctx, uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx, uint32_t core_d2, "
                    "int core_pct, int64_t min_core, uint32_t* work_a_dev, uint32_t* work_b_dev, uint64_t* n_out, uint64_t* n_split_out, "
                    "uint32_t* parent_dev, uint64_t parent_cap")
    comment = header[:decl.start()].rsplit("/*", 1)[1]
    for said in ("26-adjacent", "dlv_cc_depth_dev", "core_pct^2 * m(l) / 10000", "dlv_cc_split_dev", "DLV_EUNSUP", "Synchronous"):
        assert said in comment, said
    from delivr_cfos_amd import _lib

    assert len(_lib.SIGNATURES["dlv_cc_split_depth_dev"][1]) == 18  # (the binding takes as many arguments as the declaration)


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def discs():
    """6 x 24 x 40: two discs of radius 5, two planes thick, their centres ten voxels apart in x - they share one voxel per plane,
    the neck.  Voxels of 1.62 x 1.62 x 6.0 um: spacing (37, 10, 10) in units of 0.162 um"""
    mask = np.zeros((6, 24, 40), dtype=bool)
    yy, xx = np.ogrid[:24, :40]
    for cx in (14, 24):
        mask[2:4] |= ((yy - 12) ** 2 + (xx - cx) ** 2 <= 25)[None]
    L, n = ref.label26(mask)
    assert n == 1 and int(mask.sum()) == 322
    L.setflags(write=False)
    return L, n


@pytest.mark.parametrize("radius", [20, 30, 35])
def test_depth_cores_split_the_flat_pair(discs, radius):
    L, n = discs
    want = sd.split_depth_reference(L, n, (37, 10, 10), radius * radius, 0)
    assert (want["M"], want["K"], want["n_split"]) == (2, 2, 1)
    assert np.bincount(want["out"].ravel())[1:].tolist() == [162, 160]
    assert want["parent"].tolist() == [0, 1, 1] and ((want["out"] != 0) == (L != 0)).all()
    assert want["out"][2, 12, 14] == 1 and want["out"][2, 12, 24] == 2 and want["out"][2, 12, 19] == 1  # the neck: a tie, the first core


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_erosion_cores_do_not(discs, depth):
    L, n = discs
    want = ref.split_reference(L, n, depth)
    assert (want["M"], want["K"], want["n_split"]) == (0, 1, 0)  # two planes: the first step along z takes every voxel
    np.testing.assert_array_equal(want["out"], L)


@pytest.mark.parametrize("fraction", [50, 70, 90, 99])
def test_a_fraction_leaves_one_core_in_a_ball(fraction):
    L, n = ref.label26(ref.ball((21, 21, 21), (10, 10, 10), 8))
    want = sd.split_depth_reference(L, n, (1, 1, 1), 0, fraction)
    assert (want["M"], want["K"], want["n_split"]) == (1, 1, 0)
    np.testing.assert_array_equal(want["out"], L)


def test_the_thresholds():
    L = np.zeros((9, 9, 20), dtype=np.uint32)
    L[1:8, 1:8, 1:8] = 1    # m = 16
    L[3:6, 3:6, 10:13] = 3  # m = 4; label 2 has no voxel
    d2 = sd.depth.depth_map(L, 3)
    assert sd.thresholds(L, 3, d2, 0, 50).tolist() == [1, 4, 1, 1]
    assert sd.thresholds(L, 3, d2, 0, 51).tolist() == [1, 5, 1, 2]  # ceil(2601 * 16 / 10000) = ceil(4.16); ceil(1.04)
    assert sd.thresholds(L, 3, d2, 3, 99).tolist() == [3, 16, 3, 4]  # ceil(15.68); ceil(3.92): the peak itself is always a core
    assert sd.thresholds(L, 3, d2, 9, 0).tolist() == [9, 9, 9, 9]
    # core_d2 above m(l): label 3 has no core and stays whole; label 1 keeps one
    want = sd.split_depth_reference(L, 3, (1, 1, 1), 9, 0)
    assert want["M"] == 1 and want["K"] == 2 and want["n_split"] == 0
    # a label above n is not measured, holds no core and is refused by the device; the reference numbers it like the rest
    assert not sd.cores(L, 2, (1, 1, 1), 1, 0)[L == 3].any()
