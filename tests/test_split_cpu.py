"""Host side of the split of fused cells (settings["mi355x"]["split_fused"]): the numpy reference of dlv_cc_split_dev pinned
against its direct form and against the facts the definition was chosen by, hostlogic.split_fused_settings and finish_split."""
import importlib.util
import os

import numpy as np
import pytest


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("split_reference")


def _cube_pair():
    """two 5 x 5 x 5 cubes joined by one voxel, the first in the corner at z = y = x = 0"""
    L = np.zeros((7, 7, 12), dtype=np.uint32)
    L[0:5, 0:5, 0:5] = 1
    L[0:5, 0:5, 6:11] = 1
    L[2, 2, 5] = 1
    return L


def _dumbbell():
    """two 3 x 3 x 3 cubes and a one-voxel bridge, mirror-symmetric in x: the bridge is as far from one core as from the other"""
    L = np.zeros((5, 5, 9), dtype=np.uint32)
    L[1:4, 1:4, 1:4] = 1
    L[1:4, 1:4, 5:8] = 1
    L[2, 2, 4] = 1
    return L


def _mixed():
    rng = np.random.default_rng(3)
    L, n = ref.label26(rng.random((8, 9, 12)) < 0.3)
    return L, n


def _same(a, b):
    for k in ("out", "parent"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert (a["K"], a["n_split"], a["M"]) == (b["K"], b["n_split"], b["M"])


def test_label26_numbers_components_by_their_first_voxel():
    m = np.zeros((3, 4, 6), dtype=np.uint8)
    m[0, 0, 4] = m[0, 1, 5] = 1  # diagonal neighbours: one component, found first
    m[0, 0, 0:2] = 1
    m[2, 3, 5] = 1
    m[1, 2, 2] = 1
    L, n = ref.label26(m)
    assert n == 4 and L[0, 0, 0] == 1 and L[0, 0, 4] == L[0, 1, 5] == 2 and L[1, 2, 2] == 3 and L[2, 3, 5] == 4
    assert ((L != 0) == (m != 0)).all()


@pytest.mark.parametrize("depth", [1, 2])
def test_iterated_reference_equals_the_direct_form_on_the_cube_pair(depth):
    L = _cube_pair()
    a, b = ref.split_reference(L, 1, depth), ref.split_reference(L, 1, depth, direct=True)
    _same(a, b)
    assert a["K"] == 2 and a["n_split"] == 1  # outside the volume counts as background: the corner cube has a core at both depths


def test_iterated_reference_equals_the_direct_form_on_a_tie():
    L = _dumbbell()
    a, b = ref.split_reference(L, 1, 1), ref.split_reference(L, 1, 1, direct=True)
    _same(a, b)
    assert a["K"] == 2 and a["M"] == 2
    assert a["out"][2, 2, 4] == 1  # the bridge goes to the smaller core label
    assert (a["out"][1:4, 1:4, 1:4] == 1).all() and (a["out"][1:4, 1:4, 5:8] == 2).all()


def test_iterated_reference_equals_the_direct_form_on_random_components():
    L, n = _mixed()
    for depth, min_core in ((1, 1), (1, 2)):
        a, b = ref.split_reference(L, n, depth, min_core), ref.split_reference(L, n, depth, min_core, direct=True)
        _same(a, b)
        assert ((a["out"] != 0) == (L != 0)).all() and a["K"] >= n


def test_two_balls_of_radius_5_with_centres_8_apart():
    """the prototype's facts: one piece at depth 1..3 and at depth 6, two at depth 4 and 5"""
    shape = (20, 24, 70)
    L = (ref.ball(shape, (10, 12, 30), 5) | ref.ball(shape, (10, 12, 38), 5)).astype(np.uint32)
    assert ref.label26(L)[1] == 1
    for depth in (1, 2, 3, 6):
        r = ref.split_reference(L, 1, depth)
        assert r["K"] == 1 and r["n_split"] == 0, depth
        np.testing.assert_array_equal(r["out"], L)  # nothing to split: the output is the input
        assert r["parent"].tolist() == [0, 1]
    assert ref.split_reference(L, 1, 6)["M"] == 0  # every core is gone
    for depth in (4, 5):
        r = ref.split_reference(L, 1, depth)
        assert r["K"] == 2 and r["n_split"] == 1 and r["M"] == 2, depth
        assert ((r["out"] != 0) == (L != 0)).all()  # the foreground is preserved
        assert r["parent"].tolist() == [0, 1, 1]
        assert r["out"][10, 12, 30] == 1 and r["out"][10, 12, 38] == 2
        # mirror-symmetric in x about 34: a voxel left of it is never farther from the first core, and ties go to the first core
        assert (r["out"][:, :, :35][L[:, :, :35] != 0] == 1).all() and (r["out"][:, :, 35:] == 2).any()


def test_output_equals_input_when_no_label_has_two_cores():
    L, n = _mixed()
    r = ref.split_reference(L, n, 3)
    assert r["n_split"] == 0 and r["K"] == n
    np.testing.assert_array_equal(r["out"], L)
    np.testing.assert_array_equal(r["parent"], np.arange(n + 1))


def test_min_core_drops_small_cores():
    L = np.zeros((7, 7, 16), dtype=np.uint32)
    L[0:5, 0:5, 0:5] = 1   # core at depth 1: 3 x 3 x 3 (the outside counts as background) and the voxel under the bridge
    L[1:4, 1:4, 6:9] = 1   # core at depth 1: the centre and the voxel under the bridge
    L[2, 2, 5] = 1
    assert ref.core_labels(L, 1)[1] == 2 and np.bincount(ref.core_labels(L, 1)[0].ravel()).tolist()[1:] == [28, 2]
    assert ref.split_reference(L, 1, 1)["K"] == 2 and ref.split_reference(L, 1, 1, min_core=2)["K"] == 2
    r = ref.split_reference(L, 1, 1, min_core=3)
    assert r["K"] == 1 and r["M"] == 1 and r["n_split"] == 0
    np.testing.assert_array_equal(r["out"], L)


def test_split_fused_settings_accepts_and_refuses():
    from delivr_cfos_amd.hostlogic import SPLIT_MAX_DEPTH, split_fused_settings

    assert SPLIT_MAX_DEPTH == 16
    for s in (None, {}, {"mi355x": None}, {"mi355x": {}}, {"mi355x": {"split_fused": 0}}, {"mi355x": {"split_fused": False}},
              {"mi355x": {"split_fused": None}}, {"mi355x": {"split_fused": 0.0}}):
        assert split_fused_settings(s) is None
    assert split_fused_settings({"mi355x": {"split_fused": 1}}) == (1, 1)
    assert split_fused_settings({"mi355x": {"split_fused": 16, "split_min_core": 27}}) == (16, 27)
    assert split_fused_settings({"mi355x": {"split_fused": np.int64(4), "split_min_core": np.int32(2)}}) == (4, 2)
    assert split_fused_settings({"mi355x": {"split_fused": 3.0}}) == (3, 1)  # (an integral float, as a JSON writer may leave it)
    got = split_fused_settings({"mi355x": {"split_fused": 3.0, "split_min_core": 2.0}})
    assert got == (3, 2) and all(type(v) is int for v in got)
    for bad in (True, 2.5, 17, -1, "3", [3], float("nan"), float("inf")):
        with pytest.raises(ValueError, match="split_fused"):
            split_fused_settings({"mi355x": {"split_fused": bad}})
    for bad in (0, -3, True, False, 1.5, "2"):
        with pytest.raises(ValueError, match="split_min_core"):
            split_fused_settings({"mi355x": {"split_fused": 2, "split_min_core": bad}})
    for off in ({"split_min_core": 2}, {"split_fused": 0, "split_min_core": 2}, {"split_fused": False, "split_min_core": 1}):
        with pytest.raises(ValueError, match="split_min_core.*needs.*split_fused"):
            split_fused_settings({"mi355x": off})


def test_finish_split_on_a_hand_made_table():
    from delivr_cfos_amd.hostlogic import SPLIT_KEYS, finish_split

    assert SPLIT_KEYS == ("split_parent", "split_siblings")
    out = finish_split([0, 1, 2, 2, 3, 2, 5], 5)
    assert tuple(out) == SPLIT_KEYS
    assert out["split_parent"].dtype == np.uint32 and out["split_siblings"].dtype == np.uint32
    assert out["split_parent"].tolist() == [0, 1, 2, 2, 3, 2, 5]
    assert out["split_siblings"].tolist() == [0, 1, 3, 3, 1, 3, 1]
    empty = finish_split(np.zeros(1, dtype=np.uint32), 0)
    assert empty["split_parent"].tolist() == [0] and empty["split_siblings"].tolist() == [0]
    for bad, n in (([], 3), ([1, 1], 3), ([0, 4], 3), ([0, 0], 3)):
        with pytest.raises(ValueError):
            finish_split(bad, n)


def test_count_blobs_refuses_a_bad_value_before_any_file_is_touched(tmp_path):
    from delivr_cfos_amd.count_blobs import count_blobs

    post = tmp_path / "post"
    settings = {"postprocessing": {"output_location": str(post) + "/"}, "mi355x": {"split_fused": 17}}
    with pytest.raises(ValueError, match="split_fused"):
        count_blobs(settings, str(tmp_path / "absent"), 0, "brain", (1, 1, 4, 4, 4))
    assert not post.exists() and count_blobs.last_split is None
