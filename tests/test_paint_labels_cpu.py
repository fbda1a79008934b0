"""The host side of blob_highlighter's settings["mi355x"]["paint_from"] = "labels": the settings parser and the look-up tables
(hostlogic.paint_source, paint_luts), the numpy reference of the painting (tests/helpers/paint_reference.py) and the Z-slab planner
(blob_highlighter.plan_slabs).  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

from delivr_cfos_amd import blob_highlighter as bh
from delivr_cfos_amd import label_runs as lr
from delivr_cfos_amd.hostlogic import paint_luts, paint_source


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("paint_reference")


# ---- paint_source ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("settings", [None, {}, {"mi355x": None}, {"mi355x": {}}, {"mi355x": {"paint_from": None}},
                                      {"mi355x": {"paint_from": "boxes"}}])
def test_paint_source_defaults_to_the_boxes(settings):
    assert paint_source(settings) == "boxes"


def test_paint_source_selects_the_labels():
    assert paint_source({"mi355x": {"paint_from": "labels"}}) == "labels"


@pytest.mark.parametrize("value", ["Labels", "label", "", "runs", 1, True, ["labels"], b"labels"])
def test_paint_source_refuses_anything_else(value):
    with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['paint_from'\]"):
        paint_source({"mi355x": {"paint_from": value}})


def test_a_wrong_paint_source_is_refused_before_any_file_is_touched(tmp_path):
    missing = str(tmp_path / "nowhere")  # (none of these folders exists: reaching for one is a FileNotFoundError / OSError)
    settings = {"visualization": {"input_prediction_location": missing + "/bin/", "input_csv_location": missing + "/csv/",
                                  "output_location": missing + "/out", "no_atlas_depthmap": False, "region_id_rgb": True,
                                  "region_id_grayvalues": True},
                "postprocessing": {"output_location": missing + "/post"}, "mi355x": {"paint_from": "voxels"}}
    with pytest.raises(ValueError, match="paint_from"):
        bh.blob_highlighter(settings, ["brainA", ""], (1, 1, 4, 4, 4))
    assert not os.path.exists(missing)


# ---- paint_luts --------------------------------------------------------------------------------------------------------------
def test_paint_luts_packs_the_tables_by_label():
    ids = np.array([5, 1, 9, 3])
    red, green, blue = np.array([0, 255, 17, 1]), np.array([255, 0, 18, 2]), np.array([7, 255, 0, 3])
    graph_order = np.array([65535, 0, 1327, 255])
    rgb, region = paint_luts(ids, red, green, blue, graph_order, 9)
    assert rgb.dtype == np.uint8 and rgb.shape == (10, 3) and region.dtype == np.uint16 and region.shape == (10,)
    want_rgb = np.zeros((10, 3), dtype=np.uint8)
    want_region = np.zeros(10, dtype=np.uint16)
    want_rgb[5], want_rgb[1], want_rgb[9], want_rgb[3] = (0, 255, 7), (255, 0, 255), (17, 18, 0), (1, 2, 3)
    want_region[5], want_region[1], want_region[9], want_region[3] = 65535, 0, 1327, 255
    np.testing.assert_array_equal(rgb, want_rgb)  # 0 and 255 survive; the labels 0, 2, 4, 6, 7, 8 have no row: 0
    np.testing.assert_array_equal(region, want_region)  # 0 and 65535 survive
    assert not rgb[[0, 2, 4, 6, 7, 8]].any() and not region[[0, 2, 4, 6, 7, 8]].any()


def test_paint_luts_of_an_empty_table_are_all_background():
    none = np.zeros(0, dtype=np.int64)
    rgb, region = paint_luts(none, none, none, none, none, 3)
    assert rgb.shape == (4, 3) and region.shape == (4,) and not rgb.any() and not region.any()


def test_paint_luts_refuses_the_background_and_ids_beyond_the_labels():
    one = np.array([1])
    with pytest.raises(ValueError, match="background"):
        paint_luts(np.array([2, 0]), [1, 1], [1, 1], [1, 1], [1, 1], 4)
    with pytest.raises(IndexError, match="beyond"):
        paint_luts(np.array([5]), one, one, one, one, 4)  # n + 1
    rgb, region = paint_luts(np.array([4]), one, one, one, one, 4)  # n itself is a label
    assert region[4] == 1 and rgb[4].tolist() == [1, 1, 1]


# ---- the reference helper ----------------------------------------------------------------------------------------------------
def test_reference_of_a_hand_made_case():
    labels = np.array([[0, 1, 2], [3, 4, 2**32 - 2]], dtype=np.uint32)
    lut = np.array([99, 10, 0, 30], dtype=np.uint16)  # (entry 0 is never painted; label 2 has no colour)
    np.testing.assert_array_equal(ref.paint_by_label(labels, lut), np.array([[0, 10, 0], [30, 0, 0]], dtype=np.uint16))
    rgb = np.arange(12, dtype=np.uint8).reshape(4, 3)
    got = ref.paint_by_label(labels, rgb)
    assert got.shape == (2, 3, 3) and got.dtype == np.uint8
    assert got[0, 1].tolist() == [3, 4, 5] and got[1, 0].tolist() == [9, 10, 11] and not got[0, 0].any() and not got[1, 1:].any()
    both = ref.paint_by_label(labels, [lut, rgb])
    np.testing.assert_array_equal(both[1], got)


def test_reference_on_decoded_runs_equals_reference_on_the_labels():
    rng = np.random.default_rng(20)
    L = rng.integers(0, 40, size=(5, 7, 61), dtype=np.uint32)
    L[rng.random(L.shape) < 0.5] = 0
    L[1] = 0  # a plane of empty rows
    L[2, 3] = 17  # one run filling a row
    lut16 = rng.integers(0, 65536, size=33, dtype=np.uint16)  # (labels 33..39 lie beyond the table)
    rgb = rng.integers(0, 256, size=(33, 3), dtype=np.uint8)
    assert (L >= 33).any()
    back = lr.decode_runs(lr.encode_runs(L))
    for lut in (lut16, rgb):
        np.testing.assert_array_equal(ref.paint_by_label(back, lut), ref.paint_by_label(L, lut))
    np.testing.assert_array_equal(ref.paint_by_label(lr.decode_runs(lr.encode_runs(L), 2, 4), rgb), ref.paint_by_label(L[2:4], rgb))


# ---- the slab planner --------------------------------------------------------------------------------------------------------
def _assert_covers_once_in_order(slabs, Z):
    assert slabs[0][0] == 0 and slabs[-1][1] == Z
    for (a0, a1), (b0, b1) in zip(slabs, slabs[1:]):
        assert a1 == b0
    assert all(z0 < z1 for z0, z1 in slabs)


@pytest.mark.parametrize("Z", [1, 2, 13, 97, 100])
@pytest.mark.parametrize("slab_bytes", [1, 999, 1000, 2999, 3000, 13000, 10**9])
def test_slabs_cover_every_plane_once_in_order(monkeypatch, Z, slab_bytes):
    monkeypatch.setattr(bh, "_SLAB_BYTES", slab_bytes)
    plane_voxels, per_voxel = 100, 10  # one plane: 1000 bytes
    slabs = bh.plan_slabs(Z, plane_voxels, per_voxel)
    _assert_covers_once_in_order(slabs, Z)
    planes = max(1, slab_bytes // 1000)  # never less than one plane, never more than fit
    assert all(z1 - z0 == planes for z0, z1 in slabs[:-1]) and 1 <= slabs[-1][1] - slabs[-1][0] <= planes
    assert len(slabs) == -(-Z // planes)


def test_the_default_slab_is_two_gib():
    assert bh._SLAB_BYTES == 2 << 30
    slabs = bh.plan_slabs(1024, 2048 * 2048, 9)  # uint32 labels + RGB + region ids
    _assert_covers_once_in_order(slabs, 1024)
    assert slabs[0] == (0, (2 << 30) // (2048 * 2048 * 9))
