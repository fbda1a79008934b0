"""Host side of settings["mi355x"]["fill_holes"], no GPU: what the reference of dlv_fill_holes_u8_dev
(scipy.ndimage.binary_fill_holes, tests/helpers/fill_reference.py) gives on the hand-made volumes the GPU tests use, the method of
csrc/fill_holes.hip restated in Python against it, the key's parser, its place in the options record and the HBM check, and its
refusal under torch.distributed."""
import importlib.util
import os

import numpy as np
import pytest

from delivr_cfos_amd.hostlogic import (HOLE_KEYS, CountOptions, cell_holes_csv_text, check_hbm_budget, count_options, fill_holes_enabled,
                                       measuring_plan)


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("fill_reference")


def _tunnel():
    m = ref.three_hollow_balls()
    m[10, 11, 19:21] = False  # along x through the first ball's wall
    return m


def _face_leak():
    m = ref.cube_shell()
    m[4, 4, 7] = False
    return m


def _cup_x0():
    m = np.zeros((9, 9, 9), dtype=bool)
    m[1:7, 1:8, 0:8] = True
    m[2:6, 2:7, 0:7] = False
    return m


CASES = {  # name: (volume, voxels filled, holes, components before, components after)
    "three hollow balls": (ref.three_hollow_balls, 3269, 3, 3, 3),
    "a tunnel through one wall": (_tunnel, 2344, 2, 3, 3),
    "a leak through a face": (_face_leak, 0, 0, 1, 1),
    "a tunnel that turns over an edge": (lambda: ref.cube_shell(1), 126, 1, 1, 1),
    "the same tunnel, face-connected": (lambda: ref.cube_shell(2), 0, 0, 1, 1),
    "a cup open to z = 0": (lambda: ref.cup(0), 0, 0, 1, 1),
    "a cup open to x = 0": (_cup_x0, 0, 0, 1, 1),
    "a shell inside a shell": (ref.nested, 2679, 2, 3, 2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_reference_on_the_hand_made_volumes(name):
    make, voxels, holes, n_before, n_after = CASES[name]
    mask = make()
    filled, got_voxels, got_holes = ref.fill_reference(mask)
    assert (got_voxels, got_holes) == (voxels, holes)
    assert (filled | mask).sum() == filled.sum() == mask.sum() + voxels  # nothing but background is written
    assert ref.label26(mask)[1] == n_before and ref.label26(filled)[1] == n_after
    out = ref.expected_bytes(mask.astype(np.uint8) * 255, 2)
    assert ((out == 2) == (filled & ~mask)).all() and ((out == 255) == mask).all()


def test_the_cup_of_the_issue_open_to_z0_is_the_helpers():
    m = np.zeros((9, 9, 9), dtype=bool)
    m[0:7, 1:8, 1:8] = True
    m[0:6, 2:7, 2:7] = False
    np.testing.assert_array_equal(m, ref.cup(0))


def test_a_swallowed_cell_and_the_order_of_the_survivors():
    mask = ref.nested()
    before, _ = ref.label26(mask)
    after, n = ref.label26(ref.fill_reference(mask)[0])
    assert n == 2 and before[12, 12, 32] == 3 and after[12, 12, 32] == 2  # the far ball moves up
    assert before[12, 12, 14 - 5] == 2 and after[12, 12, 14 - 5] == 1  # the inner shell is part of the outer one now
    # a hole never holds the first voxel of the component around it: the survivors keep their order
    firsts = [np.flatnonzero(before.ravel() == l)[0] for l in (1, 3)]
    assert [int(after.ravel()[i]) for i in firsts] == [1, 2]


@pytest.mark.parametrize("face", range(6))
def test_a_cup_against_every_face_is_open(face):
    assert ref.fill_reference(ref.cup(face))[1:] == (0, 0)


GAP_CASES = {
    **{name: case[0] for name, case in CASES.items()},
    "dense 0.7": lambda: ref.dense_random((17, 21, 37), 0.7, 3),
    "dense 0.8": lambda: ref.dense_random((17, 21, 37), 0.8, 4),
    "random hollow balls": ref.random_hollow_balls,
    "checkerboard": ref.checkerboard,
    "checkerboard of columns": lambda: ref.checkerboard(planes=False),
    "boxed checkerboard": ref.boxed_checkerboard,
    "empty": lambda: np.zeros((3, 4, 5), dtype=bool),
    "full": lambda: np.ones((3, 4, 5), dtype=bool),
}


@pytest.mark.parametrize("name", list(GAP_CASES))
def test_the_method_of_the_kernels_gives_what_scipy_gives(name):
    mask = GAP_CASES[name]()
    filled, voxels, holes = ref.fill_reference(mask)
    got, got_voxels, got_holes, _ = ref.fill_by_gaps(mask)
    np.testing.assert_array_equal(got, filled)
    assert (got_voxels, got_holes) == (voxels, holes)


def test_the_numbers_of_the_random_volumes():
    assert ref.fill_reference(ref.dense_random((17, 21, 37), 0.7, 3))[1] == 1300
    assert ref.fill_reference(ref.dense_random((17, 21, 37), 0.8, 4))[1] == 1645
    assert ref.fill_reference(ref.checkerboard(planes=False))[1:] == (0, 0)
    mask = ref.checkerboard()
    assert ref.fill_reference(mask)[1:] == (14 * 14 * 62 // 2,) * 2  # every inner background voxel is a hole of its own
    assert ref.fill_by_gaps(mask)[3] == 16 * 16 * 31  # X / 2 runs per row, one gap fewer
    boxed = ref.boxed_checkerboard()
    assert ref.fill_reference(boxed)[0].all()


# ---- the key ------------------------------------------------------------------------------------------------------------------
def test_the_parser():
    assert fill_holes_enabled(None) is False and fill_holes_enabled({}) is False and fill_holes_enabled({"mi355x": None}) is False
    assert fill_holes_enabled({"mi355x": {"fill_holes": False}}) is False
    assert fill_holes_enabled({"mi355x": {"fill_holes": True}}) is True
    for bad in (1, 0, "true", 2.0, [True]):
        with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['fill_holes'\] = .*: expected true or false"):
            fill_holes_enabled({"mi355x": {"fill_holes": bad}})


def test_the_options_record():
    assert CountOptions().fill_holes is False
    assert list(CountOptions.__dataclass_fields__)[-1] == "fill_holes"  # the last field: records built positionally stay valid
    assert count_options({}, -1, -1) == CountOptions()
    assert count_options({"mi355x": {"fill_holes": True}}, -1, -1) == CountOptions(fill_holes=True)
    assert count_options({"mi355x": {"fill_holes": True, "split_fused": 2}}, -1, -1) == CountOptions(split=(2, 1), fill_holes=True)
    with pytest.raises(ValueError, match="fill_holes"):
        count_options({"mi355x": {"fill_holes": "yes"}}, -1, -1)
    assert measuring_plan(CountOptions(fill_holes=True), None) == frozenset()  # nothing is measured for it after the labelling


V = 8 * 8 * 8


def test_the_hbm_check_refuses_the_streamed_path():
    opts = CountOptions(fill_holes=True)
    check_hbm_budget(opts, frozenset(), False, 7, V, 7 * V)  # the mask and its labels fit: so does the fill
    with pytest.raises(MemoryError, match=r"settings\['mi355x'\]\['fill_holes'\] needs the mask and its labels and the gap table in HBM.*"
                                          r"slab-streamed labelling does not fill holes.*hbm_budget_gb.*switch fill_holes off"):
        check_hbm_budget(opts, frozenset(), False, 7, V, 7 * V - 1)
    check_hbm_budget(CountOptions(), frozenset(), False, 7, V, 1)  # without the key a mask above the budget is streamed
    check_hbm_budget(opts, frozenset(), True, 4, V, 1)  # a cached labelling is not filled: nothing to refuse


def test_the_table():
    stats = {"voxel_counts": np.array([90, 7, 30], dtype=np.uint32), "hole_voxels": np.array([0, 0, 12], dtype=np.uint32)}
    assert cell_holes_csv_text(stats, 2) == "Blob,Size,HoleVoxels\n1,7,0\n2,30,12\n"
    assert cell_holes_csv_text(stats, 0) == "Blob,Size,HoleVoxels\n"
    with pytest.raises(ValueError):
        cell_holes_csv_text(stats, 3)
    assert HOLE_KEYS == ("hole_voxels", "holes_filled")


def test_the_key_is_refused_under_torch_distributed_before_any_file_is_touched(tmp_path, monkeypatch):
    import torch.distributed as dist

    from delivr_cfos_amd.count_blobs import count_blobs

    for name, value in (("is_available", True), ("is_initialized", True), ("get_world_size", 2), ("get_rank", 1)):
        monkeypatch.setattr(dist, name, lambda *a, value=value, **k: value)
    post = tmp_path / "post"
    settings = {"postprocessing": {"output_location": str(post) + "/"}, "mi355x": {"fill_holes": True}}
    with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['fill_holes'\] is not available under torch.distributed \(2 ranks\)"):
        count_blobs(settings, str(tmp_path / "in"), 0, "brain", (1, 1, 4, 4, 4))  # (no engine, no input folder: refused before)
    assert not post.exists()


def test_a_hollow_cell_splits_and_the_filled_one_does_not():
    """the volume of the GPU test of split_fused with the key: on the host, with the split's own reference"""
    split = _helper("split_reference")
    mask = ref.ball((15, 15, 15), (7, 7, 7), 6) & ~ref.ball((15, 15, 15), (7, 8, 8), 3)
    filled, voxels, holes = ref.fill_reference(mask)
    assert (voxels, holes) == (123, 1)
    hollow = split.split_reference(*split.label26(mask), 2)
    whole = split.split_reference(*split.label26(filled), 2)
    assert (hollow["K"], hollow["n_split"]) == (3, 1) and (whole["K"], whole["n_split"]) == (1, 0)
