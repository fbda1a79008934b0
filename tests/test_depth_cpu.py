"""Per-cell depth (settings["mi355x"]["depth_stats"]): the host side - the scipy reference the GPU tests compare with, pinned on
hand-made cases; the parser, finish_depth, the table, the options record, the measuring plan, the HBM check and the refusal under
torch.distributed.  No GPU."""
import importlib.util
import os
import threading

import numpy as np
import pytest

from delivr_cfos_amd.hostlogic import (DEPTH_KEYS, DEPTH_NO_PEAK, DEPTH_RAW_KEYS, CountOptions, cell_depth_csv_text, check_hbm_budget,
                                       count_options, depth_stats_settings, finish_depth, measuring_plan)


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("depth_reference")


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_a_cube_in_the_open():
    lab = np.zeros((7, 7, 7), dtype=np.uint32)
    lab[2:5, 2:5, 2:5] = 1
    d2, rows = ref.depth_reference(lab, 1)
    assert d2.dtype == np.uint32 and d2[3, 3, 3] == 4
    for face in ((2, 3, 3), (4, 3, 3), (3, 2, 3), (3, 4, 3), (3, 3, 2), (3, 3, 4)):
        assert d2[face] == 1
    assert (d2[lab == 1] >= 1).all() and not d2[lab == 0].any() and int(d2.sum()) == 26 + 4
    assert rows["depth_max_sq"].tolist() == [0, 4] and rows["depth_sum_sq"].tolist() == [0, 30]
    assert rows["depth_peak_index"].tolist() == [ref.NO_PEAK, (3 * 7 + 3) * 7 + 3]
    assert [v.dtype for v in rows.values()] == [np.uint32, np.uint64, np.uint64] and list(rows) == list(DEPTH_RAW_KEYS)


def test_the_same_cube_in_a_corner_of_the_volume():
    lab = np.zeros((5, 6, 7), dtype=np.uint32)
    lab[:3, :3, :3] = 1  # the outside of the volume is background: the same depths as in the open
    d2, rows = ref.depth_reference(lab, 1)
    assert d2[1, 1, 1] == 4 and int(d2.sum()) == 30 and (d2[:3, :3, :3][np.arange(3) != 1] == 1).all()
    assert rows["depth_peak_index"][1] == (1 * 6 + 1) * 7 + 1
    full = np.ones((3, 3, 3), dtype=np.uint32)  # ... and with every face a face of the volume
    np.testing.assert_array_equal(ref.depth_map(full, 1), d2[:3, :3, :3])


def test_a_cube_of_two_voxels_a_side_peaks_at_its_first_voxel():
    lab = np.zeros((4, 5, 6), dtype=np.uint32)
    lab[1:3, 2:4, 3:5] = 1
    d2, rows = ref.depth_reference(lab, 1)
    assert (d2[lab == 1] == 1).all() and rows["depth_max_sq"][1] == 1 and rows["depth_sum_sq"][1] == 8
    assert rows["depth_peak_index"][1] == (1 * 5 + 2) * 6 + 3


def test_two_cubes_of_different_labels_sharing_a_face():
    lab = np.zeros((5, 5, 8), dtype=np.uint32)
    lab[1:4, 1:4, 1:4] = 1
    lab[1:4, 1:4, 4:7] = 2  # face to face at x = 3 | 4: each bounds the other as the background would
    d2, rows = ref.depth_reference(lab, 2)
    assert d2[2, 2, 2] == 4 and d2[2, 2, 5] == 4 and d2[2, 2, 3] == 1 and d2[2, 2, 4] == 1
    assert rows["depth_max_sq"].tolist() == [0, 4, 4] and rows["depth_sum_sq"].tolist() == [0, 30, 30]
    merged = np.where(lab > 0, 1, 0).astype(np.uint32)  # one label: the middle is deeper
    assert ref.depth_map(merged, 1)[2, 2, 3] == 4
    d2_1, rows_1 = ref.depth_reference(lab, 1)  # label 2 is above n: not measured, and still another label
    assert not d2_1[lab == 2].any() and rows_1["depth_sum_sq"].tolist() == [0, 30]
    np.testing.assert_array_equal(d2_1[lab == 1], d2[lab == 1])


def test_spacing():
    lab = np.zeros((9, 9, 9), dtype=np.uint32)
    lab[2:7, 2:7, 2:7] = 1
    d2 = ref.depth_map(lab, 1, (3, 1, 1))
    assert d2[4, 4, 4] == 9 and d2[2, 4, 4] == 9 and d2[3, 4, 4] == 9 and d2[4, 2, 4] == 1 and d2[3, 3, 3] == 4
    assert ref.depth_map(lab, 1, (1, 1, 1))[4, 4, 4] == 9 and ref.depth_map(lab, 1, (37, 10, 10))[4, 4, 4] == 900
    d2 = ref.depth_map(lab, 1, (2, 1, 3))  # z: 2 voxels of 2, y: 3 voxels of 1, x: 3 voxels of 3
    assert d2[3, 4, 4] == 9 and d2[3, 3, 4] == 4 and d2[2, 4, 4] == 4 and d2[4, 4, 2] == 9


@pytest.mark.parametrize("spacing", [(1, 1, 1), (3, 1, 1), (37, 10, 10), (2, 1, 3)])
def test_the_separable_passes_agree_with_scipy_voxel_for_voxel(spacing):
    rng = np.random.default_rng(sum(spacing))
    lab = rng.integers(1, 4, size=(6, 9, 11), dtype=np.uint32)
    lab = np.repeat(np.repeat(lab, 2, axis=1), 2, axis=2)[:, :13, :19]
    lab[rng.random(lab.shape) < 0.3] = 0
    d2, rows = ref.depth_reference(lab, 2)  # label 3 is above n
    np.testing.assert_array_equal(ref.scan_reference(lab, 2, spacing=(1, 1, 1)), d2)
    np.testing.assert_array_equal(ref.scan_reference(lab, 2, spacing), ref.depth_map(lab, 2, spacing))
    assert rows["depth_max_sq"][1:].min() >= 1 and (rows["depth_peak_index"][1:] < lab.size).all()


def test_the_rows_pick_the_first_voxel_in_raster_order_on_a_tie():
    lab = np.zeros((3, 5, 9), dtype=np.uint32)
    lab[0:3, 1:4, 1:8] = 1  # 3 x 3 x 7, cut by the z faces of the volume too: five voxels of depth 4 along x
    d2, rows = ref.depth_reference(lab, 3)
    assert rows["depth_max_sq"].tolist() == [0, 4, 0, 0] and (d2 == 4).sum() == 5
    assert rows["depth_peak_index"].tolist() == [ref.NO_PEAK, (1 * 5 + 2) * 9 + 2, ref.NO_PEAK, ref.NO_PEAK]
    assert ref.NO_PEAK == DEPTH_NO_PEAK


# ---- the key ------------------------------------------------------------------------------------------------------------------
def test_the_parser():
    for off in (None, {}, {"mi355x": None}, {"mi355x": {}}, {"mi355x": {"depth_stats": False}}, {"mi355x": {"depth_stats": None}}):
        assert depth_stats_settings(off) is None
    assert depth_stats_settings({"mi355x": {"depth_stats": True}}) == (1, 1, 1)
    assert depth_stats_settings({"mi355x": {"depth_stats": True, "depth_spacing": [37, 10, 10]}}) == (37, 10, 10)
    assert depth_stats_settings({"mi355x": {"depth_stats": True, "depth_spacing": (1, 64, np.int64(2))}}) == (1, 64, 2)
    assert all(type(w) is int for w in depth_stats_settings({"mi355x": {"depth_stats": True, "depth_spacing": (1, 64, np.int64(2))}}))
    for bad in (1, 0, "true", 2.0, [True]):
        with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['depth_stats'\] = .*: expected true or false"):
            depth_stats_settings({"mi355x": {"depth_stats": bad}})
    for bad in (3, [1, 1], [1, 1, 1, 1], [0, 1, 1], [1, 65, 1], [1, 1, -1], [1.0, 1, 1], [True, 1, 1], ["1", 1, 1], "111", [[1, 1, 1]], [None, 1, 1]):
        with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['depth_spacing'\] = .*three integers 1\.\.64"):
            depth_stats_settings({"mi355x": {"depth_stats": True, "depth_spacing": bad}})
    for off in ({}, {"depth_stats": False}):
        with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['depth_spacing'\] = \[2, 1, 1\] needs settings\['mi355x'\]\['depth_stats'\]"):
            depth_stats_settings({"mi355x": {**off, "depth_spacing": [2, 1, 1]}})
    with pytest.raises(ValueError, match="three integers"):  # (a bad spacing is named even without the switch)
        depth_stats_settings({"mi355x": {"depth_spacing": [0, 1, 1]}})


def test_the_options_record():
    assert CountOptions().depth is None
    assert count_options({}, -1, -1) == CountOptions()
    assert count_options({"mi355x": {"depth_stats": True}}, -1, -1) == CountOptions(depth=(1, 1, 1))
    assert count_options({"mi355x": {"depth_stats": True, "depth_spacing": [3, 1, 1], "shape_stats": True}}, -1, -1) == \
        CountOptions(shape=True, depth=(3, 1, 1))
    with pytest.raises(ValueError, match="depth_stats"):
        count_options({"mi355x": {"depth_stats": "yes"}}, -1, -1)
    with pytest.raises(ValueError, match="depth_spacing"):
        count_options({"mi355x": {"depth_spacing": [1, 1, 1]}}, -1, -1)


# ---- finish_depth and the table -----------------------------------------------------------------------------------------------
def _raw_of(lab, n, spacing=(1, 1, 1)):
    d2, rows = ref.depth_reference(lab, n, spacing)
    return rows, np.bincount(lab.ravel(), minlength=n + 1).astype(np.uint32)


def test_finish_depth():
    lab = np.zeros((5, 6, 9), dtype=np.uint32)
    lab[1:4, 1:4, 1:4] = 1
    lab[0, 5, 8] = 3  # label 2 has no voxel
    lab[1:3, 1:3, 5:8] = 4
    raw, counts = _raw_of(lab, 4, (3, 1, 1))  # (wz = 3: every plane of the cube is 4 in its middle and 1 around it, the first wins)
    out = finish_depth(raw, counts, lab.shape, (3, 1, 1))
    assert tuple(out) == DEPTH_KEYS
    assert out["depth_max_sq"].tolist() == [0, 4, 0, 1, 1] and out["depth_max_sq"].dtype == np.uint32
    assert out["depth_sum_sq"].tolist() == [0, 3 * (4 + 8 * 1), 0, 1, 12] and out["depth_sum_sq"].dtype == np.uint64
    assert out["depth_peak_index"].dtype == np.uint64 and out["depth_peak_index"][[0, 2]].tolist() == [0, 0]
    assert out["depth_radius"].dtype == np.float64 and out["depth_radius"].tolist() == [0.0, 2.0, 0.0, 1.0, 1.0]
    assert out["depth_mean_sq"].tolist() == [0.0, 36 / 27, 0.0, 1.0, 1.0]
    assert out["depth_peak"].dtype == np.int64 and out["depth_peak"].tolist() == [[0, 0, 0], [1, 2, 2], [0, 0, 0], [0, 5, 8], [1, 1, 5]]
    assert out["depth_spacing"] == (3, 1, 1)
    assert raw["depth_peak_index"][0] == DEPTH_NO_PEAK  # (the input is not written)
    # one rounding: the root of an integer that is no square
    raw2 = {"depth_max_sq": np.array([0, 2], np.uint32), "depth_sum_sq": np.array([0, 7], np.uint64), "depth_peak_index": np.array([DEPTH_NO_PEAK, 5], np.uint64)}
    out2 = finish_depth(raw2, np.array([0, 3]), (1, 2, 3), (1, 1, 1))
    assert out2["depth_radius"][1] == np.sqrt(2.0) and out2["depth_mean_sq"][1] == 7 / 3 and out2["depth_peak"][1].tolist() == [0, 1, 2]
    # labels and statistics that do not belong together
    with pytest.raises(RuntimeError, match="disagree on 1 label.*first label 2"):
        finish_depth(raw, np.array([0, 27, 5, 1, 6]), lab.shape, (3, 1, 1))  # voxels but no peak
    with pytest.raises(RuntimeError, match="disagree on 1 label.*first label 3"):
        finish_depth(raw, np.array([0, 27, 0, 0, 6]), lab.shape, (3, 1, 1))  # a peak without voxels
    with pytest.raises(RuntimeError, match="rows"):
        finish_depth(raw, counts[:-1], lab.shape, (3, 1, 1))
    with pytest.raises(RuntimeError, match="outside the volume"):
        finish_depth(raw, counts, (2, 6, 6), (3, 1, 1))  # (72 voxels: the peak of label 1 is voxel 74)
    empty = {"depth_max_sq": np.zeros(1, np.uint32), "depth_sum_sq": np.zeros(1, np.uint64), "depth_peak_index": np.full(1, DEPTH_NO_PEAK, np.uint64)}
    out0 = finish_depth(empty, np.zeros(1, np.uint32), (2, 2, 2), (1, 1, 1))
    assert out0["depth_peak"].shape == (1, 3) and not out0["depth_peak"].any() and out0["depth_radius"].tolist() == [0.0]


def test_the_table():
    lab = np.zeros((5, 6, 9), dtype=np.uint32)
    lab[1:4, 1:4, 1:4] = 1
    lab[1:3, 1:3, 5:8] = 3
    raw, counts = _raw_of(lab, 3)
    stats = {"voxel_counts": counts, **finish_depth(raw, counts, lab.shape, (1, 1, 1))}
    text = cell_depth_csv_text(stats, 3)
    assert text == ("Blob,Size,Radius,MeanSqDepth,PeakZ,PeakY,PeakX\n"
                    f"1,27,2.0,{30 / 27!r},2,2,2\n"
                    "2,0,0.0,0.0,0,0,0\n"
                    "3,12,1.0,1.0,1,1,5\n")
    assert cell_depth_csv_text(stats, 0) == "Blob,Size,Radius,MeanSqDepth,PeakZ,PeakY,PeakX\n"
    with pytest.raises(ValueError, match="shorter"):
        cell_depth_csv_text(stats, 4)


# ---- the plan and the budget ---------------------------------------------------------------------------------------------------
def test_the_measuring_plan():
    opts = CountOptions(depth=(3, 1, 1))
    assert measuring_plan(CountOptions(), None) == frozenset() and measuring_plan(opts, None) == {"depth"}
    std = {"voxel_counts": 0, "bounding_boxes": 0, "centroids": 0}
    same = {**std, **{k: 0 for k in DEPTH_KEYS}, "depth_spacing": (3, 1, 1)}
    assert measuring_plan(opts, same) == frozenset()
    assert measuring_plan(opts, {**same, "depth_spacing": [3, 1, 1]}) == frozenset()  # (a list in an older pickle is the same spacing)
    assert measuring_plan(opts, {**same, "depth_spacing": (1, 1, 1)}) == {"depth"}  # another spacing: other depths
    assert measuring_plan(opts, {**same, "depth_spacing": None}) == {"depth"}
    assert measuring_plan(opts, std) == {"depth"}
    for k in DEPTH_KEYS:
        assert measuring_plan(opts, {q: v for q, v in same.items() if q != k}) == {"depth"}, k
    assert measuring_plan(CountOptions(), same) == frozenset()  # not asked for: whatever the pickle holds
    # beside the shell's radius, the other recorded setting
    both = CountOptions(intensity=True, shell_radius=2, depth=(3, 1, 1))
    assert measuring_plan(both, same) == {"cells", "shell"}
    assert measuring_plan(CountOptions(shape=True, depth=(1, 1, 1)), same) == {"shape", "depth"}


def test_the_hbm_budget():
    opts = CountOptions(depth=(1, 1, 1))
    vox = 1000
    plan = measuring_plan(opts, None)
    check_hbm_budget(opts, plan, True, 4, vox, vox * 12)  # cached labels and the two scratch volumes fit
    with pytest.raises(MemoryError, match=r"settings\['mi355x'\]\['depth_stats'\] needs 8 more bytes per voxel in HBM beside the cached labels"):
        check_hbm_budget(opts, plan, True, 4, vox, vox * 12 - 1)  # holds the labels, not 8 more bytes per voxel
    check_hbm_budget(opts, frozenset(), True, 4, vox, vox * 4)  # nothing left to measure: nothing is needed
    check_hbm_budget(opts, plan, False, 9, vox, vox * 17)
    with pytest.raises(MemoryError, match=r"depth_stats.*8 more bytes per voxel in HBM beside the mask and its labels.*"
                                          r"slab-streamed labelling does not measure.*switch depth_stats off"):
        check_hbm_budget(opts, plan, False, 9, vox, vox * 17 - 1)
    check_hbm_budget(CountOptions(), frozenset(), False, 9, vox, 1)  # without the key nothing is asked


# ---- torch.distributed ---------------------------------------------------------------------------------------------------------
def test_count_blobs_under_torch_distributed_refuses_the_key_before_opening_any_file(tmp_path, monkeypatch):
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs

    ranks = _helper("thread_ranks")
    fake = ranks.ThreadRanks(2)
    fake.patch(monkeypatch, dist)
    path_in, post = str(tmp_path / "in"), str(tmp_path / "post")  # (neither exists: nothing may be opened or created)
    settings = {"postprocessing": {"output_location": post + "/"}, "blob_detection": {"input_location": path_in},
                "mi355x": {"depth_stats": True, "depth_spacing": [3, 1, 1]}}
    caught = [None] * 2

    def rank_main(rank):
        fake.bind(rank)
        try:
            count_blobs(settings, path_in, 0, "brain", (1, 1, 8, 8, 8), engine=object())  # (refused before the engine is used)
        except BaseException as exc:  # noqa: BLE001
            caught[rank] = exc

    ts = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not any(t.is_alive() for t in ts)  # nobody waits in a collective
    assert all(type(c) is ValueError for c in caught), caught
    assert len({str(c) for c in caught}) == 1
    assert "settings['mi355x']['depth_stats'] is not available under torch.distributed (2 ranks)" in str(caught[0])
    assert "nearest outside voxel on another rank" in str(caught[0])
    assert not os.path.exists(post) and not os.path.exists(path_in)
    assert count_blobs.last_depth is None
