"""Cell neighbourhoods without a GPU (settings["mi355x"]["neighbour_stats"] in count_blobs): the numpy reference of the device's
neighbour table (tests/helpers/neighbour_reference.py) against an all-voxel-pairs brute force on hand-made volumes, the parser, the
options record, the measuring plan, the HBM check, the per-cell rows of hostlogic.neighbour_summary on a hand-made graph, the two
tables, and the refusal under torch.distributed.  Integers throughout: equality, no tolerance."""
import importlib.util
import os
import threading

import numpy as np
import pytest

from delivr_cfos_amd.hostlogic import (NEIGHBOUR_KEYS, NEIGHBOUR_MAX_REACH, CountOptions, cell_neighbours_csv_text, cell_pairs_csv_text,
                                       check_hbm_budget, count_options, finish_neighbours, measuring_plan, neighbour_reach,
                                       neighbour_stats_settings, neighbour_summary)


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("neighbour_reference")


def _mi(**keys):
    return {"mi355x": keys}


# ---- the reference helper against the definition -------------------------------------------------------------------------------
def _hand_made():
    """touching cells, a cell in a corner of the volume, a label above n between two cells, a lone voxel far from anything"""
    lab = np.zeros((6, 9, 14), dtype=np.uint32)
    lab[0:2, 0:2, 0:3] = 1  # in the first corner
    lab[0:2, 2:4, 0:3] = 2  # touches 1 over a y face
    lab[2, 4, 3] = 3  # touches 2 over a corner only
    lab[4:6, 6:9, 10:14] = 4  # in the last corner
    lab[3, 5, 6:9] = 9  # above n = 5: ignored, blocks nothing
    lab[2, 4, 9] = 5
    return lab, 5


@pytest.mark.parametrize("spacing", [(1, 1, 1), (3, 1, 1), (1, 2, 5)])
def test_the_reference_against_all_voxel_pairs(spacing):
    lab, n = _hand_made()
    assert int((lab > 0).sum()) < 300
    seen = set()
    for radius_sq in (1, 2, 3, 4, 9, 27, 36, 64):
        if max(ref.reach(radius_sq, spacing)) > NEIGHBOUR_MAX_REACH:
            continue
        want = ref.brute_force_table(lab, n, spacing, radius_sq)
        assert ref.neighbour_table(lab, n, spacing, radius_sq) == want, radius_sq
        assert all(a < b <= n and 1 <= g <= radius_sq for (a, b), g in want.items())
        seen |= set(want)
    assert {(1, 2), (2, 3)} <= seen and not any(9 in k for k in seen)
    assert ((3, 5) in seen) == (spacing[2] == 1)  # six voxels apart along x
    if spacing == (1, 1, 1):
        table = ref.neighbour_table(lab, n, spacing, 64)
        assert table[(1, 2)] == 1 and table[(2, 3)] == 3  # a face, a corner
        assert table[(3, 5)] == 36  # straight through the label above n
        assert (4, 5) in table and (1, 4) not in table
        assert ref.neighbour_table(lab, 9, spacing, 64)[(5, 9)] == 3  # with n = 9 that label takes part


def test_the_reference_on_random_volumes_and_its_arrays():
    rng = np.random.default_rng(5)
    for shape, spacing, radius_sq in (((4, 5, 9), (1, 1, 1), 9), ((1, 6, 7), (37, 10, 10), 1600), ((5, 1, 3), (1, 2, 64), 4100), ((3, 7, 5), (3, 1, 1), 10)):
        lab = ((rng.random(shape) < 0.4) * rng.integers(1, 8, shape)).astype(np.uint32)
        want = ref.brute_force_table(lab, 6, spacing, radius_sq)
        assert want and ref.neighbour_table(lab, 6, spacing, radius_sq) == want
    pairs, gaps = ref.as_arrays({(2, 3): 4, (1, 9): 1, (1, 3): 7})
    assert pairs.dtype == np.uint32 and pairs.tolist() == [[1, 3], [1, 9], [2, 3]] and gaps.tolist() == [7, 1, 4]
    empty = ref.as_arrays({})
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,)
    assert ref.neighbour_table(np.zeros((2, 2, 2), np.uint32), 3, (1, 1, 1), 4) == {}


# ---- the parser ----------------------------------------------------------------------------------------------------------------------
def test_the_parser_good_values():
    for off in ({}, None, _mi(), _mi(neighbour_stats=None), _mi(neighbour_stats=False), _mi(neighbour_stats=0), _mi(neighbour_stats=0.0)):
        assert neighbour_stats_settings(off) is None
    assert neighbour_stats_settings(_mi(neighbour_stats=8)) == (64, (1, 1, 1))
    assert neighbour_stats_settings(_mi(neighbour_stats=1)) == (1, (1, 1, 1))
    assert neighbour_stats_settings(_mi(neighbour_stats=2.5)) == (6, (1, 1, 1))  # floor(6.25)
    assert neighbour_stats_settings(_mi(neighbour_stats=np.float32(1.5))) == (2, (1, 1, 1))
    assert neighbour_stats_settings(_mi(neighbour_stats=8.99)) == (80, (1, 1, 1))  # isqrt(80) = 8: still a reach of 8
    assert neighbour_stats_settings(_mi(neighbour_stats=80, depth_spacing=[37, 10, 10])) == (6400, (37, 10, 10))  # reaches 2, 8, 8
    assert neighbour_stats_settings(_mi(neighbour_stats=5, depth_spacing=(1, 2, 64))) == (25, (1, 2, 64))  # a reach of 0 along x
    got = neighbour_stats_settings(_mi(neighbour_stats=3, depth_spacing=[3, 1, 1]))
    assert got == (9, (3, 1, 1)) and type(got[0]) is int and type(got[1]) is tuple
    assert neighbour_reach(64, (1, 2, 9), "x") == (8, 4, 0) and neighbour_reach(6400, (37, 10, 10), "x") == (2, 8, 8)


def test_the_parser_bad_values_name_the_key():
    for bad in (True, "8", -1, -0.5, float("nan"), float("inf"), [8], (1, 1, 1)):
        with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['neighbour_stats'\]"):
            neighbour_stats_settings(_mi(neighbour_stats=bad))
    with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['neighbour_stats'\] = 0.5.*below one spacing unit"):
        neighbour_stats_settings(_mi(neighbour_stats=0.5))
    for bad in ([1, 1], [0, 1, 1], [1, 1, 65], [1.0, 1, 1], 3):
        with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['depth_spacing'\]"):
            neighbour_stats_settings(_mi(neighbour_stats=4, depth_spacing=bad))


def test_the_reach_limit_names_the_axis_the_reach_and_the_limit():
    assert NEIGHBOUR_MAX_REACH == 8
    with pytest.raises(ValueError, match=r"settings\['mi355x'\]\['neighbour_stats'\] = 9.*reaches 9 voxels along z.*at most 8"):
        neighbour_stats_settings(_mi(neighbour_stats=9))
    with pytest.raises(ValueError, match=r"neighbour_stats.*spacing of 10 reaches 9 voxels along y.*at most 8"):
        neighbour_stats_settings(_mi(neighbour_stats=90, depth_spacing=[37, 10, 10]))
    with pytest.raises(ValueError, match=r"spacing of 1 reaches 16 voxels along x.*at most 8"):
        neighbour_stats_settings(_mi(neighbour_stats=16, depth_spacing=[2, 2, 1]))
    assert neighbour_stats_settings(_mi(neighbour_stats=16, depth_spacing=[2, 2, 2])) == (256, (2, 2, 2))


def test_the_options_record():
    import dataclasses

    assert count_options({}, None, None) == CountOptions()
    assert CountOptions().neighbours is None
    names = [f.name for f in dataclasses.fields(CountOptions)]
    assert names[names.index("depth") + 1] == "neighbours"  # after depth
    assert names[:6] == ["bounds", "intensity", "shell_radius", "quartiles", "shape", "split"] and names[-2:] == ["split_depth", "fill_holes"]
    opts = count_options(_mi(neighbour_stats=4, depth_spacing=[2, 1, 1]), None, None)
    assert opts == CountOptions(neighbours=(16, (2, 1, 1)))  # (depth_spacing alone is the spacing of the table: depth stays off)
    both = count_options(_mi(neighbour_stats=4, depth_spacing=[2, 1, 1], depth_stats=True), None, None)
    assert both.depth == (2, 1, 1) and both.neighbours == (16, (2, 1, 1))
    assert count_options(_mi(neighbour_stats=0), None, None) == CountOptions()
    # depth_spacing without anything that measures with it is still refused, also with the key switched off
    for off in ({}, {"neighbour_stats": 0}, {"neighbour_stats": False}):
        with pytest.raises(ValueError, match="depth_spacing"):
            count_options(_mi(depth_spacing=[2, 1, 1], **off), None, None)
    # the parser runs beside depth's: a bad depth_stats is reported first
    with pytest.raises(ValueError, match="depth_stats"):
        count_options(_mi(depth_stats=3, neighbour_stats="x"), None, None)
    with pytest.raises(ValueError, match="neighbour_stats"):
        count_options(_mi(depth_stats=True, neighbour_stats="x"), None, None)


# ---- the plan and the budget ---------------------------------------------------------------------------------------------------
def test_the_measuring_plan():
    opts = CountOptions(neighbours=(64, (3, 1, 1)))
    assert measuring_plan(CountOptions(), None) == frozenset() and measuring_plan(opts, None) == {"neighbours"}
    std = {"voxel_counts": 0, "bounding_boxes": 0, "centroids": 0}
    same = {**std, **{k: 0 for k in NEIGHBOUR_KEYS}, "neighbour_radius_sq": 64, "neighbour_spacing": (3, 1, 1)}
    assert measuring_plan(opts, same) == frozenset()  # complete
    assert measuring_plan(opts, {**same, "neighbour_spacing": [3, 1, 1]}) == frozenset()
    assert measuring_plan(opts, {**same, "neighbour_radius_sq": 63}) == {"neighbours"}  # another radius
    assert measuring_plan(opts, {**same, "neighbour_spacing": (1, 1, 1)}) == {"neighbours"}  # another spacing
    assert measuring_plan(opts, std) == {"neighbours"}
    for k in NEIGHBOUR_KEYS:
        assert measuring_plan(opts, {q: v for q, v in same.items() if q != k}) == {"neighbours"}, k
    assert measuring_plan(CountOptions(), same) == frozenset()  # not asked for: whatever the pickle holds
    # its own keys, not depth_spacing: the two groups do not entangle
    both = CountOptions(depth=(3, 1, 1), neighbours=(64, (3, 1, 1)))
    assert measuring_plan(both, same) == {"depth"}
    assert measuring_plan(both, {**same, "depth_spacing": (1, 1, 1)}) == {"depth"}
    assert measuring_plan(CountOptions(depth=(1, 1, 1), neighbours=(64, (3, 1, 1))), {**same, "depth_spacing": (1, 1, 1)}) == {"depth"}
    assert len(NEIGHBOUR_KEYS) == 9 and len(set(NEIGHBOUR_KEYS)) == 9


def test_the_hbm_budget():
    opts = CountOptions(neighbours=(64, (1, 1, 1)))
    vox = 1000
    plan = measuring_plan(opts, None)
    check_hbm_budget(opts, plan, True, 4, vox, vox * 4)  # cached: nothing beside the labels
    with pytest.raises(MemoryError, match=r"settings\['mi355x'\]\['neighbour_stats'\] needs the cached labels in HBM"):
        check_hbm_budget(opts, plan, True, 4, vox, vox * 4 - 1)
    check_hbm_budget(opts, frozenset(), True, 4, vox, 1)  # nothing left to measure: nothing is needed
    check_hbm_budget(opts, plan, False, 9, vox, vox * 9)  # fresh: nothing beside the mask and its labels
    with pytest.raises(MemoryError, match=r"neighbour_stats.*the mask and its labels in HBM.*slab-streamed labelling does not measure.*"
                                          r"switch neighbour_stats off"):
        check_hbm_budget(opts, plan, False, 9, vox, vox * 9 - 1)
    # depth_stats is judged first, in the order of the work
    with pytest.raises(MemoryError, match="depth_stats"):
        both = CountOptions(depth=(1, 1, 1), neighbours=(64, (1, 1, 1)))
        check_hbm_budget(both, measuring_plan(both, None), False, 9, vox, vox * 9)
    check_hbm_budget(CountOptions(), frozenset(), False, 9, vox, 1)


# ---- the per-cell rows ---------------------------------------------------------------------------------------------------------
def _graph():
    """9 cells: {2, 5, 7} and {3, 4, 8} are clusters, 1, 6 and 9 stand alone; cell 5 is as close to 2 as to 7; cell 4 is nearest to 8"""
    pairs = np.array([[2, 5], [3, 4], [3, 8], [4, 8], [5, 7]], dtype=np.uint32)
    gaps = np.array([9, 16, 2, 1, 9], dtype=np.uint32)
    return pairs, gaps


def test_neighbour_summary_on_a_hand_made_graph():
    pairs, gaps = _graph()
    got = neighbour_summary(pairs, gaps, 9)
    assert list(got) == ["neighbour_count", "nearest_gap_sq", "nearest_cell", "cluster_id", "cluster_size"]
    assert all(v.dtype == np.uint32 and v.shape == (10,) for v in got.values())
    assert got["neighbour_count"].tolist() == [0, 0, 1, 2, 2, 2, 0, 1, 2, 0]
    assert got["nearest_gap_sq"].tolist() == [0, 0, 9, 2, 1, 9, 0, 9, 1, 0]
    assert got["nearest_cell"].tolist() == [0, 0, 5, 8, 8, 2, 0, 5, 4, 0]  # cell 5: a tie of 2 and 7 goes to the smaller label
    # numbered in the order of the smallest member: {1}, {2, 5, 7}, {3, 4, 8}, {6}, {9}
    assert got["cluster_id"].tolist() == [0, 1, 2, 3, 3, 2, 4, 2, 3, 5]
    assert got["cluster_size"].tolist() == [0, 1, 3, 3, 3, 3, 1, 3, 3, 1]
    # the order of the rows does not matter
    flipped = neighbour_summary(pairs[::-1], gaps[::-1], 9)
    assert all((flipped[k] == got[k]).all() for k in got)
    # no pair at all; no cell at all
    none = neighbour_summary(np.zeros((0, 2), np.uint32), np.zeros(0, np.uint32), 3)
    assert none["cluster_id"].tolist() == [0, 1, 2, 3] and none["cluster_size"].tolist() == [0, 1, 1, 1] and not none["neighbour_count"].any()
    zero = neighbour_summary(np.zeros((0, 2), np.uint32), np.zeros(0, np.uint32), 0)
    assert all(v.tolist() == [0] for v in zero.values())
    for bad_pairs, bad_gaps in (([[2, 1]], [1]), ([[1, 1]], [1]), ([[0, 1]], [1]), ([[1, 10]], [1]), ([[1, 2]], [0]), ([[1, 2]], [1, 2])):
        with pytest.raises(ValueError, match="neighbour_summary"):
            neighbour_summary(np.array(bad_pairs), np.array(bad_gaps), 9)


def test_finish_neighbours():
    pairs, gaps = _graph()
    table = {"a": pairs[:, 0].copy(), "b": pairs[:, 1].copy(), "gap_sq": gaps, "segments": 11}
    out = finish_neighbours(table, 9, 16, [3, 1, 1])
    assert tuple(out) == NEIGHBOUR_KEYS
    assert out["neighbour_pairs"].dtype == np.uint32 and out["neighbour_pairs"].tolist() == pairs.tolist()
    assert out["neighbour_gap_sq"].dtype == np.uint32 and out["neighbour_gap_sq"].tolist() == gaps.tolist()
    assert out["neighbour_radius_sq"] == 16 and type(out["neighbour_radius_sq"]) is int
    assert out["neighbour_spacing"] == (3, 1, 1) and type(out["neighbour_spacing"]) is tuple
    assert out["cluster_id"].tolist() == neighbour_summary(pairs, gaps, 9)["cluster_id"].tolist()
    assert measuring_plan(CountOptions(neighbours=(16, (3, 1, 1))), out) == frozenset()
    assert finish_neighbours({"a": np.zeros(0, np.uint32), "b": np.zeros(0, np.uint32), "gap_sq": np.zeros(0, np.uint32)}, 2, 1,
                             (1, 1, 1))["neighbour_pairs"].shape == (0, 2)


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def test_the_two_tables():
    pairs, gaps = _graph()
    counts = np.array([0, 5, 7, 1, 30, 2, 3, 4, 9, 6], dtype=np.uint32)
    stats = {"voxel_counts": counts, **finish_neighbours({"a": pairs[:, 0], "b": pairs[:, 1], "gap_sq": gaps}, 9, 16, (1, 1, 1))}
    assert cell_neighbours_csv_text(stats, 9) == ("Blob,Size,Neighbours,NearestCell,NearestGapSq,NearestGap,Cluster,ClusterSize\n"
                                                  "1,5,0,0,0,0.0,1,1\n"
                                                  "2,7,1,5,9,3.0,2,3\n"
                                                  f"3,1,2,8,2,{float(np.sqrt(2.0))!r},3,3\n"
                                                  "4,30,2,8,1,1.0,3,3\n"
                                                  "5,2,2,2,9,3.0,2,3\n"
                                                  "6,3,0,0,0,0.0,4,1\n"
                                                  "7,4,1,5,9,3.0,2,3\n"
                                                  "8,9,2,4,1,1.0,3,3\n"
                                                  "9,6,0,0,0,0.0,5,1\n")
    assert f"{float(np.sqrt(2.0))!r}" == "1.4142135623730951"  # (a python float's repr, as depth_radius is written)
    assert cell_neighbours_csv_text(stats, 0) == "Blob,Size,Neighbours,NearestCell,NearestGapSq,NearestGap,Cluster,ClusterSize\n"
    with pytest.raises(ValueError, match="shorter"):
        cell_neighbours_csv_text(stats, 10)
    assert cell_pairs_csv_text(stats) == ("BlobA,BlobB,GapSq,Gap\n"
                                          "2,5,9,3.0\n"
                                          "3,4,16,4.0\n"
                                          "3,8,2,1.4142135623730951\n"
                                          "4,8,1,1.0\n"
                                          "5,7,9,3.0\n")
    none = {"neighbour_pairs": np.zeros((0, 2), np.uint32), "neighbour_gap_sq": np.zeros(0, np.uint32)}
    assert cell_pairs_csv_text(none) == "BlobA,BlobB,GapSq,Gap\n"
    with pytest.raises(ValueError, match="lengths"):
        cell_pairs_csv_text({"neighbour_pairs": pairs, "neighbour_gap_sq": gaps[:-1]})


# ---- torch.distributed ---------------------------------------------------------------------------------------------------------
def test_count_blobs_under_torch_distributed_refuses_the_key_on_every_rank(tmp_path, monkeypatch):
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs

    ranks = _helper("thread_ranks")
    fake = ranks.ThreadRanks(2)
    fake.patch(monkeypatch, dist)
    path_in, post = str(tmp_path / "in"), str(tmp_path / "post")  # (neither exists: nothing may be opened or created)
    settings = {"postprocessing": {"output_location": post + "/"}, "blob_detection": {"input_location": path_in},
                "mi355x": {"neighbour_stats": 4, "depth_spacing": [3, 1, 1]}}
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
    assert "settings['mi355x']['neighbour_stats'] is not available under torch.distributed (2 ranks)" in str(caught[0])
    assert "either side of a slab cut" in str(caught[0])
    assert not os.path.exists(post) and not os.path.exists(path_in)
    assert count_blobs.last_neighbours is None
