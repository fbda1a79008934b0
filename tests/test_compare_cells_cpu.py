"""delivr_cfos_amd/compare_cells.py without a GPU: the numpy statement of the overlap table (overlap_table_np), the table work of
match_cells and the text of the four files.

The reference is tests/helpers/overlap_reference.py - a dictionary filled voxel by voxel and plain Python over it -, never the code
under test; the file texts are compared with literal strings.  Every comparison is exact equality, floats included (one IEEE
division per ratio on either side).  Every test asserts the property of its input that it is there for."""
import importlib.util
import json
import os

import numpy as np
import pytest

from delivr_cfos_amd import compare_cells as cc


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _helper("overlap_reference")
BIG = 2**32 - 2  # the largest label


def _table(pairs):
    a, b, v = ref.as_columns(pairs)
    return {"a": np.array(a, dtype=np.uint32), "b": np.array(b, dtype=np.uint32), "voxels": np.array(v, dtype=np.uint64)}


# ---- overlap_table_np ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, n_a, n_b", [(0, 12, 9), (1, 3, BIG), (2, BIG, BIG), (3, 0, 5)])
def test_overlap_table_np_against_the_dictionary_loop(seed, n_a, n_b):
    rng = np.random.default_rng(seed)
    shape = (3, 7, 19)
    values_a = np.array([0, 0, 1, 2, 3, 5, 12, 13, 40, BIG, BIG + 1], dtype=np.uint32)
    values_b = np.array([0, 1, 2, 4, 9, 10, 77, BIG, BIG + 1], dtype=np.uint32)
    a = values_a[rng.integers(0, len(values_a), size=shape)]
    b = values_b[rng.integers(0, len(values_b), size=shape)]
    a[1, 2, :] = 3  # a row of one label under changing partners
    b[2, 3, :] = BIG
    pairs, segments = ref.table(a, b, n_a, n_b)
    # what the input is there for: labels above n, the no-voxel value and the largest label are in both volumes
    assert (a == BIG + 1).any() and (b == BIG + 1).any() and (a == BIG).any() and (b == BIG).any() and (a == 0).any() and (b == 0).any()
    assert n_a == BIG or (a.astype(np.int64) > n_a).sum() > 20
    if n_a == BIG and n_b == BIG:
        assert (BIG, BIG) in pairs and not any(k[0] > BIG or k[1] > BIG for k in pairs)
    if n_a == 0:
        assert not pairs and segments == 0
    else:
        assert len(pairs) > 5 and segments > len(pairs)
    got = cc.overlap_table_np(a, b, n_a, n_b)
    ref.assert_table_equal(got, pairs, segments)
    ref.assert_table_equal(cc.overlap_table_np(a.view(np.int32), b.view(np.int32), n_a, n_b), pairs, segments)  # (a tensor's payload)


def test_overlap_table_np_refuses_what_is_no_pair_of_volumes():
    a = np.zeros((2, 3, 4), dtype=np.uint32)
    with pytest.raises(ValueError, match="one non-empty 3-D shape"):
        cc.overlap_table_np(a, a[:, :, :3], 1, 1)
    with pytest.raises(ValueError, match="one non-empty 3-D shape"):
        cc.overlap_table_np(a[0], a[0], 1, 1)
    with pytest.raises(ValueError, match="unsigned"):
        cc.overlap_table_np(a.astype(np.float32), a, 1, 1)
    with pytest.raises(ValueError, match="do not fit"):
        cc.overlap_table_np(a, a, BIG + 1, 1)


# ---- match_cells -------------------------------------------------------------------------------------------------------------
# pred 1 <-> ref 1; pred 2 fuses ref 2 and 3 (a merge, and a tie for its best: 6 voxels each); pred 3 and 4 share ref 4 (a split);
# pred 5 touches nothing (an extra); ref 5 is touched by nothing (a miss); pred 6 and ref 6 share 1 voxel of 2 + 2: IoU 1/3
COUNTS_A = [1000, 10, 20, 5, 5, 3, 2]
COUNTS_B = [990, 9, 8, 7, 12, 4, 2]
PAIRS = {(1, 1): 8, (2, 2): 6, (2, 3): 6, (3, 4): 4, (4, 4): 5, (6, 6): 1}


@pytest.mark.parametrize("min_iou", [0.0, 0.25, 1 / 3, 0.5, 1.0])
def test_match_cells_against_plain_python(min_iou):
    want = ref.match(PAIRS, COUNTS_A, COUNTS_B, min_iou)
    got = cc.match_cells(_table(PAIRS), np.array(COUNTS_A, dtype=np.uint32), np.array(COUNTS_B, dtype=np.uint32), min_iou)
    ref.assert_match_equal(got, want)
    s = got["summary"]
    if min_iou == 0.0:  # what the table is there for
        assert (s["true_pred"], s["false_pred"], s["detected_ref"], s["missed_ref"], s["merges"], s["splits"]) == (5, 1, 5, 1, 1, 1)
        assert got["pred"]["best"].tolist() == [1, 2, 4, 4, 0, 6]  # the tie of pred 2 goes to the smaller label
        assert got["ref"]["best"].tolist() == [1, 2, 2, 4, 0, 6]  # ref 4: the larger share (pred 4: 5 voxels)
        assert s["mutual_best"] == 4  # (1, 1), (2, 2), (4, 4), (6, 6)
        assert got["pred"]["best_iou"][4] == 0.0 and not got["pred"]["matched"][4] and not got["ref"]["matched"][4]
    if min_iou == 1 / 3:  # a pair whose IoU equals the threshold hits
        k = ref.as_columns(PAIRS)[0].index(6)
        assert got["pairs"]["iou"][k] == min_iou and got["pairs"]["hit"][k] and got["pred"]["matched"][5]
        assert s["true_pred"] == 3 and s["merges"] == 0 and s["splits"] == 0
    if min_iou == 1.0:
        assert s["true_pred"] == 0 and s["precision"] == 0.0 and s["recall"] == 0.0 and s["f1"] is None


def test_match_cells_with_an_empty_side():
    none = {"a": np.zeros(0, np.uint32), "b": np.zeros(0, np.uint32), "voxels": np.zeros(0, np.uint64)}
    # empty against empty: every ratio is None, and the JSON says null
    got = cc.match_cells(none, [125], [125])
    ref.assert_match_equal(got, ref.match({}, [125], [125]))
    s = got["summary"]
    assert all(s[k] is None for k in ("precision", "recall", "f1", "dice", "iou")) and s["n_pred"] == s["n_ref"] == 0
    assert "NaN" not in json.dumps(s) and json.loads(json.dumps(s))["f1"] is None
    assert all(len(got["pred"][k]) == 0 for k in cc.CELL_COLUMNS)
    # empty against non-empty, both ways
    for ca, cb in (([125], [100, 20, 5]), ([100, 20, 5], [125])):
        got = cc.match_cells(none, ca, cb)
        ref.assert_match_equal(got, ref.match({}, ca, cb))
        s = got["summary"]
        assert (s["precision"] is None) == (len(ca) == 1) and (s["recall"] is None) == (len(cb) == 1)
        assert s["f1"] is None and s["dice"] == 0.0 and s["iou"] == 0.0 and s["false_pred"] + s["missed_ref"] == 2


def test_match_cells_refuses_a_table_that_does_not_fit_the_counts():
    ca, cb = np.array(COUNTS_A), np.array(COUNTS_B)

    def run(pairs, order=None):
        t = _table(pairs)
        if order is not None:
            t = {k: v[order] for k, v in t.items()}
        return cc.match_cells(t, ca, cb)

    with pytest.raises(ValueError, match=r"pair 1 \(pred 7, ref 1, 1 voxels\) lies outside the labels 1\.\.6 x 1\.\.6"):
        run({(1, 1): 8, (7, 1): 1})
    with pytest.raises(ValueError, match=r"pair 0 \(pred 1, ref 7, 1 voxels\) lies outside"):
        run({(1, 7): 1})
    with pytest.raises(ValueError, match=r"pair 0 \(pred 0, ref 1"):
        cc.match_cells({"a": np.array([0], np.uint32), "b": np.array([1], np.uint32), "voxels": np.array([1], np.uint64)}, ca, cb)
    with pytest.raises(ValueError, match=r"pair 1 \(pred 6, ref 6, 3 voxels\) does not fit cells of 2 and 2 voxels"):
        run({(1, 1): 8, (6, 6): 3})
    with pytest.raises(ValueError, match=r"pair 0 \(pred 1, ref 2, 9 voxels\) does not fit cells of 10 and 8 voxels"):
        run({(1, 2): 9})
    with pytest.raises(ValueError, match=r"pair 2 \(pred 2, ref 2, 6 voxels\) does not lie after pair 1 \(pred 2, ref 3\)"):
        run({(1, 1): 8, (2, 2): 6, (2, 3): 6}, [0, 2, 1])
    with pytest.raises(ValueError, match=r"pair 1 \(pred 1, ref 1, 2 voxels\) does not lie after pair 0"):
        cc.match_cells({"a": np.array([1, 1], np.uint32), "b": np.array([1, 1], np.uint32), "voxels": np.array([2, 2], np.uint64)}, ca, cb)
    with pytest.raises(ValueError, match="columns"):
        cc.match_cells({"a": np.array([1], np.uint32), "b": np.array([1, 1], np.uint32), "voxels": np.array([2], np.uint64)}, ca, cb)


@pytest.mark.parametrize("bad", [-0.01, 1.01, float("nan"), float("inf"), -float("inf"), "half", None])
def test_match_cells_refuses_a_min_iou_outside_0_1(bad):
    with pytest.raises(ValueError, match="min_iou"):
        cc.match_cells(_table(PAIRS), COUNTS_A, COUNTS_B, bad)
    with pytest.raises(ValueError, match="min_iou"):
        cc.compare_cells("never-opened.npy", "never-opened.npy", min_iou=bad, engine=object())


# ---- the files ---------------------------------------------------------------------------------------------------------------
def test_the_text_of_the_four_files(tmp_path):
    result = cc.match_cells(_table({(1, 1): 2}), [94, 4, 2], [97, 3])
    want = {
        "t-pairs.csv": "pred,ref,voxels,iou\n1,1,2,0.4\n",
        "t-pred.csv": "id,voxels,partners,best,best_voxels,best_iou,matched\n1,4,1,1,2,0.4,1\n2,2,0,0,0,0.0,0\n",
        "t-ref.csv": "id,voxels,partners,best,best_voxels,best_iou,matched\n1,3,1,1,2,0.4,1\n",
        "t-summary.json": '{"n_pred": 2, "n_ref": 1, "true_pred": 1, "false_pred": 1, "detected_ref": 1, "missed_ref": 0, '
                          '"precision": 0.5, "recall": 1.0, "f1": 0.6666666666666666, "merges": 0, "splits": 0, "mutual_best": 1, '
                          '"intersection": 2, "voxels_pred": 6, "voxels_ref": 3, "dice": 0.4444444444444444, '
                          '"iou": 0.2857142857142857, "min_iou": 0.0}\n',
    }
    assert cc.result_files(result, "t") == want
    cc.write_result(result, str(tmp_path / "out"), "t")
    assert sorted(os.listdir(tmp_path / "out")) == sorted(want)  # (no .partial left)
    for fname, text in want.items():
        with open(tmp_path / "out" / fname, "rb") as fh:
            assert fh.read() == text.encode()
    # the reference's writer says the same, here and on the table of the cases above
    assert ref.files(ref.match({(1, 1): 2}, [94, 4, 2], [97, 3]), "t") == want
    for min_iou in (0.0, 1 / 3):
        got = cc.match_cells(_table(PAIRS), COUNTS_A, COUNTS_B, min_iou)
        assert cc.result_files(got) == ref.files(ref.match(PAIRS, COUNTS_A, COUNTS_B, min_iou))
    none = {"a": np.zeros(0, np.uint32), "b": np.zeros(0, np.uint32), "voxels": np.zeros(0, np.uint64)}
    empty = cc.result_files(cc.match_cells(none, [5], [5]))
    assert empty["compare-pairs.csv"] == "pred,ref,voxels,iou\n" and '"precision": null' in empty["compare-summary.json"]


# ---- open_labels: refusals that need no device ---------------------------------------------------------------------------------
def test_open_labels_refuses_before_a_file_is_read(tmp_path):
    class NoEngine:  # any use of the engine is an error here
        def __getattr__(self, name):
            raise AssertionError(f"engine.{name} must not be used")

    wide = tmp_path / "brain-7-cc3d.npy"
    np.save(str(wide), np.zeros((2, 3, 4), dtype=np.uint64))
    with pytest.raises(ValueError, match="uint64"):
        cc.open_labels(str(wide), NoEngine())
    flt = tmp_path / "prob.npy"
    np.save(str(flt), np.zeros((2, 3, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="float32"):
        cc.open_labels(str(flt), NoEngine())
    flat = tmp_path / "flat.npy"
    np.save(str(flat), np.zeros((3, 4), dtype=np.uint8))
    with pytest.raises(ValueError, match=r"shape \(3, 4\)"):
        cc.open_labels(str(flat), NoEngine())
    other = tmp_path / "labels.tif"
    other.write_bytes(b"II*\0")
    with pytest.raises(ValueError, match="expected a .npy mask"):
        cc.open_labels(str(other), NoEngine())
    with pytest.raises(ValueError, match="source of type int"):
        cc.open_labels(5, NoEngine())
    with pytest.raises(ValueError, match="uint64"):
        cc.open_labels(np.zeros((2, 3, 4), dtype=np.uint64), NoEngine())
    assert cc._count_in_name("/x/brain-a-12-cc3d.npy") == 12 and cc._count_in_name("/x/labels.npy") is None
    assert cc._count_in_name("/x/brain-cc3d.npy") is None
