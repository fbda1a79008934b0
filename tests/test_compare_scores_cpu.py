"""compare_cells with a score per prediction cell (score_curve, compare_cells(scores=...), <name>-curve.csv): the curve against a plain
loop over the cuts on hand-made overlap tables - numpy only, no device."""
import json
import math
import pickle

import numpy as np
import pytest

from delivr_cfos_amd import compare_cells as cc


def _table(pairs):
    pairs = sorted(pairs)
    return {"a": np.array([p[0] for p in pairs], dtype=np.uint32), "b": np.array([p[1] for p in pairs], dtype=np.uint32),
            "voxels": np.array([p[2] for p in pairs], dtype=np.uint64), "segments": len(pairs)}


def _loop(matched, scores):
    """the definition, cut by cut"""
    n_pred, n_ref = matched["summary"]["n_pred"], matched["summary"]["n_ref"]
    hits = [(int(a), int(b)) for a, b, h in zip(matched["pairs"]["pred"], matched["pairs"]["ref"], matched["pairs"]["hit"]) if h]
    rows, prev_recall, ap = [], 0.0, 0.0
    for t in sorted(set(scores), reverse=True):
        kept = {i for i in range(1, n_pred + 1) if scores[i - 1] >= t}
        true_pred = len({a for a, _ in hits if a in kept})
        detected = len({b for a, b in hits if a in kept})
        precision = true_pred / len(kept)
        recall = detected / n_ref if n_ref else None
        f1 = None if recall is None or precision + recall == 0 else 2 * precision * recall / (precision + recall)
        if recall is not None:
            ap += (recall - prev_recall) * precision
            prev_recall = recall
        rows.append((float(t), len(kept), true_pred, detected, precision, recall, f1))
    best = None
    for row in rows:  # descending cuts: a later equal f1 does not replace the first
        if row[6] is not None and (best is None or row[6] > best[6]):
            best = row
    return rows, {"average_precision": ap if n_ref else None, "best_f1": best and best[6], "best_f1_score": best and best[0]}


def _assert_curve(got, rows, summary):
    assert list(got["curve"]) == list(cc.CURVE_COLUMNS)
    assert len(got["curve"]["score"]) == len(rows)
    for k, col in enumerate(cc.CURVE_COLUMNS):
        arr = got["curve"][col]
        assert arr.dtype == (np.int64 if col in ("kept", "true_pred", "detected_ref") else np.float64), col
        for have, want in zip(arr.tolist(), (r[k] for r in rows)):
            assert (math.isnan(have) if want is None else have == want), (col, have, want)
    assert set(got["summary"]) == {"average_precision", "best_f1", "best_f1_score"}
    for k in ("best_f1", "best_f1_score"):
        assert got["summary"][k] == summary[k], k
    if summary["average_precision"] is None:
        assert got["summary"]["average_precision"] is None
    else:
        assert got["summary"]["average_precision"] == pytest.approx(summary["average_precision"], abs=1e-15)  # (the order of a float sum)


# prediction cells 1..6, reference cells 1..5: cell 1 merges ref 1 + 2, ref 3 is split over cells 2 + 3, cell 4 <-> ref 4 one to one,
# cells 5 and 6 are false, ref 5 is missed
PAIRS = [(1, 1, 4), (1, 2, 3), (2, 3, 2), (3, 3, 5), (4, 4, 6)]
COUNTS_A = [0, 9, 2, 6, 6, 3, 1]
COUNTS_B = [0, 5, 4, 8, 7, 2]


@pytest.mark.parametrize("scores", [[0.9, 0.8, 0.7, 0.6, 0.5, 0.4],          # all distinct
                                    [0.5, 0.9, 0.5, 0.9, 0.9, 0.5],          # ties: two cuts
                                    [0.7, 0.7, 0.7, 0.7, 0.7, 0.7],          # one cut
                                    [0.1, 0.2, 0.9, 0.3, 0.95, 0.99],        # the false cells first; the split's second half before its first
                                    [3, 1, 2, 5, 4, 0]])                     # integers
@pytest.mark.parametrize("min_iou", [0.0, 0.35])  # (0.35: the pairs (1, 2) of IoU 0.3 and (2, 3) of IoU 0.25 no longer hit)
def test_score_curve_against_the_loop_over_the_cuts(scores, min_iou):
    matched = cc.match_cells(_table(PAIRS), COUNTS_A, COUNTS_B, min_iou)
    assert matched["summary"]["merges"] == (1 if min_iou == 0.0 else 0) and matched["summary"]["splits"] == (1 if min_iou == 0.0 else 0)
    rows, summary = _loop(matched, scores)
    _assert_curve(cc.score_curve(matched, scores), rows, summary)
    _assert_curve(cc.score_curve(matched, np.array([123.0] + list(scores))), rows, summary)  # n_pred + 1 rows: row 0 is ignored
    # the last cut keeps every cell: the operating point match_cells reports
    last = rows[-1]
    assert last[1] == 6 and last[2] == matched["summary"]["true_pred"] and last[3] == matched["summary"]["detected_ref"]
    assert last[4] == matched["summary"]["precision"] and last[5] == matched["summary"]["recall"]


def test_score_curve_without_reference_cells_and_with_all_cells_false():
    no_ref = cc.match_cells(_table([]), [0, 3, 4], [0], 0.0)
    got = cc.score_curve(no_ref, [0.9, 0.6])
    _assert_curve(got, *_loop(no_ref, [0.9, 0.6]))
    assert got["summary"] == {"average_precision": None, "best_f1": None, "best_f1_score": None}
    assert np.isnan(got["curve"]["recall"]).all() and got["curve"]["precision"].tolist() == [0.0, 0.0]
    all_false = cc.match_cells(_table([]), [0, 3, 4], [0, 5, 5], 0.0)
    got = cc.score_curve(all_false, [0.6, 0.9])
    _assert_curve(got, *_loop(all_false, [0.6, 0.9]))
    assert got["summary"] == {"average_precision": 0.0, "best_f1": None, "best_f1_score": None}
    no_pred = cc.match_cells(_table([]), [0], [0, 5], 0.0)
    got = cc.score_curve(no_pred, [])
    assert len(got["curve"]["score"]) == 0 and got["summary"] == {"average_precision": 0.0, "best_f1": None, "best_f1_score": None}


def test_best_f1_takes_the_highest_cut_on_a_tie():
    # two cells, two reference cells, one to one: the cut at 0.9 has p = 1, r = 1/2 (f1 = 2/3), the cut at 0.1 adds a false cell and the
    # second reference cell's partner ... built so that both cuts give f1 = 2/3
    matched = cc.match_cells(_table([(1, 1, 2), (3, 2, 2)]), [0, 2, 2, 2, 2], [0, 2, 2], 0.0)
    scores = [0.9, 0.1, 0.1, 0.1]  # cut 0.9: p 1, r 1/2 -> 2/3; cut 0.1: p 2/4, r 1 -> 2/3
    got = cc.score_curve(matched, scores)
    assert got["curve"]["f1"].tolist() == [2 * 1 * 0.5 / 1.5, 2 * 0.5 * 1 / 1.5]
    assert got["curve"]["f1"][0] == got["curve"]["f1"][1]
    assert got["summary"]["best_f1_score"] == 0.9 and got["summary"]["best_f1"] == got["curve"]["f1"][0]


@pytest.mark.parametrize("bad", [[0.1, 0.2, 0.3], [0.1] * 8, [0.1, np.nan, 0.3, 0.4, 0.5, 0.6], [0.1, np.inf, 0.3, 0.4, 0.5, 0.6],
                                 [[0.1, 0.2, 0.3, 0.4, 0.5, 0.6]], ["a", "b", "c", "d", "e", "f"]])
def test_score_curve_refuses_scores_that_are_no_column_of_finite_numbers(bad):
    matched = cc.match_cells(_table(PAIRS), COUNTS_A, COUNTS_B, 0.0)
    with pytest.raises(ValueError, match="score"):
        cc.score_curve(matched, bad)


def test_compare_cells_judges_the_scores_before_anything_is_opened(tmp_path):
    with pytest.raises(ValueError, match="finite"):
        cc.compare_cells("never-opened.npy", "never-opened.npy", scores=[0.5, float("nan")], engine=object())
    path = str(tmp_path / "brain-stats.pickle")
    with open(path, "wb") as fh:
        pickle.dump({"voxel_counts": np.zeros(3, np.uint32), "other": np.array([0.0, np.inf, 1.0])}, fh)
    with pytest.raises(ValueError, match="confidence_max"):
        cc.compare_cells("never-opened.npy", "never-opened.npy", scores=path, engine=object())
    with pytest.raises(ValueError, match="finite"):
        cc.compare_cells("never-opened.npy", "never-opened.npy", scores=path, score_key="other", engine=object())


def test_numpy_label_volumes_through_overlap_table_np_and_the_files(tmp_path):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 7, size=(4, 6, 8)).astype(np.uint32)  # labels 1..6
    b = rng.integers(0, 4, size=(4, 6, 8)).astype(np.uint32)
    b[a == 5] = 0  # cell 5 is false
    matched = cc.match_cells(cc.overlap_table_np(a, b, 6, 3), np.bincount(a.ravel(), minlength=7), np.bincount(b.ravel(), minlength=4), 0.1)
    scores = np.array([0.0, 0.9, 0.75, 0.75, 0.6, 0.95, 0.5])  # (row 0 beside the six cells, as a pickle's column)
    result = cc.with_scores(matched, scores)
    rows, summary = _loop(matched, scores[1:].tolist())
    _assert_curve({"curve": result["curve"], "summary": {k: result["summary"][k] for k in summary}}, rows, summary)
    # without scores: today's keys, in the result and in the files; with them: one more file, three more summary entries, the rest equal
    plain = cc.result_files(matched, "x")
    assert set(matched) == {"pairs", "pred", "ref", "summary"}
    assert list(plain) == ["x-pairs.csv", "x-pred.csv", "x-ref.csv", "x-summary.json"]
    scored = cc.result_files(result, "x")
    assert list(scored) == list(plain) + ["x-curve.csv"]
    for name in ("x-pairs.csv", "x-pred.csv", "x-ref.csv"):
        assert scored[name] == plain[name]
    before, after = json.loads(plain["x-summary.json"]), json.loads(scored["x-summary.json"])
    assert list(after) == list(before) + ["average_precision", "best_f1", "best_f1_score"] and {k: after[k] for k in before} == before
    lines = scored["x-curve.csv"].split("\n")
    assert lines[0] == "score,kept,true_pred,detected_ref,precision,recall,f1" and lines[-1] == "" and len(lines) == len(rows) + 2
    assert lines[1] == ",".join([repr(rows[0][0])] + [str(v) for v in rows[0][1:4]] + ["null" if v is None else repr(float(v)) for v in rows[0][4:]])
    cc.write_result(result, str(tmp_path), "x")
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(scored)
    assert (tmp_path / "x-curve.csv").read_text() == scored["x-curve.csv"]
    # an undefined ratio is null in the file
    no_ref = cc.with_scores(cc.match_cells(_table([]), [0, 3], [0], 0.0), [0.5])
    assert cc.result_files(no_ref)["compare-curve.csv"].split("\n")[1] == "0.5,1,0,0,0.0,null,null"
