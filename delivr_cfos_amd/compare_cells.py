"""Two segmentations matched cell by cell: the overlap table of two label volumes and what follows from it - detection precision /
recall / F1, merges, splits, every cell's best partner and IoU.  The reference has no counterpart; its users score a checkpoint or a
post-processing setting this way against an annotated crop.  The table comes from the device (HipEngine.cc_overlap,
csrc/cc_overlap.hip); everything after it is table work on the host, numpy only, in int64 and float64.

The overlap table of the label volumes A (labels 1..n_a) and B (1..n_b) of one shape: the voxels that take part are those with
1 <= a <= n_a and 1 <= b <= n_b - the background and labels above n contribute nothing -, and the table lists every pair (a, b)
among them with the number of voxels that hold it, sorted by (a, b).  overlap_table_np is that definition in numpy.

    python -m delivr_cfos_amd.compare_cells PRED REF --out DIR [--name N] [--min-iou T] [--device I] [--scores PICKLE [--score-key KEY]]

PRED / REF: a uint8 mask .npy (binaries.npy, or an annotation saved the same way: labelled 26-connected as count_blobs labels), a
dense uint16 / uint32 label .npy (<brain>-<N>-cc3d.npy), or a run-length label file (<brain>-<N>-cc3d.runs).  Prints the summary as
one JSON line and writes <name>-pairs.csv, <name>-pred.csv, <name>-ref.csv and <name>-summary.json into DIR.

With a score per prediction cell - count_blobs' confidence_max of settings["mi355x"]["confidence_stats"], the threshold above which the
cell disappears - the same table gives the whole precision / recall curve (score_curve): --scores names the prediction's
<brain>-stats.pickle, --score-key the column (default confidence_max); <name>-curve.csv is written beside the others and the summary
gains average_precision, best_f1 and best_f1_score.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np

from . import label_runs

MAX_LABEL = label_runs.MAX_LABEL
CELL_COLUMNS = ("id", "voxels", "partners", "best", "best_voxels", "best_iou", "matched")
PAIR_COLUMNS = ("pred", "ref", "voxels", "iou")
CURVE_COLUMNS = ("score", "kept", "true_pred", "detected_ref", "precision", "recall", "f1")


def _as_unsigned(labels, what):
    labels = np.asarray(labels)
    if labels.dtype == np.int32:
        labels = labels.view(np.uint32)
    if labels.dtype not in (np.uint8, np.uint16, np.uint32, np.uint64):
        raise ValueError(f"{what}: labels of dtype {labels.dtype}, expected an unsigned integer type")
    return labels


def overlap_table_np(a, b, n_a: int, n_b: int) -> dict:
    """The overlap table in numpy: the definition, and what a consumer without a GPU uses.  a, b: (Z, Y, X) label volumes of one
    shape (unsigned integers, or int32 holding uint32 values).  -> HipEngine.cc_overlap's dict: {"a", "b": uint32 (P), "voxels":
    uint64 (P), "segments": S}, the pairs sorted by (a, b); S counts the maximal stretches of one pair inside the rows (z, y)."""
    a, b = _as_unsigned(a, "overlap_table_np"), _as_unsigned(b, "overlap_table_np")
    if a.ndim != 3 or a.shape != b.shape or a.size == 0:
        raise ValueError(f"overlap_table_np: volumes of shape {a.shape} and {b.shape}, expected one non-empty 3-D shape")
    n_a, n_b = int(n_a), int(n_b)
    if not (0 <= n_a <= MAX_LABEL and 0 <= n_b <= MAX_LABEL):
        raise ValueError(f"overlap_table_np: n_a = {n_a}, n_b = {n_b} do not fit the uint32 labels")
    part = (a != 0) & (a.astype(np.uint64) <= np.uint64(n_a)) & (b != 0) & (b.astype(np.uint64) <= np.uint64(n_b))
    key = np.where(part, (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64), np.uint64(0))
    start = key != 0
    start[:, :, 1:] &= key[:, :, 1:] != key[:, :, :-1]
    keys, voxels = np.unique(key[part], return_counts=True)
    return {"a": (keys >> np.uint64(32)).astype(np.uint32), "b": (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32),
            "voxels": voxels.astype(np.uint64), "segments": int(start.sum())}


def _ratio(num, den):
    """num / den in float64, None where the denominator is 0 (null in the JSON, never NaN)"""
    return None if den == 0 else float(num) / float(den)


def _side(own, other, voxels, iou, hit, counts):
    """the per-cell columns of one side: own / other = the pairs' labels on this side and on the other one"""
    n = len(counts) - 1
    out = {"id": np.arange(1, n + 1, dtype=np.int64), "voxels": counts[1:].copy(), "partners": np.zeros(n, dtype=np.int64),
           "best": np.zeros(n, dtype=np.int64), "best_voxels": np.zeros(n, dtype=np.int64), "best_iou": np.zeros(n, dtype=np.float64)}
    own, other, voxels, iou = own[hit], other[hit], voxels[hit], iou[hit]
    np.add.at(out["partners"], own - 1, 1)
    order = np.lexsort((other, -voxels, own))  # per cell: most shared voxels first, the smaller partner on a tie
    cells, first = np.unique(own[order], return_index=True)
    top = order[first]
    out["best"][cells - 1] = other[top]
    out["best_voxels"][cells - 1] = voxels[top]
    out["best_iou"][cells - 1] = iou[top]
    out["matched"] = out["partners"] > 0
    return out


def _checked_min_iou(min_iou) -> float:
    try:
        value = float(min_iou)
    except (TypeError, ValueError):
        raise ValueError(f"compare_cells: min_iou = {min_iou!r}: expected a number in [0, 1]") from None
    if not math.isfinite(value) or not 0.0 <= value <= 1.0:
        raise ValueError(f"compare_cells: min_iou = {min_iou!r}: expected a finite number in [0, 1]")
    return value


def match_cells(table: dict, counts_a, counts_b, min_iou: float = 0.0) -> dict:
    """A = the prediction, B = the reference.  table: the overlap table (HipEngine.cc_overlap / overlap_table_np); counts_a,
    counts_b: the voxels per label 0..n (HipEngine.cc_counts; row 0, the background, is not used), so n_pred = len(counts_a) - 1 and
    n_ref = len(counts_b) - 1.  Per pair iou = voxels / (counts_a[a] + counts_b[b] - voxels); a pair HITS when iou >= min_iou (with
    the default 0.0 any overlap hits).
    -> {"pairs": {"pred", "ref", "voxels": int64, "iou": float64, "hit": bool} in the table's order,
        "pred", "ref": per cell 1..n {"id", "voxels", "partners" = its hit pairs, "best" = the partner of the hit pair with the most
            shared voxels (the smaller label on a tie; 0 without a hit pair), "best_voxels", "best_iou", "matched" = partners > 0},
        "summary": n_pred, n_ref, true_pred (A cells with a hit), false_pred, detected_ref (B cells with a hit), missed_ref,
            precision = true_pred / n_pred, recall = detected_ref / n_ref, f1 = 2 * precision * recall / (precision + recall),
            merges = A cells with >= 2 hit partners (each fuses several reference cells), splits = B cells with >= 2 hit partners,
            mutual_best = hit pairs that are each other's best, and at voxel level intersection = all shared voxels, voxels_pred,
            voxels_ref, dice = 2 * intersection / (voxels_pred + voxels_ref), iou = intersection / (voxels_pred + voxels_ref -
            intersection); min_iou.  A ratio with a zero denominator is None.}
    ValueError naming the first offending pair when the table does not fit the counts (labels outside 1..n, more shared voxels than
    a cell has, pairs not strictly increasing), and for a min_iou that is not a finite number in [0, 1]."""
    min_iou = _checked_min_iou(min_iou)
    ca =np.ascontiguousarray(counts_a).astype(np.int64).ravel()
    cb = np.ascontiguousarray(counts_b).astype(np.int64).ravel()
    if len(ca) < 1 or len(cb) < 1:
        raise ValueError("match_cells: the counts hold a row per label 0..n, at least the background's")
    n_a, n_b = len(ca) - 1, len(cb) - 1
    a = np.asarray(table["a"]).astype(np.int64)
    b = np.asarray(table["b"]).astype(np.int64)
    vox_u = np.asarray(table["voxels"])
    if not (a.ndim == b.ndim == vox_u.ndim == 1 and len(a) == len(b) == len(vox_u)):
        raise ValueError(f"match_cells: the table's columns hold {a.shape}, {b.shape}, {vox_u.shape} entries")
    if vox_u.dtype.kind == "u" and len(vox_u) and int(vox_u.max()) > np.iinfo(np.int64).max:
        raise ValueError(f"match_cells: pair ({a[int(vox_u.argmax())]}, {b[int(vox_u.argmax())]}) shares {int(vox_u.max())} voxels")
    vox = vox_u.astype(np.int64)

    def pair(k):
        return f"pair {k} (pred {int(a[k])}, ref {int(b[k])}, {int(vox[k])} voxels)"

    bad = np.flatnonzero((a < 1) | (a > n_a) | (b < 1) | (b > n_b))
    if bad.size:
        raise ValueError(f"match_cells: {pair(int(bad[0]))} lies outside the labels 1..{n_a} x 1..{n_b} of the counts")
    bad = np.flatnonzero((vox < 1) | (vox > np.minimum(ca[a], cb[b])))
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"match_cells: {pair(k)} does not fit cells of {int(ca[a[k]])} and {int(cb[b[k]])} voxels")
    bad = np.flatnonzero((a[1:] < a[:-1]) | ((a[1:] == a[:-1]) & (b[1:] <= b[:-1])))
    if bad.size:
        k = int(bad[0]) + 1
        raise ValueError(f"match_cells: {pair(k)} does not lie after pair {k - 1} (pred {int(a[k - 1])}, ref {int(b[k - 1])}): the table "
                         "is sorted by (pred, ref) and unique")
    iou = vox.astype(np.float64) / (ca[a] + cb[b] - vox).astype(np.float64)
    hit = iou >= min_iou
    pred, ref = _side(a, b, vox, iou, hit, ca), _side(b, a, vox, iou, hit, cb)
    mutual = int((hit & (pred["best"][a - 1] == b) & (ref["best"][b - 1] == a)).sum())
    true_pred, detected_ref = int(pred["matched"].sum()), int(ref["matched"].sum())
    precision, recall = _ratio(true_pred, n_a), _ratio(detected_ref, n_b)
    f1 = None if precision is None or recall is None or precision + recall == 0 else 2 * precision * recall / (precision + recall)
    inter, vp, vr = int(vox.sum()), int(ca[1:].sum()), int(cb[1:].sum())
    summary = {"n_pred": n_a, "n_ref": n_b, "true_pred": true_pred, "false_pred": n_a - true_pred, "detected_ref": detected_ref,
               "missed_ref": n_b - detected_ref, "precision": precision, "recall": recall, "f1": f1,
               "merges": int((pred["partners"] >= 2).sum()), "splits": int((ref["partners"] >= 2).sum()), "mutual_best": mutual,
               "intersection": inter, "voxels_pred": vp, "voxels_ref": vr, "dice": _ratio(2 * inter, vp + vr),
               "iou": _ratio(inter, vp + vr - inter), "min_iou": min_iou}
    return {"pairs": {"pred": a, "ref": b, "voxels": vox, "iou": iou, "hit": hit}, "pred": pred, "ref": ref, "summary": summary}


def _checked_scores(scores, n_pred=None) -> np.ndarray:
    """one finite number per prediction cell as float64, row 0 of a table of n_pred + 1 rows dropped; with n_pred None the length is
    not judged yet (compare_cells looks at the values before it opens a volume)"""
    try:
        s = np.asarray(scores).astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError("score_curve: scores: expected one number per prediction cell") from None
    if s.ndim != 1 or not np.isfinite(s).all():
        raise ValueError(f"score_curve: scores of shape {s.shape}: expected a 1-D array of finite numbers (no NaN, no inf)")
    if n_pred is None:
        return s
    if len(s) not in (n_pred, n_pred + 1):
        raise ValueError(f"score_curve: {len(s)} scores beside {n_pred} prediction cells: expected {n_pred}, or {n_pred + 1} with a row 0")
    return s[1:] if len(s) == n_pred + 1 else s


def score_curve(matched: dict, scores) -> dict:
    """The detection curve of a comparison over a score per prediction cell.  matched: match_cells' dict; scores: one finite number
    per prediction cell 1..n_pred (or n_pred + 1 numbers, row 0 ignored) - ValueError for NaN, inf or another length.  For every
    distinct score t, descending: kept = the cells with score >= t, true_pred = the kept cells with a hit pair, detected_ref = the
    reference cells with a hit pair whose prediction cell is kept, precision = true_pred / kept, recall = detected_ref / n_ref, f1 as
    in match_cells.
    -> {"curve": {"score": float64, "kept", "true_pred", "detected_ref": int64, "precision", "recall", "f1": float64}, one row per
        cut - an undefined ratio (recall without a reference cell, f1 without both or with precision + recall == 0) is NaN here and
        null in the file -,
        "summary": average_precision = sum_k (recall_k - recall_{k-1}) * precision_k with recall_0 = 0 (None when n_ref == 0),
        best_f1 and best_f1_score = the largest f1 and its cut, the highest cut on a tie (None without a defined f1)}."""
    n_pred, n_ref = int(matched["summary"]["n_pred"]), int(matched["summary"]["n_ref"])
    s = _checked_scores(scores, n_pred)
    pairs = matched["pairs"]
    hit = np.asarray(pairs["hit"], dtype=bool)
    a, b = np.asarray(pairs["pred"], dtype=np.int64)[hit], np.asarray(pairs["ref"], dtype=np.int64)[hit]
    cuts = np.unique(s)[::-1]
    ascending = np.sort(s)
    kept = (n_pred - np.searchsorted(ascending, cuts, side="left")).astype(np.int64)
    true_scores = np.sort(s[np.unique(a) - 1])  # the cells with a hit pair
    true_pred = (len(true_scores) - np.searchsorted(true_scores, cuts, side="left")).astype(np.int64)
    # a reference cell is detected from its best-scored hit partner down
    ref_best = np.full(n_ref, -np.inf, dtype=np.float64)
    np.maximum.at(ref_best, b - 1, s[a - 1])
    ref_scores = np.sort(ref_best[np.isfinite(ref_best)])
    detected = (len(ref_scores) - np.searchsorted(ref_scores, cuts, side="left")).astype(np.int64)
    precision = true_pred.astype(np.float64) / kept.astype(np.float64)  # (a cut is some cell's score: kept >= 1)
    recall = detected.astype(np.float64) / float(n_ref) if n_ref else np.full(len(cuts), np.nan)
    f1 = np.full(len(cuts), np.nan)
    ok = np.isfinite(recall) & (precision + np.nan_to_num(recall) > 0)
    f1[ok] = 2 * precision[ok] * recall[ok] / (precision[ok] + recall[ok])
    ap = None if n_ref == 0 else float(np.sum(np.diff(recall, prepend=0.0) * precision))
    best = int(np.nanargmax(f1)) if np.isfinite(f1).any() else None  # (the first of equal maxima: the highest cut)
    summary = {"average_precision": ap, "best_f1": None if best is None else float(f1[best]),
               "best_f1_score": None if best is None else float(cuts[best])}
    return {"curve": {"score": cuts.astype(np.float64), "kept": kept, "true_pred": true_pred, "detected_ref": detected,
                      "precision": precision, "recall": recall, "f1": f1}, "summary": summary}


def _open_scores(scores, score_key: str):
    """compare_cells' scores: an array, or the path of a <brain>-stats.pickle whose entry score_key is the column"""
    if isinstance(scores, (str, os.PathLike)):
        import pickle

        with open(os.fspath(scores), "rb") as fh:
            stats = pickle.load(fh)
        if not isinstance(stats, dict) or score_key not in stats:
            raise ValueError(f"compare_cells: {os.fspath(scores)} holds no entry {score_key!r} (count_blobs writes confidence_max with "
                             "settings['mi355x']['confidence_stats'])")
        scores = stats[score_key]
    return _checked_scores(scores)


# ---- the sources ---------------------------------------------------------------------------------------------------------------
def _count_in_name(path: str):
    """N of a <brain>-<N>-cc3d.npy name, None for any other name"""
    parts = os.path.basename(path).split("-")
    if len(parts) >= 3 and parts[-1] == "cc3d.npy" and parts[-2].isdigit():
        return int(parts[-2])
    return None


def _largest_label(labels) -> int:
    """the largest uint32 payload of an int32 tensor in HBM"""
    lo, hi = int(labels.min()), int(labels.max())
    return hi if lo >= 0 else int(labels[labels < 0].max()) + 2**32  # (the payloads from 2^31 read negative, in their order)


def _labels_from_array(arr, engine, what: str, n=None):
    import torch

    if arr.ndim != 3 or arr.size == 0:
        raise ValueError(f"compare_cells: {what}: shape {tuple(arr.shape)}, expected a non-empty (Z, Y, X) volume")
    if arr.dtype == np.uint8:  # a mask: labelled as count_blobs labels it
        return engine.ccl26(engine.to_device(np.ascontiguousarray(arr)))
    if arr.dtype == np.uint16:  # (widened in HBM, not on the host)
        labels = torch.from_numpy(np.array(arr).view(np.int16)).to(engine.device).to(torch.int32) & 0xFFFF
    elif arr.dtype == np.uint32:
        labels = torch.from_numpy(np.array(arr).view(np.int32)).to(engine.device)
    elif arr.dtype == np.uint64:
        raise ValueError(f"compare_cells: {what} holds uint64 labels; the comparison takes labels below 2^32 - 1 (uint16 / uint32)")
    else:
        raise ValueError(f"compare_cells: {what} is {arr.dtype}; expected a uint8 mask or uint16 / uint32 labels")
    labels = labels.contiguous()
    if n is None:
        n = _largest_label(labels)
    if n > MAX_LABEL:
        raise ValueError(f"compare_cells: {what} holds the label {n}; labels lie below 2^32 - 1")
    return labels, int(n)


def open_labels(source, engine):
    """One side of a comparison -> (int32 tensor (uint32 payload) (Z, Y, X) in HBM, n).  source:
      - a path to a uint8 .npy mask: labelled 26-connected with engine.ccl26, in the order count_blobs uses;
      - a path to a dense uint16 / uint32 label .npy: n from a <brain>-<N>-cc3d.npy name, else the largest label, found on the device;
      - a path to a run-length label file (.runs: label_runs.load_runs, decoded on the device);
      - a numpy array of one of those dtypes, or a pair (int32 tensor in HBM, n).
    Anything else is a ValueError, raised from the file's header: before the file is read in full."""
    if isinstance(source, tuple) and len(source) == 2:
        labels, n = source
        engine._label_volume("compare_cells", labels)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= MAX_LABEL:
            raise ValueError(f"compare_cells: n = {n!r} beside a label tensor: expected an integer 0..2^32 - 2")
        return labels, int(n)
    if isinstance(source, np.ndarray):
        return _labels_from_array(source, engine, f"an array of shape {tuple(source.shape)}")
    if isinstance(source, (str, os.PathLike)):
        path = os.fspath(source)
        if path.endswith(".runs"):
            runs = label_runs.load_runs(path)  # (validated in full before anything is uploaded)
            return engine.cc_runs_decode(runs), int(runs["n"])
        if path.endswith(".npy"):
            try:
                arr = np.load(path, mmap_mode="r", allow_pickle=False)  # (the header; the voxels are read once the dtype is known)
            except (ValueError, EOFError) as exc:
                raise ValueError(f"compare_cells: {path}: not a .npy volume ({exc})") from None
            return _labels_from_array(arr, engine, path, None if arr.dtype == np.uint8 else _count_in_name(path))
        raise ValueError(f"compare_cells: {path}: expected a .npy mask, a .npy label volume or a .runs label file")
    raise ValueError(f"compare_cells: a source of type {type(source).__name__}: expected a path, a numpy array or (labels in HBM, n)")


# ---- the files -----------------------------------------------------------------------------------------------------------------
def _field(v) -> str:
    if isinstance(v, (bool, np.bool_)):
        return "1" if v else "0"
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    return str(int(v))


def _curve_csv(curve: dict) -> str:
    rows = [",".join(CURVE_COLUMNS)]
    rows += [",".join("null" if isinstance(v, float) and math.isnan(v) else _field(v) for v in row)
             for row in zip(*(curve[c].tolist() for c in CURVE_COLUMNS))]
    return "\n".join(rows) + "\n"


def _csv(columns, table: dict) -> str:
    rows = [",".join(columns)]
    rows += [",".join(_field(v) for v in row) for row in zip(*(table[c].tolist() for c in columns))]
    return "\n".join(rows) + "\n"


def result_files(result: dict, name: str = "compare") -> dict:
    """the four files of a comparison -> {file name: text}; floats as repr writes them, `matched` as 0 / 1, a missing ratio as null"""
    files = {f"{name}-pairs.csv": _csv(PAIR_COLUMNS, result["pairs"]), f"{name}-pred.csv": _csv(CELL_COLUMNS, result["pred"]),
             f"{name}-ref.csv": _csv(CELL_COLUMNS, result["ref"]), f"{name}-summary.json": json.dumps(result["summary"]) + "\n"}
    if "curve" in result:  # (a comparison with scores: score_curve's rows, an undefined ratio as null)
        files[f"{name}-curve.csv"] = _curve_csv(result["curve"])
    return files


def write_result(result: dict, out_dir: str, name: str = "compare") -> None:
    """each file under `<file>.partial`, then renamed: a killed run leaves no complete-looking file"""
    os.makedirs(out_dir, exist_ok=True)
    for fname, text in result_files(result, name).items():
        path = os.path.join(out_dir, fname)
        with open(path + ".partial", "w", newline="") as fh:
            fh.write(text)
        os.replace(path + ".partial", path)


def with_scores(result: dict, scores) -> dict:
    """match_cells' dict with score_curve's on top: the entry "curve", and its three numbers in the summary"""
    curve = score_curve(result, scores)
    return {**result, "curve": curve["curve"], "summary": {**result["summary"], **curve["summary"]}}


def compare_cells(pred, ref, out_dir=None, name: str = "compare", min_iou: float = 0.0, engine=None, scores=None,
                  score_key: str = "confidence_max") -> dict:
    """pred against ref (open_labels says what either may be), cell by cell -> match_cells' dict; with out_dir the files
    <name>-pairs.csv (pred,ref,voxels,iou), <name>-pred.csv and <name>-ref.csv (id,voxels,partners,best,best_voxels,best_iou,matched)
    and <name>-summary.json.  Both label volumes, the pair table and its outputs are in HBM at once: MemoryError otherwise.
    scores: one finite number per prediction cell (n_pred of them, or n_pred + 1 with a row 0), or the path of the prediction's
    <brain>-stats.pickle, whose entry score_key is taken - the result gains "curve" and the summary average_precision, best_f1 and
    best_f1_score (score_curve), and <name>-curve.csv (score,kept,true_pred,detected_ref,precision,recall,f1) is written beside the
    others.  None: results and files are what they are without scores."""
    from .engine import HipEngine

    min_iou = _checked_min_iou(min_iou)  # (judged before anything is opened)
    if scores is not None:
        scores = _open_scores(scores, score_key)  # (and so are the values; the length once n_pred is known)
    own = engine is None
    eng = engine or HipEngine(0)
    try:
        labels_a, n_a = open_labels(pred, eng)
        labels_b, n_b = open_labels(ref, eng)
        if tuple(labels_a.shape) != tuple(labels_b.shape):
            raise ValueError(f"compare_cells: the prediction has shape {tuple(labels_a.shape)}, the reference {tuple(labels_b.shape)}")
        counts_a = eng.cc_counts(labels_a, n_a).cpu().numpy().view(np.uint32)
        counts_b = eng.cc_counts(labels_b, n_b).cpu().numpy().view(np.uint32)
        table = eng.cc_overlap(labels_a, n_a, labels_b, n_b)
        del labels_a, labels_b
        result = match_cells(table, counts_a, counts_b, min_iou)
        if scores is not None:
            result = with_scores(result, scores)
        if out_dir is not None:
            write_result(result, out_dir, name)
        return result
    finally:
        if own:
            eng.close()


def main(argv=None) -> int:
    import argparse

    ap = argparse.ArgumentParser(prog="python -m delivr_cfos_amd.compare_cells", description="Match two segmentations cell by cell.")
    ap.add_argument("pred", metavar="PRED", help="the prediction: a uint8 mask .npy, a uint16 / uint32 label .npy or a .runs label file")
    ap.add_argument("ref", metavar="REF", help="the reference, in any of the same forms")
    ap.add_argument("--out", metavar="DIR", default=None, help="folder for <name>-pairs.csv, -pred.csv, -ref.csv and -summary.json")
    ap.add_argument("--name", default="compare")
    ap.add_argument("--min-iou", type=float, default=0.0, help="a pair hits when its IoU is at least this (default 0: any overlap)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--scores", metavar="PICKLE", default=None,
                    help="the prediction's <brain>-stats.pickle: adds <name>-curve.csv and average_precision / best_f1 to the summary")
    ap.add_argument("--score-key", metavar="KEY", default="confidence_max", help="the pickle's entry that scores the cells")
    args = ap.parse_args(argv)
    from .engine import HipEngine

    eng = HipEngine(args.device)
    try:
        result = compare_cells(args.pred, args.ref, args.out, args.name, args.min_iou, engine=eng, scores=args.scores,
                               score_key=args.score_key)
    finally:
        eng.close()
    print(json.dumps(result["summary"]), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
