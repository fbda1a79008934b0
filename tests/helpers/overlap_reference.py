"""The reference of the cell-by-cell comparison (delivr_cfos_amd/compare_cells.py, HipEngine.cc_overlap), written the slow way and
sharing no code with what it judges: the overlap table is a plain dictionary filled voxel by voxel, the per-cell columns and the
summary are plain Python over that dictionary, and the files are built line by line.  Integers are Python integers, ratios are
Python floats (IEEE double, one division each): every comparison against it is exact equality."""
import json

CELL_COLUMNS = ("id", "voxels", "partners", "best", "best_voxels", "best_iou", "matched")


def table(a, b, n_a, n_b):
    """a, b: (Z, Y, X) arrays of unsigned labels -> ({(a, b): voxels}, pair segments).  A voxel takes part when 1 <= a <= n_a and
    1 <= b <= n_b; a segment is a maximal stretch of one pair inside a row."""
    assert a.shape == b.shape and a.ndim == 3
    pairs, segments = {}, 0
    rows_a = a.reshape(-1, a.shape[2]).tolist()
    rows_b = b.reshape(-1, b.shape[2]).tolist()
    for row_a, row_b in zip(rows_a, rows_b):
        before = None
        for va, vb in zip(row_a, row_b):
            key = (va, vb) if 1 <= va <= n_a and 1 <= vb <= n_b else None
            if key is not None:
                pairs[key] = pairs.get(key, 0) + 1
                if key != before:
                    segments += 1
            before = key
    return pairs, segments


def counts(labels, n):
    """voxels per label 0..n (labels above n are not counted)"""
    out = [0] * (n + 1)
    for v in labels.ravel().tolist():
        if v <= n:
            out[v] += 1
    return out


def as_columns(pairs):
    """the dictionary as HipEngine.cc_overlap orders it: lists a, b, voxels sorted by (a, b)"""
    keys = sorted(pairs)
    return [k[0] for k in keys], [k[1] for k in keys], [pairs[k] for k in keys]


def _ratio(num, den):
    return None if den == 0 else num / den


def _cells(n, cell_counts, hits, side):
    """hits: [(a, b, voxels, iou)] of the hit pairs; side 0: the cells of A, 1: the cells of B"""
    rows = []
    for cell in range(1, n + 1):
        mine = [h for h in hits if h[side] == cell]
        best = (0, 0, 0.0)
        for h in mine:
            partner = h[1 - side]
            if best[0] == 0 or h[2] > best[1] or (h[2] == best[1] and partner < best[0]):
                best = (partner, h[2], h[3])
        rows.append({"id": cell, "voxels": cell_counts[cell], "partners": len(mine), "best": best[0], "best_voxels": best[1],
                     "best_iou": best[2], "matched": len(mine) > 0})
    return rows


def match(pairs, counts_a, counts_b, min_iou=0.0):
    """-> {"pairs": [(pred, ref, voxels, iou, hit)] sorted, "pred": [row dicts], "ref": [row dicts], "summary": dict}"""
    n_a, n_b = len(counts_a) - 1, len(counts_b) - 1
    listed = []
    for (a, b) in sorted(pairs):
        v = pairs[(a, b)]
        iou = v / (counts_a[a] + counts_b[b] - v)
        listed.append((a, b, v, iou, iou >= min_iou))
    hits = [p[:4] for p in listed if p[4]]
    pred, ref = _cells(n_a, counts_a, hits, 0), _cells(n_b, counts_b, hits, 1)
    true_pred = sum(1 for r in pred if r["matched"])
    detected = sum(1 for r in ref if r["matched"])
    precision, recall = _ratio(true_pred, n_a), _ratio(detected, n_b)
    f1 = None if precision is None or recall is None or precision + recall == 0 else 2 * precision * recall / (precision + recall)
    inter, vp, vr = sum(p[2] for p in listed), sum(counts_a[1:]), sum(counts_b[1:])
    mutual = sum(1 for (a, b, _, _) in hits if pred[a - 1]["best"] == b and ref[b - 1]["best"] == a)
    summary = {"n_pred": n_a, "n_ref": n_b, "true_pred": true_pred, "false_pred": n_a - true_pred, "detected_ref": detected,
               "missed_ref": n_b - detected, "precision": precision, "recall": recall, "f1": f1,
               "merges": sum(1 for r in pred if r["partners"] >= 2), "splits": sum(1 for r in ref if r["partners"] >= 2),
               "mutual_best": mutual, "intersection": inter, "voxels_pred": vp, "voxels_ref": vr, "dice": _ratio(2 * inter, vp + vr),
               "iou": _ratio(inter, vp + vr - inter), "min_iou": float(min_iou)}
    return {"pairs": listed, "pred": pred, "ref": ref, "summary": summary}


def files(result, name="compare"):
    """the four files of compare_cells as text: floats as repr writes them, matched as 0 / 1, a missing ratio as null"""
    pairs = ["pred,ref,voxels,iou"] + [f"{a},{b},{v},{iou!r}" for a, b, v, iou, _ in result["pairs"]]
    out = {f"{name}-pairs.csv": "\n".join(pairs) + "\n"}
    for side in ("pred", "ref"):
        lines = [",".join(CELL_COLUMNS)]
        for r in result[side]:
            lines.append(f"{r['id']},{r['voxels']},{r['partners']},{r['best']},{r['best_voxels']},{r['best_iou']!r},{1 if r['matched'] else 0}")
        out[f"{name}-{side}.csv"] = "\n".join(lines) + "\n"
    out[f"{name}-summary.json"] = json.dumps(result["summary"]) + "\n"
    return out


def assert_table_equal(got, pairs, segments=None):
    """got: the dict of HipEngine.cc_overlap / overlap_table_np; dtypes, order and every number"""
    a, b, v = as_columns(pairs)
    assert got["a"].dtype.name == "uint32" and got["b"].dtype.name == "uint32" and got["voxels"].dtype.name == "uint64"
    assert got["a"].shape == got["b"].shape == got["voxels"].shape == (len(a),)
    assert got["a"].tolist() == a and got["b"].tolist() == b and got["voxels"].tolist() == v
    if segments is not None:
        assert got["segments"] == segments


def assert_match_equal(got, want):
    """got: match_cells' dict (numpy columns); want: match's (plain Python)"""
    assert got["summary"] == want["summary"] and list(got["summary"]) == list(want["summary"])
    for value in got["summary"].values():
        assert value is None or type(value) in (int, float)  # (what json writes without help; never NaN: equality above)
    cols = [list(c) for c in zip(*want["pairs"])] if want["pairs"] else [[], [], [], [], []]
    for key, col in zip(("pred", "ref", "voxels", "iou", "hit"), cols):
        assert got["pairs"][key].tolist() == col, key
    for side in ("pred", "ref"):
        for key in CELL_COLUMNS:
            assert got[side][key].tolist() == [r[key] for r in want[side]], (side, key)
