"""The run-length label file of count_blobs (settings["mi355x"]["label_file"] = "runs"): the format, its numpy reference coder and
decoder, and the reader a later step uses.  Host only - numpy and nothing else; HipEngine.cc_runs_encode / cc_runs_decode are the
device's coder and decoder of the same arrays (csrc/cc_runs.hip).

A run is a maximal stretch of equal, non-zero label inside one row (z, y) of the (Z, Y, X) label volume.  A run never crosses a
row's end, and two touching runs of different labels (the cells a split leaves) are two runs.  Runs are in raster order, so one
label volume has exactly one coding:

    row_start  uint64 [Z*Y + 1]  the runs before row r = z*Y + y (the exclusive prefix sum of the runs per row); the last entry is R
    x0         uint16 [R]        the first x of a run
    x1         uint16 [R]        the LAST x of a run, inclusive (so X = 65536 fits)
    label      uint32 [R]        1..N

It needs X <= 65536 and labels below 2^32 - 1.  The file <brain>-<N>-cc3d.runs holds five arrays written back to back with
numpy's own .npy framing: a uint64[8] header (MAGIC, VERSION, Z, Y, X, N, R, 0) and the four arrays above in that order.  Its name
holds no ".npy", so the reference's cache look-ups (any entry with ".npy" and the brain's name) never match it.
"""
from __future__ import annotations

import os

import numpy as np

MAGIC = 0x534E55524C564C44  # the bytes "DLVLRUNS" read as a little-endian uint64
VERSION = 1
SUFFIX = "-cc3d.runs"
MAX_X = 65536
MAX_LABEL = 2**32 - 2  # (0xffffffff is the kernels' "no voxel")
ARRAYS = (("row_start", np.uint64), ("x0", np.uint16), ("x1", np.uint16), ("label", np.uint32))


def runs_name(brain: str, n: int) -> str:
    return f"{brain}-{int(n)}{SUFFIX}"


def encode_runs(labels) -> dict:
    """(Z, Y, X) labels (any unsigned integer dtype, or int32 / int64 holding such values) -> {"row_start", "x0", "x1", "label",
    "shape"}: the reference coder."""
    labels = np.asarray(labels)
    if labels.ndim != 3 or labels.size == 0:
        raise ValueError(f"encode_runs: expected a non-empty 3-D label volume, got shape {labels.shape}")
    Z, Y, X = (int(v) for v in labels.shape)
    if X > MAX_X:
        raise ValueError(f"encode_runs: X = {X} exceeds {MAX_X}: x0 / x1 are uint16")
    flat = labels.reshape(Z * Y, X)
    if flat.dtype == np.int32:
        flat = flat.view(np.uint32)
    fg = flat != 0
    start = fg.copy()
    start[:, 1:] &= flat[:, 1:] != flat[:, :-1]
    end = fg
    end = end.copy()
    end[:, :-1] &= flat[:, :-1] != flat[:, 1:]
    row_start = np.zeros(Z * Y + 1, dtype=np.uint64)
    np.cumsum(start.sum(axis=1, dtype=np.uint64), out=row_start[1:])
    rs, xs = np.nonzero(start)  # (raster order: rows, then x)
    _, xe = np.nonzero(end)
    lab = flat[rs, xs]
    if lab.size and int(lab.max()) > MAX_LABEL:
        raise ValueError(f"encode_runs: label {int(lab.max())} exceeds {MAX_LABEL}")
    return {"row_start": row_start, "x0": xs.astype(np.uint16), "x1": xe.astype(np.uint16), "label": lab.astype(np.uint32),
            "shape": (Z, Y, X)}


def decode_runs(runs: dict, z0: int = 0, z1=None) -> np.ndarray:
    """the planes [z0, z1) of the coded volume as a dense uint32 array: the reference decoder"""
    Z, Y, X = (int(v) for v in runs["shape"])
    z0, z1 = int(z0), Z if z1 is None else int(z1)
    if not 0 <= z0 <= z1 <= Z:
        raise ValueError(f"decode_runs: planes [{z0}, {z1}) do not lie in the {Z} planes of the coding")
    rs = np.asarray(runs["row_start"], dtype=np.uint64)[z0 * Y:z1 * Y + 1].astype(np.int64)
    out = np.zeros(((z1 - z0) * Y, X), dtype=np.uint32)
    if len(rs) < 2 or rs[-1] == rs[0]:
        return out.reshape(z1 - z0, Y, X)
    a, b = int(rs[0]), int(rs[-1])
    x0 = np.asarray(runs["x0"][a:b]).astype(np.int64)
    length = np.asarray(runs["x1"][a:b]).astype(np.int64) - x0 + 1
    row = np.repeat(np.arange(len(rs) - 1, dtype=np.int64), np.diff(rs))
    # every voxel of every run: its run's index, then its offset inside the run
    which = np.repeat(np.arange(b - a, dtype=np.int64), length)
    offset = np.arange(int(length.sum()), dtype=np.int64) - np.repeat(np.cumsum(length) - length, length)
    out[row[which], x0[which] + offset] = np.asarray(runs["label"][a:b], dtype=np.uint32)[which]
    return out.reshape(z1 - z0, Y, X)


def _header(runs: dict, n: int) -> np.ndarray:
    Z, Y, X = (int(v) for v in runs["shape"])
    return np.array([MAGIC, VERSION, Z, Y, X, int(n), len(runs["label"]), 0], dtype=np.uint64)


def save_runs(path: str, runs: dict, n=None) -> None:
    """Writes the five arrays under `<path>.partial` and renames: a killed run leaves no complete-looking file.  n: the number of
    labels N the header states (default: the largest label of the runs)."""
    if n is None:
        n = int(runs["label"].max()) if len(runs["label"]) else 0
    with open(path + ".partial", "wb") as fh:
        np.lib.format.write_array(fh, _header(runs, n), allow_pickle=False)
        for key, dtype in ARRAYS:
            np.lib.format.write_array(fh, np.ascontiguousarray(runs[key], dtype=dtype), allow_pickle=False)
    os.replace(path + ".partial", path)


def validate_runs(runs: dict, n: int, path: str = "<runs>") -> None:
    """ValueError naming `path` and the first offending row or run unless the arrays are a canonical-order coding of a volume of
    runs["shape"] with labels 1..n: row_start non-decreasing from 0 to R, x0 <= x1 < X, the runs of a row strictly ordered without
    overlap, 0 < label <= n."""
    Z, Y, X = (int(v) for v in runs["shape"])
    row_start, x0, x1, label = (np.asarray(runs[k]) for k, _ in ARRAYS)
    R = len(label)
    if Z < 1 or Y < 1 or not 1 <= X <= MAX_X:
        raise ValueError(f"{path}: shape {(Z, Y, X)} is not a volume with X <= {MAX_X}")
    if not 0 <= int(n) <= MAX_LABEL:
        raise ValueError(f"{path}: N = {n} does not fit the uint32 labels")
    if len(row_start) != Z * Y + 1 or len(x0) != R or len(x1) != R:
        raise ValueError(f"{path}: {len(row_start)} row starts, {len(x0)} / {len(x1)} / {R} x0 / x1 / label entries do not match the "
                         f"header's shape {(Z, Y, X)} and its {R} runs")
    if int(row_start[0]) != 0:
        raise ValueError(f"{path}: row_start[0] = {int(row_start[0])}, expected 0")
    down = np.flatnonzero(row_start[1:] < row_start[:-1])
    if down.size:
        raise ValueError(f"{path}: row_start decreases after row {int(down[0])}")
    if int(row_start[-1]) != R:
        raise ValueError(f"{path}: row_start ends at {int(row_start[-1])}, the file holds {R} runs")
    bad = np.flatnonzero((x0 > x1) | (x1.astype(np.int64) >= X))
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"{path}: run {k} spans x {int(x0[k])}..{int(x1[k])}, outside 0 <= x0 <= x1 < {X}")
    if R > 1:
        # run k + 1 follows run k in the same row unless a row starts at k + 1
        first_of_row = np.zeros(R + 1, dtype=bool)
        first_of_row[np.minimum(row_start, R).astype(np.int64)] = True
        clash = np.flatnonzero((x0[1:] <= x1[:-1]) & ~first_of_row[1:R])
        if clash.size:
            k = int(clash[0]) + 1
            raise ValueError(f"{path}: run {k} (x {int(x0[k])}..{int(x1[k])}) does not lie after run {k - 1} (x {int(x0[k - 1])}.."
                             f"{int(x1[k - 1])}) of its row")
    bad = np.flatnonzero((label == 0) | (label.astype(np.uint64) > np.uint64(n)))
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"{path}: run {k} holds label {int(label[k])}, outside 1..{int(n)}")


def load_runs(path: str) -> dict:
    """Reads and validates a run file -> {"row_start", "x0", "x1", "label", "shape", "n"}.  Everything is checked here, before
    anything is decoded on the host or uploaded; ValueError names the file and the first offending row or run."""
    with open(path, "rb") as fh:
        try:
            header = np.load(fh, allow_pickle=False)
        except Exception as exc:
            raise ValueError(f"{path}: not a run-length label file ({exc})") from None
        if header.dtype != np.uint64 or header.shape != (8,) or int(header[0]) != MAGIC:
            raise ValueError(f"{path}: not a run-length label file (no uint64[8] header with the magic number {MAGIC:#x})")
        if int(header[1]) != VERSION:
            raise ValueError(f"{path}: version {int(header[1])} of the run-length label file, this reader knows version {VERSION}")
        Z, Y, X, n, R = (int(v) for v in header[2:7])
        runs = {"shape": (Z, Y, X), "n": n}
        for key, dtype in ARRAYS:
            try:
                arr = np.load(fh, allow_pickle=False)
            except Exception as exc:
                raise ValueError(f"{path}: the array {key} is missing or damaged ({exc})") from None
            if arr.dtype != dtype or arr.ndim != 1:
                raise ValueError(f"{path}: the array {key} is {arr.dtype} of shape {arr.shape}, expected one axis of {np.dtype(dtype)}")
            runs[key] = arr
    if len(runs["label"]) != R:
        raise ValueError(f"{path}: the header states {R} runs, the file holds {len(runs['label'])} labels")
    validate_runs(runs, n, path)
    return runs


def load_labels(path: str, z0: int = 0, z1=None) -> np.ndarray:
    """the planes [z0, z1) of the label volume of a run file as a dense uint32 array - how a later step reads the labels"""
    return decode_runs(load_runs(path), z0, z1)
