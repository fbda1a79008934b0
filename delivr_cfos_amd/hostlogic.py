"""Host-side integer logic of the path that the reference performs in Python (no device work)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np


def padded_shape(stack_shape: Sequence[int], crop: Sequence[int]) -> Tuple[int, ...]:
    """ceil(dim / crop) * crop per axis (inference/inference.py:229-231;
    downsample/downsample_and_mask.py:390-393)."""
    return tuple(int(np.ceil(int(n) / int(c)) * int(c)) for n, c in zip(stack_shape, crop))


def arrayterator_zblock(shape_zyx: Sequence[int], buf_size: int = 1000**3) -> int:
    """Planes per block of np.lib.Arrayterator(volume[(Z,Y,X)], buf_size) - the granularity at which
    the reference erodes the re-mask (inference/inference.py:53,77-84).  Returns Z when the whole
    volume fits one block."""
    Z, Y, X = (int(v) for v in shape_zyx)
    count = int(buf_size)
    if count <= X or count // X <= Y:
        raise NotImplementedError("a single z-plane exceeds the Arrayterator buffer (Y*X > buf_size)")
    count = (count // X) // Y
    return Z if count >= Z else max(count, 1)


MAX_RANKS = 16  # DLV_MAX_RANKS (include/delivr_hip.h): ranks of one communicator


def resolve_devices(cuda_devices, setting, device_count: int, group_world: int = 1) -> List[int]:
    """The devices run_inference shards one volume over, from its ``cuda_devices`` argument ("0,1" in the reference) and
    settings["mi355x"]["devices"]:
      None / "first"  the first entry of cuda_devices, 0 when it is empty or not visible (what run_inference always did),
      "all"           every entry of cuda_devices (the reference's DataParallel spans them all),
      [i, j, ...]     these devices in this order; repeats are ranks that share a device.
    `group_world`: world size of the torch.distributed group this process is a rank of (1: none) - such a rank has one device.
    Raises ValueError for anything else: an unknown string, an empty list, an index that is negative or not visible (only the
    default keeps its fall-back to 0), more than one device inside a process group, more ranks than a communicator holds."""
    if setting is None or (isinstance(setting, str) and setting == "first"):
        first = int(str(cuda_devices).split(",")[0]) if str(cuda_devices).strip() else 0
        return [first if first < int(device_count) else 0]
    if isinstance(setting, str):
        if setting != "all":
            raise ValueError(f"settings['mi355x']['devices'] = {setting!r}: expected \"first\", \"all\" or a list of device indices")
        try:
            devs = [int(t) for t in str(cuda_devices).split(",") if t.strip()]
        except ValueError:
            raise ValueError(f"cuda_devices {cuda_devices!r}: expected comma-separated device indices") from None
        if not devs:
            raise ValueError("settings['mi355x']['devices'] = \"all\" with an empty cuda_devices")
    elif isinstance(setting, (list, tuple)):
        if not setting:
            raise ValueError("settings['mi355x']['devices']: an empty list names no device")
        if any(isinstance(d, bool) or not isinstance(d, (int, np.integer)) for d in setting):
            raise ValueError(f"settings['mi355x']['devices'] = {setting!r}: device indices must be integers")
        devs = [int(d) for d in setting]
    else:
        raise ValueError(f"settings['mi355x']['devices'] = {setting!r}: expected \"first\", \"all\" or a list of device indices")
    bad = [d for d in devs if d < 0 or d >= int(device_count)]
    if bad:
        raise ValueError(f"devices {devs}: {bad} not among the {int(device_count)} visible device(s)")
    if len(devs) > 1 and int(group_world) > 1:
        raise ValueError(f"devices {devs}: this process is one rank of a torch.distributed group of {int(group_world)} - "
                         "each rank runs on one device (its LOCAL_RANK)")
    if len(devs) > MAX_RANKS:
        raise ValueError(f"devices {devs}: at most {MAX_RANKS} ranks per process")
    return devs


def size_filter_bounds(settings, min_size, max_size) -> Optional[Tuple[int, int]]:
    """count_blobs' size filter: None when settings["mi355x"]["size_filter"] is absent or false (the reference accepts
    min_size / max_size and ignores them, and so does count_blobs then), else (lo, hi): a component is kept when
    lo <= voxels <= hi, both inclusive; a negative bound (returned as -1) is no bound, (-1, -1) keeps everything.
    Raises ValueError for min_size > max_size with both >= 0 - only with the switch on: off, the bounds are not looked at."""
    if not ((settings or {}).get("mi355x") or {}).get("size_filter"):
        return None
    lo = -1 if min_size is None else max(int(min_size), -1)
    hi = -1 if max_size is None else max(int(max_size), -1)
    if lo >= 0 and hi >= 0 and lo > hi:
        raise ValueError(f"count_blobs: min_size {lo} > max_size {hi} keeps no component (settings['mi355x']['size_filter'] is on)")
    return lo, hi


INTENSITY_KEYS = ("intensity_sum", "intensity_sumsq", "intensity_min", "intensity_max")  # what HipEngine.cc_intensity returns
INTENSITY_ABSENT_MIN = 0xFFFF  # intensity_min of a label without a voxel (with sum 0, sumsq 0, max 0)


def intensity_stats_enabled(settings) -> bool:
    """count_blobs' per-cell raw intensity statistics: on only for a truthy settings["mi355x"]["intensity_stats"]."""
    return bool(((settings or {}).get("mi355x") or {}).get("intensity_stats"))


def merge_intensity(parts) -> dict:
    """Per-slab dicts of HipEngine.cc_intensity over the same labels 0..n -> the dict of the whole volume: sums add, minima /
    maxima combine (an absent label is 0, 0, 0xFFFF, 0 - the neutral element of all four).  None entries (empty slabs) are
    skipped; with nothing left, or rows that disagree, ValueError."""
    parts = [p for p in parts if p is not None]
    if not parts:
        raise ValueError("merge_intensity: no slab to merge")
    rows = len(parts[0]["intensity_sum"])
    if any(len(p[k]) != rows for p in parts for k in INTENSITY_KEYS):
        raise ValueError("merge_intensity: the slabs do not cover the same labels")
    out = {"intensity_sum": np.zeros(rows, dtype=np.uint64), "intensity_sumsq": np.zeros(rows, dtype=np.uint64),
           "intensity_min": np.full(rows, INTENSITY_ABSENT_MIN, dtype=np.uint16), "intensity_max": np.zeros(rows, dtype=np.uint16)}
    for p in parts:
        out["intensity_sum"] += np.asarray(p["intensity_sum"], dtype=np.uint64)
        out["intensity_sumsq"] += np.asarray(p["intensity_sumsq"], dtype=np.uint64)
        np.minimum(out["intensity_min"], np.asarray(p["intensity_min"], dtype=np.uint16), out=out["intensity_min"])
        np.maximum(out["intensity_max"], np.asarray(p["intensity_max"], dtype=np.uint16), out=out["intensity_max"])
    return out


def finish_intensity(merged: dict, voxel_counts) -> dict:
    """The whole-volume accumulators (HipEngine.cc_intensity / merge_intensity) -> what count_blobs stores: the four arrays with
    row 0's minimum set to 0 (the background is not measured: its row is all zeros) and intensity_mean, float64 sum / count (0.0
    where the count is 0).  A label 1..n that reads as absent (sum 0, sumsq 0, min 0xFFFF, max 0) while cc_stats counted voxels
    for it, or that was measured while its count is 0, means labels and raw volume do not belong together: RuntimeError."""
    counts = np.asarray(voxel_counts)
    out = {k: np.array(merged[k], dtype=np.uint16 if k in ("intensity_min", "intensity_max") else np.uint64) for k in INTENSITY_KEYS}
    rows = len(out["intensity_sum"])
    if len(counts) != rows or rows < 1:
        raise RuntimeError(f"intensity statistics of {rows} rows beside voxel counts of {len(counts)}")
    absent = ((out["intensity_sum"] == 0) & (out["intensity_sumsq"] == 0) & (out["intensity_min"] == INTENSITY_ABSENT_MIN)
              & (out["intensity_max"] == 0))
    bad = np.flatnonzero(absent[1:] != (counts[1:] == 0)) + 1
    if len(bad):
        l = int(bad[0])
        raise RuntimeError(f"intensity statistics and voxel counts disagree on {len(bad)} label(s), first label {l}: "
                           f"{int(counts[l])} voxels counted, {'none' if absent[l] else 'some'} measured - labels and raw volume of different brains?")
    out["intensity_min"][0] = 0
    mean = np.zeros(rows, dtype=np.float64)
    np.divide(out["intensity_sum"].astype(np.float64), counts.astype(np.float64), out=mean, where=counts != 0)
    mean[0] = 0.0  # (row 0's count is the background's, its sum is not taken)
    out["intensity_mean"] = mean
    return out


SHELL_KEYS = ("shell_voxels", "shell_sum", "shell_sumsq", "shell_min", "shell_max", "shell_mean", "contrast")  # finish_shell's keys
SHELL_MAX_RADIUS = 16  # dlv_cc_shell_dev's largest radius


def background_shell_radius(settings) -> int:
    """count_blobs' per-cell local background: 0 when settings["mi355x"]["background_shell"] is absent, false or 0, else the
    shell radius in voxels, an integer 1..16.  ValueError for anything else (true, a float, a string, a value outside the
    range) and for a radius without settings["mi355x"]["intensity_stats"]: the shell is measured beside the cells."""
    value = ((settings or {}).get("mi355x") or {}).get("background_shell")
    if value is None or value is False or (not isinstance(value, bool) and isinstance(value, (int, np.integer)) and int(value) == 0):
        return 0
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= SHELL_MAX_RADIUS:
        raise ValueError(f"settings['mi355x']['background_shell'] = {value!r}: expected a shell radius in voxels, an integer "
                         f"1..{SHELL_MAX_RADIUS} (0 / false: off)")
    if not intensity_stats_enabled(settings):
        raise ValueError(f"settings['mi355x']['background_shell'] = {int(value)} needs settings['mi355x']['intensity_stats']: the shell is "
                         "measured beside the cells")
    return int(value)


def merge_shell(parts):
    """Per-slab (HipEngine.cc_intensity dict of the shell volume, its uint32 voxel counts per label) -> the pair of the whole
    volume: merge_intensity plus a sum of the counts.  None entries (empty slabs) are skipped."""
    parts = [p for p in parts if p is not None]
    merged = merge_intensity([p[0] for p in parts])
    rows = len(merged["intensity_sum"])
    counts = np.zeros(rows, dtype=np.uint64)
    for _, c in parts:
        if len(c) != rows:
            raise ValueError("merge_shell: the slabs do not cover the same labels")
        counts += np.asarray(c, dtype=np.uint64)
    return merged, counts


def finish_shell(parts: dict, shell_counts, intensity_mean) -> dict:
    """The accumulators of the shell volume (HipEngine.cc_intensity on HipEngine.cc_shell's result, or merge_shell's) with the
    shell's voxel counts per label (cc_counts) and the cells' intensity_mean -> what count_blobs stores, N+1 rows each, row 0 all
    zeros: shell_voxels uint32, shell_sum / shell_sumsq uint64, shell_min / shell_max uint16 (0 for a cell without a shell),
    shell_mean float64 = sum / voxels and contrast float64 = intensity_mean / shell_mean (both 0.0 without a shell; a shell
    voxel is not 0 in the raw volume, so the mean of a shell with a voxel is positive).  RuntimeError when a label was measured
    and not counted, or counted and not measured."""
    counts = np.asarray(shell_counts).astype(np.uint64)
    cells = np.asarray(intensity_mean, dtype=np.float64)
    rows = len(counts)
    if rows < 1 or len(cells) != rows or any(len(parts[k]) != rows for k in INTENSITY_KEYS):
        raise RuntimeError(f"shell statistics of {[len(parts[k]) for k in INTENSITY_KEYS]} rows beside shell counts of {rows} and "
                           f"cell means of {len(cells)}")
    if int(counts.max()) > 0xFFFFFFFF:
        raise RuntimeError("a shell of more than 2^32 - 1 voxels")
    counts = counts.copy()
    counts[0] = 0  # (row 0 of cc_counts is the voxels outside every shell)
    s, q = np.array(parts["intensity_sum"], dtype=np.uint64), np.array(parts["intensity_sumsq"], dtype=np.uint64)
    lo, hi = np.array(parts["intensity_min"], dtype=np.uint16), np.array(parts["intensity_max"], dtype=np.uint16)
    absent = (s == 0) & (q == 0) & (lo == INTENSITY_ABSENT_MIN) & (hi == 0)
    bad = np.flatnonzero(absent[1:] != (counts[1:] == 0)) + 1
    if len(bad):
        l = int(bad[0])
        raise RuntimeError(f"shell statistics and shell counts disagree on {len(bad)} label(s), first label {l}: "
                           f"{int(counts[l])} voxels counted, {'none' if absent[l] else 'some'} measured")
    lo[absent] = 0
    for a in (s, q, lo, hi):
        a[0] = 0
    mean = np.zeros(rows, dtype=np.float64)
    np.divide(s.astype(np.float64), counts.astype(np.float64), out=mean, where=counts != 0)
    contrast = np.zeros(rows, dtype=np.float64)
    np.divide(cells, mean, out=contrast, where=counts != 0)
    return {"shell_voxels": counts.astype(np.uint32), "shell_sum": s, "shell_sumsq": q, "shell_min": lo, "shell_max": hi,
            "shell_mean": mean, "contrast": contrast}


QUARTILE_LEVELS = (25, 50, 75)  # the levels count_blobs asks HipEngine.cc_quantiles for
QUARTILE_KEYS = ("intensity_q25", "intensity_median", "intensity_q75")  # finish_quartiles' keys
SHELL_QUARTILE_KEYS = ("shell_q25", "shell_median", "shell_q75", "contrast_median")  # finish_shell_quartiles' keys


def intensity_quartiles_enabled(settings) -> bool:
    """count_blobs' per-cell intensity quartiles: False when settings["mi355x"]["intensity_quartiles"] is absent or false, True
    when it is true.  ValueError for anything but a bool, and for true without settings["mi355x"]["intensity_stats"]: the
    quartiles are taken beside the moment statistics, from the raw tensor uploaded for them."""
    value = ((settings or {}).get("mi355x") or {}).get("intensity_quartiles")
    if value is None or value is False:
        return False
    if value is not True:
        raise ValueError(f"settings['mi355x']['intensity_quartiles'] = {value!r}: expected true or false")
    if not intensity_stats_enabled(settings):
        raise ValueError("settings['mi355x']['intensity_quartiles'] needs settings['mi355x']['intensity_stats']: the quartiles are "
                         "measured beside the cells' moment statistics")
    return True


def _quartile_columns(values, counts, expected, what: str):
    """HipEngine.cc_quantiles' pair for QUARTILE_LEVELS, checked against the voxel counts another kernel took -> three uint16
    columns of N+1 rows, row 0 zero (a label without a voxel reads 0 already)"""
    values = np.asarray(values)
    counts, expected = np.asarray(counts).astype(np.uint64), np.asarray(expected).astype(np.uint64)
    rows = len(expected)
    if rows < 1 or values.shape != (rows, len(QUARTILE_LEVELS)) or len(counts) != rows:
        raise RuntimeError(f"{what} quartiles of shape {values.shape} with {len(counts)} counts beside voxel counts of {rows}")
    bad = np.flatnonzero(counts[1:] != expected[1:]) + 1
    if len(bad):
        l = int(bad[0])
        raise RuntimeError(f"{what} quartiles and voxel counts disagree on {len(bad)} label(s), first label {l}: "
                           f"{int(expected[l])} voxels counted, {int(counts[l])} measured - labels and statistics of different brains?")
    cols = [np.array(values[:, k], dtype=np.uint16) for k in range(len(QUARTILE_LEVELS))]
    for c in cols:
        c[0] = 0
    return cols


def finish_quartiles(values, counts, voxel_counts) -> dict:
    """HipEngine.cc_quantiles' (values, counts) of the final labels for the levels QUARTILE_LEVELS -> what count_blobs stores:
    intensity_q25, intensity_median (the lower median), intensity_q75, uint16, N+1 rows, row 0 zero.  RuntimeError naming the first
    label when the measured counts and voxel_counts[1:] disagree."""
    return dict(zip(QUARTILE_KEYS, _quartile_columns(values, counts, voxel_counts, "intensity")))


def finish_shell_quartiles(values, counts, shell_voxels, intensity_median) -> dict:
    """HipEngine.cc_quantiles' pair of the shell volume with finish_shell's shell_voxels and the cells' intensity_median -> shell_q25,
    shell_median, shell_q75 uint16 (0 for a cell without a shell) and contrast_median float64 = intensity_median / shell_median
    (0.0 without a shell; a shell voxel is not 0 in the raw volume, so the median of a shell with a voxel is positive).
    RuntimeError when the measured counts and shell_voxels[1:] disagree."""
    out = dict(zip(SHELL_QUARTILE_KEYS, _quartile_columns(values, counts, shell_voxels, "shell")))
    cells = np.asarray(intensity_median)
    if len(cells) != len(out["shell_median"]):
        raise RuntimeError(f"shell quartiles of {len(out['shell_median'])} rows beside cell medians of {len(cells)}")
    present = np.asarray(shell_voxels) != 0
    present[0] = False
    contrast = np.zeros(len(cells), dtype=np.float64)
    np.divide(cells.astype(np.float64), out["shell_median"].astype(np.float64), out=contrast, where=present)
    out["contrast_median"] = contrast
    return out


def cell_quartiles_csv_text(stats: dict, n: int) -> str:
    """count_blobs' cell_quartiles/<brain>.csv: header ``Blob,Size,Q25,Median,Q75``, one row per label 1..N - all N, as
    cell_intensity_csv_text - integers written plainly, every line ended by a newline.  With finish_shell_quartiles' keys and
    shell_voxels in `stats` the columns ``ShellSize,ShellQ25,ShellMedian,ShellQ75,ContrastMedian`` follow, the float as repr."""
    n = int(n)
    cols = [np.asarray(stats[k])[1:n + 1].tolist() for k in ("voxel_counts",) + QUARTILE_KEYS]
    shell = all(k in stats for k in SHELL_QUARTILE_KEYS + ("shell_voxels",))
    if shell:
        cols += [np.asarray(stats[k])[1:n + 1].tolist() for k in ("shell_voxels",) + SHELL_QUARTILE_KEYS[:3]]
        cols.append(np.asarray(stats["contrast_median"], dtype=np.float64)[1:n + 1].tolist())
    if any(len(c) != n for c in cols):
        raise ValueError("statistics shorter than the label count")
    if not shell:
        lines = ["Blob,Size,Q25,Median,Q75"]
        lines.extend(f"{i},{c},{a},{b},{d}" for i, (c, a, b, d) in enumerate(zip(*cols), 1))
    else:
        lines = ["Blob,Size,Q25,Median,Q75,ShellSize,ShellQ25,ShellMedian,ShellQ75,ContrastMedian"]
        lines.extend(f"{i},{c},{a},{b},{d},{sc},{sa},{sb},{sd},{ct!r}" for i, (c, a, b, d, sc, sa, sb, sd, ct) in enumerate(zip(*cols), 1))
    return "\n".join(lines) + "\n"


CONFIDENCE_SCALE = 1 << 24  # the fixed point of a probability: q = rint(clamp(p, 0, 1) * CONFIDENCE_SCALE)
CONFIDENCE_RAW_KEYS = ("confidence_sum", "confidence_min_q", "confidence_max_q", "confidence_peak_index")  # what HipEngine.cc_confidence returns
CONFIDENCE_KEYS = ("confidence_sum", "confidence_min", "confidence_max", "confidence_mean", "confidence_peak")  # finish_confidence's keys
CONFIDENCE_ABSENT_MIN = 0xFFFFFFFF  # confidence_min_q of a label without a voxel (with sum 0, max 0 and the peak below)
CONFIDENCE_NO_PEAK = 2**64 - 1  # confidence_peak_index of a label without a voxel
_CONFIDENCE_RAW_DTYPES = (np.uint64, np.uint32, np.uint32, np.uint64)


def confidence_stats_enabled(settings) -> bool:
    """count_blobs' per-cell confidence: False when settings["mi355x"]["confidence_stats"] is absent or false, True when it is
    true.  ValueError for anything but a bool."""
    value = ((settings or {}).get("mi355x") or {}).get("confidence_stats")
    if value is None or value is False:
        return False
    if value is not True:
        raise ValueError(f"settings['mi355x']['confidence_stats'] = {value!r}: expected true or false")
    return True


def quantise_confidence(prob) -> np.ndarray:
    """q(p) of HipEngine.cc_confidence in numpy: uint32 rint(clamp(p, 0, 1) * 2^24) of float32 probabilities, NaN as 0 (the
    product is exact in float32, rint rounds half to even)"""
    p = np.asarray(prob, dtype=np.float32)
    p = np.clip(np.where(np.isnan(p), np.float32(0), p), 0, 1).astype(np.float32)
    return np.rint(p * np.float32(CONFIDENCE_SCALE)).astype(np.uint32)


def merge_confidence(parts) -> dict:
    """Per-slab (HipEngine.cc_confidence dict, lo, plane) over the same labels 0..n - lo: the slab's first plane in the whole
    volume, plane: the voxels Y * X of a plane - -> the dict of the whole volume: sums add, minima / maxima combine, a slab's peak
    index becomes global by adding lo * plane, and of two peaks the larger q wins, the smaller global index on a tie (an absent
    label is 0, 0xFFFFFFFF, 0, 2^64 - 1: it loses against every voxel).  None entries (empty slabs) are skipped; with nothing left,
    or rows that disagree, ValueError."""
    parts = [p for p in parts if p is not None]
    if not parts:
        raise ValueError("merge_confidence: no slab to merge")
    rows = len(parts[0][0]["confidence_sum"])
    if any(len(p[0][k]) != rows for p in parts for k in CONFIDENCE_RAW_KEYS):
        raise ValueError("merge_confidence: the slabs do not cover the same labels")
    total = np.zeros(rows, dtype=np.uint64)
    lo_q = np.full(rows, CONFIDENCE_ABSENT_MIN, dtype=np.uint32)
    hi_q = np.zeros(rows, dtype=np.uint32)
    peak = np.full(rows, CONFIDENCE_NO_PEAK, dtype=np.uint64)
    for part, lo, plane in parts:
        s, mn, mx, idx = (np.asarray(part[k], dtype=dt) for k, dt in zip(CONFIDENCE_RAW_KEYS, _CONFIDENCE_RAW_DTYPES))
        if int(lo) < 0 or int(plane) < 1:
            raise ValueError(f"merge_confidence: a slab that starts at plane {lo} of planes of {plane} voxels")
        there = idx != np.uint64(CONFIDENCE_NO_PEAK)
        glob = np.where(there, idx + np.uint64(int(lo) * int(plane)), np.uint64(CONFIDENCE_NO_PEAK))
        total += s
        np.minimum(lo_q, mn, out=lo_q)
        wins = (mx > hi_q) | ((mx == hi_q) & (glob < peak))
        hi_q = np.where(wins, mx, hi_q)
        peak = np.where(wins, glob, peak)
    return {"confidence_sum": total, "confidence_min_q": lo_q, "confidence_max_q": hi_q, "confidence_peak_index": peak}


def finish_confidence(merged: dict, voxel_counts, shape) -> dict:
    """The whole-volume accumulators (HipEngine.cc_confidence / merge_confidence) of a volume of `shape` (Z, Y, X) -> what count_blobs
    stores, N+1 rows each: confidence_sum uint64 (fixed point: CONFIDENCE_SCALE is 1.0), confidence_min / confidence_max float64 =
    q / 2^24, confidence_mean float64 = sum / (count * 2^24) and confidence_peak int64 (N+1, 3), the z, y, x of the voxel of largest
    probability, the first in raster order on a tie.  Row 0 and a label without a voxel read 0 and a peak of -1.  ValueError when a
    label with voxels has no peak, one without voxels has one, or a peak lies outside the volume: labels and probabilities do not
    belong together."""
    counts = np.asarray(voxel_counts)
    s, mn, mx, idx = (np.array(merged[k], dtype=dt) for k, dt in zip(CONFIDENCE_RAW_KEYS, _CONFIDENCE_RAW_DTYPES))
    Z, Y, X = (int(v) for v in shape)
    rows = len(s)
    if len(counts) != rows or rows < 1 or any(len(a) != rows for a in (mn, mx, idx)):
        raise ValueError(f"confidence statistics of {rows} rows beside voxel counts of {len(counts)}")
    present = idx != np.uint64(CONFIDENCE_NO_PEAK)
    present[0] = False  # (the background is not measured)
    bad = np.flatnonzero(present[1:] != (counts[1:] != 0)) + 1
    if len(bad):
        l = int(bad[0])
        raise ValueError(f"confidence statistics and voxel counts disagree on {len(bad)} label(s), first label {l}: "
                         f"{int(counts[l])} voxels counted, {'a' if present[l] else 'no'} peak measured - labels and probabilities of "
                         "different brains?")
    if present.any() and int(idx[present].max()) >= Z * Y * X:
        raise ValueError(f"a confidence peak at index {int(idx[present].max())} outside the volume of shape {(Z, Y, X)}")
    scale = float(CONFIDENCE_SCALE)
    out_sum = np.where(present, s, 0).astype(np.uint64)
    lo = np.where(present, mn, 0).astype(np.float64) / scale
    hi = np.where(present, mx, 0).astype(np.float64) / scale
    mean = np.zeros(rows, dtype=np.float64)
    np.divide(out_sum.astype(np.float64), counts.astype(np.float64) * scale, out=mean, where=present)
    at = np.where(present, idx, 0).astype(np.int64)
    peak = np.stack([at // (Y * X), (at // X) % Y, at % X], axis=1)
    peak[~present] = -1
    return {"confidence_sum": out_sum, "confidence_min": lo, "confidence_max": hi, "confidence_mean": mean, "confidence_peak": peak}


def cell_confidence_csv_text(stats: dict, n: int) -> str:
    """count_blobs' cell_confidence/<brain>.csv: header ``id,voxels,confidence_mean,confidence_min,confidence_max,peak_z,peak_y,
    peak_x``, one row per label 1..N - all N, as cell_intensity_csv_text - integers written plainly, floats as repr of the float64
    value, every line ended by a newline."""
    n = int(n)
    counts = np.asarray(stats["voxel_counts"])[1:n + 1].tolist()
    floats = [np.asarray(stats[k], dtype=np.float64)[1:n + 1].tolist() for k in ("confidence_mean", "confidence_min", "confidence_max")]
    peak = np.asarray(stats["confidence_peak"], dtype=np.int64)[1:n + 1].tolist()
    if any(len(c) != n for c in [counts, peak] + floats):
        raise ValueError("statistics shorter than the label count")
    lines = ["id,voxels,confidence_mean,confidence_min,confidence_max,peak_z,peak_y,peak_x"]
    lines.extend(f"{i},{c},{m!r},{lo!r},{hi!r},{z},{y},{x}" for i, (c, m, lo, hi, (z, y, x)) in enumerate(zip(counts, *floats, peak), 1))
    return "\n".join(lines) + "\n"


SPLIT_KEYS = ("split_parent", "split_siblings")  # finish_split's keys
SPLIT_MAX_DEPTH = 16  # dlv_cc_split_dev's largest depth


def _is_integral(value) -> bool:
    """an int, a numpy integer or a float with an integral value - never a bool"""
    if isinstance(value, bool):
        return False
    if isinstance(value, (int, np.integer)):
        return True
    return isinstance(value, (float, np.floating)) and np.isfinite(value) and float(value) == int(value)


def split_fused_settings(settings):
    """count_blobs' split of fused cells: None when settings["mi355x"]["split_fused"] is absent, false or 0, else
    (depth, min_core): the erosion depth, an integer 1..16, and settings["mi355x"]["split_min_core"], the smallest core in voxels,
    an integer >= 1 (default 1).  ValueError for anything else (true, a float that is not integral, a string, a value outside the
    range) and for split_min_core without split_fused - unless split_radius or split_fraction is there, whose split it then belongs
    to (split_depth_settings)."""
    mi = (settings or {}).get("mi355x") or {}
    value, min_core = mi.get("split_fused"), mi.get("split_min_core")
    off = value is None or value is False or (_is_integral(value) and int(value) == 0)
    if not off and (not _is_integral(value) or not 1 <= int(value) <= SPLIT_MAX_DEPTH):
        raise ValueError(f"settings['mi355x']['split_fused'] = {value!r}: expected an erosion depth in voxels, an integer "
                         f"1..{SPLIT_MAX_DEPTH} (0 / false: off)")
    if min_core is not None and (not _is_integral(min_core) or int(min_core) < 1):
        raise ValueError(f"settings['mi355x']['split_min_core'] = {min_core!r}: expected the smallest core in voxels, an integer >= 1")
    if off:
        if min_core is not None and mi.get("split_radius") is None and mi.get("split_fraction") is None:
            raise ValueError(f"settings['mi355x']['split_min_core'] = {min_core!r} needs settings['mi355x']['split_fused']: it is the "
                             "smallest core the split counts")
        return None
    return int(value), 1 if min_core is None else int(min_core)


SPLIT_MAX_CORE_D2 = 2**32 - 1  # dlv_cc_split_depth_dev's core_d2 is a uint32


def split_depth_settings(settings):
    """count_blobs' split of fused cells by Euclidean depth cores: None when settings["mi355x"] holds neither "split_radius" nor
    "split_fraction", else (core_d2, fraction, min_core, spacing).  split_radius = r, an int or a float above 0 in the unit of
    depth_spacing: a core voxel lies at least r from the outside of its cell, core_d2 = ceil(r * r) (0 without the key).
    split_fraction = p, an integer 1..99: ... and at least p per cent of its cell's inscribed radius (0 without the key).  min_core:
    split_min_core, as for split_fused.  spacing: depth_spacing = [wz, wy, wx], three integers 1..64 (default [1, 1, 1]).
    ValueError for anything else (a bool, a radius that is not finite or whose square exceeds 2^32 - 1) and for either key together
    with split_fused: the two splits are alternatives."""
    mi = (settings or {}).get("mi355x") or {}
    radius, fraction, min_core = mi.get("split_radius"), mi.get("split_fraction"), mi.get("split_min_core")
    if radius is None and fraction is None:
        return None
    core_d2 = 0
    if radius is not None:
        if (isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or not np.isfinite(radius)
                or not radius > 0):
            raise ValueError(f"settings['mi355x']['split_radius'] = {radius!r}: expected the distance of a core voxel from the outside "
                             "of its cell, a number above 0 in the unit of depth_spacing")
        core_d2 = int(math.ceil(float(radius) * float(radius))) if isinstance(radius, (float, np.floating)) else int(radius) ** 2
        if core_d2 > SPLIT_MAX_CORE_D2:
            raise ValueError(f"settings['mi355x']['split_radius'] = {radius!r}: its square, {core_d2}, exceeds {SPLIT_MAX_CORE_D2}")
    if fraction is not None and (not _is_integral(fraction) or not 1 <= int(fraction) <= 99):
        raise ValueError(f"settings['mi355x']['split_fraction'] = {fraction!r}: expected a percentage of the cell's inscribed radius, "
                         "an integer 1..99")
    if min_core is not None and (not _is_integral(min_core) or int(min_core) < 1):
        raise ValueError(f"settings['mi355x']['split_min_core'] = {min_core!r}: expected the smallest core in voxels, an integer >= 1")
    if split_fused_settings(settings) is not None:
        key = "split_radius" if radius is not None else "split_fraction"
        raise ValueError(f"settings['mi355x']['split_fused'] = {mi.get('split_fused')!r} and settings['mi355x']['{key}'] = {mi.get(key)!r} "
                         "are alternatives: erosion cores counted in voxels, or depth cores in the unit of depth_spacing; give one")
    spacing = _depth_spacing(mi)
    return (core_d2, 0 if fraction is None else int(fraction), 1 if min_core is None else int(min_core),
            (1, 1, 1) if spacing is None else spacing)


def finish_split(parent, n_before: int) -> dict:
    """HipEngine.cc_split's parent table (K+1 rows: parent[j] = the label piece j was cut from, 1..n_before; parent[0] = 0) -> what
    count_blobs stores, K+1 rows each, row 0 zero: split_parent uint32 and split_siblings uint32 = the number of pieces with the
    same parent (1 for a cell that was not split).  ValueError for a table without row 0 or with a parent outside 1..n_before."""
    parent = np.array(parent, dtype=np.uint32).reshape(-1)
    n_before = int(n_before)
    if len(parent) < 1 or parent[0] != 0:
        raise ValueError("finish_split: the parent table needs a row 0 that is 0")
    if len(parent) > 1 and (int(parent[1:].min()) < 1 or int(parent[1:].max()) > n_before):
        raise ValueError(f"finish_split: a parent outside 1..{n_before}")
    pieces = np.bincount(parent[1:], minlength=n_before + 1)
    siblings = pieces[parent].astype(np.uint32)
    siblings[0] = 0
    return {"split_parent": parent, "split_siblings": siblings}


def cell_intensity_csv_text(stats: dict, n: int) -> str:
    """count_blobs' cell_intensity/<brain>.csv: header ``Blob,Size,Min,Max,Sum,SumSq,Mean``, one row per label 1..N - all N:
    this table has no reference to mirror, so none of its quirks (cells_csv_text drops the last label) - integers written
    plainly, Mean as repr of the float64 value, every line ended by a newline.  With finish_shell's keys in `stats` (all of
    them) the columns ``ShellSize,ShellMin,ShellMax,ShellSum,ShellSumSq,ShellMean,Contrast`` follow Mean, floats as repr."""
    n = int(n)
    cols = [np.asarray(stats[k])[1:n + 1].tolist() for k in ("voxel_counts", "intensity_min", "intensity_max", "intensity_sum",
                                                              "intensity_sumsq")]
    mean = np.asarray(stats["intensity_mean"], dtype=np.float64)[1:n + 1].tolist()
    if any(len(c) != n for c in cols) or len(mean) != n:
        raise ValueError("statistics shorter than the label count")
    if not all(k in stats for k in SHELL_KEYS):
        lines = ["Blob,Size,Min,Max,Sum,SumSq,Mean"]
        lines.extend(f"{i},{c},{lo},{hi},{s},{q},{m!r}" for i, (c, lo, hi, s, q, m) in enumerate(zip(*cols, mean), 1))
        return "\n".join(lines) + "\n"
    cols += [np.asarray(stats[k])[1:n + 1].tolist() for k in ("shell_voxels", "shell_min", "shell_max", "shell_sum", "shell_sumsq")]
    floats = [np.asarray(stats[k], dtype=np.float64)[1:n + 1].tolist() for k in ("shell_mean", "contrast")]
    if any(len(c) != n for c in cols + floats):
        raise ValueError("statistics shorter than the label count")
    lines = ["Blob,Size,Min,Max,Sum,SumSq,Mean,ShellSize,ShellMin,ShellMax,ShellSum,ShellSumSq,ShellMean,Contrast"]
    lines.extend(f"{i},{c},{lo},{hi},{s},{q},{m!r},{sc},{slo},{shi},{ss},{sq},{sm!r},{ct!r}"
                 for i, (c, lo, hi, s, q, sc, slo, shi, ss, sq, m, sm, ct) in enumerate(zip(*cols, mean, *floats), 1))
    return "\n".join(lines) + "\n"


SHAPE_RAW_KEYS = ("shape_counts", "shape_sums", "shape_moments", "shape_faces", "shape_surface_voxels")  # what HipEngine.cc_shape returns
SHAPE_KEYS = ("shape_sums", "shape_moments", "shape_faces", "shape_surface_voxels", "shape_covariance", "shape_axes",
              "shape_elongation", "shape_sphericity")  # finish_shape's keys
_SHAPE_RAW_LAYOUT = {"shape_counts": (np.uint32, ()), "shape_sums": (np.uint64, (3,)), "shape_moments": (np.uint64, (6,)),
                     "shape_faces": (np.uint64, (3,)), "shape_surface_voxels": (np.uint32, ())}
_MOMENT_AXES = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # zz, yy, xx, zy, zx, yx


def shape_stats_enabled(settings) -> bool:
    """count_blobs' per-cell shape statistics: on only for a truthy settings["mi355x"]["shape_stats"]."""
    return bool(((settings or {}).get("mi355x") or {}).get("shape_stats"))


def merge_shape(parts) -> dict:
    """Per-slab dicts of HipEngine.cc_shape over the same labels 0..n -> the dict of the whole volume: every array adds (an absent
    label is all zero).  None entries (empty slabs) are skipped; with nothing left, or rows that disagree, ValueError."""
    parts = [p for p in parts if p is not None]
    if not parts:
        raise ValueError("merge_shape: no slab to merge")
    rows = len(parts[0]["shape_counts"])
    if any(np.shape(p[k]) != (rows,) + _SHAPE_RAW_LAYOUT[k][1] for p in parts for k in SHAPE_RAW_KEYS):
        raise ValueError("merge_shape: the slabs do not cover the same labels")
    out = {k: np.zeros((rows,) + tail, dtype=dt) for k, (dt, tail) in _SHAPE_RAW_LAYOUT.items()}
    for p in parts:
        for k, (dt, _) in _SHAPE_RAW_LAYOUT.items():
            out[k] += np.asarray(p[k], dtype=dt)
    return out


def _shape_numerators(n: np.ndarray, S: np.ndarray, M: np.ndarray) -> np.ndarray:
    """n * S_ab - S_a * S_b per label and moment as float64, each the exact integer rounded once.  The sums are shifted to the
    origin o = floor(centroid) in wrapping uint64 arithmetic: S'_a = S_a - n o_a lies in [0, n), S'_aa = sum (a - o_a)^2 is below
    2^64 and so exact, and the numerator does not depend on the origin.  While n * max S'_aa + n^2 stays below 2^62 - every real
    cell - the wrapped numerator read as int64 is the true one (|S'_ab| <= max S'_aa by Cauchy-Schwarz); the other labels are
    recomputed with Python integers."""
    nn = np.where(n == 0, 1, n).astype(np.uint64)
    o = S // nn[:, None]
    Ss = S - nn[:, None] * o
    num = np.empty(M.shape, dtype=np.float64)
    diag_max = np.zeros(len(n), dtype=np.float64)
    for j, (a, b) in enumerate(_MOMENT_AXES):
        Ms = M[:, j] - o[:, a] * S[:, b] - o[:, b] * S[:, a] + nn * o[:, a] * o[:, b]
        if a == b:
            np.maximum(diag_max, Ms.astype(np.float64), out=diag_max)
        num[:, j] = (nn * Ms - Ss[:, a] * Ss[:, b]).view(np.int64).astype(np.float64)
    nf = nn.astype(np.float64)
    for l in np.flatnonzero(nf * diag_max * (1 + 2.0**-50) + nf * nf >= 2.0**62).tolist():
        k, s, m = int(n[l]), [int(v) for v in S[l]], [int(v) for v in M[l]]
        num[l] = [float(k * m[j] - s[a] * s[b]) for j, (a, b) in enumerate(_MOMENT_AXES)]
    num[n == 0] = 0.0
    return num


def finish_shape(merged: dict, voxel_counts) -> dict:
    """The whole-volume accumulators (HipEngine.cc_shape / merge_shape) -> what count_blobs stores, N+1 rows each, row 0 all zero:
    shape_sums, shape_moments, shape_faces uint64 and shape_surface_voxels uint32, the exact integers, and
      shape_covariance  float64 (N+1, 6), order zz, yy, xx, zy, zx, yx: (n S_ab - S_a S_b) / n^2, plus 1/12 on zz, yy, xx - the
                        covariance of the solid made of the cell's unit cubes (a single voxel is not degenerate).  The numerator
                        is exact, converted to float64 once and divided once;
      shape_axes        float64 (N+1, 3): the eigenvalues of that covariance, descending (np.linalg.eigvalsh), clipped below at 0;
      shape_elongation  sqrt(axes[:, 0] / axes[:, 2]), at least 1, finite because of the 1/12;
      shape_sphericity  pi^(1/3) (6 n)^(2/3) / (faces_z + faces_y + faces_x): the area is the DIGITAL face count, not a smooth
                        surface estimate, so a cube of any size gives (pi/6)^(1/3) ~ 0.806 and a digital ball about 2/3.
    A label without a voxel has zeros everywhere.  RuntimeError when the measured counts of the labels 1..N differ from
    voxel_counts: labels and statistics do not belong together."""
    counts = np.asarray(voxel_counts)
    raw = {k: np.array(merged[k], dtype=dt) for k, (dt, _) in _SHAPE_RAW_LAYOUT.items()}
    rows = len(raw["shape_counts"])
    if len(counts) != rows or rows < 1 or any(raw[k].shape != (rows,) + tail for k, (_, tail) in _SHAPE_RAW_LAYOUT.items()):
        raise RuntimeError(f"shape statistics of {rows} rows beside voxel counts of {len(counts)}")
    bad = np.flatnonzero(raw["shape_counts"][1:] != counts[1:]) + 1
    if len(bad):
        l = int(bad[0])
        raise RuntimeError(f"shape statistics and voxel counts disagree on {len(bad)} label(s), first label {l}: "
                           f"{int(counts[l])} voxels counted, {int(raw['shape_counts'][l])} measured - labels and statistics of "
                           "different brains?")
    n = raw.pop("shape_counts").astype(np.uint64)
    n[0] = 0
    for a in raw.values():
        a[0] = 0
    present = n != 0
    nf = np.where(present, n, 1).astype(np.float64)
    cov = _shape_numerators(n, raw["shape_sums"], raw["shape_moments"]) / (nf * nf)[:, None]
    cov[:, :3] += 1.0 / 12.0
    cov[~present] = 0.0
    mat = np.empty((rows, 3, 3), dtype=np.float64)
    for j, (a, b) in enumerate(_MOMENT_AXES):
        mat[:, a, b] = mat[:, b, a] = cov[:, j]
    axes = np.maximum(np.linalg.eigvalsh(mat)[:, ::-1], 0.0)
    elong = np.zeros(rows, dtype=np.float64)
    np.sqrt(np.divide(axes[:, 0], axes[:, 2], out=elong, where=present), out=elong)
    area = raw["shape_faces"].sum(axis=1).astype(np.float64)
    spher = np.zeros(rows, dtype=np.float64)
    np.divide(np.pi ** (1.0 / 3.0) * (6.0 * nf) ** (2.0 / 3.0), area, out=spher, where=present & (area > 0))
    return {**raw, "shape_covariance": cov, "shape_axes": np.ascontiguousarray(axes), "shape_elongation": elong,
            "shape_sphericity": spher}


def cell_shape_csv_text(stats: dict, n: int) -> str:
    """count_blobs' cell_shape/<brain>.csv: header ``Blob,Size,FacesZ,FacesY,FacesX,SurfaceVoxels,VarMajor,VarMid,VarMinor,
    Elongation,Sphericity``, one row per label 1..N - all N, as cell_intensity_csv_text - integers written plainly, floats as
    repr of the float64 value, every line ended by a newline."""
    n = int(n)
    ints = [np.asarray(stats["voxel_counts"])[1:n + 1].tolist()]
    ints += [np.asarray(stats["shape_faces"])[1:n + 1, k].tolist() for k in range(3)]
    ints.append(np.asarray(stats["shape_surface_voxels"])[1:n + 1].tolist())
    floats = [np.asarray(stats["shape_axes"], dtype=np.float64)[1:n + 1, k].tolist() for k in range(3)]
    floats += [np.asarray(stats[k], dtype=np.float64)[1:n + 1].tolist() for k in ("shape_elongation", "shape_sphericity")]
    if any(len(c) != n for c in ints + floats):
        raise ValueError("statistics shorter than the label count")
    lines = ["Blob,Size,FacesZ,FacesY,FacesX,SurfaceVoxels,VarMajor,VarMid,VarMinor,Elongation,Sphericity"]
    lines.extend(f"{i},{c},{fz},{fy},{fx},{sv},{a0!r},{a1!r},{a2!r},{el!r},{sp!r}"
                 for i, (c, fz, fy, fx, sv, a0, a1, a2, el, sp) in enumerate(zip(*ints, *floats), 1))
    return "\n".join(lines) + "\n"


DEPTH_RAW_KEYS = ("depth_max_sq", "depth_sum_sq", "depth_peak_index")  # what HipEngine.cc_depth returns
DEPTH_KEYS = DEPTH_RAW_KEYS + ("depth_radius", "depth_mean_sq", "depth_peak", "depth_spacing")  # finish_depth's keys
DEPTH_NO_PEAK = 2**64 - 1  # depth_peak_index of a label without a voxel
DEPTH_MAX_SPACING = 64  # dlv_cc_depth_dev's largest spacing
_DEPTH_RAW_DTYPES = (np.uint32, np.uint64, np.uint64)


def _depth_spacing(mi):
    """settings["mi355x"]["depth_spacing"] as a tuple (wz, wy, wx), None without the key; ValueError for anything but three integers
    1..64"""
    spacing = mi.get("depth_spacing")
    if spacing is None:
        return None
    if (not isinstance(spacing, (list, tuple)) or len(spacing) != 3
            or any(isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 1 <= int(w) <= DEPTH_MAX_SPACING for w in spacing)):
        raise ValueError(f"settings['mi355x']['depth_spacing'] = {spacing!r}: expected the voxel spacing [wz, wy, wx], three "
                         f"integers 1..{DEPTH_MAX_SPACING}")
    return tuple(int(w) for w in spacing)


def depth_stats_settings(settings):
    """count_blobs' per-cell depth: None when settings["mi355x"]["depth_stats"] is absent or false, else the voxel spacing
    (wz, wy, wx) of the distance map: settings["mi355x"]["depth_spacing"], three integers 1..64 (default [1, 1, 1]).  ValueError for
    a depth_stats that is not a bool, for a spacing that is anything else (a bool, a float, two values, a value outside the range)
    and for depth_spacing without depth_stats - unless split_radius, split_fraction or neighbour_stats is there, which measure with it
    too."""
    mi = (settings or {}).get("mi355x") or {}
    value = mi.get("depth_stats")
    if value is not None and value is not True and value is not False:
        raise ValueError(f"settings['mi355x']['depth_stats'] = {value!r}: expected true or false")
    spacing = _depth_spacing(mi)
    if not value:
        # (split_radius / split_fraction / neighbour_stats measure with the same spacing: split_depth_settings, neighbour_stats_settings)
        if spacing is not None and mi.get("split_radius") is None and mi.get("split_fraction") is None and not _neighbour_stats_given(mi):
            raise ValueError(f"settings['mi355x']['depth_spacing'] = {mi.get('depth_spacing')!r} needs settings['mi355x']['depth_stats']: "
                             "it is the voxel spacing of the depth map")
        return None
    return (1, 1, 1) if spacing is None else spacing


def finish_depth(raw: dict, voxel_counts, shape, spacing) -> dict:
    """HipEngine.cc_depth's arrays of a volume of `shape` (Z, Y, X), measured with `spacing` (wz, wy, wx) -> what count_blobs stores,
    N+1 rows each, row 0 zero: depth_max_sq uint32, depth_sum_sq uint64 and depth_peak_index uint64, the exact integers (the
    squared distances are in spacing units); depth_radius float64 = sqrt(depth_max_sq), the radius of the largest ball inscribed in
    the cell, one rounding; depth_mean_sq float64 = depth_sum_sq / voxel_count; depth_peak int64 (N+1, 3), the z, y, x of the
    deepest voxel - always a voxel of the cell, the first in raster order on a tie; depth_spacing, the tuple.  A label without a
    voxel has zeros everywhere.  RuntimeError for rows that do not match the voxel counts, for a label 1..N with voxels but no peak
    (or a peak without voxels) and for a peak outside the volume: labels and statistics do not belong together."""
    counts = np.asarray(voxel_counts)
    mx, sm, idx = (np.array(raw[k], dtype=dt) for k, dt in zip(DEPTH_RAW_KEYS, _DEPTH_RAW_DTYPES))
    Z, Y, X = (int(v) for v in shape)
    rows = len(mx)
    if rows < 1 or len(counts) != rows or mx.shape != (rows,) or sm.shape != (rows,) or idx.shape != (rows,):
        raise RuntimeError(f"depth statistics of {rows} rows beside voxel counts of {len(counts)}")
    present = idx != np.uint64(DEPTH_NO_PEAK)
    present[0] = False
    bad = np.flatnonzero(present[1:] != (counts[1:] != 0)) + 1
    if len(bad):
        l = int(bad[0])
        raise RuntimeError(f"depth statistics and voxel counts disagree on {len(bad)} label(s), first label {l}: "
                           f"{int(counts[l])} voxels counted, {'a' if present[l] else 'no'} deepest voxel measured - labels and "
                           "statistics of different brains?")
    if present.any() and int(idx[present].max()) >= Z * Y * X:
        raise RuntimeError(f"a depth peak at index {int(idx[present].max())} outside the volume of shape {(Z, Y, X)}")
    mx[~present] = 0
    sm[~present] = 0
    idx[~present] = 0
    radius = np.sqrt(mx.astype(np.float64))
    mean = np.zeros(rows, dtype=np.float64)
    np.divide(sm.astype(np.float64), counts.astype(np.float64), out=mean, where=present)
    peak = np.stack(np.unravel_index(idx.astype(np.int64), (Z, Y, X)), axis=1).astype(np.int64)
    return {"depth_max_sq": mx, "depth_sum_sq": sm, "depth_peak_index": idx, "depth_radius": radius, "depth_mean_sq": mean,
            "depth_peak": peak, "depth_spacing": tuple(int(w) for w in spacing)}


def cell_depth_csv_text(stats: dict, n: int) -> str:
    """count_blobs' cell_depth/<brain>.csv: header ``Blob,Size,Radius,MeanSqDepth,PeakZ,PeakY,PeakX``, one row per label 1..N - all
    N, as cell_intensity_csv_text - integers written plainly, floats as repr of the float64 value, every line ended by a newline."""
    n = int(n)
    counts = np.asarray(stats["voxel_counts"])[1:n + 1].tolist()
    floats = [np.asarray(stats[k], dtype=np.float64)[1:n + 1].tolist() for k in ("depth_radius", "depth_mean_sq")]
    peak = np.asarray(stats["depth_peak"], dtype=np.int64)[1:n + 1].tolist()
    if any(len(c) != n for c in [counts, peak] + floats):
        raise ValueError("statistics shorter than the label count")
    lines = ["Blob,Size,Radius,MeanSqDepth,PeakZ,PeakY,PeakX"]
    lines.extend(f"{i},{c},{r!r},{m!r},{z},{y},{x}" for i, (c, r, m, (z, y, x)) in enumerate(zip(counts, *floats, peak), 1))
    return "\n".join(lines) + "\n"

NEIGHBOUR_KEYS = ("neighbour_pairs", "neighbour_gap_sq", "neighbour_radius_sq", "neighbour_spacing", "neighbour_count", "nearest_gap_sq",
                  "nearest_cell", "cluster_id", "cluster_size")  # what settings["mi355x"]["neighbour_stats"] adds to the statistics
NEIGHBOUR_MAX_REACH = 8  # dlv_cc_neighbours_dev's largest reach in voxels along an axis (NB_MAX_REACH of csrc/cc_neighbours.hip)


def _neighbour_stats_given(mi) -> bool:
    """settings["mi355x"]["neighbour_stats"] is there and not switched off (absent, false or 0)"""
    value = mi.get("neighbour_stats")
    return value is not None and value is not False and not (_is_number(value) and value == 0)


def _is_number(value) -> bool:
    return not isinstance(value, (bool, np.bool_)) and isinstance(value, (int, float, np.integer, np.floating))


def neighbour_reach(radius_sq: int, spacing, what: str) -> Tuple[int, int, int]:
    """The reach of a squared radius along z, y, x in voxels, floor(sqrt(radius_sq) / w); ValueError, starting with `what` and naming
    the axis, its reach and the limit, where one exceeds NEIGHBOUR_MAX_REACH."""
    root = math.isqrt(int(radius_sq))
    reach = tuple(root // int(w) for w in spacing)
    for axis, w, rho in zip("zyx", spacing, reach):
        if rho > NEIGHBOUR_MAX_REACH:
            raise ValueError(f"{what} = {int(radius_sq)} over a spacing of {int(w)} reaches {rho} voxels along {axis}, this version "
                             f"supports a reach of at most {NEIGHBOUR_MAX_REACH} voxels on every axis; take a smaller radius")
    return reach


def neighbour_stats_settings(settings):
    """count_blobs' cell neighbourhoods: None when settings["mi355x"]["neighbour_stats"] is absent, false or 0, else
    (R2, (wz, wy, wx)): the key is the radius r, a number above 0 in the unit of depth_spacing - two cells are neighbours when a voxel
    of one lies within r of a voxel of the other -, R2 = floor(r * r), and the spacing is settings["mi355x"]["depth_spacing"], three
    integers 1..64 (default [1, 1, 1]).  ValueError, naming the key, for anything but such a number (a bool, a string, a negative
    or non-finite value), for a radius below one spacing unit (R2 = 0: no two voxels are that close), for a bad spacing and for a
    radius that reaches more than NEIGHBOUR_MAX_REACH voxels along an axis."""
    mi = (settings or {}).get("mi355x") or {}
    value = mi.get("neighbour_stats")
    if not _neighbour_stats_given(mi):
        return None
    key = "settings['mi355x']['neighbour_stats']"
    if not _is_number(value) or not math.isfinite(float(value)) or value < 0:
        raise ValueError(f"{key} = {value!r}: expected the radius within which two cells are neighbours, a number above 0 in the unit "
                         "of depth_spacing (0 / false: off)")
    radius_sq = math.floor(float(value) * float(value)) if isinstance(value, (float, np.floating)) else int(value) * int(value)
    if radius_sq < 1:
        raise ValueError(f"{key} = {value!r}: a radius below one spacing unit finds no pair of voxels; expected at least 1")
    spacing = _depth_spacing(mi)
    spacing = (1, 1, 1) if spacing is None else spacing
    neighbour_reach(radius_sq, spacing, f"{key} = {value!r}: the squared radius")
    return radius_sq, spacing


def neighbour_summary(pairs, gap_sq, n: int) -> dict:
    """The per-cell rows of a neighbour table, host numpy work with no GPU.  pairs: (P, 2) labels a < b in 1..n, unique; gap_sq: (P)
    their squared gaps, all >= 1.  -> N+1 rows each, row 0 zero: neighbour_count uint32, the degree of the cell in the graph;
    nearest_gap_sq uint32, its smallest gap (0: no neighbour); nearest_cell uint32, the partner at that gap, the smallest label on a
    tie (0: none); cluster_id uint32, the connected components of the graph numbered 1.. in the order of their smallest member (a
    cell without a neighbour is a cluster of its own); cluster_size uint32, the cells of its cluster."""
    n = int(n)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    gaps = np.asarray(gap_sq, dtype=np.int64).reshape(-1)
    if len(gaps) != len(pairs):
        raise ValueError(f"neighbour_summary: {len(pairs)} pairs beside {len(gaps)} gaps")
    if len(pairs) and (pairs.min() < 1 or pairs.max() > n or (pairs[:, 0] >= pairs[:, 1]).any() or gaps.min() < 1):
        raise ValueError(f"neighbour_summary: expected pairs a < b of labels 1..{n} with gaps >= 1")
    src = np.concatenate([pairs[:, 0], pairs[:, 1]])
    dst = np.concatenate([pairs[:, 1], pairs[:, 0]])
    gap = np.concatenate([gaps, gaps])
    count = np.bincount(src, minlength=n + 1).astype(np.uint32)
    nearest_gap, nearest_cell = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    order = np.lexsort((dst, gap, src))  # by cell, then gap, then partner: the first row of a cell is its nearest
    cells, first = np.unique(src[order], return_index=True)
    nearest_gap[cells] = gap[order][first]
    nearest_cell[cells] = dst[order][first]
    cluster_id = np.zeros(n + 1, dtype=np.uint32)
    if n > 0:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components

        graph = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0] - 1, pairs[:, 1] - 1)), shape=(n, n))
        _, comp = connected_components(graph, directed=False)
        # (numbered in the order of their smallest member: of the first cell that belongs to them)
        _, first_cell, inverse = np.unique(comp, return_index=True, return_inverse=True)
        rank = np.empty(len(first_cell), dtype=np.int64)
        rank[np.argsort(first_cell, kind="stable")] = np.arange(1, len(first_cell) + 1)
        cluster_id[1:] = rank[inverse.reshape(-1)]
    sizes = np.bincount(cluster_id, minlength=1)
    sizes[0] = 0
    return {"neighbour_count": count, "nearest_gap_sq": nearest_gap, "nearest_cell": nearest_cell, "cluster_id": cluster_id,
            "cluster_size": sizes[cluster_id].astype(np.uint32)}


def finish_neighbours(table: dict, n: int, radius_sq: int, spacing) -> dict:
    """HipEngine.cc_neighbours' table of the labels 1..n, taken with `radius_sq` and `spacing` -> what count_blobs stores
    (NEIGHBOUR_KEYS): neighbour_pairs uint32 (P, 2), a < b, sorted by (a, b); neighbour_gap_sq uint32 (P); neighbour_radius_sq and
    neighbour_spacing, how they were measured; and neighbour_summary's per-cell rows."""
    pairs = np.stack([np.asarray(table["a"], dtype=np.uint32), np.asarray(table["b"], dtype=np.uint32)], axis=1)
    gaps = np.ascontiguousarray(table["gap_sq"], dtype=np.uint32)
    out = {"neighbour_pairs": pairs, "neighbour_gap_sq": gaps, "neighbour_radius_sq": int(radius_sq),
           "neighbour_spacing": tuple(int(w) for w in spacing)}
    out.update(neighbour_summary(pairs, gaps, n))
    return out


def cell_neighbours_csv_text(stats: dict, n: int) -> str:
    """count_blobs' cell_neighbours/<brain>.csv: header ``Blob,Size,Neighbours,NearestCell,NearestGapSq,NearestGap,Cluster,ClusterSize``,
    one row per label 1..N - all N, as cell_depth_csv_text - integers written plainly, NearestGap = sqrt(NearestGapSq) as repr of the
    float64 value (as depth_radius; 0.0 for a cell without a neighbour), every line ended by a newline."""
    n = int(n)
    ints = [np.asarray(stats[k])[1:n + 1].tolist() for k in ("voxel_counts", "neighbour_count", "nearest_cell", "nearest_gap_sq",
                                                             "cluster_id", "cluster_size")]
    gap = np.sqrt(np.asarray(stats["nearest_gap_sq"], dtype=np.float64))[1:n + 1].tolist()
    if any(len(c) != n for c in ints + [gap]):
        raise ValueError("statistics shorter than the label count")
    lines = ["Blob,Size,Neighbours,NearestCell,NearestGapSq,NearestGap,Cluster,ClusterSize"]
    lines.extend(f"{i},{c},{k},{nc},{g2},{g!r},{ci},{cs}" for i, (c, k, nc, g2, ci, cs, g) in enumerate(zip(*ints, gap), 1))
    return "\n".join(lines) + "\n"


def cell_pairs_csv_text(stats: dict) -> str:
    """count_blobs' cell_pairs/<brain>.csv: header ``BlobA,BlobB,GapSq,Gap``, one row per pair of neighbour_pairs in its order (sorted
    by (a, b)); Gap = sqrt(GapSq) as repr of the float64 value."""
    pairs = np.asarray(stats["neighbour_pairs"]).reshape(-1, 2).tolist()
    gaps = np.asarray(stats["neighbour_gap_sq"])
    if len(gaps) != len(pairs):
        raise ValueError("neighbour pairs and gaps of different lengths")
    roots = np.sqrt(gaps.astype(np.float64)).tolist()
    lines = ["BlobA,BlobB,GapSq,Gap"]
    lines.extend(f"{a},{b},{g2},{g!r}" for (a, b), g2, g in zip(pairs, gaps.tolist(), roots))
    return "\n".join(lines) + "\n"


def fill_holes_enabled(settings) -> bool:
    """count_blobs' hole filling of the cell mask: False when settings["mi355x"]["fill_holes"] is absent or false, True when it is
    true.  ValueError for anything but a bool."""
    value = ((settings or {}).get("mi355x") or {}).get("fill_holes")
    if value is None or value is False:
        return False
    if value is not True:
        raise ValueError(f"settings['mi355x']['fill_holes'] = {value!r}: expected true or false")
    return True


HOLE_KEYS = ("hole_voxels", "holes_filled")  # what settings["mi355x"]["fill_holes"] adds to the statistics
FILL_VALUE = 2  # the byte count_blobs' fill writes into the mask in HBM: binaries.npy holds 0 and 1


def cell_holes_csv_text(stats: dict, n: int) -> str:
    """The table of settings["mi355x"]["fill_holes"], one row per label 1..n: the cell's size after the fill and the voxels the
    fill added to it."""
    n = int(n)
    cols = [np.asarray(stats[k])[1:n + 1].tolist() for k in ("voxel_counts", "hole_voxels")]
    if any(len(c) != n for c in cols):
        raise ValueError("statistics shorter than the label count")
    lines = ["Blob,Size,HoleVoxels"]
    lines.extend(f"{i},{c},{h}" for i, (c, h) in enumerate(zip(*cols), 1))
    return "\n".join(lines) + "\n"


LABEL_FILE_FORMATS = ("dense", "runs")


def label_file_format(settings) -> str:
    """settings["mi355x"]["label_file"]: "dense" (or absent) - the reference's <brain>-<N>-cc3d.npy; "runs" - the run-length file
    <brain>-<N>-cc3d.runs (label_runs.py) in its place.  ValueError for anything else."""
    value = ((settings or {}).get("mi355x") or {}).get("label_file")
    if value is None:
        return "dense"
    if not isinstance(value, str) or value not in LABEL_FILE_FORMATS:
        raise ValueError(f"settings['mi355x']['label_file'] = {value!r}: expected \"dense\" (the default: the reference's .npy label "
                         "volume) or \"runs\" (the run-length label file)")
    return value


@dataclass(frozen=True)
class CountOptions:
    """count_blobs' opt-in keys of settings["mi355x"], each as its parser returns it (count_options builds the record from the
    settings); the defaults are a run without any key"""
    bounds: Optional[Tuple[int, int]] = None  # size_filter_bounds
    intensity: bool = False  # intensity_stats_enabled
    shell_radius: int = 0  # background_shell_radius
    quartiles: bool = False  # intensity_quartiles_enabled
    shape: bool = False  # shape_stats_enabled
    split: Optional[Tuple[int, int]] = None  # split_fused_settings
    label_file: str = "dense"  # label_file_format
    confidence: bool = False  # confidence_stats_enabled
    depth: Optional[Tuple[int, int, int]] = None  # depth_stats_settings
    neighbours: Optional[Tuple[int, Tuple[int, int, int]]] = None  # neighbour_stats_settings: (R2, spacing)
    split_depth: Optional[Tuple[int, int, int, Tuple[int, int, int]]] = None  # split_depth_settings: (core_d2, fraction, min_core, spacing)
    fill_holes: bool = False  # fill_holes_enabled (the last field: tests/test_fill_holes_cpu.py pins it)

    @property
    def runs_file(self) -> bool:
        """the labels go to (and a cached labelling may come from) the run-length file"""
        return self.label_file == "runs"

    @property
    def filter_active(self) -> bool:
        """the size filter removes something only with the switch on and a bound given"""
        return self.bounds is not None and (self.bounds[0] >= 0 or self.bounds[1] >= 0)

    @property
    def shell_bytes_per_voxel(self) -> int:
        """HBM of HipEngine.cc_shell beside the labels and the raw volume: the shell volume, and the scratch volume above radius 1"""
        return 0 if not self.shell_radius else (4 if self.shell_radius == 1 else 8)


def count_options(settings, min_size, max_size) -> CountOptions:
    """The record of count_blobs' opt-in keys.  The parsers run in this order, so with several bad keys the first one's ValueError
    is raised."""
    bounds = size_filter_bounds(settings, min_size, max_size)
    shell_radius = background_shell_radius(settings)
    quartiles = intensity_quartiles_enabled(settings)
    split = split_fused_settings(settings)
    split_depth = split_depth_settings(settings)
    shape = shape_stats_enabled(settings)
    confidence = confidence_stats_enabled(settings)
    fill = fill_holes_enabled(settings)
    depth = depth_stats_settings(settings)
    neighbours = neighbour_stats_settings(settings)
    return CountOptions(bounds=bounds, intensity=intensity_stats_enabled(settings), shell_radius=shell_radius, quartiles=quartiles,
                        shape=shape, split=split, label_file=label_file_format(settings), confidence=confidence,
                        fill_holes=fill, depth=depth, neighbours=neighbours, split_depth=split_depth)


INTENSITY_STATS_KEYS = INTENSITY_KEYS + ("intensity_mean",)  # what settings["mi355x"]["intensity_stats"] adds to the statistics
SHELL_STATS_KEYS = SHELL_KEYS + ("shell_radius",)  # ... and settings["mi355x"]["background_shell"]
SHELL_QUARTILE_STATS_KEYS = SHELL_QUARTILE_KEYS + ("shell_radius",)  # ... and both with settings["mi355x"]["intensity_quartiles"]
RAW_GROUPS = frozenset(("cells", "shell", "cell_quartiles", "shell_quartiles"))  # the groups of measuring_plan taken from the raw volume


def _same_setting(stored, asked) -> bool:
    """a setting recorded in the pickle (an int, or a sequence of ints) is the one asked for"""
    if isinstance(asked, tuple):
        return isinstance(stored, (tuple, list, np.ndarray)) and tuple(int(v) for v in stored) == asked
    return stored == asked


def measuring_plan(opts: CountOptions, stats: Optional[dict]) -> frozenset:
    """The groups of per-cell statistics count_blobs has to measure: those `opts` asks for and `stats` - the cached pickle, None
    without one - does not hold completely.  A group is complete with every key of its row; a row that lists shell_radius also needs
    the radius asked for (shells of another radius are other shells), one that lists depth_spacing the spacing asked for, and the
    neighbour table its own neighbour_radius_sq and neighbour_spacing (not depth_spacing: the two groups do not entangle)."""
    shell = opts.shell_radius > 0
    nb_radius_sq, nb_spacing = opts.neighbours if opts.neighbours is not None else (None, None)
    settings_keys = {"shell_radius": opts.shell_radius, "depth_spacing": opts.depth,  # the keys that record how a row was measured
                     "neighbour_radius_sq": nb_radius_sq, "neighbour_spacing": nb_spacing}
    rows = (("cells", opts.intensity, INTENSITY_STATS_KEYS),
            ("shell", opts.intensity and shell, SHELL_STATS_KEYS),
            ("cell_quartiles", opts.quartiles, QUARTILE_KEYS),
            ("shell_quartiles", opts.quartiles and shell, SHELL_QUARTILE_STATS_KEYS),
            ("shape", opts.shape, SHAPE_KEYS),
            ("confidence", opts.confidence, CONFIDENCE_KEYS),
            ("depth", opts.depth is not None, DEPTH_KEYS),
            ("neighbours", opts.neighbours is not None, NEIGHBOUR_KEYS))

    def complete(keys) -> bool:
        return (stats is not None and all(k in stats for k in keys)
                and all(k not in keys or _same_setting(stats[k], asked) for k, asked in settings_keys.items()))

    return frozenset(group for group, asked, keys in rows if asked and not complete(keys))


_HBM_FRESH = ("fill_holes", "intensity_stats", "background_shell", "intensity_quartiles", "confidence_stats", "shape_stats", "depth_stats", "neighbour_stats", "split_fused", "split_radius", "size_filter", "label_file")
_HBM_CACHED = ("label_file", "shape_stats", "depth_stats", "neighbour_stats", "intensity_stats", "background_shell", "intensity_quartiles", "confidence_stats")  # (cached labels are not split or filtered)


def check_hbm_budget(opts: CountOptions, measured, cached: bool, base: int, voxels: int, budget: int, runs_decoded: bool = False) -> None:
    """count_blobs' HBM check of the opt-in keys.  Resident are `base` bytes per voxel: the mask and its labels of a fresh labelling
    (streaming.ccl_bytes_per_voxel()), or the cached labels (4).  measured: the groups (measuring_plan) that are going to be taken -
    of a fresh labelling all that are asked for, measuring_plan(opts, None).  MemoryError for the first key, in the order the work
    is done, whose volumes do not fit `budget` bytes beside that; a fresh labelling above the budget alone is slab-streamed
    (streaming.py), which measures, splits and filters nothing and writes the dense label file only.  runs_decoded: the cached
    labelling is a run-length file that is about to be decoded into HBM (there is no slab-wise way round that)."""
    resident = "the cached labels" if cached else "the mask and its labels"
    raw = bool(RAW_GROUPS & measured)
    s = opts.shell_bytes_per_voxel
    rows = {  # key: (it applies, its value in the settings, bytes per voxel beside the resident ones, what it needs, what streaming lacks)
        # (the mask, 1 of the resident bytes, stays until the filled voxels are counted under the final labels: through the split
        # and the filter; the gap table of the fill - 8 bytes per row, 10 per gap - is made before the labels exist)
        "fill_holes": (opts.fill_holes, "", 0, f"{resident} and the gap table in HBM", "fill holes"),
        "intensity_stats": (raw, "", 2, f"the raw volume in HBM beside {resident}", "measure"),
        "background_shell": ("shell" in measured, f" = {opts.shell_radius}", 2 + s,
                             f"{s} more bytes per voxel in HBM beside {resident} and the raw volume", None),
        "intensity_quartiles": (bool(measured & {"cell_quartiles", "shell_quartiles"}), "", 2 + s + 2,
                                f"up to 2 more bytes per voxel in HBM beside {resident}, the raw volume{' and the shell' if s else ''}", None),
        "confidence_stats": ("confidence" in measured, "", 4, f"the probabilities (4 more bytes per voxel) in HBM beside {resident}", "measure"),
        "shape_stats": ("shape" in measured, "", 0, f"{resident} in HBM", "measure"),
        "depth_stats": ("depth" in measured, "", 8, f"8 more bytes per voxel in HBM beside {resident}", "measure"),
        # (the pair table and the outputs of the neighbour table are sized from the count: HipEngine.cc_neighbours checks them)
        "neighbour_stats": ("neighbours" in measured, "", 0, f"{resident} in HBM", "measure"),
        "split_fused": (opts.split is not None, f" = {opts.split and opts.split[0]}", 8,
                        f"8 more bytes per voxel in HBM beside {resident}", "split"),
        "split_radius": (opts.split_depth is not None, " / ['split_fraction']", 8,
                         f"8 more bytes per voxel in HBM beside {resident}", "split"),
        "size_filter": (opts.filter_active, "", 0, f"{resident} in HBM", "filter"),
        "label_file": (opts.runs_file and (runs_decoded or not cached), ' = "runs"', 0, f"{resident} in HBM", "write run-length labels"),
    }
    for key in _HBM_CACHED if cached else _HBM_FRESH:
        applies, value, extra, clause, lacks = rows[key]
        need = int(voxels) * (int(base) + extra)
        if applies and need > budget:
            streamed = f" and the slab-streamed labelling does not {lacks}" if lacks and not cached else ""
            raise MemoryError(f"delivr_cfos_amd (DLV_ENOMEM): settings['mi355x']['{key}']{value} needs {clause} ({need / 2**30:.1f} GiB), "
                              f"the HBM budget is {budget / 2**30:.1f} GiB{streamed}; raise settings['mi355x']['hbm_budget_gb'] or "
                              f"switch {key} off")


def pass_schedule(tta: bool) -> List[Tuple[Optional[int], int]]:
    """(flip_dim, repeat) per DISTINCT pass.  The reference runs 1 plain pass, then 4 x {noise,
    noise + flip Z (dim 2), noise + flip Y (dim 3)} (inference/inference.py:261-279); its noise is
    N(0, <=1e-3) on raw uint16-scale intensities (sliding_window_inferer.py:212-215), i.e. nil, so the
    13 passes collapse to plain x5, flipZ x4, flipY x4."""
    if not tta:
        return [(None, 1)]
    return [(None, 5), (2, 4), (3, 4)]


def cells_csv_text(stats: dict, n: int) -> str:
    """The text pandas writes for the reference's cell table (count_blobs.py:98-114): header
    ``,Blob,Coords,Size``; one row per label 1..N-1 (the reference's ``range(1, N)`` drops the last
    label); index column always 0; Coords = python repr of [z, y, x] floats, quoted by the CSV
    writer because it contains commas."""
    cent = np.asarray(stats["centroids"], dtype=np.float64)[1:max(int(n), 1)].tolist()  # (python floats: repr as pandas writes them)
    counts = np.asarray(stats["voxel_counts"])[1:max(int(n), 1)].tolist()
    lines = [",Blob,Coords,Size"]
    lines.extend(f'0,{i},"{c!r}",{k}' for i, (c, k) in enumerate(zip(cent, counts), 1))
    return "\n".join(lines) + "\n"


def cells_csv_bytes(stats: dict, n: int) -> bytes:
    """cells_csv_text through the library's host-side writer (dlv_cells_csv: C, ~0.1 s for 540 k cells instead of 0.8 s of Python
    string formatting - the same text, compared case by case in tests/test_host_cpu.py)"""
    import ctypes as C

    from . import _lib

    lib = _lib.load()
    counts = np.ascontiguousarray(stats["voxel_counts"], dtype=np.uint32)
    cent = np.ascontiguousarray(stats["centroids"], dtype=np.float64)
    n = int(n)
    if len(counts) < n or cent.shape[0] < n or cent.shape[1:] != (3,):
        raise ValueError("statistics shorter than the label count")
    buf = C.create_string_buffer(64 + 128 * max(n, 1))
    ln = C.c_size_t()
    rc = lib.dlv_cells_csv(counts.ctypes.data_as(C.c_void_p), cent.ctypes.data_as(C.c_void_p), n, buf, len(buf), C.byref(ln))
    if rc != 0:
        raise _lib.DelivrHipError(rc, "dlv_cells_csv failed")
    return buf.raw[: ln.value]


def csv_name(shape_zyx: Sequence[int], brain: str) -> str:
    """f"{bin_img.shape}_{brain}.csv" (count_blobs.py:113): "(Z, Y, X)_<brain>.csv"."""
    return f"{tuple(int(v) for v in shape_zyx)}_{brain.replace('.nii.gz', '')}.csv"


def scale_cell_coords(coords_zyx, original_shape: Sequence[int], downsampled_shape: Sequence[int], direction: str = "down"):
    """Cell-coordinate scaling of automate_mBrainaligner.py:261-284: factor = original/downsampled
    per axis; "down" divides (original -> atlas space), "up" multiplies."""
    f = np.asarray(original_shape, dtype=np.float64) / np.asarray(downsampled_shape, dtype=np.float64)
    c = np.asarray(coords_zyx, dtype=np.float64)
    return c / f if direction == "down" else c * f


def downsample_ratios(steps: dict) -> Tuple[int, int, int]:
    """(z, y, x) integer block-mean factors from config.json's mask_detection.downsample_steps
    (downsample/downsample_and_mask.py:161-163): round(downsample_um / original_um)."""
    return (round(steps["downsample_um_z"] / steps["original_um_z"]),
            round(steps["downsample_um_y"] / steps["original_um_y"]),
            round(steps["downsample_um_x"] / steps["original_um_x"]))


def padded_boxes(bounding_boxes: np.ndarray, cc_ids, shape_zyx, times: int = 1) -> np.ndarray:
    """Half-open slices the reference paints for the listed cells (blob_highlighter.py:18-23, :112-113): the inclusive
    cc3d box with every upper end moved up by one, `times` times, each time only while it is still below the axis
    length (pad_bb mutates the statistics in place, so the region-id loop - which runs after the RGB loop - sees boxes
    that were already padded once: times=2).  Returns (n,6) int32 [z0,z1,y0,y1,x0,x1]."""
    bb = np.asarray(bounding_boxes)[np.asarray(cc_ids, dtype=np.int64)].astype(np.int64)
    dims = np.asarray(shape_zyx, dtype=np.int64)
    out = np.empty((len(bb), 6), dtype=np.int64)
    out[:, 0::2] = bb[:, 0::2]
    hi = bb[:, 1::2].copy()
    for _ in range(times):
        hi = np.where(hi < dims[None, :], hi + 1, hi)
    out[:, 1::2] = hi
    return out.astype(np.int32)


PAINT_SOURCES = ("boxes", "labels")


def paint_source(settings) -> str:
    """settings["mi355x"]["paint_from"]: "boxes" (or absent) - the reference's painting of padded bounding boxes times binaries.npy;
    "labels" - every voxel gets the value of the cell whose label it carries (blob_highlighter's docstring).  ValueError for
    anything else."""
    value = ((settings or {}).get("mi355x") or {}).get("paint_from")
    if value is None:
        return "boxes"
    if not isinstance(value, str) or value not in PAINT_SOURCES:
        raise ValueError(f"settings['mi355x']['paint_from'] = {value!r}: expected \"boxes\" (the default: the reference's padded "
                         "bounding boxes) or \"labels\" (each voxel coloured by its own label)")
    return value


def paint_luts(ids, red, green, blue, graph_order, n: int):
    """The look-up tables of the "labels" painting for a label volume with the labels 1..n: rgb (n + 1, 3) uint8 and region
    (n + 1,) uint16, indexed by label.  connected_component_id IS the label (the box path indexes stats["bounding_boxes"][id], which
    cc3d indexes by label); a label without a row of the cell table keeps 0, and so does entry 0, the background.  The values wrap
    into their type as the box path's .astype does.  ValueError for an id of 0, IndexError for an id above n (the box path's
    "beyond the statistics table"); blob_highlighter has refused duplicate ids before."""
    ids = np.asarray(ids, dtype=np.int64)
    n = int(n)
    if ids.size and int(ids.min()) < 1:
        raise ValueError(f"connected_component_id {int(ids.min())}: label 0 is the background, a cell's label is 1..{n}")
    if ids.size and int(ids.max()) > n:
        raise IndexError(f"connected_component_id {int(ids.max())} beyond the {n} labels of the label volume")
    rgb = np.zeros((n + 1, 3), dtype=np.uint8)
    region = np.zeros(n + 1, dtype=np.uint16)
    for c, col in enumerate((red, green, blue)):
        rgb[ids, c] = np.asarray(col).astype(np.uint8)
    region[ids] = np.asarray(graph_order).astype(np.uint16)
    return rgb, region


def max_window_multiplicity(starts, roi) -> int:
    """Largest number of windows covering one voxel, for the (n,3) window starts of the reference's enumeration
    (inference/sliding_window_inferer.py:143-145) and the window size: the peak of the count map after one pass."""
    import numpy as np

    starts = np.asarray(starts)
    mult = 1
    for k in range(3):
        st = np.unique(starts[:, k])
        ev = np.concatenate([np.stack([st, np.ones_like(st)], 1), np.stack([st + int(roi[k]), -np.ones_like(st)], 1)])
        ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]  # closings (-1) before openings (+1) at equal coordinates
        mult *= int(np.cumsum(ev[:, 1]).max())
    return mult


def affine_apply(matrix34, coords_zyx):
    """Maps (n,3) cell coordinates (z,y,x) found in a volume produced by HipEngine.affine_warp_u16 back into the index
    space of its input: c_in = M . (c_out, 1) - the coordinate leg of BASELINE config 5 (the reference moves cell
    coordinates, never volumes: automate_mBrainaligner.py:261-284 scales them, the registration binaries warp them)."""
    import numpy as np

    m = np.asarray(matrix34, dtype=np.float64).reshape(3, 4)
    c = np.asarray(coords_zyx, dtype=np.float64).reshape(-1, 3)
    return c @ m[:, :3].T + m[:, 3]
