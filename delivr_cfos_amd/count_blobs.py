"""Mirror of the reference's ``count_blobs.py`` (count_blobs :36-118, caches :10-34): 26-connected
components + statistics on the device instead of cc3d, same files out.

in : <path_in>/<brain>/binary_segmentations/binaries.npy ('|u1', (Z,Y,X), 128-byte header)   (:45-46)
out: <post_out>/<brain>-<N>-cc3d.npy (labels), <post_out>/<brain>-stats.pickle
     (dict voxel_counts / bounding_boxes / centroids), <post_out>(Z, Y, X)_<brain>.csv          (:65,86-88,113-114)
     with settings["mi355x"]["label_file"] = "runs": <post_out>/<brain>-<N>-cc3d.runs (label_runs.py) in place of the .npy labels
"""
from __future__ import annotations

import datetime
import os
import pickle
from typing import NamedTuple, Optional

import numpy as np

from . import hostio, label_runs
from .hostlogic import (FILL_VALUE, QUARTILE_LEVELS, RAW_GROUPS, SHELL_KEYS, SHELL_QUARTILE_KEYS, CountOptions, cell_confidence_csv_text,
                        cell_depth_csv_text, cell_holes_csv_text, cell_intensity_csv_text, cell_neighbours_csv_text, cell_pairs_csv_text,
                        cell_quartiles_csv_text, cell_shape_csv_text, cells_csv_bytes, check_hbm_budget,
                        count_options, csv_name, finish_confidence, finish_depth, finish_intensity, finish_neighbours, finish_quartiles, finish_shape, finish_shell,
                        finish_shell_quartiles, finish_split, measuring_plan, merge_confidence, merge_intensity, merge_shape,
                        merge_shell)


def _find_cached(path: str, suffix: str, brain: str):
    """The LAST directory entry (os.listdir order, as the reference iterates) whose name holds `suffix` and `brain`; False
    when there is none - what the reference's three cache look-ups return (count_blobs.py:10-34, blob_highlighter.py)."""
    hits = [x for x in os.listdir(path) if suffix in x and brain in x]
    return os.path.join(path, hits[-1]) if hits else False


def load_cached_brain(settings, brain):
    """reference :10-21"""
    return _find_cached(settings["postprocessing"]["output_location"], ".npy", brain)


def load_cached_stats(settings, brain):
    """reference :23-34"""
    return _find_cached(settings["postprocessing"]["output_location"], ".pickle", brain)


def load_cached_runs(settings, brain):
    """The cached labelling of a run with settings["mi355x"]["label_file"] = "runs": the LAST directory entry (as _find_cached)
    named <brain>-<N>-cc3d.runs in the output folder -> (path, N from the name), or False.  The name holds no ".npy": the dense
    look-up above never matches it."""
    path = settings["postprocessing"]["output_location"]
    hits = [x for x in os.listdir(path) if x.startswith(brain + "-") and x.endswith(label_runs.SUFFIX)]
    if not hits:
        return False
    n = hits[-1][len(brain) + 1:-len(label_runs.SUFFIX)]
    if not n.isdigit():
        raise ValueError(f"count_blobs: {os.path.join(path, hits[-1])}: no component count between the brain's name and {label_runs.SUFFIX}")
    return os.path.join(path, hits[-1]), int(n)


def _label_dtype(n: int):
    # cc3d picks the smallest unsigned type that holds the label count [3P-recall]
    return np.uint16 if n < 2**16 else np.uint32


def _labels_in_file_dtype(labels_dev, n: int):
    """the uint32 labels (held in an int32 tensor) in the width of the file's dtype, converted in HBM: a volume with fewer
    than 2^16 components crosses PCIe and reaches the file as 2 bytes per voxel"""
    if _label_dtype(n) == np.uint16:
        import torch

        return labels_dev.to(torch.int16)  # (labels < 2^16: the low half is the value)
    return labels_dev


def _even_slabs(Z: int, world: int):
    cuts = [(Z * r) // world for r in range(world + 1)]
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def _keep_mask(counts: np.ndarray, bounds) -> np.ndarray:
    """the labels dlv_cc_size_filter_dev keeps, from their voxel counts (host side of the sharded path and of last_filter)"""
    keep = np.ones(len(counts), dtype=bool)
    if bounds[0] >= 0:
        keep &= counts >= bounds[0]
    if bounds[1] >= 0:
        keep &= counts <= bounds[1]
    keep[0] = False
    return keep


def _note_filter(bounds, n_before: int, n_kept: int, voxels_removed: int, quiet: bool = False):
    count_blobs.last_filter = {"min_size": int(bounds[0]), "max_size": int(bounds[1]), "n_before": int(n_before), "n_kept": int(n_kept),
                               "voxels_removed": int(voxels_removed)}
    if not quiet:
        print(f"size filter (min_size {bounds[0]}, max_size {bounds[1]}): kept {n_kept} of {n_before} components, "
              f"removed {voxels_removed} voxels")


def _note_split(split, n_before: int, n_after: int, components_split: int):
    count_blobs.last_split = {"depth": int(split[0]), "min_core": int(split[1]), "n_before": int(n_before), "n_after": int(n_after),
                              "components_split": int(components_split)}
    print(f"split of fused cells (depth {split[0]}, min_core {split[1]}): {components_split} of {n_before} components split, "
          f"{n_after} cells")


def _note_split_depth(split_depth, radius, n_before: int, n_after: int, components_split: int):
    core_d2, fraction, min_core, spacing = split_depth
    count_blobs.last_split = {"core_d2": int(core_d2), "fraction": int(fraction), "spacing": tuple(int(w) for w in spacing),
                              "min_core": int(min_core), "n_before": int(n_before), "n_after": int(n_after),
                              "components_split": int(components_split)}
    print(f"split of fused cells (radius {radius}: core_d2 {core_d2}, fraction {fraction} %, spacing {list(spacing)}, min_core {min_core}): "
          f"{components_split} of {n_before} components split, {n_after} cells")


def _note_fill(voxels_filled: int, holes: int, n_after: int):
    # (the components before the fill are not named: the cells a cavity swallowed are only known from a second labelling)
    count_blobs.last_fill = {"holes": int(holes), "voxels_filled": int(voxels_filled), "n_after": int(n_after)}
    print(f"fill of holes: {holes} holes filled, {voxels_filled} voxels added, {n_after} components after the fill")


def _note_neighbours(neighbours, stats, n: int):
    radius_sq, spacing = neighbours
    pairs = int(len(stats["neighbour_gap_sq"]))
    sizes = np.asarray(stats["cluster_size"])[1:n + 1]
    ids = np.asarray(stats["cluster_id"])[1:n + 1]
    clusters = int(len(np.unique(ids[sizes >= 2])))
    alone = int(np.count_nonzero(np.asarray(stats["neighbour_count"])[1:n + 1] == 0))
    count_blobs.last_neighbours = {"n": int(n), "radius_sq": int(radius_sq), "spacing": tuple(int(w) for w in spacing), "pairs": pairs,
                                   "clusters": clusters, "cells_without_neighbour": alone}
    print(f"cell neighbourhoods (radius_sq {radius_sq}, spacing {list(spacing)}): {pairs} pairs, {clusters} clusters of two or more "
          f"cells, {alone} of {n} cells without a neighbour")


def _open_raw_volume(settings, brain, shape):
    """The raw volume of settings["mi355x"]["intensity_stats"]: the first *.npy (sorted) under <blob_detection input>/<brain>/
    masked_niftis - the file run_inference reads - as a read-only memmap without its leading singleton axes -> (memmap, path).
    FileNotFoundError without the folder or a file in it; ValueError unless it is a C-ordered uint16 volume at least as large as
    the stack on every axis (the file is padded to window multiples)."""
    nifti_dir = os.path.join(settings["blob_detection"]["input_location"], brain, "masked_niftis")
    files = sorted(f for f in os.listdir(nifti_dir) if f.endswith(".npy"))
    if not files:
        raise FileNotFoundError(f"count_blobs: settings['mi355x']['intensity_stats'] needs the raw volume, no .npy file in {nifti_dir}")
    path = os.path.join(nifti_dir, files[0])
    vol = np.load(path, mmap_mode="r")
    while vol.ndim > 3 and vol.shape[0] == 1:
        vol = vol[0]
    if vol.dtype != np.uint16 or vol.ndim != 3 or not vol.flags.c_contiguous or any(r < v for r, v in zip(vol.shape, shape)):
        raise ValueError(f"count_blobs: the raw volume {path} ({vol.dtype}, shape {tuple(vol.shape)}) is not a C-ordered uint16 volume "
                         f"that holds the stack of shape {tuple(shape)}")
    return vol, path


def _open_prob_volume(path_in, brain, shape):
    """The probabilities of settings["mi355x"]["confidence_stats"]: <path_in>/<brain>/binary_segmentations/network_output.npy, the
    file run_inference writes next to binaries.npy with FLAGS.SAVE_ACTIVATED_OUTPUT, as a read-only memmap -> (memmap, path).
    FileNotFoundError without the file; ValueError unless it is a C-ordered '<f4' volume of exactly the stack's shape."""
    path = os.path.join(path_in, brain, "binary_segmentations", "network_output.npy")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"count_blobs: settings['mi355x']['confidence_stats'] needs the probabilities {path}: run step 2 with "
                                "FLAGS.SAVE_ACTIVATED_OUTPUT")
    vol = np.load(path, mmap_mode="r")
    if vol.dtype != np.dtype("<f4") or vol.ndim != 3 or not vol.flags.c_contiguous or tuple(vol.shape) != tuple(shape):
        raise ValueError(f"count_blobs: {path} ({vol.dtype}, shape {tuple(vol.shape)}) is not the C-ordered '<f4' volume of shape "
                         f"{tuple(shape)} that step 2 writes with FLAGS.SAVE_ACTIVATED_OUTPUT")
    return vol, path


def _measure_confidence(eng, labels_dev, prob_planes, N) -> dict:
    """prob_planes: the planes of the probability memmap that lie under labels_dev.  One upload of them, HipEngine.cc_confidence, and
    the tensor is gone when this returns."""
    prob_dev = hostio.upload(eng, prob_planes, what="h2d_prob")
    try:
        return eng.cc_confidence(labels_dev, prob_dev, N)
    finally:
        del prob_dev


class _Measured(NamedTuple):
    """what _measure_raw took from the raw volume; None for what the plan did not ask for"""
    cells: Optional[dict]  # HipEngine.cc_intensity's dict of the cells - hostlogic.finish_intensity's / merge_intensity's input
    shell: Optional[tuple]  # (cc_intensity's dict of the shell volume, its voxel counts per label 0..N as uint32) - finish_shell's / merge_shell's
    cell_quartiles: Optional[tuple]  # HipEngine.cc_quantiles' pair for hostlogic.QUARTILE_LEVELS, of the cells
    shell_quartiles: Optional[tuple]  # ... of the shell volume
    quartiles_s: float  # the seconds spent in cc_quantiles


def _measure_raw(eng, labels_dev, raw_planes, N, opts, plan, keep=None) -> _Measured:
    """raw_planes: the planes of the raw memmap that lie under labels_dev (whole planes: the Y / X padding stays, the pitches
    describe it).  One upload of them serves whatever `plan` (hostlogic.measuring_plan) asks of the cells and of their shells of
    radius opts.shell_radius; the shell volume is built once for its moments and its quartiles.  keep: (first, planes) - the planes of
    labels_dev that count (a slab extended by its neighbours' planes: the cells and the shell of the slab alone).  The raw tensor
    is gone when this returns."""
    import time

    raw_dev = hostio.upload(eng, raw_planes, what="h2d_raw")
    kept = slice(None) if keep is None else slice(keep[0], keep[0] + keep[1])
    raw_kept = raw_dev[kept]
    quartiles_s = 0.0

    def quartiles_of(volume):
        nonlocal quartiles_s
        t0 = time.perf_counter()
        pair = eng.cc_quantiles(volume, raw_kept, N, QUARTILE_LEVELS)
        quartiles_s += time.perf_counter() - t0
        return pair

    try:
        cells = eng.cc_intensity(labels_dev[kept], raw_kept, N) if "cells" in plan else None
        cell_q = quartiles_of(labels_dev[kept]) if "cell_quartiles" in plan else None
        shell = shell_q = None
        if plan & {"shell", "shell_quartiles"}:
            shell_vol = eng.cc_shell(labels_dev, opts.shell_radius, raw_dev)[kept]
            if "shell" in plan:
                shell = (eng.cc_intensity(shell_vol, raw_kept, N), eng.cc_counts(shell_vol, N).cpu().numpy().view(np.uint32))
            if "shell_quartiles" in plan:
                shell_q = quartiles_of(shell_vol)
        return _Measured(cells, shell, cell_q, shell_q, quartiles_s)
    finally:
        del raw_dev, raw_kept


def _slab_with_neighbour_planes(labels, dist, rank, world, radius):
    """The slab `labels` of a sharded run extended by `radius` planes of the final global labels from either neighbour slab
    (exchanged as parallel.ccl_sharded exchanges its boundary plane) -> (extended slab, index of the slab's first plane in it:
    `radius`, or 0 on rank 0).  Every slab holds at least `radius` planes (count_blobs checked)."""
    import torch

    from .parallel import _needs_host_staging

    stage = _needs_host_staging(labels, dist)
    ops, got = [], {}
    for peer, mine in ((rank - 1, labels[:radius]), (rank + 1, labels[-radius:])):
        if 0 <= peer < world:
            t = mine.contiguous()
            ops.append(dist.P2POp(dist.isend, t.cpu() if stage else t, peer))
            got[peer] = torch.empty_like(t, device="cpu") if stage else torch.empty_like(t)
            ops.append(dist.P2POp(dist.irecv, got[peer], peer))
    for req in dist.batch_isend_irecv(ops):
        req.wait()
    up, down = got.get(rank - 1), got.get(rank + 1)
    extended = torch.cat([t.to(labels.device) for t in (up, labels, down) if t is not None])
    return extended, (radius if rank > 0 else 0)


def _measure_raw_of_slab(eng, labels, dist, rank, world, raw_vol, lo, hi, N, opts, plan) -> _Measured:
    """_measure_raw for the slab [lo, hi) of a sharded run.  The shell of a voxel depends on the labels within opts.shell_radius
    planes of it only, so every rank takes that many planes of the final global labels from either neighbour
    (_slab_with_neighbour_planes), expands the extended slab and keeps its own planes - exactly the planes [lo, hi) of the whole
    volume's shell."""
    if not opts.shell_radius:
        return _measure_raw(eng, labels, raw_vol[lo:hi], N, opts, plan)
    extended, first = _slab_with_neighbour_planes(labels, dist, rank, world, opts.shell_radius)
    return _measure_raw(eng, extended, raw_vol[lo - first:lo - first + int(extended.shape[0])], N, opts, plan, keep=(first, hi - lo))


def _write_table(path_out, folder, brain, text):
    """<output_location>/<folder>/<brain>.csv - in a sub-folder, so that no cache look-up (_find_cached: any entry with '.npy' /
    '.pickle' and the brain's name) and no reader of the reference's CSV ever matches it"""
    folder = os.path.join(path_out, folder)
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, f"{brain}.csv"), "w", newline="") as fh:
        fh.write(text)


def _write_tables(path_out, brain, stats, N, opts, raw_file, prob_file=None):
    """the tables of the opt-in statistics `opts` asks for, and what count_blobs.last_intensity / last_quartiles / last_shape /
    last_confidence / last_depth / last_neighbours say"""
    def for_table(shell_keys):  # (shell entries of a cached pickle do not reach the table of a run without the key)
        return stats if opts.shell_radius else {k: v for k, v in stats.items() if k not in shell_keys}

    if opts.intensity:
        _write_table(path_out, "cell_intensity", brain, cell_intensity_csv_text(for_table(SHELL_KEYS), N))
        count_blobs.last_intensity = {"n": int(N), "raw_file": raw_file}
        if opts.shell_radius:
            count_blobs.last_intensity["shell_radius"] = int(opts.shell_radius)
    if opts.quartiles:
        _write_table(path_out, "cell_quartiles", brain, cell_quartiles_csv_text(for_table(SHELL_QUARTILE_KEYS), N))
        count_blobs.last_quartiles = {"n": int(N)}
    if opts.shape:
        _write_table(path_out, "cell_shape", brain, cell_shape_csv_text(stats, N))
        count_blobs.last_shape = {"n": int(N)}
    if opts.confidence:
        _write_table(path_out, "cell_confidence", brain, cell_confidence_csv_text(stats, N))
        count_blobs.last_confidence = {"n": int(N), "prob_file": prob_file}
    if opts.depth is not None:
        _write_table(path_out, "cell_depth", brain, cell_depth_csv_text(stats, N))
        count_blobs.last_depth = {"n": int(N), "spacing": tuple(opts.depth)}
    if opts.neighbours is not None:
        _write_table(path_out, "cell_neighbours", brain, cell_neighbours_csv_text(stats, N))
        _write_table(path_out, "cell_pairs", brain, cell_pairs_csv_text(stats))
        _note_neighbours(opts.neighbours, stats, N)
    if opts.fill_holes and "hole_voxels" in stats:  # (a cached labelling is not filled: its pickle may lack the key)
        _write_table(path_out, "cell_holes", brain, cell_holes_csv_text(stats, N))


def _count_blobs_sharded(eng, bin_img, dist, path_out, brain, opts=CountOptions(), raw_vol=None, prob_vol=None):
    """One process per GPU: every rank labels a Z-slab of the mask, seams are merged (parallel.ccl_sharded) and every
    rank writes ITS label slab straight into the output .npy (rank 0 creates the file once N - and with it the label
    dtype - is known); only the merged statistics travel to rank 0.  No rank ever holds the whole label volume (17 GB for
    1024x2048x2048).  opts: the opt-in keys (hostlogic.CountOptions; count_blobs refused those a slab cannot serve).  Size
    filter: every rank counts the voxels of the global labels in its slab, the counts are summed over the ranks, every rank
    applies the same filter to its slab and the statistics are taken on the filtered labels.  Intensity and shell statistics:
    every rank measures planes [lo, hi) of raw_vol under its final global labels (_measure_raw_of_slab), rank 0 merges the parts
    into its stats.  Shape statistics: every rank takes one plane of the final global labels from either neighbour slab (a face
    of a voxel is exposed or not by its neighbour across the cut), measures its own planes of the extended slab with their
    absolute z (HipEngine.cc_shape) and rank 0 adds the parts up.  Confidence: every rank uploads planes [lo, hi) of prob_vol and
    measures them under its final global labels - no neighbour planes are needed -, rank 0 merges the parts, a slab's peak made
    global by its first plane (hostlogic.merge_confidence).  Returns (N, stats | None)."""
    from .parallel import ccl_sharded, merge_stats

    rank, world = dist.get_rank(), dist.get_world_size()
    Z, Y, X = bin_img.shape
    slabs = _even_slabs(Z, world)
    lo, hi = slabs[rank]
    slab = hostio.upload(eng, bin_img[lo:hi], what="h2d_mask") if hi > lo else None
    bounds = opts.bounds
    if not opts.filter_active:
        labels, N, stats = ccl_sharded(eng, slab, slabs, rank, dist, (Z, Y, X))
    else:
        labels, n_before, _ = ccl_sharded(eng, slab, slabs, rank, dist, (Z, Y, X), want_stats=False)
        # a rank that fails here must not leave the others waiting in the next collective: the error text travels with the
        # counts, and the outcome of the filter is exchanged before the statistics are gathered (as for the slab writes below)
        mine, failed = None, None
        try:
            if labels is not None:
                mine = eng.cc_counts(labels, n_before).cpu().numpy().view(np.uint32)
        except Exception as exc:
            failed = f"rank {rank}: {exc!r}"
        parts = [None] * world
        dist.all_gather_object(parts, (mine, failed))
        bad = [f for _, f in parts if f]
        if bad:
            raise RuntimeError("count_blobs: counting the voxels per label failed: " + "; ".join(bad))
        total = np.zeros(n_before + 1, dtype=np.uint64)
        for part, _ in parts:
            if part is not None:
                total += part
        keep = _keep_mask(total, bounds)
        N = int(keep.sum())
        raw, failed = None, None
        try:
            if labels is not None:
                kept = eng.cc_size_filter(labels, n_before, bounds[0], bounds[1], counts=np.minimum(total, 2**32 - 1).astype(np.uint32))
                if kept != N:
                    raise RuntimeError(f"kept {kept} components, the summed counts say {N}")
                raw = eng.cc_stats_raw(labels, N)
        except Exception as exc:
            failed = f"rank {rank}: {exc!r}"
        _raise_if_any_failed(dist, failed, "count_blobs: the size filter")
        _note_filter(bounds, n_before, N, int(total[1:][~keep[1:]].sum()), quiet=rank != 0)
        raws = [None] * world
        dist.gather_object(raw, raws if rank == 0 else None, dst=0)
        stats = None
        if rank == 0:  # (the labels are global and final already: identity tables)
            stats = merge_stats([np.arange(N + 1, dtype=np.uint32)] * world, raws, [s[0] for s in slabs], (Z, Y, X), N)
    if opts.intensity:
        plan = measuring_plan(opts, None)

        def measure_slab():  # (a rank without a plane has no part)
            if labels is not None:
                return _measure_raw_of_slab(eng, labels, dist, rank, world, raw_vol, lo, hi, N, opts, plan)

        def merge_measured(parts):
            stats.update(finish_intensity(merge_intensity([p and p.cells for p in parts]), stats["voxel_counts"]))
            if opts.shell_radius:
                stats.update(finish_shell(*merge_shell([p and p.shell for p in parts]), stats["intensity_mean"]))
                stats["shell_radius"] = int(opts.shell_radius)

        _on_every_slab(dist, "the intensity statistics", measure_slab, merge_measured)
    if opts.confidence:
        def confidence_of_slab():  # (after the raw tensor of the intensity statistics is gone: the two uploads never coexist)
            if labels is not None:
                return _measure_confidence(eng, labels, prob_vol[lo:hi], N), lo, Y * X

        _on_every_slab(dist, "the confidence statistics", confidence_of_slab,
                       lambda parts: stats.update(finish_confidence(merge_confidence(parts), stats["voxel_counts"], (Z, Y, X))))
    if opts.shape:
        def shape_of_slab():
            if labels is not None:
                extended, first = _slab_with_neighbour_planes(labels, dist, rank, world, 1)
                return eng.cc_shape(extended, N, keep=(first, hi - lo), z_abs0=lo - first)

        _on_every_slab(dist, "the shape statistics", shape_of_slab,
                       lambda parts: stats.update(finish_shape(merge_shape(parts), stats["voxel_counts"])))
    out_path = os.path.join(path_out, f"{brain}-{N}-cc3d.npy")
    err = [None]
    if rank == 0:
        try:
            np.lib.format.open_memmap(out_path, mode="w+", dtype=_label_dtype(N), shape=(Z, Y, X)).flush()
        except Exception as exc:  # every rank must learn about it: they all wait in the broadcast below
            err[0] = repr(exc)
    dist.broadcast_object_list(err, src=0)
    if err[0] is not None:
        raise RuntimeError(f"count_blobs: rank 0 could not create {out_path}: {err[0]}")
    # every rank writes ITS slab into the one file: path_out must be a directory all ranks share.  The outcome of every
    # write is exchanged - a rank that cannot see or write the file (node-local path, ENOSPC) must not leave the others
    # waiting in a barrier
    mine = None
    try:
        if hi > lo:
            mm = np.load(out_path, mmap_mode="r")
            off = int(mm.offset) + lo * Y * X * mm.dtype.itemsize
            del mm
            hostio.download(eng, _labels_in_file_dtype(labels, N), out_path, offset=off, what="d2h_labels", sparse=True)  # (rank 0 created the file just now)
    except Exception as exc:
        mine = f"rank {rank}: {exc!r}"
    _raise_if_any_failed(dist, mine, f"count_blobs: writing the label slabs into {out_path} (path_out must be shared by all ranks)")
    return N, stats


def _on_every_slab(dist, what: str, measure, merge):
    """One statistic of a sharded run: every rank runs measure() for its part (None on a rank without a plane), the parts are
    gathered on rank 0 and merge(parts) runs there.  The outcome of every rank's pass, and then of rank 0's merge, is exchanged
    before the next collective: a rank that fails never leaves the others waiting, all raise together."""
    rank = dist.get_rank()
    part, failed = None, None
    try:
        part = measure()
    except Exception as exc:
        failed = f"rank {rank}: {exc!r}"
    _raise_if_any_failed(dist, failed, f"count_blobs: {what}")
    parts = [None] * dist.get_world_size()
    dist.gather_object(part, parts if rank == 0 else None, dst=0)
    failed = None
    if rank == 0:
        try:
            merge(parts)
        except Exception as exc:
            failed = f"rank 0: {exc!r}"
    _raise_if_any_failed(dist, failed, f"count_blobs: merging {what}")


def _raise_if_any_failed(dist, mine, what: str):
    """all_gather of every rank's error text (None = fine): all ranks raise together or none does"""
    outcomes = [None] * dist.get_world_size()
    dist.all_gather_object(outcomes, mine)
    bad = [o for o in outcomes if o]
    if bad:
        raise RuntimeError(f"{what} failed: " + "; ".join(bad))


def count_blobs(settings, path_in, brain_i, brain, stack_shape, min_size=-1, max_size=-1, engine=None, defer_write=False):  # noqa: C901
    """Same positional parameters as the reference.  ``engine``: a HipEngine to use (default: the process-wide engine of the
    device, engine.shared_engine - the one run_inference used, with its workspaces).  ``defer_write``: return when the statistics
    and the CSV are written - the label volume keeps streaming into its file on a background worker (hostio.wait_deferred() joins;
    the file appears under its name only when complete), so that the next brain's labelling does not wait for 17 GB of writes.  Under torch.distributed (one process per GPU) the labelling is sharded over the
    ranks along z; rank 0 writes the statistics and the CSV, every rank writes its slab of the labels and returns N.
    Rank 0 alone looks for a cached labelling and tells the others which branch to take, so the ranks cannot disagree
    about the collectives that follow (different cache views on a shared file system); a failure on rank 0 reaches the
    other ranks as an error instead of a hang.

    ``min_size`` / ``max_size``: ignored, as the reference ignores them, unless ``settings["mi355x"]["size_filter"]`` is true.
    Then a component is kept when min_size <= voxels <= max_size (inclusive; a negative bound is no bound), the survivors are
    renumbered 1..K in the order they had and everything written - label file, its name and dtype, statistics, CSV - is what
    the mask without the removed components would have given; ``count_blobs.last_filter`` holds the numbers.  A cached label
    file is reused as it is: the bounds are NOT re-applied to it.  A mask that needs the slab-streamed path (larger than the
    HBM budget) is refused with the filter on.

    ``settings["mi355x"]["intensity_stats"]`` true: the raw volume run_inference read (the first .npy under
    <blob_detection input_location>/<brain>/masked_niftis) is measured under the final labels on the device - per label the
    sum, the sum of squares, the minimum and the maximum of the raw intensities, exact integers, and their mean.  The five arrays
    become keys of <brain>-stats.pickle (intensity_sum / _sumsq / _min / _max / _mean, N+1 rows, row 0 zero), the table goes to
    <output_location>/cell_intensity/<brain>.csv and ``count_blobs.last_intensity`` holds {"n", "raw_file"}.  Cached labels are
    measured too, and a cached pickle without the keys is rewritten with them.  A missing or too small raw volume is an error
    before any file is written; a mask that needs the slab-streamed path is refused.  Off or absent: nothing of this happens.

    ``settings["mi355x"]["background_shell"]`` = r (1..16, with intensity_stats on): every cell's local background is measured as
    well.  The final labels are expanded by r synchronous steps of a 26-neighbourhood minimum (a background voxel goes to the
    smallest label among the cells nearest to it in Chebyshev distance, if that is at most r); the expanded voxels that belong to no
    cell and are not 0 in the raw volume (0 is "outside the tissue") are the cell's shell.  The pickle gains shell_voxels, shell_sum /
    _sumsq / _min / _max / _mean, contrast (= intensity_mean / shell_mean; 0.0 for a cell without a shell) and shell_radius, the table
    the matching columns and ``count_blobs.last_intensity`` "shell_radius".  A cached pickle without these keys, or with another
    shell_radius, is completed.  Needs 4 (r = 1) or 8 more bytes of HBM per voxel; under torch.distributed every slab must hold at
    least r planes.  Off, 0 or absent: nothing of this happens.

    ``settings["mi355x"]["shape_stats"]`` true (on its own: no raw volume is opened): the shape of every cell is measured on the final
    labels on the device - second-order moments of the voxel coordinates and the exposed faces per axis, exact integers.  The pickle
    gains shape_sums / _moments / _faces / _surface_voxels and the derived shape_covariance, shape_axes (principal-axis variances),
    shape_elongation and shape_sphericity (hostlogic.finish_shape), the table goes to <output_location>/cell_shape/<brain>.csv and
    ``count_blobs.last_shape`` holds {"n"}.  Cached labels are measured too, and a cached pickle without the keys is rewritten with
    them.  Needs no further volume in HBM; a mask that needs the slab-streamed path is refused; under torch.distributed every slab
    must hold a plane.  Off or absent: nothing of this happens.

    ``settings["mi355x"]["intensity_quartiles"]`` true (with intensity_stats on): order statistics beside the moments.  With a cell's m
    raw values sorted ascending, level p reads v[(p * (m - 1)) // 100] - the lower quantile, a value the cell holds - taken on the
    device on the final labels (HipEngine.cc_quantiles).  The pickle gains intensity_q25 / intensity_median / intensity_q75 (uint16,
    N+1 rows, row 0 zero) and, with background_shell, shell_q25 / shell_median / shell_q75 (0 without a shell) and contrast_median
    (= intensity_median / shell_median, 0.0 without a shell); the table goes to <output_location>/cell_quartiles/<brain>.csv and
    ``count_blobs.last_quartiles`` holds {"n"}.  Cached labels are measured too, and a cached pickle without the keys - or, with a
    shell, with another shell_radius - is completed.  Budgeted as 2 more bytes of HBM per voxel; refused with ValueError on every
    rank under torch.distributed: quantiles of the parts of a cell cut by a slab do not combine.  Off or absent: nothing of this happens.

    ``settings["mi355x"]["split_fused"]`` = d (1..16; ``split_min_core`` = m, default 1): fused cells are split on the device right
    after the labelling, before the size filter, so that min_size / max_size apply to the final cells.  The labels are eroded d
    times with the 6 face neighbours (outside the volume counts as background); what is left are the cores, 26-connected, those of
    fewer than m voxels dropped.  A component with two or more cores is divided among them - every voxel goes to the core nearest to
    it in 26-steps through its own component, to the first core on a tie - and all cells are renumbered in raster order of their
    first voxel (HipEngine.cc_split).  Everything written afterwards - label file, its name and dtype, statistics, CSV, the
    intensity, shell and shape statistics - is what the split labels give; the pickle gains split_parent (the component a cell was
    cut from, as the labelling numbered it), split_siblings (the cells that share that component and are still there after the size
    filter; 1 for a cell that was not split) and split_depth, and ``count_blobs.last_split`` holds {"depth", "min_core", "n_before",
    "n_after", "components_split"}.  A cached label file is reused as it is: it is NOT split again.  Needs 8 more bytes of HBM per
    voxel while it runs; a mask that needs the slab-streamed path is refused.  Under torch.distributed the key is refused with
    ValueError on every rank: the growth has no bounded reach, so a slab cannot be split on its own.  Off, 0 or absent: nothing of
    this happens.

    ``settings["mi355x"]["split_radius"]`` = r and / or ``settings["mi355x"]["split_fraction"]`` = p (``depth_spacing`` = [wz, wy, wx],
    default [1, 1, 1]; ``split_min_core`` as above): the same split with other cores, for stacks whose voxels are not cubes - one
    erosion step of split_fused takes 6 um along z and 1.6 um along y and x off the reference's voxels, and a nucleus of two planes
    is gone after the first.  The cores are the voxels that lie at least r - a number above 0 in the unit of depth_spacing, taken as
    core_d2 = ceil(r * r) - from the outside of their cell, and at least p per cent (an integer 1..99) of their cell's inscribed
    radius: the exact label-wise distance map of depth_stats, thresholded per cell (HipEngine.cc_split_depth).  With p every cell
    has a core; a cell thinner than r has none and stays whole.  Growth, numbering, the place in the order, split_parent and
    split_siblings, the cached labelling that is NOT split again, the 8 bytes of HBM per voxel and the refusals - slab-streamed
    mask: MemoryError; torch.distributed: ValueError on every rank - are those of split_fused, and the two are alternatives: both
    at once is a ValueError.  The pickle gains split_core_d2, split_fraction and split_spacing (and no split_depth: that is the
    erosion depth), and ``count_blobs.last_split`` holds {"core_d2", "fraction", "spacing", "min_core", "n_before", "n_after",
    "components_split"}.  depth_stats in the same run shares the spacing and is measured after the split, on the final labels.
    Absent: nothing of this happens, and no new kernel is launched.

    ``settings["mi355x"]["label_file"]`` = "runs": the final labels - after the split and the size filter - are run-length coded on
    the device (HipEngine.cc_runs_encode) and written as <brain>-<N>-cc3d.runs (label_runs.py: the format, and load_labels for the
    steps that read it) by the same side thread, under the same ``defer_write`` contract; NO dense .npy file is written and the label
    volume never crosses PCIe.  Statistics, CSV and tables are what they are without the key, and ``count_blobs.last_timings`` gains
    runs_encode_s.  A dense .npy cache still wins; without one a run file in the output folder is the cached labelling (N from its
    name, checked against its header; the file is validated in full), not split or filtered again, and decoded into HBM only when
    something is still to be measured - with a complete pickle nothing is uploaded.  Decoded labels above the HBM budget and a mask
    that needs the slab-streamed path are refused (MemoryError), torch.distributed is refused with ValueError on every rank.
    "dense" or absent: nothing of this happens, and a .runs file in the folder is ignored.

    ``settings["mi355x"]["confidence_stats"]`` true (on its own: no raw volume is opened): how sure the network was about every cell.
    The blended probabilities step 2 writes with FLAGS.SAVE_ACTIVATED_OUTPUT - <path_in>/<brain>/binary_segmentations/network_output.npy,
    next to binaries.npy, '<f4' of exactly the stack's shape - are uploaded once the raw tensor of the intensity statistics is gone and
    measured under the final labels on the device (HipEngine.cc_confidence): every probability in fixed point, q = rint(clamp(p, 0, 1) *
    2^24), NaN as 0, and per label the sum, the minimum, the maximum and the peak - the voxel of largest q, the first in raster order on
    a tie - in integers.  The pickle gains confidence_sum (uint64, fixed point), confidence_min / _max / _mean (float64) and
    confidence_peak (int64 (N+1, 3): z, y, x; row 0: zeros and -1), the table goes to <output_location>/cell_confidence/<brain>.csv,
    ``count_blobs.last_confidence`` holds {"n", "prob_file"} and ``count_blobs.last_timings`` gains confidence_s.  A cell's
    confidence_max is the ``threshold`` above which it disappears: compare_cells(scores=...) turns the column into a precision /
    recall curve.  Cached labels - dense or decoded runs - are measured too, and a cached pickle without the keys is completed.  A
    missing file, or one of another dtype or shape, is an error before any file is written; needs 4 more bytes of HBM per voxel; a mask
    that needs the slab-streamed path is refused.  Under torch.distributed every rank measures the planes of its slab and rank 0
    merges the parts.  A batch that ran step 2 with ``defer_write`` must join it (hostio.wait_deferred()) before this step, as for
    binaries.npy: both files stream out on the same workers and appear under their names only when complete.  Off or absent: nothing
    of this happens.

    ``settings["mi355x"]["fill_holes"]`` true: the holes of the mask are filled on the device between the upload and the labelling
    (HipEngine.fill_holes).  A hole is a 6-connected background component that reaches no face of the volume - exactly
    scipy.ndimage.binary_fill_holes(mask != 0): background that leaves a cavity only over an edge or a corner is sealed in, a cavity
    open to a face of the volume stays, and a cell inside the cavity of another is swallowed by it.  The order is fill, label, split,
    size filter, measure, write: everything written - label file (dense or runs), its name, statistics, CSV (``Size`` is the filled
    size), tables - is what the filled mask gives.  The mask stays in HBM, 1 byte per voxel, until the filled voxels have been counted
    under the final labels (HipEngine.cc_count_marked); the pickle gains hole_voxels (uint32, N+1 rows, row 0 zero: the voxels the fill
    added to each final cell) and holes_filled (the holes of the whole mask), the table goes to <output_location>/cell_holes/<brain>.csv,
    ``count_blobs.last_fill`` holds {"holes", "voxels_filled", "n_after"} and ``count_blobs.last_timings`` gains fill_holes_s and
    hole_voxels_s.  binaries.npy is step 2's file and is NOT rewritten: blob_highlighter's default box path multiplies by it and
    leaves the cavities unpainted, "paint_from": "labels" paints them.  A cached labelling - dense or runs - is reused as it is: it is
    NOT filled.  A mask that needs the slab-streamed path is refused (MemoryError), torch.distributed is refused with ValueError on
    every rank: a cavity that crosses a slab cut is closed on neither side.  Off or absent: nothing of this happens, and no new kernel
    is launched.

    ``settings["mi355x"]["depth_stats"]`` true (on its own: no raw volume is opened; ``depth_spacing`` = [wz, wy, wx], integers 1..64,
    default [1, 1, 1]): how thick every cell is and where its middle lies.  The exact squared Euclidean distance of every voxel of a
    cell to the nearest voxel outside it - the background, a touching cell and the outside of the volume alike -, in units of the
    spacing, is taken on the final labels on the device (HipEngine.cc_depth), where shape_stats is measured: after fill, split and
    filter.  The pickle gains depth_max_sq (uint32), depth_sum_sq and depth_peak_index (uint64), the exact integers, and the derived
    depth_radius (the radius of the largest inscribed ball), depth_mean_sq, depth_peak (int64 (N+1, 3): z, y, x of the deepest voxel,
    which always lies inside the cell) and depth_spacing (hostlogic.finish_depth); the table goes to
    <output_location>/cell_depth/<brain>.csv, ``count_blobs.last_depth`` holds {"n", "spacing"} and ``count_blobs.last_timings``
    gains depth_s.  Cached labels - dense or decoded runs - are measured too, and a cached pickle without the keys, or with another
    depth_spacing, is completed.  Needs 8 more bytes of HBM per voxel while it runs; a mask that needs the slab-streamed path is
    refused (MemoryError).  Under torch.distributed the key is refused with ValueError on every rank: a cell that crosses a slab cut
    has its nearest outside voxel on another rank.  Off or absent: nothing of this happens, and no new kernel is launched.

    ``settings["mi355x"]["neighbour_stats"]`` = r (a number above 0 in the unit of ``depth_spacing``, default [1, 1, 1]; on its own: no
    raw volume is opened): how the cells lie relative to each other.  Two cells are neighbours when a voxel of one lies within r of
    a voxel of the other; their gap is the exact smallest such distance, squared, in integers (R2 = floor(r * r); along every axis
    r may reach at most 8 voxels - a larger radius is a ValueError that names the axis).  The table is taken on the final labels on
    the device (HipEngine.cc_neighbours), after fill, split and filter, where depth_stats is measured.  The pickle gains
    neighbour_pairs (uint32 (P, 2), a < b, sorted), neighbour_gap_sq (uint32 (P)), neighbour_radius_sq, neighbour_spacing and the
    per-cell rows of hostlogic.neighbour_summary: neighbour_count, nearest_gap_sq and nearest_cell (0: no neighbour within r),
    cluster_id and cluster_size (the connected components of the graph; a cell without a neighbour is its own cluster).  The tables
    go to <output_location>/cell_neighbours/<brain>.csv (one row per cell) and <output_location>/cell_pairs/<brain>.csv (one row per
    pair), ``count_blobs.last_neighbours`` holds {"n", "radius_sq", "spacing", "pairs", "clusters", "cells_without_neighbour"} and
    ``count_blobs.last_timings`` gains neighbours_s.  Cached labels - dense or decoded runs - are measured too, and a cached pickle
    without the keys, or with another neighbour_radius_sq or neighbour_spacing, is completed.  Needs only the labels in HBM beside
    the pair table, which is sized from a counting pass and checked against the HBM budget; a mask that needs the slab-streamed
    path is refused (MemoryError).  Under torch.distributed the key is refused with ValueError on every rank: two neighbouring cells
    can lie on either side of a slab cut.  Off, 0 or absent: nothing of this happens, and no new kernel is launched."""
    from .engine import shared_engine

    count_blobs.last_filter = None  # set by a run that filtered
    count_blobs.last_quartiles = None  # set by a run with settings["mi355x"]["intensity_quartiles"]
    count_blobs.last_intensity = None  # set by a run with settings["mi355x"]["intensity_stats"]
    count_blobs.last_shape = None  # set by a run with settings["mi355x"]["shape_stats"]
    count_blobs.last_split = None  # set by a run that split (settings["mi355x"]["split_fused"], or "split_radius" / "split_fraction")
    count_blobs.last_confidence = None  # set by a run with settings["mi355x"]["confidence_stats"]
    count_blobs.last_fill = None  # set by a run that filled holes (settings["mi355x"]["fill_holes"])
    count_blobs.last_depth = None  # set by a run with settings["mi355x"]["depth_stats"]
    count_blobs.last_neighbours = None  # set by a run with settings["mi355x"]["neighbour_stats"]
    opts = count_options(settings, min_size, max_size)  # (a bad key raises here, before any file is touched)
    split, shell_radius = opts.split, opts.shell_radius
    if opts.bounds is None and any(v is not None and int(v) >= 0 for v in (min_size, max_size)):
        print(f"min_size {min_size} / max_size {max_size} are ignored, as in the reference; "
              "settings['mi355x']['size_filter'] = true applies them")

    try:
        import torch.distributed as dist
        sharded = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    except ImportError:  # pragma: no cover
        dist, sharded = None, False
    rank = dist.get_rank() if sharded else 0

    shape = tuple(int(v) for v in stack_shape[2:])
    if sharded and split is not None:
        # every rank reads the same settings: all raise, before any collective, or none does
        raise ValueError(f"count_blobs: settings['mi355x']['split_fused'] = {split[0]} is not available under torch.distributed "
                         f"({dist.get_world_size()} ranks): a core grows back through its whole component, so a Z-slab cannot be split on "
                         "its own; run step 3 on one device or switch split_fused off")
    if sharded and opts.split_depth is not None:
        # (as for split_fused: all raise, before any collective, or none does)
        raise ValueError(f"count_blobs: settings['mi355x']['split_radius'] / ['split_fraction'] is not available under torch.distributed "
                         f"({dist.get_world_size()} ranks): a core grows back through its whole component, so a Z-slab cannot be split on "
                         "its own; run step 3 on one device or switch split_radius and split_fraction off")
    if sharded and opts.fill_holes:
        # (as for split_fused: all raise, before any collective, or none does)
        raise ValueError(f"count_blobs: settings['mi355x']['fill_holes'] is not available under torch.distributed "
                         f"({dist.get_world_size()} ranks): a cavity that crosses a slab cut is closed on neither side, so a Z-slab cannot "
                         "be filled on its own; run step 3 on one device or switch fill_holes off")
    if sharded and opts.depth is not None:
        # (as for split_fused: all raise, before any collective, or none does)
        raise ValueError(f"count_blobs: settings['mi355x']['depth_stats'] is not available under torch.distributed "
                         f"({dist.get_world_size()} ranks): a cell that crosses a slab cut has its nearest outside voxel on another "
                         "rank, so a Z-slab cannot be measured on its own; run step 3 on one device or switch depth_stats off")
    if sharded and opts.neighbours is not None:
        # (as for split_fused: all raise, before any collective, or none does)
        raise ValueError(f"count_blobs: settings['mi355x']['neighbour_stats'] is not available under torch.distributed "
                         f"({dist.get_world_size()} ranks): two neighbouring cells can lie on either side of a slab cut, so a Z-slab "
                         "cannot be measured on its own; run step 3 on one device or switch neighbour_stats off")
    if sharded and opts.runs_file:
        # (as for split_fused: all raise, before any collective, or none does)
        raise ValueError(f"count_blobs: settings['mi355x']['label_file'] = \"runs\" is not available under torch.distributed "
                         f"({dist.get_world_size()} ranks): every rank writes its slab into the one dense label file, and the runs of a "
                         "slab are not a part of the volume's run file; run step 3 on one device or leave label_file at \"dense\"")
    if sharded and opts.quartiles:
        # (as for split_fused: all raise, before any collective, or none does)
        raise ValueError(f"count_blobs: settings['mi355x']['intensity_quartiles'] is not available under torch.distributed "
                         f"({dist.get_world_size()} ranks): the values of a cell that crosses a slab cut lie on two ranks, and quantiles "
                         "of parts do not combine; run step 3 on one device or switch intensity_quartiles off")
    if sharded and shell_radius:
        # every rank computes the same slabs: all raise, before any collective, or none does
        thin = [hi - lo for lo, hi in _even_slabs(shape[0], dist.get_world_size()) if hi - lo < shell_radius]
        if thin:
            raise ValueError(f"count_blobs: settings['mi355x']['background_shell'] = {shell_radius} needs Z-slabs of at least {shell_radius} "
                             f"planes on every rank, {shape[0]} planes over {dist.get_world_size()} ranks give slabs of {min(thin)}")
    if sharded and opts.shape:
        # (a face across a cut is judged from the neighbour slab's plane: the same check with a radius of 1)
        thin = [hi - lo for lo, hi in _even_slabs(shape[0], dist.get_world_size()) if hi - lo < 1]
        if thin:
            raise ValueError(f"count_blobs: settings['mi355x']['shape_stats'] needs Z-slabs of at least 1 plane on every rank, "
                             f"{shape[0]} planes over {dist.get_world_size()} ranks give slabs of {min(thin)}")
    raw_vol, raw_file = None, None
    if opts.intensity:  # (before any file is written; under torch.distributed all ranks raise or none does)
        failed = None
        try:
            raw_vol, raw_file = _open_raw_volume(settings, brain, shape)
        except (OSError, ValueError) as exc:
            if not sharded:
                raise
            failed = f"rank {rank}: {exc!r}"
        if sharded:
            _raise_if_any_failed(dist, failed, "count_blobs: opening the raw volume of the intensity statistics")
    prob_vol, prob_file = None, None
    if opts.confidence:  # (as for the raw volume: before any file is written, and all ranks raise or none does)
        failed = None
        try:
            prob_vol, prob_file = _open_prob_volume(path_in, brain, shape)
        except (OSError, ValueError) as exc:
            if not sharded:
                raise
            failed = f"rank {rank}: {exc!r}"
        if sharded:
            _raise_if_any_failed(dist, failed, "count_blobs: opening the probabilities of the confidence statistics")
    path_out = settings["postprocessing"]["output_location"]
    os.makedirs(path_out, exist_ok=True)  # (every rank may get here first)
    len_b = len(os.listdir(path_in))
    start = datetime.datetime.now()
    print(f"{start} Now postprocessing inference for {brain} - {brain_i}/{len_b}")
    brain_path = os.path.join(path_in, brain, "binary_segmentations", "binaries.npy")
    bin_img = np.memmap(brain_path, dtype=np.uint8, mode="r", shape=shape, offset=128)
    eng = engine or shared_engine(int(os.environ.get("LOCAL_RANK", 0)) if sharded else 0)
    if sharded:
        branch = [None]
        if rank == 0:
            try:
                branch[0] = ("cached", bool(load_cached_brain(settings, brain)))
            except Exception as exc:
                branch[0] = ("error", repr(exc))
        dist.broadcast_object_list(branch, src=0)
        if branch[0][0] == "error":
            raise RuntimeError(f"count_blobs: rank 0 failed while looking for a cached labelling: {branch[0][1]}")
        if not branch[0][1]:
            N, stats = _count_blobs_sharded(eng, bin_img, dist, path_out, brain, opts, raw_vol, prob_vol)
            mine = None
            if rank == 0:
                try:
                    with open(os.path.join(path_out, f"{brain}-stats.pickle"), "wb") as fh:
                        pickle.dump(stats, fh, protocol=pickle.HIGHEST_PROTOCOL)
                    with open(path_out + csv_name(bin_img.shape, brain), "wb") as fh:
                        fh.write(cells_csv_bytes(stats, N))
                    _write_tables(path_out, brain, stats, N, opts, raw_file, prob_file)
                    end = datetime.datetime.now()
                    print(f"{end} {brain} {brain_i} / {len_b} Done ({dist.get_world_size()} ranks); Took {end - start}")
                except Exception as exc:
                    mine = f"rank 0: {exc!r}"
            _raise_if_any_failed(dist, mine, "count_blobs: writing the statistics / CSV")
            return N
        if rank != 0:
            # a cached labelling exists: rank 0 alone re-uses it (and writes the statistics / CSV), the others wait for
            # N - or for the error rank 0 ran into
            box = [None]
            dist.broadcast_object_list(box, src=0)
            if isinstance(box[0], tuple):
                raise RuntimeError(f"count_blobs: rank 0 failed on the cached labelling: {box[0][1]}")
            return box[0]
    result = [("error", "rank 0 did not finish")]
    try:
        import time

        N, stats, labels_written = _count_blobs_single(settings, brain, bin_img, eng, path_out, start, opts, raw_vol, prob_vol)
        t_csv = time.perf_counter()
        with open(path_out + csv_name(bin_img.shape, brain), "wb") as fh:
            fh.write(cells_csv_bytes(stats, N))  # (the text pandas writes for the reference, formatted by the library: dlv_cells_csv)
        _write_tables(path_out, brain, stats, N, opts, raw_file, prob_file)
        count_blobs.last_timings["csv_s"] = time.perf_counter() - t_csv
        t_join = time.perf_counter()
        if defer_write:
            hostio.submit_deferred(eng, labels_written)
        else:
            labels_written()  # the label volume has been streaming into its file since the labelling finished
        count_blobs.last_timings["wait_for_labels_s"] = time.perf_counter() - t_join
        result = [N]
    except Exception as exc:
        result = [("error", repr(exc))]
        raise
    finally:
        if sharded:  # always: N, or the error the waiting ranks re-raise
            dist.broadcast_object_list(result, src=0)
    end = datetime.datetime.now()
    print(f"{end} {brain} {brain_i} / {len_b} Done; Took {end - start}")
    return N


def _count_blobs_single(settings, brain, bin_img, eng, path_out, start, opts=CountOptions(), raw_vol=None, prob_vol=None):
    """The one-device path (also rank 0 of a sharded run that found a cached labelling): returns (N, stats, wait) - wait()
    returns when the label file is complete (it is written by a side thread while the statistics, the pickle and the CSV are
    made: 17 GB at the 4-7 GB/s one file takes from the kernel) and re-raises what that thread ran into.  opts: the opt-in keys
    (hostlogic.CountOptions).  A fresh labelling is split, then filtered, between dlv_ccl26_dev and the label write - the two
    scratch volumes of the split are gone before the raw volume is uploaded, so the two peaks do not add.  The labels - fresh or
    cached - are measured after cc_stats: what hostlogic.measuring_plan finds missing, from one upload of raw_vol (_measure_raw), then
    the confidence from one upload of prob_vol (_measure_confidence: the raw tensor is gone by then), then the shape accumulators,
    then the depth (HipEngine.cc_depth), then the neighbour table (HipEngine.cc_neighbours); the pickle is written once, after the
    last of these."""
    import time

    bounds, split = opts.bounds, opts.split
    labels_dev = None
    wait = lambda: None  # noqa: E731
    tm = count_blobs.last_timings = {}
    t_prev = [time.perf_counter()]

    def mark(name):
        now = time.perf_counter()
        tm[name + "_s"] = now - t_prev[0]
        t_prev[0] = now
    try:
        cached = load_cached_brain(settings, brain)
        # (a dense cache wins, as without the key; without one, and with label_file = "runs", a run file is the cached labelling)
        cached_runs = load_cached_runs(settings, brain) if opts.runs_file and not cached else False
        runs = None
        from .streaming import ccl_bytes_per_voxel, ccl_streamed, hbm_budget_bytes

        budget = hbm_budget_bytes(eng, settings)
        need = int(bin_img.size) * ccl_bytes_per_voxel()
        Z = int(bin_img.shape[0])
        fresh = not cached and not cached_runs
        if fresh:  # (size_filter is judged here too: refused exactly when the mask would be slab-streamed)
            check_hbm_budget(opts, measuring_plan(opts, None), False, ccl_bytes_per_voxel(), int(bin_img.size), budget)
        if fresh and need > budget:
            # the mask + its uint32 labels do not fit this GPU: Z-slabs through the device, seams merged on the host
            # (streaming.py) - the reference's counterpart is cc3d writing into an out_file memmap (:59-64)
            plane = int(bin_img.shape[1]) * int(bin_img.shape[2]) * ccl_bytes_per_voxel()
            n_slabs = -(-need // max(budget, 1))
            if plane > budget or n_slabs > bin_img.shape[0]:
                raise MemoryError(f"delivr_cfos_amd (DLV_ENOMEM): one mask plane with its labels and scratch needs {plane / 2**20:.1f} MiB, "
                                  f"the HBM budget is {budget / 2**20:.1f} MiB; raise settings['mi355x']['hbm_budget_gb']")
            print(f"No cached brain found; mask + labels of {need / 2**30:.1f} GiB exceed the HBM budget of {budget / 2**30:.1f} GiB: "
                  f"connected components on {n_slabs} Z-slabs...")
            made = {}

            def create_output(n):
                # written under a name load_cached_brain does NOT match (no '.npy' suffix) and renamed when pass 2 has finished:
                # a run killed while it renumbers the slabs must not leave a complete-looking label file behind as a cache
                made["path"] = os.path.join(path_out, f"{brain}-{n}-cc3d.npy")
                made["tmp"] = os.path.join(path_out, f".{brain}-{n}-cc3d.partial")
                return np.lib.format.open_memmap(made["tmp"], mode="w+", dtype=_label_dtype(n), shape=tuple(bin_img.shape))

            N, stats = ccl_streamed(eng, bin_img, int(n_slabs), os.path.join(path_out, f".{brain}-provisional-u32.tmp"), create_output)
            if made:
                os.replace(made["tmp"], made["path"])
            with open(os.path.join(path_out, f"{brain}-stats.pickle"), "wb") as fh:
                pickle.dump(stats, fh, protocol=pickle.HIGHEST_PROTOCOL)
            return N, stats, wait
        if fresh:
            print("No cached brain found, performing connected components on the GPU...")
            # binaries.npy -> HBM and the label volume -> its .npy both stream through pinned staging with parallel
            # readers / writers (hostio.py): 4.3 GB in and 17 GB out for a 1024 x 2048 x 2048 brain, around 20 ms of kernels
            mask_dev = hostio.upload(eng, bin_img, what="h2d_mask")
            mark("upload")
            filled = None
            if opts.fill_holes:
                filled = eng.fill_holes(mask_dev, FILL_VALUE)
                mark("fill_holes")
            labels_dev, N = eng.ccl26(mask_dev)
            if filled is None:
                del mask_dev
            mark("ccl26")
            if filled is not None:
                _note_fill(filled[0], filled[1], N)
            split_parent = None
            if split is not None:
                n_components = N
                N, split_parent, components_split = eng.cc_split(labels_dev, N, split[0], split[1])
                _note_split(split, n_components, N, components_split)
                mark("split")
            elif opts.split_depth is not None:
                n_components = N
                core_d2, fraction, min_core, spacing = opts.split_depth
                N, split_parent, components_split = eng.cc_split_depth(labels_dev, N, spacing, core_d2, fraction, min_core)
                _note_split_depth(opts.split_depth, (settings.get("mi355x") or {}).get("split_radius"), n_components, N, components_split)
                mark("split")
            if opts.filter_active:
                n_before = N
                counts_dev = eng.cc_counts(labels_dev, N)
                N = eng.cc_size_filter(labels_dev, N, bounds[0], bounds[1], counts=counts_dev)
                counts = counts_dev.cpu().numpy().view(np.uint32).astype(np.uint64)
                _note_filter(bounds, n_before, N, int(counts[1:][~_keep_mask(counts, bounds)[1:]].sum()))
                if split_parent is not None:  # (the rows of the cells the filter kept, in their order)
                    split_parent = np.concatenate([split_parent[:1], split_parent[1:][_keep_mask(counts, bounds)[1:]]])
                del counts_dev
                mark("size_filter")
            hole_voxels = None
            if filled is not None:  # (under the final labels; the filled voxels of the cells the filter removed carry label 0)
                hole_voxels = eng.cc_count_marked(labels_dev, mask_dev, N, FILL_VALUE).cpu().numpy().view(np.uint32).copy()
                hole_voxels[0] = 0
                del mask_dev
                mark("hole_voxels")
            from concurrent.futures import ThreadPoolExecutor

            writer = ThreadPoolExecutor(max_workers=1, thread_name_prefix="dlv-labels")
            if opts.runs_file:
                # the labels are coded in HBM: megabytes of runs cross PCIe and reach <brain>-<N>-cc3d.runs, no dense file is written
                # (as below: <name>.partial and a rename, on a side thread - which touches host arrays only)
                fresh_runs = eng.cc_runs_encode(labels_dev)
                mark("runs_encode")
                fut = writer.submit(label_runs.save_runs, os.path.join(path_out, label_runs.runs_name(brain, N)), fresh_runs, N)
                del fresh_runs
            else:
                final = os.path.join(path_out, f"{brain}-{N}-cc3d.npy")
                # (written as <name>.partial and renamed: never a partly written file under the cache's name) - by a side thread that
                # touches torch's copy stream only, never the context, while this thread goes on to the statistics and the CSV
                file_labels = _labels_in_file_dtype(labels_dev, N)
                eng.sync()
                fut = writer.submit(hostio.save_npy, eng, file_labels, final, _label_dtype(N), "d2h_labels", True, True)

            def wait(fut=fut, writer=writer):
                try:
                    fut.result()
                finally:
                    writer.shutdown(wait=True)

            labels = None
            mark("start_label_write")
        else:
            if cached_runs:
                cached, N = cached_runs
                runs = label_runs.load_runs(cached)  # (validated in full before anything is decoded or uploaded)
                if runs["n"] != N or tuple(runs["shape"]) != tuple(int(v) for v in bin_img.shape):
                    raise ValueError(f"count_blobs: {cached} holds {runs['n']} components of a volume of shape {tuple(runs['shape'])}, its "
                                     f"name and the mask say {N} components and {tuple(int(v) for v in bin_img.shape)}")
            else:
                N = int(cached.split("/")[-1].split("-")[1])
            print(f"Cached brain found at {cached} with {N} components, loading...")
            if opts.filter_active:
                print(f"size filter: the cached labelling is reused as it is, min_size {bounds[0]} / max_size {bounds[1]} are not applied to it")
            if split is not None:
                print(f"split of fused cells: the cached labelling is reused as it is, it is not split (depth {split[0]}) again")
            if opts.split_depth is not None:
                print(f"split of fused cells: the cached labelling is reused as it is, it is not split (core_d2 {opts.split_depth[0]}, "
                      f"fraction {opts.split_depth[1]} %) again")
            if opts.fill_holes:
                print("fill of holes: the cached labelling is reused as it is, its holes are not filled")
            split_parent, hole_voxels, filled = None, None, None
            labels = None if runs is not None else np.load(cached, mmap_mode="r")
        mid = datetime.datetime.now()
        print(f"{mid} labelling+writing/loading took {mid - start} : {N}")
        cached_stats = load_cached_stats(settings, brain)

        def cached_labels_to_device():
            import torch

            if runs is not None:  # (decoded in HBM from the runs: only they cross PCIe)
                return eng.cc_runs_decode(runs)
            if labels.dtype == np.uint32:
                return hostio.upload(eng, labels, what="h2d_labels")
            if labels.dtype == np.uint16:  # widened in HBM, not on the host
                return hostio.upload(eng, labels, what="h2d_labels").view(torch.int16).to(torch.int32) & 0xFFFF
            return torch.from_numpy(np.ascontiguousarray(labels).astype(np.uint32).view(np.int32)).to(eng.device)

        def write_stats(path):
            with open(path, "wb") as fh:
                pickle.dump(stats, fh, protocol=pickle.HIGHEST_PROTOCOL)

        stats = None
        if cached_stats:
            print(f"Found stats at {cached_stats}")
            with open(cached_stats, "rb") as fh:
                stats = pickle.load(fh)
        plan = measuring_plan(opts, stats)  # (what the cached pickle lacks; without one, all that is asked for)
        if labels_dev is None:
            # (a run file is decoded only when something is still to be measured; with a complete pickle nothing is uploaded)
            check_hbm_budget(opts, plan, True, 4, int(bin_img.size if runs is not None else labels.size), budget,
                             runs_decoded=runs is not None and bool(plan or not cached_stats))
        if not cached_stats:
            if labels_dev is None and runs is None and int(labels.size) * 4 > budget:
                # cached labels that do not fit the HBM budget: statistics slab by slab (raw sums add up; streaming.py)
                from .streaming import stats_streamed

                stats = stats_streamed(eng, labels, N, budget)
            else:
                if labels_dev is None:
                    labels_dev = cached_labels_to_device()
                stats = eng.cc_stats(labels_dev, N)
            if split_parent is not None:
                stats.update(finish_split(split_parent, count_blobs.last_split["n_before"]))
                if split is not None:
                    stats["split_depth"] = int(split[0])
                else:
                    stats["split_core_d2"], stats["split_fraction"] = int(opts.split_depth[0]), int(opts.split_depth[1])
                    stats["split_spacing"] = tuple(int(w) for w in opts.split_depth[3])
            if hole_voxels is not None:
                stats["hole_voxels"], stats["holes_filled"] = hole_voxels, int(filled[1])
            if not plan:
                write_stats(os.path.join(path_out, f"{brain}-stats.pickle"))
            mark("stats")
        elif hole_voxels is not None:  # (a pickle found beside a fresh labelling is completed, as for the measured keys)
            stats["hole_voxels"], stats["holes_filled"] = hole_voxels, int(filled[1])
            write_stats(cached_stats)
        if plan & RAW_GROUPS:
            if labels_dev is None:
                labels_dev = cached_labels_to_device()
            got = _measure_raw(eng, labels_dev, raw_vol[:Z], N, opts, plan)
            if got.cells is not None:
                stats.update(finish_intensity(got.cells, stats["voxel_counts"]))
            if got.shell is not None:
                stats.update(finish_shell(*got.shell, stats["intensity_mean"]))
                stats["shell_radius"] = int(opts.shell_radius)
            if got.cell_quartiles is not None:
                stats.update(finish_quartiles(*got.cell_quartiles, stats["voxel_counts"]))
            if got.shell_quartiles is not None:
                stats.update(finish_shell_quartiles(*got.shell_quartiles, stats["shell_voxels"], stats["intensity_median"]))
            # (a cached pickle without the keys is rewritten: the keys added, its entries untouched)
            if not plan & {"confidence", "shape", "depth", "neighbours"}:
                write_stats(cached_stats or os.path.join(path_out, f"{brain}-stats.pickle"))
            mark("intensity")
            if opts.quartiles:  # (HipEngine.cc_quantiles is synchronous: its share of the time since the last mark)
                tm["intensity_s"] -= got.quartiles_s
                tm["quartiles_s"] = got.quartiles_s
        if "confidence" in plan:
            if labels_dev is None:
                labels_dev = cached_labels_to_device()
            stats.update(finish_confidence(_measure_confidence(eng, labels_dev, prob_vol, N), stats["voxel_counts"], bin_img.shape))
            if not plan & {"shape", "depth", "neighbours"}:
                write_stats(cached_stats or os.path.join(path_out, f"{brain}-stats.pickle"))  # (as above: completed, not replaced)
            mark("confidence")
        if "shape" in plan:
            if labels_dev is None:
                labels_dev = cached_labels_to_device()
            stats.update(finish_shape(eng.cc_shape(labels_dev, N), stats["voxel_counts"]))
            if not plan & {"depth", "neighbours"}:
                write_stats(cached_stats or os.path.join(path_out, f"{brain}-stats.pickle"))  # (as above: completed, not replaced)
            mark("shape")
        if "depth" in plan:
            if labels_dev is None:
                labels_dev = cached_labels_to_device()
            # (the two scratch volumes of the distance map are gone when cc_depth returns)
            stats.update(finish_depth(eng.cc_depth(labels_dev, N, opts.depth), stats["voxel_counts"], bin_img.shape, opts.depth))
            if "neighbours" not in plan:
                write_stats(cached_stats or os.path.join(path_out, f"{brain}-stats.pickle"))  # (as above: completed, not replaced)
            mark("depth")
        if "neighbours" in plan:
            if labels_dev is None:
                labels_dev = cached_labels_to_device()
            radius_sq, spacing = opts.neighbours
            # (the pair table and the outputs are sized from the count and checked against the HBM budget in there)
            stats.update(finish_neighbours(eng.cc_neighbours(labels_dev, N, spacing, radius_sq, settings=settings), N, radius_sq, spacing))
            write_stats(cached_stats or os.path.join(path_out, f"{brain}-stats.pickle"))  # (as above: completed, not replaced)
            mark("neighbours")
    except BaseException:
        try:
            wait()  # (do not leave the writer thread behind an error of this one)
        except Exception:
            pass
        raise
    # note: the reference takes min_size / max_size and never reads them (count_blobs.py:105); here they apply with
    # settings["mi355x"]["size_filter"] (above, right after the labelling)
    return N, stats, wait
