"""Mirror of the reference's ``blob_highlighter.py`` (blob_highlighter :38-169): colour every detected cell by its atlas
region, on the device.  Same call, same inputs, same plane files:

in : <input_prediction_location>/<dir containing brain>/binary_segmentations/binaries.npy  ('|u1', (Z,Y,X), 128-byte header)  (:62)
     <input_csv_location>/cells_<brain>*.csv  columns connected_component_id, acronym, red, green, blue, graph_order          (:66-71)
     <postprocessing.output_location>/<brain>-stats.pickle when present, else CCL-26 + statistics on the device              (:78-92)
out: <output_location>/<brain>_rgb_tiffs/<brain>rgb_C0{0,1,2}_z####.tif     uint8   (region_id_rgb, :94-133)
     <output_location>/<brain>/<brain>_region_id_tiffs/region_id_####.tif   uint16  (region_id_grayvalues, :137-161)

The per-cell loop (bounding box x colour, later boxes overwrite earlier ones) is one scatter + one gather on the GPU
(csrc/paint.hip); the box arithmetic, including pad_bb's in-place mutation of the statistics between the two loops, is
hostlogic.padded_boxes.  Planes are written as LZW-compressed TIFF like the reference's (native writer, tiffio.py).

settings["mi355x"]["paint_from"] = "labels" (opt-in; "boxes", the default, is everything above, byte for byte) colours every voxel
by its OWN label instead: the same files, names, dtypes and LZW planes, but a voxel holds the value of the cell whose label it
carries and 0 elsewhere (csrc/cc_paint.hip).  The boxes are gone, and with them what only boxes brought: no padding of the box,
no second padding for the region-id planes, no "might accidentally re-color other blobs close by" (:110) where boxes of
neighbouring cells overlap - which for the siblings count_blobs' split_fused cuts out of one fused component is nearly everywhere.
The labels are those of count_blobs, looked up in its cache order: a dense <brain>-<N>-cc3d.npy, else the run-length file
<brain>-<N>-cc3d.runs (painted straight from the runs, the label volume is never built), else binaries.npy is labelled again on
the device; with a label file binaries.npy is not read at all.  The volume is painted in Z-slabs of at most _SLAB_BYTES, each
downloaded and written before the next one is painted, so the host never holds more than a slab.  no_atlas_depthmap is unaffected.
"""
from __future__ import annotations

import csv
import datetime
import os
import pickle

import numpy as np

from . import label_runs
from .hostlogic import padded_boxes, paint_luts, paint_source
from .tiffio import write_tiff_plane

_SLAB_BYTES = 2 << 30  # "labels" mode: the labels of a Z-slab in HBM plus all of its output planes


def load_cached_stats(settings, brain):
    """reference :25-36"""
    from .count_blobs import _find_cached

    return _find_cached(settings["postprocessing"]["output_location"], ".pickle", brain)


def read_cell_table(path: str) -> dict:
    """pd.read_csv(path, index_col=0) + the 'bgr' filter (:70-71) without pandas: columns as numpy arrays."""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    head = rows[0]
    col = {name: i for i, name in enumerate(head)}
    for need in ("connected_component_id", "acronym", "red", "green", "blue", "graph_order"):
        if need not in col:
            raise KeyError(f"{path}: column {need!r} missing")
    body = [r for r in rows[1:] if r and r[col["acronym"]] != "bgr"]

    def ints(name):
        return np.array([int(float(r[col[name]])) for r in body], dtype=np.int64)

    return {"connected_component_id": ints("connected_component_id"), "red": ints("red"), "green": ints("green"),
            "blue": ints("blue"), "graph_order": ints("graph_order")}


def plan_slabs(Z: int, plane_voxels: int, bytes_per_voxel: int):
    """The Z-slabs [(z0, z1), ...] of the "labels" painting: whole planes, in order, covering [0, Z) once; as many planes as
    _SLAB_BYTES holds at bytes_per_voxel (labels + output planes), never less than one."""
    step = max(1, int(_SLAB_BYTES) // max(1, int(plane_voxels) * int(bytes_per_voxel)))
    return [(z, min(z + step, int(Z))) for z in range(0, int(Z), step)]


def _open_labels(settings, brain, shape, path_brain_binary, eng):
    """The labels of the "labels" painting, in count_blobs' cache order -> (N, label bytes per voxel a slab holds in HBM,
    labels_of(z0, z1)): labels_of gives the planes [z0, z1) as an int32 tensor in HBM, or - for a run file - the runs themselves."""
    import torch

    from .count_blobs import load_cached_brain, load_cached_runs

    cached = load_cached_brain(settings, brain)
    if cached:
        name = os.path.basename(cached).split("-")
        if len(name) < 2 or not name[-2].isdigit():
            raise ValueError(f"blob_highlighter: {cached}: no component count in the name of the label file (<brain>-<N>-cc3d.npy)")
        n = int(name[-2])
        labels = np.load(cached, mmap_mode="r")
        if labels.dtype == np.uint64:
            raise ValueError(f"blob_highlighter: {cached} holds uint64 labels; the painter takes labels below 2^32 - 1 (uint16 / uint32 files)")
        if tuple(labels.shape) != shape:
            raise ValueError(f"blob_highlighter: {cached} has shape {tuple(labels.shape)}, the stack is {shape}")
        print(f"Painting from the labels of {cached} ({n} components)")

        def dense(z0, z1):
            part = np.array(labels[z0:z1])  # (one slab of the memmap)
            if part.dtype == np.uint16:  # widened in HBM, not on the host
                return torch.from_numpy(part.view(np.int16)).to(eng.device).to(torch.int32) & 0xFFFF
            return torch.from_numpy(part.astype(np.uint32, copy=False).view(np.int32)).to(eng.device)

        return n, labels.dtype.itemsize + (4 if labels.dtype.itemsize < 4 else 0), dense
    cached_runs = load_cached_runs(settings, brain)
    if cached_runs:
        path, n = cached_runs
        runs = label_runs.load_runs(path)  # (validated in full before anything is uploaded)
        if runs["n"] != n or tuple(runs["shape"]) != shape:
            raise ValueError(f"blob_highlighter: {path} holds {runs['n']} components of a volume of shape {tuple(runs['shape'])}, its "
                             f"name and the stack say {n} components and {shape}")
        print(f"Painting from the runs of {path} ({n} components)")
        return n, 0, lambda z0, z1: runs
    print(f"{datetime.datetime.now()} : No label file found, labelling the brain")
    bin_img = np.memmap(path_brain_binary, dtype=np.uint8, mode="r", shape=shape, offset=128)
    labels_dev, n = eng.ccl26(eng.to_device(np.ascontiguousarray(bin_img)))
    cached_stats = load_cached_stats(settings, brain)
    if cached_stats:
        with open(cached_stats, "rb") as fh:
            n_stats = len(pickle.load(fh)["bounding_boxes"]) - 1
        if n_stats != n:
            raise ValueError(f"blob_highlighter: {cached_stats} describes {n_stats} components, labelling binaries.npy again found {n}: "
                             "the cells of that run were split or filtered after the labelling, and their ids are not the labels "
                             "found here; painting from the labels needs the label file of that run (<brain>-<N>-cc3d.npy or .runs)")
    return n, 4, lambda z0, z1: labels_dev[z0:z1]


def _highlight_from_labels(settings, brain, shape, cells, path_brain_binary, path_out, path_out_rgb, eng):
    """the "labels" mode of blob_highlighter (module docstring): both requested outputs of a slab come from one kernel pass"""
    viz = settings["visualization"]
    want_rgb, want_gray = bool(viz.get("region_id_rgb")), bool(viz.get("region_id_grayvalues"))
    n, label_bytes, labels_of = _open_labels(settings, brain, shape, path_brain_binary, eng)
    rgb, region = paint_luts(cells["connected_component_id"], cells["red"], cells["green"], cells["blue"], cells["graph_order"], n)
    print(f"{datetime.datetime.now()} : Generating region_id gray-value tiffs")
    if want_gray:
        path_out_region_id = os.path.join(path_out, brain, brain + "_region_id_tiffs")
        os.makedirs(path_out_region_id, exist_ok=True)
    if not (want_rgb or want_gray):
        return
    luts = {"rgb": rgb if want_rgb else None, "u16": region if want_gray else None}
    per_voxel = label_bytes + (3 if want_rgb else 0) + (2 if want_gray else 0)
    print(f"{datetime.datetime.now()} : coloring blobs by their labels")
    for z0, z1 in plan_slabs(shape[0], shape[1] * shape[2], per_voxel):
        src = labels_of(z0, z1)
        planes = eng.paint_runs(src, z0, z1, **luts) if isinstance(src, dict) else eng.paint_labels(src, **luts)
        del src
        chans, gray = planes if want_rgb and want_gray else ((planes, None) if want_rgb else (None, planes))
        if want_rgb:
            for c, img in enumerate(chans):
                host = img.cpu().numpy()
                for z in range(z0, z1):
                    write_tiff_plane(os.path.join(path_out_rgb, brain + f"rgb_C0{c}_z" + str(z).zfill(4) + ".tif"), host[z - z0])
        if want_gray:
            host = gray.cpu().numpy()
            for z in range(z0, z1):
                write_tiff_plane(os.path.join(path_out_region_id, "region_id_" + str(z).zfill(4) + ".tif"), host[z - z0])
        del planes, chans, gray


def blob_highlighter(settings, brain_item, stack_shape, engine=None):
    """Same positional parameters as the reference (:38).  ``engine``: a HipEngine to reuse."""
    import torch

    from .engine import HipEngine

    brain = brain_item[0]
    viz = settings["visualization"]
    if viz.get("no_atlas_depthmap"):
        # "only map the blobs over their distance from the sample's outside" (:163-165; no atlas, hence no cell table -
        # the reference skips loading it at :67-69).  Its depth_map_blobs cannot run (IndexError at blob_depthmap.py:139);
        # the mirror implements what the function states after that line (blob_depthmap.py in this package)
        from .blob_depthmap import depth_map_blobs

        depth_map_blobs(settings, brain, stack_shape, engine=engine)
        print(f"{datetime.datetime.now()} : Cleanup")
        return
    mode = paint_source(settings)  # (a wrong key is refused before any file is touched)
    path_binary = viz["input_prediction_location"]
    path_cell_csv = viz["input_csv_location"]
    path_out = viz["output_location"]
    path_out_rgb = os.path.join(path_out, brain + "_rgb_tiffs")
    os.makedirs(path_out_rgb, exist_ok=True)
    path_brain_binary = path_binary + [x for x in os.listdir(path_binary) if brain in x][0] + "/binary_segmentations/binaries.npy"
    path_brain_cell_csv = path_cell_csv + [x for x in os.listdir(path_cell_csv) if "cells_" + brain in x and ".csv" in x][0]
    print(path_brain_cell_csv)
    print(f"{datetime.datetime.now()} : Loading csv")
    cells = read_cell_table(path_brain_cell_csv)
    ids = cells["connected_component_id"]
    if len(np.unique(ids)) != len(ids):
        raise ValueError("connected_component_id values must be unique (the reference's broadcast fails on duplicates, :156)")
    print(f"{datetime.datetime.now()} : Loading brain")
    shape = tuple(int(v) for v in stack_shape[2:])
    if mode == "labels":
        eng = engine or HipEngine(0)
        try:
            _highlight_from_labels(settings, brain, shape, cells, path_brain_binary, path_out, path_out_rgb, eng)
        finally:
            if engine is None:
                eng.close()
        print(f"{datetime.datetime.now()} : Cleanup")
        return
    bin_img = np.memmap(path_brain_binary, dtype=np.uint8, mode="r", shape=shape, offset=128)
    own = engine is None
    eng = engine or HipEngine(0)
    try:
        bin_dev = eng.to_device(np.ascontiguousarray(bin_img))
        cached = load_cached_stats(settings, brain)
        if not cached:
            labels, n = eng.ccl26(bin_dev)
            stats = eng.cc_stats(labels, n)
            del labels
        else:
            print(f"Found stats at {cached}")
            with open(cached, "rb") as fh:
                stats = pickle.load(fh)
        bboxes = np.asarray(stats["bounding_boxes"])
        if len(ids) and int(ids.max()) >= len(bboxes):
            raise IndexError("connected_component_id beyond the statistics table")
        pads = 0
        if viz.get("region_id_rgb"):
            print(f"{datetime.datetime.now()} : coloring blobs")
            pads += 1
            boxes = padded_boxes(bboxes, ids, shape, pads)
            chans = eng.paint_boxes(bin_dev, boxes, [cells[c].astype(np.uint8) for c in ("red", "green", "blue")])
            print(f"{datetime.datetime.now()} : Generating RGB tiffs")
            for c, img in enumerate(chans):
                host = img.cpu().numpy()
                for z in range(shape[0]):
                    write_tiff_plane(os.path.join(path_out_rgb, brain + f"rgb_C0{c}_z" + str(z).zfill(4) + ".tif"), host[z])
            del chans
        print(f"{datetime.datetime.now()} : Generating region_id gray-value tiffs")
        if viz.get("region_id_grayvalues"):
            path_out_region_id = os.path.join(path_out, brain, brain + "_region_id_tiffs")
            os.makedirs(path_out_region_id, exist_ok=True)
            pads += 1  # pad_bb already moved these boxes once if the RGB loop ran (in-place mutation of the statistics)
            boxes = padded_boxes(bboxes, ids, shape, pads)
            (rid,) = eng.paint_boxes(bin_dev, boxes, [cells["graph_order"].astype(np.uint16)])
            host = rid.cpu().numpy()
            for z in range(shape[0]):
                write_tiff_plane(os.path.join(path_out_region_id, "region_id_" + str(z).zfill(4) + ".tif"), host[z])
    finally:
        if own:
            eng.close()
    print(f"{datetime.datetime.now()} : Cleanup")
