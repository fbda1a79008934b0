"""What settings["mi355x"]["neighbour_stats"] costs in step 3, and where the time goes (profiles/README.md, "cc_neighbours").  One
process, one device.

Step wall: count_blobs file to file on tmpfs on the bench's synthetic cell mask (the c3 brain, seed 2, raw > 6500; default
1024 x 2048 x 2048) with label_file = "runs" in every arm (the 17 GB dense label file and the spread of its write are not what is
compared): no key, neighbour_stats = 8 at spacing [1, 1, 1] and neighbour_stats = 80 at spacing [37, 10, 10] - alternating, three
runs each in fresh folders after one unmeasured warm-up of each.  neighbours_s is the measurement (the two scans, the compaction,
the sort and hostlogic.neighbour_summary), csv_s the formatting of every table of the run.

Kernel time: HipEngine.cc_neighbours on the labels of the same mask at both settings, the DlvProf brackets of the library (count,
table - which includes the clearing of the table -, compact) as means of `reps` calls after a warm-up, beside cc_stats_kernel on the
same labels and torch's copy of a uint32 volume of the mask's size in the same process.  The floor of a scan is one read of the
labels, 4 bytes per voxel, at the copy's rate.  Checked in the script: the table of a crop of 12 x 128 x 256 voxels from the middle
of the volume equals the numpy statement of tests/helpers/neighbour_reference.py.  One JSON line each.       python profiles/cc_neighbours_perf.py [folder [Z [reps]]]"""
import importlib.util
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ARMS = {"none": {}, "r8_111": {"neighbour_stats": 8, "depth_spacing": [1, 1, 1]},
        "r80_37_10_10": {"neighbour_stats": 80, "depth_spacing": [37, 10, 10]}}
CROP = (12, 128, 256)  # voxels compared with the numpy reference (17^3 shifted comparisons of the crop at a reach of 8)


def _reference():
    spec = importlib.util.spec_from_file_location("neighbour_reference", os.path.join(ROOT, "tests", "helpers", "neighbour_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cell_mask(shape, device):
    from delivr_cfos_amd.synth import synth_volume_torch

    return (synth_volume_torch(shape, 2, device).view(torch.int16) > 6500).to(torch.uint8)


def _copy_rate(voxels, device, reps):
    """bytes per second of dst.copy_(src) on two uint32 volumes of `voxels`: 8 bytes per voxel"""
    src = torch.zeros(voxels, dtype=torch.int32, device=device)
    dst = torch.empty_like(src)
    dst.copy_(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        dst.copy_(src)
    b.record()
    b.synchronize()
    return voxels * 8 * reps / (a.elapsed_time(b) * 1e-3)


def main(base, Z, reps):
    from delivr_cfos_amd import hostio
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.engine import shared_engine
    from delivr_cfos_amd.hostlogic import neighbour_stats_settings

    shape = (Z, 2048, 2048)
    vox = Z * 2048 * 2048
    d = tempfile.mkdtemp(prefix="dlv_neighbours_", dir=base)
    try:
        eng = shared_engine(0)
        cells = _cell_mask(shape, eng.device)
        seg = os.path.join(d, "in", "brain", "binary_segmentations")
        os.makedirs(seg)
        hostio.save_npy(eng, cells, os.path.join(seg, "binaries.npy"), np.uint8, what="d2h_mask")
        path_in = os.path.join(d, "in")

        def run(tag, arm):
            post = os.path.join(d, tag)
            settings = {"postprocessing": {"output_location": post + "/"}, "mi355x": {"label_file": "runs", **ARMS[arm]}}
            t0 = time.perf_counter()
            n = count_blobs(settings, path_in, 0, "brain", (1, 1) + shape)
            wall = time.perf_counter() - t0
            shutil.rmtree(post)
            return {"arm": arm, "wall_s": round(wall, 4), "n": int(n), "last_neighbours": count_blobs.last_neighbours,
                    "timings": {k: round(v, 4) for k, v in count_blobs.last_timings.items()}}

        for arm in ARMS:  # the unmeasured warm-up: context, workspaces, pinned staging
            run(f"warm_{arm}", arm)
        results = [run(f"run_{arm}_{k}", arm) for k in range(3) for arm in ARMS]
        of = lambda arm, key: [r["timings"].get(key) if key != "wall_s" else r["wall_s"] for r in results if r["arm"] == arm]  # noqa: E731
        print(json.dumps({"shape": shape, "files_on": base, "runs": results,
                          "median_wall_s": {arm: statistics.median(of(arm, "wall_s")) for arm in ARMS},
                          "min_max_wall_s": {arm: [min(of(arm, "wall_s")), max(of(arm, "wall_s"))] for arm in ARMS},
                          "median_neighbours_s": {arm: statistics.median(of(arm, "neighbours_s")) for arm in ARMS if arm != "none"},
                          "median_csv_s": {arm: statistics.median(of(arm, "csv_s")) for arm in ARMS}}), flush=True)

        torch.cuda.empty_cache()
        copy = _copy_rate(vox, eng.device, reps)
        torch.cuda.empty_cache()
        labels, n = eng.ccl26(cells)
        del cells
        ref = _reference()
        z0 = max(0, Z // 2 - CROP[0] // 2)
        crop = labels[z0:z0 + CROP[0], 1024:1024 + CROP[1], 1024:1024 + CROP[2]].contiguous()
        crop_np = crop.cpu().numpy().view(np.uint32)
        for arm in ("r8_111", "r80_37_10_10"):
            radius_sq, spacing = neighbour_stats_settings({"mi355x": ARMS[arm]})
            want = ref.neighbour_table(crop_np, n, spacing, radius_sq)
            assert len(want) > 0
            ref.assert_table_equal(eng.cc_neighbours(crop, n, spacing, radius_sq), want)
            table = eng.cc_neighbours(labels, n, spacing, radius_sq)  # warm-up, outside the timed window
            eng.cc_stats(labels, n)
            eng.prof_enable(True)
            eng.prof_reset()
            for _ in range(reps):
                eng.cc_neighbours(labels, n, spacing, radius_sq)
                eng.cc_stats(labels, n)
            eng.sync()
            rep = eng.prof_report()
            eng.prof_enable(False)
            ms = {k: round(v["total_ms"] / v["launches"], 4) for k, v in rep.items() if k.startswith("cc_") and v["launches"]}
            S, P = table["segments"], len(table["gap_sq"])
            bound = min(S, n * (n - 1) // 2)
            cap = 1 << (2 * bound - 1).bit_length() if bound else 0
            floor_ms = vox * 4 / copy * 1e3
            print(json.dumps({"input": "cell mask", "shape": shape, "n": n, "spacing": spacing, "radius_sq": radius_sq, "reps": reps,
                              "segments": S, "pairs": P, "table_slots": cap, "table_MiB": round(cap * 16 / 2**20, 1),
                              "copy_GBps": round(copy / 1e9, 1), "floor_ms": round(floor_ms, 4), "ms_per_call": ms,
                              "count_to_floor": round(ms["cc_neighbours_count"] / floor_ms, 2) if "cc_neighbours_count" in ms else None,
                              "table_to_floor": round(ms["cc_neighbours_table"] / floor_ms, 2) if "cc_neighbours_table" in ms else None}),
                  flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/dev/shm", int(sys.argv[2]) if len(sys.argv) > 2 else 1024,
         int(sys.argv[3]) if len(sys.argv) > 3 else 3)
