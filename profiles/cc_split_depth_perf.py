"""What settings["mi355x"]["split_radius"] costs in step 3 beside no split and beside split_fused, and where the time goes
(profiles/README.md, "cc_split_depth").  One process, one device.

Step wall: count_blobs file to file on tmpfs on the bench's synthetic cell mask (the c3 brain, seed 2, raw > 6500; default
1024 x 2048 x 2048) with label_file = "runs" in every arm (the 17 GB dense label file and the spread of its write are not what is
compared): no split key, split_fused = 2, split_radius = 1.5 at spacing [1, 1, 1] and split_radius = 15 at spacing [37, 10, 10] -
alternating, three runs each in fresh folders after one unmeasured warm-up of each.

Kernel time: HipEngine.cc_split_depth on the labels of the same mask at both spacings, the DlvProf brackets of the library (the
three depth passes, the threshold kernel, the growth, the numbering) as means of `reps` calls after a warm-up, beside torch's copy of a
uint32 volume of the mask's size in the same process; the threshold kernel moves 9 bytes per voxel (labels and map read, mask written).
One JSON line each.       python profiles/cc_split_depth_perf.py [folder [Z [reps]]]"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

ARMS = {"none": {}, "split_fused": {"split_fused": 2},
        "radius_111": {"split_radius": 1.5, "depth_spacing": [1, 1, 1]},
        "radius_37_10_10": {"split_radius": 15, "depth_spacing": [37, 10, 10]}}
CORES_BYTES = 9  # per voxel: the labels and the map read, the byte mask written


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
    from delivr_cfos_amd.hostlogic import split_depth_settings

    shape = (Z, 2048, 2048)
    vox = Z * 2048 * 2048
    d = tempfile.mkdtemp(prefix="dlv_split_depth_", dir=base)
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
            return {"arm": arm, "wall_s": round(wall, 4), "n": int(n), "last_split": count_blobs.last_split,
                    "timings": {k: round(v, 4) for k, v in count_blobs.last_timings.items()}}

        for arm in ARMS:  # the unmeasured warm-up: context, workspaces, pinned staging
            run(f"warm_{arm}", arm)
        results = [run(f"run_{arm}_{k}", arm) for k in range(3) for arm in ARMS]
        walls = {arm: [r["wall_s"] for r in results if r["arm"] == arm] for arm in ARMS}
        splits = {arm: [r["timings"].get("split_s") for r in results if r["arm"] == arm] for arm in ARMS if arm != "none"}
        print(json.dumps({"shape": shape, "files_on": base, "runs": results,
                          "median_wall_s": {arm: statistics.median(w) for arm, w in walls.items()},
                          "min_max_wall_s": {arm: [min(w), max(w)] for arm, w in walls.items()},
                          "median_split_s": {arm: statistics.median(s) for arm, s in splits.items()},
                          "min_max_split_s": {arm: [min(s), max(s)] for arm, s in splits.items()}}), flush=True)

        torch.cuda.empty_cache()
        copy = _copy_rate(vox, eng.device, reps)
        torch.cuda.empty_cache()
        labels0, n = eng.ccl26(cells)
        del cells
        for arm in ("radius_111", "radius_37_10_10"):
            core_d2, fraction, min_core, spacing = split_depth_settings({"mi355x": ARMS[arm]})
            eng.cc_split_depth(labels0.clone(), n, spacing, core_d2, fraction, min_core)  # warm-up, outside the timed window
            eng.prof_enable(True)
            eng.prof_reset()
            for _ in range(reps):
                labels = labels0.clone()
                K, _, n_split = eng.cc_split_depth(labels, n, spacing, core_d2, fraction, min_core)
                del labels
            eng.sync()
            rep = eng.prof_report()
            eng.prof_enable(False)
            ms = {k: round(v["total_ms"] / reps, 4) for k, v in rep.items() if k.startswith("cc_") and v["launches"]}
            cores_ms = ms.get("cc_split_depth_cores")
            print(json.dumps({"input": "cell mask", "shape": shape, "n": n, "spacing": spacing, "core_d2": core_d2, "reps": reps, "K": K,
                              "components_split": n_split, "copy_GBps": round(copy / 1e9, 1), "ms_per_call": ms,
                              "cores_GBps": round(vox * CORES_BYTES / cores_ms / 1e6, 1) if cores_ms else None,
                              "cores_of_copy": round(vox * CORES_BYTES / cores_ms / 1e-3 / copy, 3) if cores_ms else None}), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/dev/shm", int(sys.argv[2]) if len(sys.argv) > 2 else 1024,
         int(sys.argv[3]) if len(sys.argv) > 3 else 3)
