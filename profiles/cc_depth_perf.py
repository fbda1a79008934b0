"""In-library kernel time of the three passes of dlv_cc_depth_dev beside the copy rate of the same process (profiles/README.md,
"cc_depth"), and what settings["mi355x"]["depth_stats"] adds to step 3.

Kernel time (default): the labels of the bench's synthetic cell mask (the c3 brain, seed 2, raw > 6500; default 1024 x 2048 x 2048)
with spacings (1, 1, 1) and (37, 10, 10), and the adversarial input, one solid component of 256^3 in a volume of 258^3, where the
walks are as long as the block is thick.  The times are the DlvProf events around each pass; the copy rate is torch's copy of a
uint32 volume of the mask's size (4 bytes read and 4 written per voxel), timed with events in the same process.  One JSON line per
input.       python profiles/cc_depth_perf.py [Z [reps]]

Step wall (--step): count_blobs file to file on tmpfs on the same mask with label_file = "runs" in both arms (the 17 GB dense label
file and the spread of its write are not what is compared), without the key against depth_stats, alternating, three runs each in
fresh folders after one unmeasured warm-up of each.  One JSON line.       python profiles/cc_depth_perf.py --step [folder [Z]]"""
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

PASSES = ("cc_depth_x", "cc_depth_y", "cc_depth_z")
PASS_BYTES = 12  # per voxel and pass, nominal: labels or the previous map read, the map written (x: written twice)


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


def _time_passes(eng, labels, n, spacing, reps):
    got = eng.cc_depth(labels, n, spacing)  # warm-up, outside the timed window
    eng.prof_enable(True)
    eng.prof_reset()
    for _ in range(reps):
        eng.cc_depth(labels, n, spacing)
    eng.sync()
    rep = eng.prof_report()
    eng.prof_enable(False)
    return got, {k: rep[k]["total_ms"] / rep[k]["launches"] for k in PASSES}


def kernel_times(Z, reps):
    from delivr_cfos_amd.engine import HipEngine

    eng = HipEngine(0)
    shape = (Z, 2048, 2048)
    vox = Z * 2048 * 2048
    copy = _copy_rate(vox, eng.device, reps)
    torch.cuda.empty_cache()
    labels, n = eng.ccl26(_cell_mask(shape, eng.device))
    counts = eng.cc_counts(labels, n).cpu().numpy().view(np.uint32)
    for spacing in ((1, 1, 1), (37, 10, 10)):
        got, ms = _time_passes(eng, labels, n, spacing, reps)
        # every cell has a deepest voxel, and a sum of at least one per voxel
        sane = bool((got["depth_max_sq"][1:] >= 1).all() and (got["depth_sum_sq"][1:] >= counts[1:]).all()
                    and (got["depth_peak_index"][1:] < vox).all())
        print(json.dumps({"input": "cell mask", "shape": shape, "n": n, "spacing": spacing, "reps": reps, "rows_sane": sane,
                          "foreground": round(int(counts[1:].sum()) / vox, 5), "largest_depth_sq": int(got["depth_max_sq"].max()),
                          "copy_GBps": round(copy / 1e9, 1),
                          **{f"{k}_ms": round(v, 4) for k, v in ms.items()}, "total_ms": round(sum(ms.values()), 4),
                          **{f"{k}_GBps": round(vox * PASS_BYTES / v / 1e6, 1) for k, v in ms.items()},
                          **{f"{k}_of_copy": round(vox * PASS_BYTES / v / 1e-3 / copy, 3) for k, v in ms.items()}}), flush=True)
    del labels
    torch.cuda.empty_cache()
    side = 256
    solid = torch.zeros((side + 2,) * 3, dtype=torch.int32, device=eng.device)
    solid[1:-1, 1:-1, 1:-1] = 1
    got, ms = _time_passes(eng, solid, 1, (1, 1, 1), reps)
    svox = (side + 2) ** 3
    print(json.dumps({"input": "one solid component", "shape": tuple(solid.shape), "side": side, "reps": reps,
                      "largest_depth_sq": int(got["depth_max_sq"][1]), "depth_ok": int(got["depth_max_sq"][1]) == (side // 2) ** 2,
                      **{f"{k}_ms": round(v, 4) for k, v in ms.items()}, "total_ms": round(sum(ms.values()), 4),
                      **{f"{k}_GBps": round(svox * PASS_BYTES / v / 1e6, 1) for k, v in ms.items()}}), flush=True)
    eng.close()


def step_walls(base, Z):
    from delivr_cfos_amd import hostio
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.engine import shared_engine

    shape = (Z, 2048, 2048)
    d = tempfile.mkdtemp(prefix="dlv_depth_", dir=base)
    try:
        eng = shared_engine(0)
        cells = _cell_mask(shape, eng.device)
        seg = os.path.join(d, "in", "brain", "binary_segmentations")
        os.makedirs(seg)
        hostio.save_npy(eng, cells, os.path.join(seg, "binaries.npy"), np.uint8, what="d2h_mask")
        del cells
        torch.cuda.empty_cache()
        path_in = os.path.join(d, "in")

        def run(tag, key):
            post = os.path.join(d, tag)
            settings = {"postprocessing": {"output_location": post + "/"}, "mi355x": {"label_file": "runs"}}
            if key:
                settings["mi355x"]["depth_stats"] = True
            t0 = time.perf_counter()
            n = count_blobs(settings, path_in, 0, "brain", (1, 1) + shape)
            wall = time.perf_counter() - t0
            shutil.rmtree(post)
            return {"depth_stats": key, "wall_s": round(wall, 4), "n": int(n),
                    "timings": {k: round(v, 4) for k, v in count_blobs.last_timings.items()}}

        for key in (False, True):  # the unmeasured warm-up: context, workspaces, pinned staging
            run(f"warm_{int(key)}", key)
        results = [run(f"run_{int(key)}_{k}", key) for k in range(3) for key in (False, True)]
        walls = {key: [r["wall_s"] for r in results if r["depth_stats"] == key] for key in (False, True)}
        print(json.dumps({"shape": shape, "files_on": base, "runs": results,
                          "median_wall_s": {"without": statistics.median(walls[False]), "with": statistics.median(walls[True])},
                          "min_max_wall_s": {"without": [min(walls[False]), max(walls[False])],
                                             "with": [min(walls[True]), max(walls[True])]}}), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        step_walls(sys.argv[2] if len(sys.argv) > 2 else "/dev/shm", int(sys.argv[3]) if len(sys.argv) > 3 else 1024)
    else:
        kernel_times(int(sys.argv[1]) if len(sys.argv) > 1 else 1024, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
