"""In-library kernel time of dlv_cc_confidence_dev beside dlv_cc_intensity_dev on the same labels (profiles/README.md,
"cc_confidence"), and what settings["mi355x"]["confidence_stats"] adds to step 3.

Kernel time (default): the labels of the bench's synthetic cell mask (the c3 brain, seed 2, raw > 6500; default 1024 x 2048 x 2048),
its raw volume, and probabilities made for it - uniform in [0.5, 1] inside the mask, in [0, 0.5) outside; the calls alternate, the times
are the DlvProf events around each kernel.  The fixed-point sums of every row are compared with torch's int64 index_add_ in the same
run.  One JSON line.       python profiles/cc_confidence_perf.py [Z [reps]]

Step wall (--step): count_blobs file to file on tmpfs on the same mask - 1024 x 2048 x 2048 when the folder holds the 17 GB
probability file beside the mask, else 512 x 2048 x 2048 - with label_file = "runs" in both (the 17 GB dense label file and the spread
of its write are not what is compared), without the key against confidence_stats, alternating, three runs each in fresh folders
after one unmeasured warm-up of each.  One JSON line.       python profiles/cc_confidence_perf.py --step [folder]"""
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


def _cell_mask_and_probabilities(shape, device):
    from delivr_cfos_amd.synth import synth_volume_torch

    vol = synth_volume_torch(shape, 2, device)
    cells = vol.view(torch.int16) > 6500
    gen = torch.Generator(device=device).manual_seed(5)
    prob = torch.rand(shape, device=device, generator=gen, dtype=torch.float32)
    prob.mul_(0.5)
    prob.add_(cells.to(torch.float32), alpha=0.5)  # (a cell's voxels lie in [0.5, 1], as at the default threshold)
    return vol, cells.to(torch.uint8), prob


def kernel_times(Z, reps):
    from delivr_cfos_amd.engine import HipEngine

    shape = (Z, 2048, 2048)
    eng = HipEngine(0)
    raw, mask, prob = _cell_mask_and_probabilities(shape, eng.device)
    labels, n = eng.ccl26(mask)
    del mask
    eng.cc_intensity(labels, raw, n)  # warm-up of both, outside the timed window
    got = eng.cc_confidence(labels, prob, n)
    sums_ok = True
    planes = 64  # (the int64 temporaries of the whole volume would be 8 bytes per voxel each)
    ref = torch.zeros(n + 1, dtype=torch.int64, device=eng.device)
    for z in range(0, Z, planes):
        q = torch.round(prob[z:z + planes].clamp(0, 1) * 16777216.0).to(torch.int64)  # (round: half to even)
        ref.index_add_(0, (labels[z:z + planes].reshape(-1).to(torch.int64) & 0xFFFFFFFF), q.reshape(-1))
    ref[0] = 0
    sums_ok = bool((ref.cpu().numpy().astype("uint64") == got["confidence_sum"]).all())
    del ref, q
    eng.prof_enable(True)
    eng.prof_reset()
    for _ in range(reps):
        eng.cc_intensity(labels, raw, n)
        eng.cc_confidence(labels, prob, n)
    eng.sync()
    rep = eng.prof_report()
    eng.prof_enable(False)
    vox = Z * 2048 * 2048
    ms = {k: rep[k]["total_ms"] / rep[k]["launches"] for k in ("cc_intensity", "cc_confidence")}
    print(json.dumps({"shape": shape, "n": n, "reps": reps, "sums_equal_torch": sums_ok,
                      "cc_intensity_ms": round(ms["cc_intensity"], 4), "cc_confidence_ms": round(ms["cc_confidence"], 4),
                      "ratio": round(ms["cc_confidence"] / ms["cc_intensity"], 3),
                      "cc_intensity_GBps": round(vox * 6 / ms["cc_intensity"] / 1e6, 1),
                      "cc_confidence_GBps": round(vox * 8 / ms["cc_confidence"] / 1e6, 1)}), flush=True)
    eng.close()


def step_walls(base):
    from delivr_cfos_amd import hostio
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.engine import shared_engine

    free = shutil.disk_usage(base).free
    shape = (1024, 2048, 2048) if free > (17 << 30) + (5 << 30) + (4 << 30) else (512, 2048, 2048)
    d = tempfile.mkdtemp(prefix="dlv_conf_", dir=base)
    try:
        eng = shared_engine(0)
        raw, cells, prob = _cell_mask_and_probabilities(shape, eng.device)
        del raw
        seg = os.path.join(d, "in", "brain", "binary_segmentations")
        os.makedirs(seg)
        hostio.save_npy(eng, cells, os.path.join(seg, "binaries.npy"), np.uint8, what="d2h_mask")
        hostio.save_npy(eng, prob, os.path.join(seg, "network_output.npy"), np.float32, what="d2h_prob")
        del cells, prob
        torch.cuda.empty_cache()
        path_in = os.path.join(d, "in")

        def run(tag, key):
            post = os.path.join(d, tag)
            settings = {"postprocessing": {"output_location": post + "/"}, "mi355x": {"label_file": "runs"}}
            if key:
                settings["mi355x"]["confidence_stats"] = True
            t0 = time.perf_counter()
            n = count_blobs(settings, path_in, 0, "brain", (1, 1) + shape)
            wall = time.perf_counter() - t0
            shutil.rmtree(post)
            return {"confidence_stats": key, "wall_s": round(wall, 4), "n": int(n),
                    "h2d_prob_GBps": round(hostio.last_transfer["h2d_prob"]["GBps"], 1) if key else None,
                    "timings": {k: round(v, 4) for k, v in count_blobs.last_timings.items()}}

        for key in (False, True):  # the unmeasured warm-up: context, workspaces, pinned staging
            run(f"warm_{int(key)}", key)
        results = [run(f"run_{int(key)}_{k}", key) for k in range(3) for key in (False, True)]
        walls = {key: [r["wall_s"] for r in results if r["confidence_stats"] == key] for key in (False, True)}
        print(json.dumps({"shape": shape, "files_on": base, "runs": results,
                          "median_wall_s": {"without": statistics.median(walls[False]), "with": statistics.median(walls[True])},
                          "spread_s": {"without": round(max(walls[False]) - min(walls[False]), 4),
                                       "with": round(max(walls[True]) - min(walls[True]), 4)}}), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        step_walls(sys.argv[2] if len(sys.argv) > 2 else "/dev/shm")
    else:
        kernel_times(int(sys.argv[1]) if len(sys.argv) > 1 else 1024, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
