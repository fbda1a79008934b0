"""The run-length label coder (dlv_cc_runs_count_dev + dlv_cc_runs_emit_dev) and its decoder (dlv_cc_runs_decode_dev) beside
dlv_cc_stats_dev on the same labels (profiles/README.md, "cc_runs"), and what the run file does to step 3.

Kernel time (default): the labels of cc_shape_perf.py's two masks (default 512^3) - a sparse one, about 1 % foreground in 2 x 2 x 2
cubes, and a dense one, a 50 % random mask; the calls alternate, the times are the DlvProf events around the kernels.  The round
trip is checked in the script: the decoded volume equals the labels, and the device's runs equal label_runs.encode_runs on the
first 32 planes.  One JSON line per mask: ms, GB/s (8 bytes per voxel read for the encode, 4 written for the decode), R and the run
file's bytes per voxel.       python profiles/cc_runs_perf.py [N [reps]]

Step wall (--step): count_blobs file to file on tmpfs on the bench's synthetic cell mask (the c3 brain, seed 2, raw > 6500) -
1024 x 2048 x 2048 when the folder holds the 17 GB dense file, else 512 x 2048 x 2048 - the default against label_file = "runs",
alternating, three runs each in fresh folders after one unmeasured warm-up of each; then one more "runs" call in the last folder:
the re-run from the run-file cache with a complete pickle.  One JSON line.       python profiles/cc_runs_perf.py --step [folder]"""
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

from delivr_cfos_amd import label_runs  # noqa: E402
from delivr_cfos_amd.engine import HipEngine  # noqa: E402


def kernel_times(side, reps):
    shape = (side, side, side)
    eng = HipEngine(0)
    gen = torch.Generator(device=eng.device).manual_seed(3)

    def sparse_mask():
        cells = side // 8
        seeds = torch.rand((cells, cells, cells), device=eng.device, generator=gen) < 0.64  # 0.64 * 8 / 512 = 1 % of the voxels
        mask = torch.zeros(shape, dtype=torch.uint8, device=eng.device)
        for dz in (3, 4):
            for dy in (3, 4):
                for dx in (3, 4):
                    mask[dz::8, dy::8, dx::8][:cells, :cells, :cells] = seeds
        return mask

    def dense_mask():
        return (torch.rand(shape, device=eng.device, generator=gen) < 0.5).to(torch.uint8)

    for name, make in (("sparse", sparse_mask), ("dense", dense_mask)):
        labels, n = eng.ccl26(make())
        eng.cc_stats(labels, n)  # warm-up of all three, outside the timed window
        runs = eng.cc_runs_encode(labels)
        out = torch.empty_like(labels)
        out.view(torch.uint8).fill_(0xAB)
        eng.cc_runs_decode(runs, out=out)
        head = min(32, side)
        want = label_runs.encode_runs(labels[:head].cpu().numpy().view(np.uint32))
        r_head = int(want["row_start"][-1])
        same = bool(torch.equal(out, labels)) and bool((runs["row_start"][:head * side + 1] == want["row_start"]).all()) and all(
            bool((runs[k][:r_head] == want[k]).all()) for k in ("x0", "x1", "label"))
        eng.prof_enable(True)
        eng.prof_reset()
        for _ in range(reps):
            eng.cc_stats(labels, n)
            eng.cc_runs_encode(labels)
            eng.cc_runs_decode(runs, out=out)
        eng.sync()
        rep = eng.prof_report()
        eng.prof_enable(False)
        vox = side ** 3
        ms = {k: rep[k]["total_ms"] / rep[k]["launches"] for k in ("cc_stats", "cc_runs_count", "cc_runs_emit", "cc_runs_decode")}
        enc = ms["cc_runs_count"] + ms["cc_runs_emit"]
        R = len(runs["label"])
        file_bytes = 8 * R + 8 * len(runs["row_start"])
        print(json.dumps({"mask": name, "shape": shape, "n": n, "reps": reps, "round_trip_equal": same, "runs": R,
                          "runs_per_voxel": round(R / vox, 5), "file_bytes_per_voxel": round(file_bytes / vox, 4),
                          "cc_stats_ms": round(ms["cc_stats"], 4), "cc_runs_count_ms": round(ms["cc_runs_count"], 4),
                          "cc_runs_emit_ms": round(ms["cc_runs_emit"], 4), "encode_ms": round(enc, 4),
                          "encode_to_cc_stats": round(enc / ms["cc_stats"], 3), "cc_runs_decode_ms": round(ms["cc_runs_decode"], 4),
                          "encode_GBps": round(vox * 8 / enc / 1e6, 1), "decode_GBps": round(vox * 4 / ms["cc_runs_decode"] / 1e6, 1),
                          "cc_stats_GBps": round(vox * 4 / ms["cc_stats"] / 1e6, 1)}), flush=True)
        del labels, out
    eng.close()


def step_walls(base):
    from delivr_cfos_amd import hostio
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.engine import shared_engine
    from delivr_cfos_amd.synth import synth_volume_torch

    free = shutil.disk_usage(base).free
    shape = (1024, 2048, 2048) if free > 2 * (17 << 30) + (5 << 30) else (512, 2048, 2048)
    d = tempfile.mkdtemp(prefix="dlv_runs_", dir=base)
    try:
        eng = shared_engine(0)
        vol = synth_volume_torch(shape, 2, eng.device)
        cells = (vol.view(torch.int16) > 6500).to(torch.uint8)
        del vol
        path_in = os.path.join(d, "in")
        os.makedirs(os.path.join(path_in, "brain", "binary_segmentations"))
        hostio.save_npy(eng, cells, os.path.join(path_in, "brain", "binary_segmentations", "binaries.npy"), np.uint8, what="d2h_mask")
        del cells
        torch.cuda.empty_cache()

        def run(tag, fmt, post=None):
            post = post or os.path.join(d, tag)
            settings = {"postprocessing": {"output_location": post + "/"}}
            if fmt == "runs":
                settings["mi355x"] = {"label_file": "runs"}
            t0 = time.perf_counter()
            n = count_blobs(settings, path_in, 0, "brain", (1, 1) + shape)
            wall = time.perf_counter() - t0
            files = {f: os.path.getsize(os.path.join(post, f)) for f in os.listdir(post) if "cc3d" in f}
            return {"format": fmt, "wall_s": round(wall, 4), "n": int(n), "label_file_bytes": files,
                    "timings": {k: round(v, 4) for k, v in count_blobs.last_timings.items()}}, post

        for fmt in ("dense", "runs"):  # the unmeasured warm-up: context, workspaces, pinned staging
            shutil.rmtree(run(f"warm_{fmt}", fmt)[1])
        results, last_runs = [], None
        for k in range(3):
            for fmt in ("dense", "runs"):
                rec, post = run(f"{fmt}_{k}", fmt)
                results.append(rec)
                if fmt == "runs" and k == 2:
                    last_runs = post
                else:
                    shutil.rmtree(post)
        cached, _ = run("", "runs", last_runs)
        walls = {fmt: [r["wall_s"] for r in results if r["format"] == fmt] for fmt in ("dense", "runs")}
        med = {fmt: statistics.median(w) for fmt, w in walls.items()}
        spread = max(walls["dense"]) - min(walls["dense"])
        print(json.dumps({"shape": shape, "files_on": base, "runs": results, "median_wall_s": med, "dense_spread_s": round(spread, 4),
                          "runs_below_dense_by_more_than_the_spread": bool(med["dense"] - med["runs"] > spread),
                          "rerun_from_the_run_file_cache_with_a_complete_pickle": cached}), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        step_walls(sys.argv[2] if len(sys.argv) > 2 else "/dev/shm")
    else:
        kernel_times(int(sys.argv[1]) if len(sys.argv) > 1 else 512, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
