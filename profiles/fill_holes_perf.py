"""What settings["mi355x"]["fill_holes"] costs (profiles/README.md, "fill_holes"): dlv_fill_holes_u8_dev beside dlv_ccl26_dev on the
same mask in the same process.

Two masks: the bench's synthetic cell mask (the c3 brain, seed 2, raw > 6500; default 1024 x 2048 x 2048), which has next to no
holes, and the same mask hollowed - every cell without its 6-neighbour erosion, so that every cell that has an inner voxel becomes a
sealed shell one voxel thick.

Kernel time: the DlvProf events around the launches of each call ("fill_holes", "ccl26"), alternating, the fill on a fresh copy of
the mask each time; a second fill of the filled mask must find nothing, and on the hollowed mask the result is compared with the
unhollowed one ("restores_the_cells": equal only when the cells themselves have no hole).
Step wall: count_blobs file to file on tmpfs with label_file = "runs" in both (the 17 GB dense label file and the spread of its
write are not what is compared), without the key against fill_holes, alternating, three runs each in fresh folders after one
unmeasured warm-up of each; the steps are count_blobs.last_timings.  One JSON line per mask.
        python profiles/fill_holes_perf.py [Z [folder]]"""
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


def _cell_mask(shape, device):
    from delivr_cfos_amd.synth import synth_volume_torch

    return (synth_volume_torch(shape, 2, device).view(torch.int16) > 6500).to(torch.uint8)


def _erode6(mask):
    """one step with the 6 face neighbours, outside the volume counting as background"""
    out = mask.clone()
    out[0], out[-1], out[:, 0], out[:, -1], out[:, :, 0], out[:, :, -1] = (0,) * 6
    out[1:] &= mask[:-1]
    out[:-1] &= mask[1:]
    out[:, 1:] &= mask[:, :-1]
    out[:, :-1] &= mask[:, 1:]
    out[:, :, 1:] &= mask[:, :, :-1]
    out[:, :, :-1] &= mask[:, :, 1:]
    return out


def kernel_times(eng, mask, reps, restored=None):
    work = mask.clone()
    voxels, holes = eng.fill_holes(work)  # warm-up of both, outside the timed window
    labels, n = eng.ccl26(work)
    again = eng.fill_holes((work != 0).to(torch.uint8))
    same = None if restored is None else bool(torch.equal(work != 0, restored != 0))
    del labels
    eng.prof_enable(True)
    eng.prof_reset()
    for _ in range(reps):
        work.copy_(mask)
        eng.fill_holes(work)
        labels, n = eng.ccl26(work)
        del labels
    eng.sync()
    rep = eng.prof_report()
    eng.prof_enable(False)
    ms = {k: rep[k]["total_ms"] / rep[k]["launches"] for k in ("fill_holes", "ccl26")}
    return {"voxels_filled": voxels, "holes": holes, "components_after": n, "second_fill": list(again), "restores_the_cells": same,
            "foreground": round(float((mask != 0).float().mean()), 5), "fill_holes_ms": round(ms["fill_holes"], 4),
            "ccl26_ms": round(ms["ccl26"], 4), "ratio": round(ms["fill_holes"] / ms["ccl26"], 3)}


def step_walls(eng, mask, base, tag):
    from delivr_cfos_amd import hostio
    from delivr_cfos_amd.count_blobs import count_blobs

    shape = tuple(int(v) for v in mask.shape)
    d = tempfile.mkdtemp(prefix="dlv_fill_", dir=base)
    try:
        seg = os.path.join(d, "in", "brain", "binary_segmentations")
        os.makedirs(seg)
        hostio.save_npy(eng, mask, os.path.join(seg, "binaries.npy"), np.uint8, what="d2h_mask")
        path_in = os.path.join(d, "in")

        def run(name, key):
            post = os.path.join(d, name)
            settings = {"postprocessing": {"output_location": post + "/"}, "mi355x": {"label_file": "runs"}}
            if key:
                settings["mi355x"]["fill_holes"] = True
            t0 = time.perf_counter()
            n = count_blobs(settings, path_in, 0, "brain", (1, 1) + shape, engine=eng)
            wall = time.perf_counter() - t0
            shutil.rmtree(post)
            return {"fill_holes": key, "wall_s": round(wall, 4), "n": int(n), "last_fill": count_blobs.last_fill,
                    "timings": {k: round(v, 4) for k, v in count_blobs.last_timings.items()}}

        for key in (False, True):  # the unmeasured warm-up: workspaces, pinned staging
            run(f"warm_{int(key)}", key)
        results = [run(f"run_{int(key)}_{k}", key) for k in range(3) for key in (False, True)]
        walls = {key: [r["wall_s"] for r in results if r["fill_holes"] == key] for key in (False, True)}
        keyed = [r["timings"] for r in results if r["fill_holes"]]
        return {"mask": tag, "shape": shape, "files_on": base, "runs": results,
                "median_wall_s": {"without": statistics.median(walls[False]), "with": statistics.median(walls[True])},
                "median_fill_holes_s": statistics.median(t["fill_holes_s"] for t in keyed),
                "median_ccl26_s": statistics.median(t["ccl26_s"] for t in keyed),
                "median_hole_voxels_s": statistics.median(t["hole_voxels_s"] for t in keyed)}
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    from delivr_cfos_amd.engine import shared_engine

    Z = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    base = sys.argv[2] if len(sys.argv) > 2 else "/dev/shm"
    eng = shared_engine(0)
    cells = _cell_mask((Z, 2048, 2048), eng.device)
    inner = _erode6(cells)
    hollow = cells & ~inner
    del inner
    for tag, mask, restored in (("cells", cells, None), ("hollowed cells", hollow, cells)):
        print(json.dumps({"mask": tag, "shape": tuple(mask.shape), "kernels": kernel_times(eng, mask, 3, restored)}), flush=True)
    for tag, mask in (("cells", cells), ("hollowed cells", hollow)):
        print(json.dumps(step_walls(eng, mask, base, tag)), flush=True)
