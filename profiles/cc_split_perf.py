"""dlv_cc_split_dev on the bench's cell mask ("cc_split"): the c3 synthetic brain (1024 x 2048 x 2048, seed 2), cells =
raw > 6500 as bench.py's ccl26_cells extra takes them, labelled once.  Per depth (2 and 4): the wall clock of HipEngine.cc_split -
what count_blobs.last_timings["split_s"] brackets - and the library's profile brackets (cc_split and its parts; the ccl26 inside it
is the labelling of the cores), after one warm-up call that sizes the scratch slots.  Yardstick: dlv_ccl26_dev on the same mask +
dlv_cc_shell_dev at radius = depth on the same labels, the same number of full-volume sweeps.  A second mask, the cells grown by one
voxel (3 x 3 x 3 maximum), fuses neighbours and gives the growth something to do.  Prints one JSON line.
python profiles/cc_split_perf.py [Z Y X]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from delivr_cfos_amd.engine import HipEngine  # noqa: E402
from delivr_cfos_amd.synth import synth_volume_torch  # noqa: E402

shape = tuple(int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (1024, 2048, 2048)
eng = HipEngine(0)
vol = synth_volume_torch(shape, 2, eng.device)
cells = (vol.view(torch.int16) > 6500).to(torch.uint8)
del vol
out = {"shape": shape}


def brackets(rep):
    return {name: round(v["total_ms"], 3) for name, v in sorted(rep.items())}


def measure(mask, tag, depths):
    labels0, n = eng.ccl26(mask)
    out[f"{tag}_components"] = n
    out[f"{tag}_foreground"] = float((mask != 0).sum()) / mask.numel()
    warm = labels0.clone()
    eng.cc_split(warm, n, depths[0])  # warm-up: scratch slots, the allocator's blocks
    del warm
    for d in depths:
        labels = labels0.clone()
        eng.sync()
        torch.cuda.synchronize()
        eng.prof_enable(True)
        eng.prof_reset()
        t0 = time.perf_counter()
        K, parent, n_split = eng.cc_split(labels, n, d)
        wall = 1e3 * (time.perf_counter() - t0)
        rep = brackets(eng.prof_report())
        del labels
        eng.prof_reset()
        eng.ccl26(mask)
        shell = eng.cc_shell(labels0, d, None)
        eng.sync()
        yard = brackets(eng.prof_report())
        del shell
        eng.prof_enable(False)
        out[f"{tag}_depth{d}"] = {"cells_after": K, "components_split": n_split, "wall_ms": round(wall, 3), "brackets_ms": rep,
                                  "yardstick_ms": yard, "yardstick_sum_ms": round(yard["ccl26"] + yard["cc_shell"], 3)}


measure(cells, "cells", (2, 4))
grown = torch.empty_like(cells)
for z0 in range(0, shape[0], 64):  # (chunks with a one-plane halo: the fp16 temporaries stay small)
    lo, hi = max(z0 - 1, 0), min(z0 + 65, shape[0])
    part = torch.nn.functional.max_pool3d(cells[lo:hi].to(torch.float16)[None, None], 3, 1, 1)[0, 0]
    grown[z0:min(z0 + 64, shape[0])] = part[z0 - lo:z0 - lo + min(64, shape[0] - z0)].to(torch.uint8)
    del part
del cells
measure(grown, "grown", (2,))
print(json.dumps(out))
eng.close()
