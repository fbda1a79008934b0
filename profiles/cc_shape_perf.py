"""In-library kernel time of dlv_cc_shape_dev beside dlv_cc_stats_dev on the same labels (profiles/README.md, "cc_shape"): the
labels of two masks of the same shape (default 512^3) - a sparse one, about 1 % foreground in small blobs (2 x 2 x 2 cubes on a
random tenth of an 8-voxel lattice), and a dense one, a 50 % random mask; the calls alternate, the times are the DlvProf events
around each kernel.  Prints one JSON line per mask.  python profiles/cc_shape_perf.py [N [reps]]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from delivr_cfos_amd.engine import HipEngine  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
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
    stats = eng.cc_stats(labels, n)  # warm-up of both, outside the timed window
    got = eng.cc_shape(labels, n)
    # the counts and the coordinate sums against cc_stats' own: every row
    same = bool((got["shape_counts"][1:] == stats["voxel_counts"][1:]).all())
    cent = got["shape_sums"][1:].astype("float64") / got["shape_counts"][1:, None]
    same = same and bool((cent == stats["centroids"][1:]).all())
    eng.prof_enable(True)
    eng.prof_reset()
    for _ in range(reps):
        eng.cc_stats(labels, n)
        eng.cc_shape(labels, n)
    rep = eng.prof_report()
    eng.prof_enable(False)
    vox = side ** 3
    ms = {k: rep[k]["total_ms"] / rep[k]["launches"] for k in ("cc_stats", "cc_shape")}
    print(json.dumps({"mask": name, "shape": shape, "n": n, "foreground": round(int(stats["voxel_counts"][1:].sum()) / vox, 4), "reps": reps,
                      "counts_and_centroids_equal_cc_stats": same, "cc_stats_ms": round(ms["cc_stats"], 4),
                      "cc_shape_ms": round(ms["cc_shape"], 4), "ratio": round(ms["cc_shape"] / ms["cc_stats"], 3),
                      "cc_stats_GBps": round(vox * 4 / ms["cc_stats"] / 1e6, 1), "cc_shape_GBps": round(vox * 4 / ms["cc_shape"] / 1e6, 1)}),
          flush=True)
    del labels
eng.close()
