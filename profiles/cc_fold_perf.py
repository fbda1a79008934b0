"""In-library kernel time of every call of dlv_cc_stats_dev, dlv_cc_counts_dev, dlv_cc_intensity_dev and dlv_cc_shape_dev, to set two
builds of the library beside each other (profiles/README.md, "cc_fold"): the masks of cc_intensity_perf.py (512^3, random 3 %) and
cc_shape_perf.py (sparse 1 %, dense 50 %), a warm-up of the four calls, then five rounds of them with the DlvProf events read after
each call.  One process measures one library (DLV_LIB names another build under delivr_cfos_amd/lib/); the digests of all
outputs are printed so that two libraries can be held to the same results.  Prints one JSON line per mask.
python profiles/cc_fold_perf.py TAG"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from delivr_cfos_amd.engine import HipEngine  # noqa: E402

tag = sys.argv[1]
side, reps = 512, 5
shape = (side, side, side)
eng = HipEngine(0)


def random_mask(gen, density):
    return (torch.rand(shape, device=eng.device, generator=gen) < density).to(torch.uint8)


def sparse_mask(gen):
    cells = side // 8
    seeds = torch.rand((cells, cells, cells), device=eng.device, generator=gen) < 0.64
    mask = torch.zeros(shape, dtype=torch.uint8, device=eng.device)
    for dz in (3, 4):
        for dy in (3, 4):
            for dx in (3, 4):
                mask[dz::8, dy::8, dx::8][:cells, :cells, :cells] = seeds
    return mask


def digest(d):
    h = hashlib.sha256()
    for k in sorted(d):
        h.update(d[k].tobytes())
    return h.hexdigest()[:12]


# "random3": cc_intensity_perf.py's generator state (seed 3: mask, then raw); "sparse", "dense": cc_shape_perf.py's (seed 3: sparse, dense)
gen = torch.Generator(device=eng.device).manual_seed(3)
mask3 = random_mask(gen, 0.03)
raw = (torch.randint(0, 65536, shape, dtype=torch.int32, device=eng.device, generator=gen) - 32768).to(torch.int16)
gen = torch.Generator(device=eng.device).manual_seed(3)
masks = (("random3", mask3), ("sparse", sparse_mask(gen)), ("dense", random_mask(gen, 0.5)))
del mask3
calls = {"cc_stats": lambda lab, n: eng.cc_stats(lab, n), "cc_counts": lambda lab, n: {"c": eng.cc_counts(lab, n).cpu().numpy()},
         "cc_intensity": lambda lab, n: eng.cc_intensity(lab, raw, n), "cc_shape": lambda lab, n: eng.cc_shape(lab, n)}
for name, mask in masks:
    labels, n = eng.ccl26(mask)
    sums = {k: digest(f(labels, n)) for k, f in calls.items()}  # warm-up of all four; the digests are compared across libraries
    eng.prof_enable(True)
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            eng.prof_reset()
            f(labels, n)
            rep = eng.prof_report()
            assert rep[k]["launches"] == 1
            times[k].append(round(rep[k]["total_ms"], 4))
    eng.prof_enable(False)
    print(json.dumps({"lib": tag, "mask": name, "n": n, "ms": times, "digest": sums}), flush=True)
    del labels
eng.close()
