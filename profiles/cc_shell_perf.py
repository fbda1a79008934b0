"""In-library kernel time of dlv_cc_shell_dev beside dlv_ccl26_dev and dlv_cc_intensity_dev on the same volume (profiles/README.md,
"cc_shell"): the labels of a random mask (default 512^3, 3 % foreground) and a random uint16 raw volume of the same shape; after a
warm-up of every call the calls alternate, the times are the DlvProf events around each call's kernels (cc_shell: its memsets and
its r sweeps).  The shell of every radius is compared with torch's max-pool form of the same expansion in the same run.  Prints
one JSON line.  python profiles/cc_shell_perf.py [N [density [reps]]]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from delivr_cfos_amd.engine import HipEngine  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 512
density = float(sys.argv[2]) if len(sys.argv) > 2 else 0.03
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
radii = (1, 3, 5)
shape = (side, side, side)
eng = HipEngine(0)
gen = torch.Generator(device=eng.device).manual_seed(3)
mask = (torch.rand(shape, device=eng.device, generator=gen) < density).to(torch.uint8)
raw = (torch.randint(0, 65536, shape, dtype=torch.int32, device=eng.device, generator=gen) - 32768).to(torch.int16)  # (uint16 payload)
labels, n = eng.ccl26(mask)
eng.cc_intensity(labels, raw, n)  # warm-up, outside the timed window


def expanded(lab, r):
    """the same expansion with torch: the smallest non-zero label of the 3x3x3 neighbourhood is n + 1 - max_pool(n + 1 - label);
    float32 holds every label below 2^24 exactly, float64 the others"""
    e = lab.to(torch.float32 if n + 1 < 2 ** 24 else torch.float64)
    for _ in range(r):
        inv = torch.where(e > 0, n + 1 - e, torch.zeros_like(e))
        m = torch.nn.functional.max_pool3d(inv[None, None], 3, 1, 1)[0, 0]
        e = torch.where(e > 0, e, torch.where(m > 0, n + 1 - m, torch.zeros_like(m)))
    return e.to(torch.int32)


equal, shell_voxels = {}, {}
for r in radii:
    shell = eng.cc_shell(labels, r, raw)
    ref = torch.where((labels == 0) & (raw != 0), expanded(labels, r), torch.zeros_like(labels))
    equal[r] = bool(torch.equal(shell, ref))
    shell_voxels[r] = int((shell != 0).sum())
    del shell, ref
ms = {}
for r in radii:  # (one DlvProf label for every radius: a window per radius)
    eng.prof_enable(True)
    eng.prof_reset()
    for _ in range(reps):
        eng.ccl26(mask)
        eng.cc_intensity(labels, raw, n)
        eng.cc_shell(labels, r, raw)
    rep = eng.prof_report()
    for k in ("ccl26", "cc_intensity"):
        ms.setdefault(k, []).append(sum(v["total_ms"] for name, v in rep.items() if name == k or name.startswith(k + "_")) / reps)
    ms[f"cc_shell_r{r}"] = rep["cc_shell"]["total_ms"] / rep["cc_shell"]["launches"]
    names = sorted(rep)
vox = side ** 3
out = {"shape": shape, "density": density, "n": n, "reps": reps, "prof_names": names,
       "shell_equals_torch": equal, "shell_voxels": shell_voxels,
       "ccl26_ms": [round(v, 4) for v in ms["ccl26"]], "cc_intensity_ms": [round(v, 4) for v in ms["cc_intensity"]]}
for r in radii:
    t = ms[f"cc_shell_r{r}"]
    out[f"cc_shell_r{r}_ms"] = round(t, 4)
    out[f"cc_shell_r{r}_ms_per_sweep"] = round(t / r, 4)
    out[f"cc_shell_r{r}_over_cc_intensity"] = round(t / (sum(ms["cc_intensity"]) / len(ms["cc_intensity"])), 2)
    out[f"cc_shell_r{r}_GBps_at_8B_per_voxel_and_sweep"] = round(vox * 8 * r / t / 1e6, 1)
print(json.dumps(out))
eng.close()
