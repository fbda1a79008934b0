"""In-library kernel time of dlv_cc_intensity_dev beside dlv_cc_stats_dev on the same labels (profiles/README.md, "cc_intensity"):
the labels of a random mask (default 512^3, 3 % foreground) and a random uint16 raw volume of the same shape; the calls alternate,
the times are the DlvProf events around each kernel.  Prints one JSON line.  python profiles/cc_intensity_perf.py [N [density [reps]]]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from delivr_cfos_amd.engine import HipEngine  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 512
density = float(sys.argv[2]) if len(sys.argv) > 2 else 0.03
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
shape = (side, side, side)
eng = HipEngine(0)
gen = torch.Generator(device=eng.device).manual_seed(3)
mask = (torch.rand(shape, device=eng.device, generator=gen) < density).to(torch.uint8)
raw = (torch.randint(0, 65536, shape, dtype=torch.int32, device=eng.device, generator=gen) - 32768).to(torch.int16)  # (uint16 payload)
labels, n = eng.ccl26(mask)
del mask
stats = eng.cc_stats(labels, n)  # warm-up of both, outside the timed window
got = eng.cc_intensity(labels, raw, n)
# the sums at this size against torch (int64 index_add_): every row
ref = torch.zeros(n + 1, dtype=torch.int64, device=eng.device)
ref.index_add_(0, labels.view(-1).to(torch.int64), (raw.view(-1).to(torch.int64) & 0xFFFF))
ref[0] = 0
sums_ok = bool((ref.cpu().numpy().astype("uint64") == got["intensity_sum"]).all())
del ref
eng.prof_enable(True)
eng.prof_reset()
for _ in range(reps):
    eng.cc_stats(labels, n)
    eng.cc_intensity(labels, raw, n)
rep = eng.prof_report()
vox = side ** 3
ms = {k: rep[k]["total_ms"] / rep[k]["launches"] for k in ("cc_stats", "cc_intensity")}
print(json.dumps({"shape": shape, "density": density, "n": n, "foreground": int(stats["voxel_counts"][1:].sum()), "reps": reps,
                  "sums_equal_torch": sums_ok,
                  "cc_stats_ms": round(ms["cc_stats"], 4), "cc_intensity_ms": round(ms["cc_intensity"], 4),
                  "ratio": round(ms["cc_intensity"] / ms["cc_stats"], 3),
                  "cc_stats_GBps": round(vox * 4 / ms["cc_stats"] / 1e6, 1), "cc_intensity_GBps": round(vox * 6 / ms["cc_intensity"] / 1e6, 1)}))
eng.close()
