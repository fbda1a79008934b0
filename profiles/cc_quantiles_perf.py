"""In-library kernel time of dlv_cc_quantiles_dev's kernels (counts, gather, select) beside dlv_cc_intensity_dev on the same tensors
in the same process (profiles/README.md, "cc_quantiles"): (a) the bench's synthetic brain (delivr_cfos_amd.synth, default
256 x 1024 x 1024) with the bench's synthetic cell mask (raw > 6500) as labels and the volume itself as raw; (b) one synthetic
label of 2^27 voxels under random raw - the segment one workgroup selects alone.  The calls alternate, the times are the DlvProf
events around each kernel; the quartiles are checked against a 65536-bin histogram in torch.  Prints one JSON line per case.
python profiles/cc_quantiles_perf.py [Z Y X [reps]]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from delivr_cfos_amd.engine import HipEngine  # noqa: E402
from delivr_cfos_amd.synth import synth_volume_torch  # noqa: E402

shape = tuple(int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (256, 1024, 1024)
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
LEVELS = (25, 50, 75)
eng = HipEngine(0)


def lower_quantiles_of_one_label(raw):
    """the levels of ALL voxels of raw as one segment, from a histogram: the first value whose cumulative count exceeds the rank"""
    hist = torch.bincount(raw.view(-1).to(torch.int32) & 0xFFFF, minlength=65536).cumsum(0)
    m = raw.numel()
    ranks = torch.tensor([(p * (m - 1)) // 100 for p in LEVELS], device=raw.device)
    return torch.searchsorted(hist, ranks, right=True).cpu().numpy().astype(np.uint16)


def measure(name, labels, raw, n, extra):
    values, counts = eng.cc_quantiles(labels, raw, n, LEVELS)  # warm-up of both, outside the timed window
    moments = eng.cc_intensity(labels, raw, n)
    eng.prof_enable(True)
    eng.prof_reset()
    for _ in range(reps):
        eng.cc_intensity(labels, raw, n)
        eng.cc_quantiles(labels, raw, n, LEVELS)
    rep = eng.prof_report()
    eng.prof_enable(False)
    ms = {k: rep[k]["total_ms"] / rep[k]["launches"] for k in ("cc_intensity", "cc_counts", "cc_quantiles_gather", "cc_quantiles_select")}
    pair = ms["cc_quantiles_gather"] + ms["cc_quantiles_select"]
    fg = int(counts.sum())
    inside = bool(((values[:, 0] >= np.where(counts > 0, moments["intensity_min"], 0)) & (values[:, 2] <= moments["intensity_max"])).all())
    print(json.dumps({"case": name, "shape": tuple(labels.shape), "n": n, "foreground": fg, "largest_label": int(counts.max()),
                      "labels_above_512_voxels": int((counts > 512).sum()), "reps": reps, **extra, "quartiles_inside_min_max": inside,
                      **{k + "_ms": round(v, 4) for k, v in ms.items()}, "gather_plus_select_ms": round(pair, 4),
                      "gather_over_cc_intensity": round(ms["cc_quantiles_gather"] / ms["cc_intensity"], 3),
                      "pair_over_cc_intensity": round(pair / ms["cc_intensity"], 3),
                      "cc_intensity_GBps": round(labels.numel() * 6 / ms["cc_intensity"] / 1e6, 1),
                      "gather_GBps": round((labels.numel() * 6 + fg * 2) / ms["cc_quantiles_gather"] / 1e6, 1)}), flush=True)
    return values, counts


# (a) the bench's brain and its cell mask
vol = synth_volume_torch(shape, 1, eng.device)
cells = (vol.view(torch.int16) > 6500).to(torch.uint8)  # (bench.py's "synthetic cells themselves")
labels, n = eng.ccl26(cells)
del cells
values, counts = measure("cells", labels, vol, n, {})
del labels, vol

# (b) one label of 2^27 voxels
one = torch.ones((128, 1024, 1024), dtype=torch.int32, device=eng.device)
gen = torch.Generator(device=eng.device).manual_seed(3)
raw = (torch.randint(0, 65536, tuple(one.shape), dtype=torch.int32, device=eng.device, generator=gen) - 32768).to(torch.int16)  # (uint16 payload)
expected = lower_quantiles_of_one_label(raw)
got, _ = eng.cc_quantiles(one, raw, 1, LEVELS)
measure("one_label_2^27", one, raw, 1, {"equal_torch_histogram": bool((got[1] == expected).all())})
eng.close()
