"""The overlap table of two label volumes (dlv_cc_overlap_count_dev + dlv_cc_overlap_dev, csrc/cc_overlap.hip) beside dlv_cc_stats_dev
on the labels of A (profiles/README.md, "cc_overlap").

Cases: the labels of cc_runs_perf.py's sparse mask (default 512^3, about 1 % foreground in 2 x 2 x 2 cubes) against the labels of the
same mask moved by one voxel along x; the labels of a 50 % random mask against those of another 50 % random mask; and, with --brain,
the bench's synthetic cell mask (the c3 brain, seed 2, raw > 6500; 1024 x 2048 x 2048 when both label volumes, the mask and the
labelling's scratch fit the device, else 512 x 2048 x 2048) against itself moved by one voxel.  The calls alternate; the times are
the DlvProf events around the kernels (cc_overlap_table brackets the clearing of the table and the insert kernel).  Checked in the
script: the device's table of the first 16 planes equals compare_cells.overlap_table_np, and the voxels of the whole table add up to
the voxels that take part.  One JSON line per case: ms, GB/s (8 bytes per voxel read by the count and by the insert), S, P, the
table's bytes.       python profiles/cc_overlap_perf.py [N [reps]] [--brain]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from delivr_cfos_amd import compare_cells  # noqa: E402
from delivr_cfos_amd.engine import HipEngine  # noqa: E402


def moved(mask):
    out = torch.zeros_like(mask)
    out[:, :, 1:] = mask[:, :, :-1]
    return out


def measure(eng, name, mask_a, mask_b, reps):
    shape = tuple(mask_a.shape)
    a, n_a = eng.ccl26(mask_a)
    b, n_b = eng.ccl26(mask_b)
    del mask_a, mask_b
    torch.cuda.empty_cache()
    eng.cc_stats(a, n_a)  # warm-up of both, outside the timed window
    table = eng.cc_overlap(a, n_a, b, n_b)
    head = min(16, shape[0])
    want = compare_cells.overlap_table_np(a[:head].cpu().numpy().view(np.uint32), b[:head].cpu().numpy().view(np.uint32), n_a, n_b)
    got = eng.cc_overlap(a[:head], n_a, b[:head], n_b)
    same = got["segments"] == want["segments"] and all(np.array_equal(got[k], want[k]) for k in ("a", "b", "voxels"))
    both = int(((a != 0) & (b != 0)).sum())
    eng.prof_enable(True)
    eng.prof_reset()
    for _ in range(reps):
        eng.cc_stats(a, n_a)
        eng.cc_overlap(a, n_a, b, n_b)
    eng.sync()
    rep = eng.prof_report()
    eng.prof_enable(False)
    vox = shape[0] * shape[1] * shape[2]
    ms = {k: rep[k]["total_ms"] / rep[k]["launches"] for k in ("cc_stats", "cc_overlap_count", "cc_overlap_table", "cc_overlap_compact")}
    S, P = table["segments"], len(table["a"])
    bound = min(S, n_a * n_b)
    cap = 1 << (2 * bound - 1).bit_length() if bound else 0
    print(json.dumps({"case": name, "shape": shape, "n_a": n_a, "n_b": n_b, "reps": reps, "head_equals_numpy": bool(same),
                      "voxels_add_up": int(table["voxels"].sum()) == both, "segments": S, "pairs": P, "table_slots": cap,
                      "table_bytes": cap * 16, "largest_pair_voxels": int(table["voxels"].max()) if P else 0,
                      "cc_stats_ms": round(ms["cc_stats"], 4), "count_ms": round(ms["cc_overlap_count"], 4),
                      "table_ms": round(ms["cc_overlap_table"], 4), "compact_ms": round(ms["cc_overlap_compact"], 4),
                      "count_to_cc_stats": round(ms["cc_overlap_count"] / ms["cc_stats"], 3),
                      "table_to_cc_stats": round(ms["cc_overlap_table"] / ms["cc_stats"], 3),
                      "count_GBps": round(vox * 8 / ms["cc_overlap_count"] / 1e6, 1),
                      "table_GBps": round(vox * 8 / ms["cc_overlap_table"] / 1e6, 1),
                      "cc_stats_GBps": round(vox * 4 / ms["cc_stats"] / 1e6, 1)}), flush=True)


def main(side, reps, brain):
    eng = HipEngine(0)
    gen = torch.Generator(device=eng.device).manual_seed(3)
    shape = (side, side, side)

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

    sparse = sparse_mask()
    measure(eng, "sparse, 1 %, against itself moved by one voxel", sparse, moved(sparse), reps)
    del sparse
    measure(eng, "dense, 50 % random, against another 50 % random", dense_mask(), dense_mask(), reps)
    if brain:
        from delivr_cfos_amd.synth import synth_volume_torch

        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(eng.device)
        big = (1024, 2048, 2048) if free > 100 * (1 << 30) else (512, 2048, 2048)  # two label volumes, a mask, the labelling's scratch
        vol = synth_volume_torch(big, 2, eng.device)
        cells = (vol.view(torch.int16) > 6500).to(torch.uint8)
        del vol
        measure(eng, "the bench's cell mask against itself moved by one voxel", cells, moved(cells), max(1, reps // 2))
    eng.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--brain"]
    main(int(args[0]) if args else 512, int(args[1]) if len(args) > 1 else 5, "--brain" in sys.argv[1:])
