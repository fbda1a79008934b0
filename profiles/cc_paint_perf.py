"""Painting RGB + region-id planes from the labels (dlv_paint_runs_dev, dlv_paint_labels_dev) beside the box path
(dlv_paint_owner_dev + four dlv_paint_apply_dev) on the same cells (profiles/README.md, "cc_paint").

The labels of cc_runs_perf.py's two masks (default 512^3) - a sparse one, about 1 % foreground in 2 x 2 x 2 cubes, and a dense one,
a 50 % random mask.  Every cell is listed, with random colours and region ids; the box path gets the cells' bounding boxes padded
once, in label order.  All buffers are allocated and uploaded before the timed window; the three paths alternate, each call
between two device events on the engine's stream (the box path's five calls between one pair); after two unmeasured rounds the
median over the repetitions is reported, with the algorithmic bytes of each path over that time:
    runs    8 (n_rows + 1) + 8 R read, 5 per voxel written
    labels  4 per voxel read, 5 written
    boxes   4 per voxel cleared (owner), 1 read + 4 updated per voxel of every box, then 4 x (4 + 1) per voxel read and 5 written
The planes are checked in the script: both label painters agree, and on the sparse mask - where no box reaches another cell - they
equal the box path's.  One JSON line per mask.       python profiles/cc_paint_perf.py [N [reps]]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from delivr_cfos_amd.engine import HipEngine  # noqa: E402
from delivr_cfos_amd.hostlogic import padded_boxes, paint_luts  # noqa: E402


def main(side, reps):
    shape = (side, side, side)
    eng = HipEngine(0)
    gen = torch.Generator(device=eng.device).manual_seed(3)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

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
        mask = make()
        labels, n = eng.ccl26(mask)
        stats = eng.cc_stats(labels, n)
        runs = eng.cc_runs_encode(labels)
        R = len(runs["label"])
        rng = np.random.default_rng(7)
        ids = np.arange(1, n + 1)
        red, green, blue = (rng.integers(1, 256, size=n).astype(np.uint8) for _ in range(3))
        region = rng.integers(1, 65536, size=n).astype(np.uint16)
        lut_rgb, lut_region = paint_luts(ids, red, green, blue, region, n)
        wide = lut_rgb.astype(np.uint32)
        lut_rgb_dev = torch.from_numpy((wide[:, 0] | (wide[:, 1] << 8) | (wide[:, 2] << 16)).view(np.int32).copy()).to(eng.device)
        lut_u16_dev = torch.from_numpy(lut_region.view(np.int16).copy()).to(eng.device)
        rs_dev = torch.from_numpy(runs["row_start"].view(np.int64).copy()).to(eng.device)
        x0_dev, x1_dev = (torch.from_numpy(runs[k].view(np.int16).copy()).to(eng.device) for k in ("x0", "x1"))
        lab_dev = torch.from_numpy(runs["label"].view(np.int32).copy()).to(eng.device)
        boxes = np.ascontiguousarray(padded_boxes(stats["bounding_boxes"], ids, shape, 1))
        boxes_dev = torch.from_numpy(boxes).to(eng.device)
        box_voxels = int(np.prod(np.diff(boxes.astype(np.int64).reshape(-1, 3, 2), axis=2)[:, :, 0], axis=1).sum())
        values = [torch.from_numpy(v.view(np.int8 if v.dtype == np.uint8 else np.int16).copy()).to(eng.device) for v in (red, green, blue, region)]
        owner = torch.empty(shape, dtype=torch.int32, device=eng.device)

        def planes():
            out = [torch.empty(shape, dtype=torch.uint8, device=eng.device) for _ in range(3)]
            out.append(torch.empty(shape, dtype=torch.uint16, device=eng.device))
            for t in out:
                t.view(torch.uint8).fill_(0xAB)
            return out

        out_runs, out_labels, out_boxes = planes(), planes(), planes()

        def from_runs():
            eng._check(eng.lib.dlv_paint_runs_dev(eng.ctx, p(rs_dev), side * side, side, p(x0_dev), p(x1_dev), p(lab_dev), R, n + 1,
                                                  p(lut_rgb_dev), p(lut_u16_dev), *(p(t) for t in out_runs)))

        def from_labels():
            eng._check(eng.lib.dlv_paint_labels_dev(eng.ctx, p(labels), side, side, side, n + 1, p(lut_rgb_dev), p(lut_u16_dev),
                                                    *(p(t) for t in out_labels)))

        def from_boxes():
            eng._check(eng.lib.dlv_paint_owner_dev(eng.ctx, p(mask), side, side, side, p(boxes_dev), boxes.ctypes.data_as(C.c_void_p), n, p(owner)))
            for v, out in zip(values, out_boxes):
                eng._check(eng.lib.dlv_paint_apply_dev(eng.ctx, p(owner), p(mask), side ** 3, p(v), v.element_size(), p(out)))

        paths = (("runs", from_runs), ("labels", from_labels), ("boxes", from_boxes))
        times = {k: [] for k, _ in paths}
        eng._enter()
        for rep in range(reps + 2):  # (two unmeasured rounds: code objects, workspaces)
            for key, call in paths:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(eng.tstream)
                call()
                b.record(eng.tstream)
                b.synchronize()
                if rep >= 2:
                    times[key].append(a.elapsed_time(b))
        eng._leave()
        eng.sync()
        same_painters = all(bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for a, b in zip(out_runs, out_labels))
        same_as_boxes = all(bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for a, b in zip(out_labels, out_boxes))
        painted = int((out_labels[3].view(torch.int16) != 0).sum())
        vox = side ** 3
        nbytes = {"runs": 8 * (side * side + 1) + 8 * R + 5 * vox, "labels": 9 * vox, "boxes": 4 * vox + 5 * box_voxels + 4 * 5 * vox + 5 * vox}
        rec = {"mask": name, "shape": shape, "n": n, "runs": R, "reps": reps, "foreground": round(painted / vox, 4),
               "runs_equal_labels": same_painters, "labels_equal_boxes": same_as_boxes, "box_voxels": box_voxels}
        for key, _ in paths:
            ms = statistics.median(times[key])
            rec[key + "_ms"] = round(ms, 4)
            rec[key + "_min_max_ms"] = [round(min(times[key]), 4), round(max(times[key]), 4)]
            rec[key + "_bytes"] = nbytes[key]
            rec[key + "_GBps"] = round(nbytes[key] / ms / 1e6, 1)
        print(json.dumps(rec), flush=True)
        del labels, mask, owner, out_runs, out_labels, out_boxes
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
