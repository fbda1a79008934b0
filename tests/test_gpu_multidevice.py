"""run_inference over several devices from one process (settings["mi355x"]["devices"]) and the Gaussian blend of the C-ABI
sharded pass (dlv_sw_infer_sharded_wsum).  Ranks that share device 0 exercise the same plan, slab, staging and seam code as
ranks on distinct GPUs (their seams move by device copies instead of RCCL); the last test runs RCCL between two GPUs when the
box has them.  The baseline of every run_inference check is the same call without the setting."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZBLOCK = 24  # erosion z-blocks of 24 planes (instead of one block for a small stack): block edges fall inside and between slabs


def _volume(shape, seed):
    """tissue with a background top (whole windows skip the network) and a hole inside (the erosion has work near seams)"""
    from delivr_cfos_amd.synth import synth_volume_np

    vol = synth_volume_np(shape, seed=seed, dense=True)
    vol[shape[0] - 8:] = 0
    vol[30:40, 15:30, 50:65] = 0
    return vol


def _write_padded_npy(path, vol, crop):
    from delivr_cfos_amd.hostlogic import padded_shape

    pad = padded_shape(vol.shape, crop)
    out = np.lib.format.open_memmap(path, mode="w+", dtype=np.uint16, shape=(1, 1) + pad)
    out[0, 0, : vol.shape[0], : vol.shape[1], : vol.shape[2]] = vol
    out.flush()
    return pad


def _scaled(sd, key, factor):
    out = {k: v.clone() for k, v in sd.items()}
    out[f"module.{key}.conv.weight"] *= factor
    out[f"module.{key}.conv.bias"] *= factor
    return out


def _settings(crop, precision, devices=None, blend=None, save_activated=False):
    s = {"blob_detection": {"window_dimensions": {"window_dim_0": crop[0], "window_dim_1": crop[1], "window_dim_2": crop[2]}},
         "mi355x": {"precision": precision}, "FLAGS": {"SAVE_ACTIVATED_OUTPUT": save_activated}}
    if devices is not None:
        s["mi355x"]["devices"] = devices
    if blend is not None:
        s["mi355x"]["blend"] = blend
    return s


def _one_device_mean(vol, crop, sd, precision, tta, gaussian=False):
    """mean logits of the one-device passes over the padded volume (what the mask thresholds) and one pass's stats"""
    import torch
    from delivr_cfos_amd.engine import HipEngine
    from delivr_cfos_amd.hostlogic import padded_shape, pass_schedule

    pad = padded_shape(vol.shape, crop)
    padded = np.zeros(pad, dtype=np.uint16)
    padded[: vol.shape[0], : vol.shape[1], : vol.shape[2]] = vol
    eng = HipEngine(0)
    eng.load_state_dict({"state_dict": sd})
    v = eng.to_device(padded)
    acc = torch.zeros(pad, dtype=torch.float32, device=eng.device)
    cnt = torch.zeros(pad, dtype=torch.float32 if gaussian else torch.uint8, device=eng.device)
    for flip_dim, repeat in pass_schedule(tta):
        if gaussian:
            st = eng.sw_infer(eng.make_sw_params(pad, crop, 0.5, flip_dim, 0, precision, repeat=repeat, blend="gaussian", wsum=cnt),
                              v, acc)
        else:
            st = eng.sw_infer(eng.make_sw_params(pad, crop, 0.5, flip_dim, 0, precision, repeat=repeat), v, acc, cnt)
    eng.sync()
    mean = (acc / cnt.float().clamp_min(1e-30)).cpu().numpy()[: vol.shape[0], : vol.shape[1], : vol.shape[2]]
    eng.close()
    return mean, st


def _run(tmp_path, name, vol, crop, sd, settings, tta=False, threshold=0.5):
    from delivr_cfos_amd.inference import run_inference

    nifti = os.path.join(str(tmp_path), "masked_nifti.npy")
    if not os.path.isfile(nifti):
        _write_padded_npy(nifti, vol, crop)
    out = run_inference([nifti], str(tmp_path / name), (1, 1) + vol.shape, comment="b", tta=tta, threshold=threshold,
                        crop_size=crop, state_dict={"state_dict": sd}, settings=settings)
    seg = os.path.join(out, "binary_segmentations")
    prob = os.path.join(seg, "network_output.npy")
    return (np.load(os.path.join(seg, "binaries.npy")), np.load(prob) if os.path.isfile(prob) else None,
            run_inference.last_shards)


def _check_shards(shards, world, devices, st, Z):
    assert shards is not None and len(shards) == world
    assert [s["device"] for s in shards] == list(devices)
    assert sum(s["windows"] for s in shards) == st["n_windows"]
    assert sum(s["skipped"] for s in shards) == st["n_skipped"]
    assert st["n_skipped"] > 0  # (the background top: some windows skip the network)
    lo = 0
    for s in shards:  # the owned ranges partition [0, Z) in rank order; a slab holds what its rank owns
        assert s["owned"][0] == lo and s["owned"][1] >= lo, shards
        if s["owned"][1] > s["owned"][0]:
            assert s["slab"][0] <= s["owned"][0] and s["slab"][1] >= s["owned"][1], s
        lo = s["owned"][1]
    assert lo == Z, shards
    assert sum(1 for s in shards if s["owned"][1] > s["owned"][0]) >= 2  # really sharded


def _check_masks(m1, m2, mean, threshold):
    assert m2.dtype == m1.dtype == np.uint8 and m2.shape == m1.shape
    assert m1.any() and not m1.all()
    near = np.abs(mean - np.log(threshold / (1.0 - threshold))) <= 1e-5
    diff = m1 != m2
    assert not (diff & ~near).any(), int((diff & ~near).sum())
    assert int(diff.sum()) <= 4, int(diff.sum())


@pytest.fixture
def small_zblocks(monkeypatch):
    """erosion z-blocks of ZBLOCK planes for the one-device baseline and the sharded run alike (the reference's Arrayterator
    rule gives one block for a stack this small)"""
    import delivr_cfos_amd.hostlogic as hl
    import delivr_cfos_amd.inference.inference as inf

    real = hl.arrayterator_zblock

    def zb(shape, buf_size=1000**3):
        return min(real(shape, buf_size), ZBLOCK)

    monkeypatch.setattr(hl, "arrayterator_zblock", zb)
    monkeypatch.setattr(inf, "arrayterator_zblock", zb)


# ---- 1. C ABI: the Gaussian blend of the sharded pass -------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("roi", [(32, 32, 32), (64, 64, 32)])
def test_c_abi_sharded_gaussian_blend_with_per_rank_weight_sums(world, roi):
    """dlv_sw_infer_sharded_wsum on ranks that share device 0: on the planes a rank owns, the sums and the weight sums equal the
    one-device Gaussian pass to 1e-5 relative (a seam adds the neighbour's partial sums as one term).  The old entry refuses a
    Gaussian pass over several ranks that would share one p->wsum_dev."""
    import torch
    from delivr_cfos_amd._lib import DLV_EINVAL, DelivrHipError
    from delivr_cfos_amd.engine import HipComm, HipEngine
    from delivr_cfos_amd.weights import random_state_dict

    shape, er, nb = (160, 64, 96), 7, 24
    vol = _volume(shape, seed=41)
    vol[100:] = 0
    sd = random_state_dict(3)
    one = HipEngine(0)
    one.load_state_dict({"state_dict": sd})
    v = one.to_device(vol)
    acc1 = torch.zeros(shape, dtype=torch.float32, device="cuda")
    ws1 = torch.zeros(shape, dtype=torch.float32, device="cuda")
    st1 = one.sw_infer(one.make_sw_params(shape, roi, 0.5, None, 0, "fp16", blend="gaussian", wsum=ws1), v, acc1)
    p = one.make_sw_params(shape, roi, 0.5, None, 0, "fp16", blend="gaussian")
    wmax = one.window_max(p, v)
    one.sync()

    comm = HipComm([0] * world)
    comm.engines[0].load_state_dict({"state_dict": sd})
    comm.bcast_weights(0)
    plan = comm.make_plan(p, np.where(wmax > 0, 1.0, 0.02).astype(np.float32))
    slabs, vols, accs, wss = [], [], [], []
    for r in range(world):
        lo, hi = plan.slab(r, shape[0], er, nb)
        slabs.append((lo, hi - lo))
        vols.append(v[lo:hi].clone())
        accs.append(torch.zeros((hi - lo,) + shape[1:], dtype=torch.float32, device="cuda"))
        wss.append(torch.zeros((hi - lo,) + shape[1:], dtype=torch.float32, device="cuda"))
    stats = comm.sw_infer_sharded(p, plan, slabs, vols, accs, wsums=wss)
    assert sum(s["n_windows"] for s in stats) == st1["n_windows"] and sum(s["n_skipped"] for s in stats) == st1["n_skipped"]
    torch.cuda.synchronize()
    covered, seams = 0, 0
    for r in range(world):
        olo, ohi = plan.z_owned[r]
        if ohi <= olo:
            continue
        lo = slabs[r][0]
        for mine, ref in ((accs[r], acc1), (wss[r], ws1)):
            d = (mine[olo - lo:ohi - lo] - ref[olo:ohi]).abs()
            assert float(d.max()) <= 1e-5 * max(float(ref[olo:ohi].abs().max()), 1.0), (r, float(d.max()))
        assert float(wss[r][olo - lo:ohi - lo].min()) > 0.0  # every owned plane holds weights
        covered += ohi - olo
        seams += len(plan.recvs(r))
    assert covered == shape[0] and seams >= world - 1

    # one p->wsum_dev for every rank: refused, naming the new entry
    shared = torch.zeros((max(n for _lo, n in slabs),) + shape[1:], dtype=torch.float32, device="cuda")
    q = one.make_sw_params(shape, roi, 0.5, None, 0, "fp16", blend="gaussian", wsum=shared)
    with pytest.raises(DelivrHipError, match="dlv_sw_infer_sharded_wsum") as ei:
        comm.sw_infer_sharded(q, plan, slabs, vols, accs)
    assert ei.value.code == DLV_EINVAL
    comm.close()
    one.close()


# ---- 2-4. run_inference on ranks that share device 0 ---------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("precision,crop", [("fp32", (32, 32, 32)), ("fp16", (32, 32, 32)), ("fp16", (64, 64, 32))])
def test_run_inference_on_shared_device_ranks_equals_the_default_call(tmp_path, small_zblocks, world, precision, crop):
    from delivr_cfos_amd.weights import random_state_dict

    vol = _volume((70, 45, 90), seed=43)
    sd = random_state_dict(8)
    m1, _p1, sh1 = _run(tmp_path, "one", vol, crop, sd, _settings(crop, precision))
    assert sh1 is None
    m2, _p2, sh2 = _run(tmp_path, "many", vol, crop, sd, _settings(crop, precision, devices=[0] * world))
    mean, st = _one_device_mean(vol, crop, sd, precision, False)
    _check_masks(m1, m2, mean, 0.5)
    _check_shards(sh2, world, [0] * world, st, vol.shape[0])


@pytest.mark.parametrize("world", [2, 3])
def test_run_inference_on_shared_device_ranks_with_tta_count_map_and_network_output(tmp_path, small_zblocks, world):
    """13-pass TTA (3 weighted passes), threshold 0.4 (the uint8 count map travels with the sums) and network_output.npy"""
    from delivr_cfos_amd.weights import random_state_dict

    crop = (32, 32, 32)
    vol = _volume((70, 45, 90), seed=47)
    sd = random_state_dict(9)
    m1, p1, _ = _run(tmp_path, "one", vol, crop, sd, _settings(crop, "fp16", save_activated=True), tta=True, threshold=0.4)
    m2, p2, sh2 = _run(tmp_path, "many", vol, crop, sd, _settings(crop, "fp16", devices=[0] * world, save_activated=True), tta=True,
                       threshold=0.4)
    mean, st = _one_device_mean(vol, crop, sd, "fp16", True)
    _check_masks(m1, m2, mean, 0.4)
    _check_shards(sh2, world, [0] * world, st, vol.shape[0])
    assert p1 is not None and p2 is not None and p2.dtype == np.float32 and p2.shape == p1.shape
    assert float(np.abs(p2 - p1).max()) <= 1e-5


def test_run_inference_gaussian_blend_on_shared_device_ranks(tmp_path, small_zblocks):
    """blend "gaussian" with threshold 0.4: the per-rank weight sums cross the seams (dlv_sw_infer_sharded_wsum)"""
    from delivr_cfos_amd.weights import random_state_dict

    crop = (32, 32, 32)
    vol = _volume((70, 45, 90), seed=53)
    sd = random_state_dict(10)
    m1, p1, _ = _run(tmp_path, "one", vol, crop, sd, _settings(crop, "fp16", blend="gaussian", save_activated=True), threshold=0.4)
    m2, p2, sh2 = _run(tmp_path, "many", vol, crop, sd, _settings(crop, "fp16", devices=[0, 0], blend="gaussian", save_activated=True),
                       threshold=0.4)
    mean, st = _one_device_mean(vol, crop, sd, "fp16", False, gaussian=True)
    _check_masks(m1, m2, mean, 0.4)
    _check_shards(sh2, 2, [0, 0], st, vol.shape[0])
    assert float(np.abs(p2 - p1).max()) <= 1e-5


# ---- 5. range guard ----------------------------------------------------------------------------------------------------------
def test_run_inference_range_guard_on_every_rank(tmp_path, capsys):
    """a checkpoint whose down_1 conv overflows fp16: dlv_comm_range_recover gives both ranks the same block shift, the passes
    repeat in fp16 (never the bf16 last resort) and the mask equals the one-device recovery's"""
    from delivr_cfos_amd.weights import random_state_dict

    crop = (32, 32, 32)
    vol = _volume((72, 64, 64), seed=9)
    big = _scaled(random_state_dict(6), "down_1.convs.conv_0", 1.0e6)
    m1, _p, _s = _run(tmp_path, "one", vol, crop, big, _settings(crop, "fp16"))
    capsys.readouterr()
    m2, _p, sh2 = _run(tmp_path, "many", vol, crop, big, _settings(crop, "fp16", devices=[0, 0]))
    out = capsys.readouterr().out
    assert "storing its raw output scaled by 2^-" in out and "on every rank" in out, out
    assert "bf16 operands" not in out, out
    assert sh2 is not None and len(sh2) == 2
    assert m1.any() and m2.shape == m1.shape
    assert int((m1 != m2).sum()) <= 4, int((m1 != m2).sum())


# ---- 6. the CLI --------------------------------------------------------------------------------------------------------------
def _uncompressed_tiff(path, plane):
    import struct

    h, w = plane.shape
    data = plane.astype("<u2").tobytes()
    tags = [(256, 3, w), (257, 3, h), (258, 3, 16), (259, 3, 1), (262, 3, 1), (273, 4, 8), (277, 3, 1), (278, 3, h),
            (279, 4, len(data))]
    with open(path, "wb") as fh:
        fh.write(b"II" + struct.pack("<HI", 42, 8 + len(data)))
        fh.write(data)
        fh.write(struct.pack("<H", len(tags)))
        for tag, typ, val in tags:
            fh.write(struct.pack("<HHI", tag, typ, 1) + (struct.pack("<HH", val, 0) if typ == 3 else struct.pack("<I", val)))
        fh.write(struct.pack("<I", 0))


def _cli_tree(root, vol, crop, wfile, brain, devices):
    raw_dir = os.path.join(root, "raw", brain)
    os.makedirs(raw_dir)
    for z in range(vol.shape[0]):
        _uncompressed_tiff(os.path.join(raw_dir, f"Z{z:04d}.tif"), vol[z])
    mask_dir = os.path.join(root, "out", "01_mask", brain, "masked_niftis")
    os.makedirs(mask_dir)
    _write_padded_npy(os.path.join(mask_dir, "masked_nifti.npy"), vol, crop)
    cfg = {
        "raw_location": os.path.join(root, "raw") + "/", "output_location": os.path.join(root, "out") + "/",
        "mask_detection": {"output_location": os.path.join(root, "out", "01_mask") + "/"},
        "blob_detection": {"input_location": os.path.join(root, "out", "01_mask") + "/", "model_location": wfile,
                           "output_location": os.path.join(root, "out", "02_blob") + "/",
                           "window_dimensions": {"window_dim_0": crop[0], "window_dim_1": crop[1], "window_dim_2": crop[2]}},
        "postprocessing": {"input_location": os.path.join(root, "out", "02_blob") + "/",
                           "output_location": os.path.join(root, "out", "03_post") + "/", "min_size": -1, "max_size": -1},
        "mi355x": {} if devices is None else {"devices": devices},
        "FLAGS": {"ABSPATHS": True, "LOAD_ALL_RAM": True, "TEST_TIME_AUGMENTATION": False, "MASK_DOWNSAMPLE": False,
                  "BLOB_DETECTION": True, "POSTPROCESSING": True, "ATLAS_ALIGNMENT": False, "REGION_ASSIGNMENT": False,
                  "VISUALIZATION": False, "SAVE_ACTIVATED_OUTPUT": False},
    }
    cfg_path = os.path.join(root, "config.json")
    with open(cfg_path, "w") as fh:
        json.dump(cfg, fh)
    return cfg_path


def test_cli_with_devices_writes_the_files_of_the_one_device_run(tmp_path):
    """python -m delivr_cfos_amd config.json (steps 2 and 3) in fresh processes, once as shipped and once with "devices": [0, 0]:
    binaries.npy, the label file, the statistics pickle and the CSV are byte-identical.  The input is first checked to hold no
    voxel whose mean logit is within 1e-5 of the threshold (where the seam sums' fp32 association could flip a voxel)."""
    import torch
    from delivr_cfos_amd.weights import random_state_dict

    from oracle.delivr_oracle import erode_l1

    brain, crop = "brainM", (32, 32, 32)
    # logits 100x wider than the random checkpoint's (~0.3): a voxel within 1e-5 of the threshold becomes rare
    sd = {k: (v * 100.0 if k.startswith("module.final_conv.") else v.clone()) for k, v in random_state_dict(11).items()}
    for seed in (59, 60, 61, 62, 63):  # the first volume none of whose voxels that can enter the mask sits on the threshold
        vol = _volume((70, 45, 90), seed=seed)
        mean, _st = _one_device_mean(vol, crop, sd, "fp16", False)
        if not ((np.abs(mean) <= 1e-5) & (erode_l1((vol > 0).astype(np.uint8), 30) > 0)).any():
            break
    else:
        pytest.fail("every candidate volume has a voxel on the threshold")
    wfile = os.path.join(str(tmp_path), "weights.tar")
    torch.save({"state_dict": sd}, wfile)
    files = {}
    for name, devices in (("one", None), ("many", [0, 0])):
        root = os.path.join(str(tmp_path), name)
        cfg = _cli_tree(root, vol, crop, wfile, brain, devices)
        r = subprocess.run([sys.executable, "-m", "delivr_cfos_amd", cfg], cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
        post = os.path.join(root, "out", "03_post")
        got = {"binaries.npy": open(os.path.join(root, "out", "02_blob", brain, "binary_segmentations", "binaries.npy"), "rb").read()}
        for f in sorted(os.listdir(post)):
            got[f] = open(os.path.join(post, f), "rb").read()
        files[name] = got
    assert sorted(files["one"]) == sorted(files["many"]), (sorted(files["one"]), sorted(files["many"]))
    assert any(f.endswith("-cc3d.npy") for f in files["one"]) and any(f.endswith(".csv") for f in files["one"])
    for f in files["one"]:
        assert files["one"][f] == files["many"][f], f
    assert np.load(os.path.join(str(tmp_path), "one", "out", "02_blob", brain, "binary_segmentations", "binaries.npy")).any()
    stats = pickle.loads(files["one"][f"{brain}-stats.pickle"])
    assert len(stats["voxel_counts"]) > 1


# ---- 7. distinct devices: the RCCL seam exchange -----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_run_inference_on_two_distinct_devices(tmp_path, small_zblocks, precision):
    import torch
    from delivr_cfos_amd.weights import random_state_dict

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    crop = (32, 32, 32)
    vol = _volume((70, 45, 90), seed=61)
    sd = random_state_dict(12)
    m1, _p, _s = _run(tmp_path, "one", vol, crop, sd, _settings(crop, precision))
    m2, _p, sh2 = _run(tmp_path, "many", vol, crop, sd, _settings(crop, precision, devices=[0, 1]))
    mean, st = _one_device_mean(vol, crop, sd, precision, False)
    _check_masks(m1, m2, mean, 0.5)
    _check_shards(sh2, 2, [0, 1], st, vol.shape[0])
