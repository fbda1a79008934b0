"""bench.py's plain line and its --dump-outputs: a plain run times exactly --steps passes and leaves every leg of --full out, and
what it dumps is the mask and logit sums of its last timed pass - the same files whether --full runs after it or not, and
(up to the seam sums' fp32 association) whether one rank or two computed them."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("mask_row_counts", "mask_sample", "logit_sum_sample")


def _json_line(out):
    lines = [l for l in out.strip().splitlines() if l.startswith("{") and '"metric"' in l]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def _bench(args, env=None, launcher=()):
    r = subprocess.run([sys.executable, *launcher, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return _json_line(r.stdout)


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in FILES}


def test_plain_line_is_lean_and_dumps_what_the_full_run_dumps(tmp_path):
    common = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "tiny"]
    plain = _bench(common + ["--dump-outputs", str(tmp_path / "plain")])
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["full"] is False
    assert plain["metric"].startswith("voxels/sec") and plain["unit"] == "voxels/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "f16" and plain["ms_per_step"] > 0
    assert plain["value"] == pytest.approx(128 * 256 * 256 / (plain["ms_per_step"] * 1e-3), rel=1e-9)
    for leg in ("kernels", "roofline", "value_dense", "other_format", "ms_per_step_profiled", "extras", "step_walls", "cpu_baseline"):
        assert plain[leg] is None, leg
    a = _load(tmp_path / "plain")
    assert all(v.dtype == np.float32 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["mask_row_counts"].shape == (128, 256) and a["mask_sample"].shape == a["logit_sum_sample"].shape
    assert plain["outputs"]["sample_positions"] == a["mask_sample"].size > 0
    assert int(a["mask_row_counts"].sum()) == plain["config"]["mask_voxels"] > 0
    assert set(np.unique(a["mask_sample"]).tolist()) <= {0.0, 1.0} and np.isfinite(a["logit_sum_sample"]).all()

    # every leg of --full after the timed passes (the CPU leg and the step walls aside): the dump is taken before them
    full = _bench(common + ["--full", "--no-cpu-baseline", "--no-step-walls", "--dump-outputs", str(tmp_path / "full")])
    assert full["full"] is True and full["kernels"] and full["value_dense"] and full["extras"] and full["other_format"]
    assert full["config"]["mask_voxels"] == plain["config"]["mask_voxels"]
    assert full["config"]["mask_checksum"] == plain["config"]["mask_checksum"]
    b = _load(tmp_path / "full")
    for k in FILES:  # same inputs, deterministic blend: bit for bit
        assert np.array_equal(a[k], b[k]), k


def test_two_ranks_dump_the_single_rank_outputs(tmp_path):
    common = ["--steps", "1", "--warmup", "0", "--workload", "tiny"]
    env = dict(os.environ)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    _bench(["--gpus", "1", *common, "--dump-outputs", str(tmp_path / "one")], env=env)
    env["DLV_BENCH_SAME_DEVICE"] = "1"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    _bench(["--gpus", "2", *common, "--dump-outputs", str(tmp_path / "two")], env=env,
           launcher=("-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                     "--master-port", str(port)))
    a, b = _load(tmp_path / "one"), _load(tmp_path / "two")
    # the seam sums associate differently in fp32: a voxel whose mean logit is within rounding of 0 may flip
    assert np.abs(a["mask_row_counts"] - b["mask_row_counts"]).sum() <= 2
    assert np.abs(a["mask_sample"] - b["mask_sample"]).sum() <= 2
    np.testing.assert_allclose(b["logit_sum_sample"], a["logit_sum_sample"], rtol=1e-5, atol=1e-3)
