"""No-GPU checks of the boundary: the C-ABI library loads, exports every symbol the header
declares, and its host-only tiler agrees with the reference's window enumeration."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ensure_built():
    from delivr_cfos_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib


def test_library_exports_every_declared_symbol():
    _lib = _ensure_built()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "delivr_hip.h")).read()
    assert not re.search(r"\bdlv_(debug|diag)_[a-z0-9_]+\s*\(", header), "test hooks belong in include/delivr_hip_diag.h, not in the drop-in boundary"
    diag = open(os.path.join(ROOT, "include", "delivr_hip_diag.h")).read()
    declared = set(re.findall(r"\b(dlv_[a-z0-9_]+)\s*\(", header)) | set(re.findall(r"\b(dlv_[a-z0-9_]+)\s*\(", diag))
    declared -= {"dlv_ctx"}
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"libdelivr_hip.so does not export {name}"
        assert name in _lib.SIGNATURES, f"ctypes binding lacks {name}"
    assert set(_lib.SIGNATURES) == declared
    assert lib.dlv_abi_version() == 2


def test_library_loaded_before_torch_shares_torch_hip_runtime():
    """_lib.load() in a process that has not imported torch yet (build() then smoke(), or this file's tests ahead of the GPU
    ones): the library must bind to the libamdhip64 torch brings, not map ROCm's beside it - with two HIP runtimes in one
    process every context of the library fails to create."""
    import ast
    import subprocess
    import sys

    _ensure_built()
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "from delivr_cfos_amd import _lib\n"
            "_lib.load()\n"
            "import torch\n"
            "print(sorted({l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}))\n")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    runtimes = ast.literal_eval(r.stdout.strip().splitlines()[-1])
    assert len(runtimes) == 1, runtimes


def test_host_tiler_matches_reference_golden(golden_dir):
    _lib = _ensure_built()
    lib = _lib.load()
    g = np.load(os.path.join(golden_dir, "ref_tiler.npz"))
    for i in range(int(g["n_cases"])):
        p = _lib.SwParams()
        p.Zp, p.Yp, p.Xp = (int(v) for v in g[f"case{i}_image"])
        for k in range(3):
            p.roi[k] = int(g[f"case{i}_roi"][k])
        p.overlap = 0.5
        n = C.c_int64()
        assert lib.dlv_sw_num_windows(C.byref(p), C.byref(n)) == 0
        ref = g[f"case{i}_starts"]
        assert n.value == len(ref)
        buf = np.zeros((n.value, 3), dtype=np.int64)
        assert lib.dlv_sw_window_starts(C.byref(p), buf.ctypes.data_as(C.POINTER(C.c_int64)), n.value) == 0
        np.testing.assert_array_equal(buf, ref)


def test_bad_geometry_is_an_error_code():
    _lib = _ensure_built()
    lib = _lib.load()
    p = _lib.SwParams()
    p.Zp, p.Yp, p.Xp = 32, 32, 32
    p.roi[0], p.roi[1], p.roi[2] = 64, 32, 32  # roi larger than the (padded) volume
    p.overlap = 0.5
    n = C.c_int64()
    assert lib.dlv_sw_num_windows(C.byref(p), C.byref(n)) == _lib.DLV_EUNSUP
    p.roi[0] = 32
    p.overlap = 1.0
    assert lib.dlv_sw_num_windows(C.byref(p), C.byref(n)) == _lib.DLV_EINVAL


def test_plain_c_host_compiles_links_and_fails_loudly_without_gpu(tmp_path):
    """examples/c_host.c drives the path through include/delivr_hip.h from C99 (no Python, no torch): the header is
    valid C, every entry point it uses links against libdelivr_hip.so, and without a GPU the program says so and exits
    non-zero (on the GPU box it runs the pass: see INTEGRATION.md)."""
    import shutil
    import subprocess

    import torch

    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lib_dir = os.path.join(ROOT, "delivr_cfos_amd", "lib")
    exe = str(tmp_path / "c_host")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "c_host.c"), "-o", exe, "-L" + lib_dir, "-ldelivr_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,--allow-shlib-undefined", "-lm"])
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c",
                           os.path.join(ROOT, "include", "delivr_hip.h")])
    # `--plan N` is host logic only (dlv_shard_plan_make / dlv_shard_slab): it must agree with the Python planner
    from delivr_cfos_amd import parallel
    from oracle import delivr_oracle as orc
    r = subprocess.run([exe, "--plan", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    starts = orc.window_list((48, 64, 64), (32, 32, 32), 0.5)
    plan = parallel.make_plan(starts, 32, 48, 3)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3
    for rank, line in enumerate(lines):
        (wb, we), (cl, ch), (ol, oh) = plan.win_ranges[rank], plan.z_computed[rank], plan.z_owned[rank]
        z0, z1 = plan.slab(rank, 48, erode_iters=3)
        assert line == (f"rank {rank}: windows [{wb},{we}) computes [{cl},{ch}) owns [{ol},{oh}) holds [{z0},{z1})"), line
    if torch.cuda.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 2 and "needs an MI355X" in r.stderr
        r = subprocess.run([exe, "--gpus", "2", "--same-device"], capture_output=True, text=True)
        assert r.returncode == 2 and "dlv_comm_init_all" in r.stderr
