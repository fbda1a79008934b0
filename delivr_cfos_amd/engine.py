"""HipEngine - one libdelivr_hip context bound to one MI355X, driven with torch tensors.

torch is only the device-memory container here (and, across ranks, the RCCL front end): every
computation below is a call through the C ABI (include/delivr_hip.h).  There is no CPU
fallback; constructing an engine without a visible GPU raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import PREC_BF16, PREC_BF16_ALL, PREC_F16, PREC_F32, DelivrHipError

# "bf16": bf16 operands / storage at levels 1-4, fp16 at full resolution (include/delivr_hip.h DLV_PREC_BF16);
# "bf16_all": bf16 at every level
PRECISIONS = {"fp32": PREC_F32, "f32": PREC_F32, "bf16": PREC_BF16, "fp16": PREC_F16, "f16": PREC_F16, "bf16_all": PREC_BF16_ALL}
RANGE_GUARDED = ("fp16", "f16", "bf16")  # formats with fp16 tensors: DLV_ERANGE is recoverable (range_guard.py)

# checkpoint keys of the 18 conv blocks in forward order (include/delivr_hip.h)
CONV_BLOCKS = (
    ["conv_0.conv_0", "conv_0.conv_1"]
    + [f"down_{k}.convs.conv_{j}" for k in (1, 2, 3, 4) for j in (0, 1)]
    + [f"upcat_{k}.convs.conv_{j}" for k in (4, 3, 2, 1) for j in (0, 1)]
)
DECONV_BLOCKS = [f"upcat_{k}.upsample.deconv" for k in (4, 3, 2, 1)]


def strip_state_dict(checkpoint) -> Dict[str, "np.ndarray"]:
    """Accepts what torch.load(model_weights) returns in the reference: a dict holding
    "state_dict" (inference/inference.py:222) or "model_state" (inference_nifti_load.py:215), keys
    prefixed "module." by DataParallel; or a bare state_dict."""
    sd = checkpoint
    if isinstance(sd, dict):
        for key in ("state_dict", "model_state"):
            if key in sd and isinstance(sd[key], dict):
                sd = sd[key]
                break
    out = {}
    for k, v in sd.items():
        if k.startswith("module."):
            k = k[len("module."):]
        out[k] = v
    return out


class HipComm:
    """One process, N devices: dlv_comm_init_all / dlv_bcast_weights / dlv_sw_infer_sharded (the C-ABI form of the
    DataParallel replacement; the multi-process form lives in parallel.py).  `engines[r]` drives rank r's context."""

    def __init__(self, devices: Sequence[int]):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("delivr_cfos_amd needs an MI355X: there is no CPU fallback for the HIP path")
        self.torch = torch
        self.lib = _lib.load()
        self.devices = [int(d) for d in devices]
        arr = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        rc = self.lib.dlv_comm_init_all(len(self.devices), arr, C.byref(h))
        if rc != 0:
            why = self.lib.dlv_comm_last_error(None)  # (NULL: the reason the last init of this thread failed)
            raise DelivrHipError(rc, "dlv_comm_init_all failed: " + (why.decode() if why else "several devices need librccl.so"))
        self.handle = h
        self.engines = [HipEngine(d, _ctx=C.c_void_p(self.lib.dlv_comm_ctx(h, r))) for r, d in enumerate(self.devices)]

    def close(self):
        if getattr(self, "handle", None):
            self.lib.dlv_comm_destroy(self.handle)
            self.handle = None
            for e in self.engines:
                e.ctx = None

    def _check(self, rc: int):
        if rc != 0:
            raise DelivrHipError(rc, self.lib.dlv_comm_last_error(self.handle).decode(errors="replace"))

    @property
    def uses_rccl(self) -> bool:
        return bool(self.lib.dlv_comm_uses_rccl(self.handle))

    def selftest(self, nbytes: int = 64 << 20) -> None:
        """Ring exchange + broadcast of `nbytes` through the communicator's transport, compared word for word."""
        self._check(self.lib.dlv_comm_selftest(self.handle, int(nbytes)))

    def bcast_weights(self, root: int = 0):
        self._check(self.lib.dlv_bcast_weights(self.handle, int(root)))
        for e in self.engines:
            e.features = self.engines[root].features

    def range_recover(self) -> int:
        """dlv_comm_range_recover after sw_infer_sharded raised DLV_ERANGE: the same next block shifts on every rank
        -> number of blocks changed (raises DLV_ERANGE when nothing is left)"""
        n = C.c_int()
        self._check(self.lib.dlv_comm_range_recover(self.handle, C.byref(n)))
        return n.value

    def make_plan(self, params, weights=None):
        from .parallel import plan_from_params

        return plan_from_params(params, len(self.devices), weights)

    def sw_infer_sharded(self, params, plan, slabs, vols, accs, cnts=None, wsums=None):
        """slabs[r] = (z0, nz); vols / accs / cnts: per-rank tensors on devices[r] holding those planes.  wsums: per-rank fp32
        weight-sum slabs of the Gaussian blend (dlv_sw_infer_sharded_wsum; params.wsum_dev is then ignored)."""
        n = len(self.devices)
        pc = _lib.ShardPlanC()
        pc.world, pc.n_windows = n, plan.n_windows
        for r in range(n):
            pc.win_begin[r], pc.win_end[r] = plan.win_ranges[r]
            pc.z_comp_lo[r], pc.z_comp_hi[r] = plan.z_computed[r]
            pc.z_own_lo[r], pc.z_own_hi[r] = plan.z_owned[r]
        z0 = (C.c_int * n)(*[int(s[0]) for s in slabs])
        nz = (C.c_int * n)(*[int(s[1]) for s in slabs])
        torch = self.torch
        vp = (C.c_void_p * n)(*[self.engines[r]._dev(vols[r], torch.uint16, "vol").value for r in range(n)])
        ap = (C.c_void_p * n)(*[self.engines[r]._dev(accs[r], torch.float32, "acc").value for r in range(n)])
        cp = None
        if cnts is not None:
            cp = (C.c_void_p * n)(*[self.engines[r]._dev(cnts[r], torch.uint8, "cnt").value for r in range(n)])
        st = (_lib.SwStats * n)()
        for d in set(self.devices):
            torch.cuda.synchronize(d)
        if wsums is None:
            self._check(self.lib.dlv_sw_infer_sharded(self.handle, C.byref(params), C.byref(pc), z0, nz, vp, ap, cp, st))
        else:
            wp = (C.c_void_p * n)(*[self.engines[r]._dev(wsums[r], torch.float32, "wsum").value for r in range(n)])
            self._check(self.lib.dlv_sw_infer_sharded_wsum(self.handle, C.byref(params), C.byref(pc), z0, nz, vp, ap, cp, wp, st))
        return [{"n_windows": s.n_windows, "n_skipped": s.n_skipped, "n_forward_launches": s.n_forward_launches} for s in st]


_shared_engines: Dict[int, "HipEngine"] = {}
_shared_comms: Dict[Tuple[int, ...], HipComm] = {}


def shared_comm(devices: Sequence[int]) -> HipComm:
    """The process-wide communicator of a device tuple (run_inference with settings["mi355x"]["devices"]): initialised once per
    process like shared_engine's engines, its contexts keep their workspaces and seam staging between brains."""
    key = tuple(int(d) for d in devices)
    comm = _shared_comms.get(key)
    if comm is None or comm.handle is None:
        comm = HipComm(key)
        _shared_comms[key] = comm
    return comm


def shared_engine(device: int = 0) -> "HipEngine":
    """The process-wide engine of a device.  run_inference and count_blobs use it by default, so that one `python -m
    delivr_cfos_amd` run keeps its context between steps and brains: the workspaces of a pass (~35 GB) and of the labelling
    (~2 GB) and the pinned staging ring are allocated once and never handed back to the driver in between (large allocations
    that follow a release took up to seconds on this platform: profiles/r06r_alloc_probe2.json).  The reference's counterpart is PyTorch's caching allocator living as long as the process."""
    eng = _shared_engines.get(int(device))
    if eng is None or eng.ctx is None:
        eng = HipEngine(int(device))
        eng.shared = True
        _shared_engines[int(device)] = eng
    return eng


def layer_plan(window, switches=None, precision="fp16", batch=1, features=(32, 32, 64, 128, 256, 32)):
    """Which kernel runs each layer of one forward of a sliding-window pass over `window` = (d, h, w), under the dlv_diag_set
    `switches` {name: value} - dlv_diag_plan: what the forward itself consults (csrc/layer_plan.h), computed on the host; needs
    no GPU and no engine.  Returns {"conv": 18 dicts, "deconv": 4, "pool": 4, "labels": [(label, flops, bytes)] in launch order};
    kernels by name (_lib.PLAN_CONV_KERNELS / PLAN_DECONV_KERNELS), None = not launched."""
    lib = _lib.load()
    sw = dict(switches or {})
    names = (C.c_char_p * max(1, len(sw)))(*[k.encode() for k in sw])
    values = (C.c_int * max(1, len(sw)))(*[int(v) for v in sw.values()])
    out = _lib.LayerPlan()
    rc = lib.dlv_diag_plan((C.c_int * 6)(*features), names, values, len(sw), {"bf16_all": 0, "fp16": 1, "bf16": 2}[precision], int(batch),
                           *(int(v) for v in window), C.byref(out))
    if rc != 0:
        raise DelivrHipError(rc, f"dlv_diag_plan: window {tuple(window)}, switches {sw}")

    def fields(st, kernels):
        d = {name: getattr(st, name) for name, _ in st._fields_}
        d["kernel"] = None if st.kernel < 0 else kernels[st.kernel]
        return d

    return {"conv": [fields(c, _lib.PLAN_CONV_KERNELS) for c in out.conv],
            "deconv": [fields(c, _lib.PLAN_DECONV_KERNELS) for c in out.deconv],
            "pool": [{name: getattr(p, name) for name, _ in p._fields_} for p in out.pool],
            "labels": [(out.labels[i].value.decode(), out.flops[i], out.bytes[i]) for i in range(out.n_labels)]}


class HipEngine:
    shared = False  # True: owned by shared_engine() - callers that "own" their engine must not close it

    def __init__(self, device: int = 0, _ctx=None):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("delivr_cfos_amd needs an MI355X (torch.cuda.is_available() is False); "
                               "there is no CPU fallback for the HIP path")
        self.torch = torch
        self.lib = _lib.load()
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        self.features: Optional[Tuple[int, ...]] = None
        self._keep = []
        self._owns_ctx = _ctx is None
        if _ctx is not None:
            # a context owned by a HipComm: it runs on its own stream (dlv_stream); torch work is ordered against it by
            # device-wide synchronisation in _enter/_leave
            self.ctx = _ctx
            self.tstream = torch.cuda.ExternalStream(self.lib.dlv_stream(_ctx), device=self.device)
            return
        self.tstream = torch.cuda.Stream(device=self.device)
        ctx = C.c_void_p()
        rc = self.lib.dlv_ctx_create(self.device_index, C.c_void_p(self.tstream.cuda_stream), C.byref(ctx))
        if rc != 0:
            raise DelivrHipError(rc, "dlv_ctx_create failed")
        self.ctx = ctx

    # ---- plumbing ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None) and getattr(self, "_owns_ctx", True):
            self.lib.dlv_ctx_destroy(self.ctx)
        self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise DelivrHipError(rc, self.lib.dlv_last_error(self.ctx).decode(errors="replace"))

    def _enter(self):
        """kernels run on the engine stream: order them after whatever torch queued so far"""
        self.tstream.wait_stream(self.torch.cuda.current_stream(self.device))

    def _leave(self):
        self.torch.cuda.current_stream(self.device).wait_stream(self.tstream)

    def sync(self):
        self._check(self.lib.dlv_sync(self.ctx))

    def _dev(self, t, dtype, name):
        torch = self.torch
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise TypeError(f"{name}: expected a torch tensor on {self.device}, got {type(t)} on "
                            f"{getattr(t, 'device', None)}")
        if t.dtype != dtype:
            raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: tensor must be contiguous")
        return C.c_void_p(t.data_ptr())

    def to_device(self, arr, dtype=None):
        """numpy / torch-cpu -> tensor in HBM (uint16 volumes go through torch.uint16)."""
        torch = self.torch
        if isinstance(arr, torch.Tensor):
            t = arr
        else:
            a = np.ascontiguousarray(arr)
            if not a.flags.writeable:  # (a read-only memmap: torch.from_numpy on it is undefined behaviour; big volumes
                a = np.array(a)        # go through upload_volume, which never wraps the memmap)
            t = torch.from_numpy(a)
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        return t.to(self.device).contiguous()

    def upload_volume(self, arr, z_lo: int = 0, z_hi: Optional[int] = None, chunk_bytes: int = 64 << 20):
        """Host uint16 volume (numpy array or memmap, (..., Z, Y, X)) -> planes [z_lo, z_hi) in HBM through the pinned staging
        ring of hostio.upload: a memmapped .npy is read with parallel preads straight into pinned memory (no whole-volume
        pageable copy; the reference memmaps the file too, inference/inference.py:234), the copy engine moves the previous
        chunk meanwhile, and a rank of a sharded run reads only the planes of its slab."""
        from . import hostio

        a = arr if isinstance(arr, np.ndarray) else np.asarray(arr)
        lead = a.shape[:-3]
        if any(int(v) != 1 for v in lead):
            raise ValueError("one volume, one channel expected")
        if a.dtype != np.uint16:
            raise TypeError(f"upload_volume: uint16 volume expected, got {a.dtype}")
        view = a.reshape(a.shape[-3:])
        Z, Y, X = (int(v) for v in view.shape)
        z_hi = Z if z_hi is None else int(z_hi)
        out = self.torch.empty(tuple(int(v) for v in lead) + (z_hi - z_lo, Y, X), dtype=self.torch.uint16, device=self.device)
        hostio.upload(self, view[z_lo:z_hi], out=out, chunk_bytes=chunk_bytes, what="h2d_volume")
        return out

    # ---- weights -----------------------------------------------------------------------------------
    def load_state_dict(self, checkpoint) -> None:
        """dlv_unet_load from a MONAI BasicUNet checkpoint (inference/inference.py:190-200,222)."""
        torch = self.torch
        sd = strip_state_dict(checkpoint)
        w = _lib.UnetWeights()
        keep = []

        def ptr(key):
            if key not in sd:
                raise KeyError(f"checkpoint has no '{key}' (expected MONAI BasicUNet names)")
            v = sd[key]
            a = v.detach().cpu().float().contiguous().numpy() if isinstance(v, torch.Tensor) else np.ascontiguousarray(v, np.float32)
            keep.append(a)
            return a.ctypes.data_as(C.c_void_p).value, a.shape

        feats = []
        for i, blk in enumerate(CONV_BLOCKS):
            w.conv_w[i], shp = ptr(f"{blk}.conv.weight")
            w.conv_b[i], _ = ptr(f"{blk}.conv.bias")
            w.norm_g[i], _ = ptr(f"{blk}.adn.N.weight")
            w.norm_b[i], _ = ptr(f"{blk}.adn.N.bias")
            if tuple(shp[2:]) != (3, 3, 3):
                raise ValueError(f"{blk}.conv.weight has shape {shp}")
            feats.append(shp)
        for j, blk in enumerate(DECONV_BLOCKS):
            w.deconv_w[j], shp = ptr(f"{blk}.weight")
            w.deconv_b[j], _ = ptr(f"{blk}.bias")
            if tuple(shp[2:]) != (2, 2, 2):
                raise ValueError(f"{blk}.weight has shape {shp}")
        w.final_w, fshape = ptr("final_conv.weight")
        w.final_b, _ = ptr("final_conv.bias")
        features = (feats[0][0], feats[2][0], feats[4][0], feats[6][0], feats[8][0], feats[16][0])
        if feats[0][1] != 1 or fshape[0] != 1 or fshape[1] != features[5]:
            raise ValueError("only in_channels=1 / out_channels=1 networks are supported (inference.py:190-197)")
        for k in range(6):
            w.features[k] = int(features[k])
        self._enter()
        self._check(self.lib.dlv_unet_load(self.ctx, C.byref(w)))
        self._leave()
        self.features = tuple(int(f) for f in features)

    def weight_blob(self):
        """The packed parameters in HBM as a uint8 torch tensor view (for an RCCL broadcast)."""
        n = C.c_size_t()
        p = C.c_void_p()
        self._check(self.lib.dlv_unet_blob_size(self.ctx, C.byref(n)))
        self._check(self.lib.dlv_unet_blob_dev(self.ctx, C.byref(p)))
        return _tensor_view(self.torch, p.value, n.value, self.device)

    def alloc_weight_blob(self, features: Sequence[int]):
        arr = (C.c_int * 6)(*[int(f) for f in features])
        self._check(self.lib.dlv_unet_alloc_blob(self.ctx, arr))
        self.features = tuple(int(f) for f in features)

    # ---- forward -----------------------------------------------------------------------------------
    def unet_forward(self, x, precision: str = "fp32"):
        """(B,1,d,h,w) fp32 tensor in HBM -> logits (B,1,d,h,w) fp32."""
        torch = self.torch
        if x.dim() != 5 or x.shape[1] != 1:
            raise ValueError("x must be (B,1,d,h,w)")
        out = torch.empty_like(x)
        B, _, d, h, w = x.shape
        self._enter()
        self._check(self.lib.dlv_unet_forward_dev(self.ctx, self._dev(x, torch.float32, "x"),
                                                  self._dev(out, torch.float32, "out"), B, d, h, w,
                                                  PRECISIONS[precision]))
        self._leave()
        return out

    def diag_set(self, name: str, value: int = 1) -> None:
        """a kernel-selection switch of this context (include/delivr_hip_diag.h: dlv_diag_set) - tests and A/B runs; the library
        reads no such switch from the environment"""
        self._check(self.lib.dlv_diag_set(self.ctx, name.encode(), int(value)))

    _BLOCK_COUT = (0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 5, 5)  # features[] index of each conv block's Cout

    def debug_layer16(self, kind: int, op: str = "conv", index: int = 0, in1=None, ss1=None, in2=None, vol=None,
                      flip_dim=None, precision: str = "bf16", skip_shape=None, pool=False, writeback=True, seam=False,
                      acc=None, starts=None, scale: float = 1.0, bw=None, bmin: float = 0.0, wsum=None):
        """test hook (dlv_debug_layer16): one conv block (op "conv", in1 raw where ss1 = its (B, c1, 2) scale/shift is given),
        the folded first conv of upcat_1 (op "folded": in1 fine skip tensor, in2 ACTIVATED coarse tensor) or the stem (op
        "stem": vol = B uint16 windows (B, D, H, W)).  kind 0 final output, 2 raw output, 3 scale/shift (B, Cout, 2).
        kind 1 (op "conv"): transposed conv `index` of in1 (raw where ss1 is given) -> (B, Cout, 2D, 2H, 2W), or replicate-padded
        to skip_shape (each dimension 2 x the input's or one more).
        op "norm": the InstanceNorm + Mish pass over the raw in1 with ss1 -> the tensor as the pass leaves it, or with pool
        (out, pooled); writeback False: pool only, out stays raw; seam: the mixed mode's format change (fp16: pooled in bf16,
        needs pool; bf16: activated in fp16, no pool).  op "final": the 1x1x1 conv on the raw in1 (B, 32, D, H, W) with ss1 ->
        logits (B, D, H, W).  op "final" with acc (fp32 (Z, Yp, Xp)): the blend mode - the B windows, forwarded flipped along
        flip_dim, are un-flipped and added into acc at starts (B, 3) times `scale`, or with bw (fp32, D + H + W factors) times
        max(bw[z] bw[D + y] bw[D + H + x], bmin) * scale, which wsum (shaped like acc, optional) collects; returns the report alone.
        Returns (out, report): report names the kernels that ran and how the raw output is stored (delivr_hip_diag.h)."""
        torch = self.torch
        a = _lib.DebugLayerArgs()
        a.kind, a.index, a.flip_dim = int(kind), int(index), -1 if flip_dim is None else int(flip_dim)
        a.op = {"conv": 0, "folded": 1, "stem": 2, "norm": 3, "final": 4}[op]
        if op == "stem":
            B, D, H, W = vol.shape
            a.vol = self._dev(vol, torch.uint16, "vol").value
            a.index = 0
        else:
            B, c1, D, H, W = in1.shape
            a.in1, a.c1 = self._dev(in1, torch.float32, "in1").value, int(c1)
            if in2 is not None:
                a.in2, a.c2 = self._dev(in2, torch.float32, "in2").value, int(in2.shape[1])
            if ss1 is not None:
                if tuple(ss1.shape) != (B, c1, 2):
                    raise ValueError(f"ss1: expected shape {(B, c1, 2)}, got {tuple(ss1.shape)}")
                a.ss1 = self._dev(ss1, torch.float32, "ss1").value
        if op == "folded":
            a.index = 16
        out2 = None
        if op == "norm":
            shape = (B, c1, D, H, W)
            if pool:
                out2 = torch.empty((B, c1, D // 2, H // 2, W // 2), dtype=torch.float32, device=self.device)
                a.out2 = self._dev(out2, torch.float32, "out2").value
            a.writeback, a.fmt_out = int(bool(writeback)), int(bool(seam))
        elif op == "final":
            shape = (B, D, H, W)
        elif kind == 1:
            if a.index < 0 or a.index >= len(DECONV_BLOCKS):
                raise ValueError("deconv index must be 0..3")
            cout = (self.features[4] // 2, self.features[3] // 2, self.features[2] // 2, self.features[1])[a.index]
            sk = (2 * D, 2 * H, 2 * W) if skip_shape is None else tuple(int(v) for v in skip_shape)
            if skip_shape is not None:
                a.sD, a.sH, a.sW = sk
            shape = (B, cout) + sk
        else:
            cout = self.features[self._BLOCK_COUT[a.index]] if op != "stem" else self.features[0]
            shape = (B, cout, 2) if kind == 3 else (B, cout, D, H, W)
        blend = acc is not None
        if blend:
            if op != "final":
                raise ValueError("acc: the blend mode belongs to op 'final'")
            st = np.ascontiguousarray(starts, dtype=np.intc)
            if st.shape != (B, 3) or acc.dim() != 3:
                raise ValueError(f"blend: starts (B, 3) and a (Z, Yp, Xp) accumulator expected, got {st.shape}, {tuple(acc.shape)}")
            if np.any(st[:, 0] + D > acc.shape[0]):  # (the hook checks the rest: it knows the Yp x Xp of a plane, not their number)
                raise ValueError("blend: a window leaves the accumulator's planes")
            a.starts = st.ctypes.data_as(C.POINTER(C.c_int))
            a.acc = self._dev(acc, torch.float32, "acc").value
            a.Yp, a.Xp, a.scale, a.bmin = int(acc.shape[1]), int(acc.shape[2]), float(scale), float(bmin)
            if bw is not None:
                if bw.numel() != D + H + W:
                    raise ValueError("blend: bw holds D + H + W factors")
                a.bw = self._dev(bw, torch.float32, "bw").value
            if wsum is not None:
                if wsum.shape != acc.shape:
                    raise ValueError("blend: wsum is shaped like acc")
                a.wsum = self._dev(wsum, torch.float32, "wsum").value
            out = None
        else:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
            a.out = self._dev(out, torch.float32, "out").value
        a.B, a.D, a.H, a.W = int(B), int(D), int(H), int(W)
        self._check(self.lib.dlv_debug_set_format(self.ctx, PREC_F16 if precision in ("fp16", "f16") else PREC_BF16_ALL))
        self._enter()
        self._check(self.lib.dlv_debug_layer16(self.ctx, C.byref(a)))
        self._leave()
        zr = a.ran_zreg
        nm = a.ran_norm
        report = {
            "zreg": None if not zr else "{}_c{}_t{}_{}".format("f16" if zr & 2 else "bf16", 64 if zr & 4 else 32, 16 if zr & 8 else 8,
                                                              ("adda1" if zr & 16 else "add") if zr & 32 else ("a1" if zr & 16 else "a0")),
            "upconv": {0: None, 1: "upconv2", 2: "upconv2m"}[a.ran_upconv],
            "stem": bool(a.ran_stem),
            "drops_bias": bool(a.drops_bias),
            "drops_fold_const": bool(a.drops_fold_const),
            "raw_scale": float(a.raw_scale),
            # what the launchers recorded: the conv family (a name of _lib.PLAN_CONV_KERNELS) with its template parameters, ...
            "conv": None if a.ran_conv < 0 else _lib.PLAN_CONV_KERNELS[a.ran_conv],
            "tx": a.ran_tx, "ncb": a.ran_ncb, "wlds": bool(a.ran_wlds), "grid": a.ran_grid, "items": a.ran_items,
            # ... the transposed-conv kernel (_lib.PLAN_DECONV_KERNELS), ...
            "deconv": None if a.ran_deconv < 0 else _lib.PLAN_DECONV_KERNELS[a.ran_deconv],
            "gpw": a.ran_gpw, "pad": bool(a.ran_pad),
            # ... and the last normalisation pass before the report was taken (None: none ran)
            "norm": None if not nm else {"rows": bool(nm & 2), "pooled": bool(nm & 4), "writeback": bool(nm & 8), "nt": bool(nm & 16),
                                         "seam": bool(nm & 32)},
            "norm_passes": a.ran_norm_passes,
        }
        if blend:
            return report
        if op == "norm" and pool:
            return out, out2, report
        return out, report

    # ---- sliding window ----------------------------------------------------------------------------
    def make_sw_params(self, padded_shape, roi, overlap=0.5, flip_dim=None, skip_threshold=0, precision="fp16",
                       sw_batch=0, win_range=None, slab=None, repeat=1, blend="constant", sigma_scale=0.125,
                       wsum=None) -> _lib.SwParams:
        p = _lib.SwParams()
        p.Zp, p.Yp, p.Xp = (int(v) for v in padded_shape)
        for k in range(3):
            p.roi[k] = int(roi[k])
        p.overlap = float(overlap)
        p.flip_dim = -1 if flip_dim is None else int(flip_dim)
        p.skip_threshold = int(skip_threshold)
        p.precision = PRECISIONS[precision]
        p.sw_batch = int(sw_batch)
        p.win_begin, p.win_end = (0, 0) if win_range is None else (int(win_range[0]), int(win_range[1]))
        p.z0, p.nz = (0, 0) if slab is None else (int(slab[0]), int(slab[1]))
        p.repeat = int(repeat)
        # "constant" is what the reference does (its mode="gaussian" argument is ignored); "gaussian" = MONAI's
        # importance map as an option, with `wsum` (fp32 tensor shaped like acc, optional) collecting the weight sums
        p.blend_mode = {"constant": 0, "gaussian": 1}[blend]
        p.sigma_scale = float(sigma_scale)
        if wsum is not None:
            if blend != "gaussian":
                raise ValueError("wsum is the float count map of the Gaussian blend")
            p.wsum_dev = self._dev(wsum, self.torch.float32, "wsum").value
            p._keep = wsum
        return p

    def num_windows(self, params) -> int:
        n = C.c_int64()
        rc = self.lib.dlv_sw_num_windows(C.byref(params), C.byref(n))
        if rc != 0:
            raise DelivrHipError(rc, "dlv_sw_num_windows: bad geometry")
        return n.value

    def window_starts(self, params) -> np.ndarray:
        n = self.num_windows(params)
        buf = np.zeros((n, 3), dtype=np.int64)
        rc = self.lib.dlv_sw_window_starts(C.byref(params), buf.ctypes.data_as(C.POINTER(C.c_int64)), n)
        if rc != 0:
            raise DelivrHipError(rc, "dlv_sw_window_starts failed")
        return buf

    def window_max(self, params, vol) -> np.ndarray:
        """Per-window maximum (int32, reference window order): windows with max <= skip_threshold are background."""
        n = self.num_windows(params)
        if params.win_end > 0 or params.win_begin > 0:  # a shard of the window list: out[i] = window win_begin + i
            n = max(min(int(params.win_end) if params.win_end > 0 else n, n) - max(int(params.win_begin), 0), 0)
        out = np.zeros(n, dtype=np.int32)
        if n == 0:
            return out
        self._enter()
        self._check(self.lib.dlv_sw_window_max_dev(self.ctx, C.byref(params), self._dev(vol, self.torch.uint16, "vol"),
                                                   out.ctypes.data_as(C.POINTER(C.c_int32)), n))
        self._leave()
        return out

    def reserve(self, params, stack_shape=None) -> None:
        """dlv_reserve_dev: allocate now what a pass with `params` (and the finalize of `stack_shape`) will ask for.  Meant for a
        second thread while the volume is read; the engine must not be used by another thread meanwhile."""
        Z, Y, X = (int(v) for v in stack_shape) if stack_shape is not None else (0, 0, 0)
        self._check(self.lib.dlv_reserve_dev(self.ctx, C.byref(params), Z, Y, X))

    def sw_infer(self, params, vol, acc, cnt=None) -> dict:
        """One sliding-window pass; vol uint16 (nz,Yp,Xp), acc fp32 and cnt uint8 (optional) are
        mutated in place (inference/sliding_window_inferer.py:232-251)."""
        torch = self.torch
        st = _lib.SwStats()
        self._enter()
        self._check(self.lib.dlv_sw_infer_dev(
            self.ctx, C.byref(params), self._dev(vol, torch.uint16, "vol"), self._dev(acc, torch.float32, "acc"),
            self._dev(cnt, torch.uint8, "cnt") if cnt is not None else None, C.byref(st)))
        self._leave()
        return {"n_windows": st.n_windows, "n_skipped": st.n_skipped, "n_forward_launches": st.n_forward_launches}

    # ---- finalize ----------------------------------------------------------------------------------
    def finalize(self, acc, cnt, raw, stack_shape, threshold=0.5, erode_iters=30, zblock=0, want_prob=False, out=None):
        """-> uint8 (Z,Y,X) binaries [, fp32 sigmoid] (inference/inference.py:285-299, :31-95).  `out`: a uint8 (Z,Y,X) tensor to
        write the mask into (allocated ahead of the passes)."""
        torch = self.torch
        Z, Y, X = (int(v) for v in stack_shape)
        Yp, Xp = int(acc.shape[-2]), int(acc.shape[-1])
        if cnt is not None and cnt.dtype == torch.float32:
            # Gaussian blend: the count map holds weight sums; the mean logit is formed here, the kernel sees no count
            acc = acc / cnt.clamp_min(torch.finfo(torch.float32).tiny)
            cnt = None
        if out is None:
            out = torch.empty((Z, Y, X), dtype=torch.uint8, device=self.device)
        elif tuple(out.shape) != (Z, Y, X):
            raise ValueError(f"finalize: out has shape {tuple(out.shape)}, the stack {(Z, Y, X)}")
        prob = torch.empty((Z, Y, X), dtype=torch.float32, device=self.device) if want_prob else None
        self._enter()
        self._check(self.lib.dlv_finalize_dev(
            self.ctx, self._dev(acc, torch.float32, "acc"),
            self._dev(cnt, torch.uint8, "cnt") if cnt is not None else None, self._dev(raw, torch.uint16, "raw"),
            Yp, Xp, Z, Y, X, float(threshold), int(erode_iters), int(zblock),
            self._dev(out, torch.uint8, "out"), self._dev(prob, torch.float32, "prob") if want_prob else None))
        self._leave()
        return (out, prob) if want_prob else out

    def finalize_slab(self, acc, cnt, raw, z_abs0: int, stack_yx, threshold=0.5, erode_iters=30, zblock=0, want_prob=False):
        """finalize on a Z-slab: acc / cnt / raw hold planes [z_abs0, z_abs0 + nz) (nz = acc.shape[0]); the erosion's z-blocks
        sit at absolute multiples of zblock (dlv_finalize_slab_dev).  -> uint8 (nz, Y, X) [, fp32 sigmoid]."""
        torch = self.torch
        nz = int(acc.shape[0])
        Y, X = (int(v) for v in stack_yx)
        Yp, Xp = int(acc.shape[-2]), int(acc.shape[-1])
        if cnt is not None and cnt.dtype == torch.float32:
            acc = acc / cnt.clamp_min(torch.finfo(torch.float32).tiny)
            cnt = None
        out = torch.empty((nz, Y, X), dtype=torch.uint8, device=self.device)
        prob = torch.empty((nz, Y, X), dtype=torch.float32, device=self.device) if want_prob else None
        self._enter()
        self._check(self.lib.dlv_finalize_slab_dev(
            self.ctx, self._dev(acc, torch.float32, "acc"), self._dev(cnt, torch.uint8, "cnt") if cnt is not None else None,
            self._dev(raw, torch.uint16, "raw"), Yp, Xp, int(z_abs0), nz, Y, X, float(threshold), int(erode_iters), int(zblock),
            self._dev(out, torch.uint8, "out"), self._dev(prob, torch.float32, "prob") if want_prob else None))
        self._leave()
        return (out, prob) if want_prob else out

    def finalize_ran(self) -> dict:
        """what the last finalize / finalize_slab of this context launched (include/delivr_hip_diag.h: dlv_finalize_ran) - tests"""
        out = _lib.FinalizeRan()
        self._check(self.lib.dlv_diag_finalize_ran(self.ctx, C.byref(out)))
        return {name: int(getattr(out, name)) for name, _ in out._fields_}

    # ---- connected components ----------------------------------------------------------------------
    def ccl26(self, mask):
        """uint8 (Z,Y,X) in HBM -> (labels uint32 tensor in HBM (stored in an int32 tensor), N)."""
        torch = self.torch
        Z, Y, X = (int(v) for v in mask.shape)
        labels = torch.empty((Z, Y, X), dtype=torch.int32, device=self.device)  # uint32 payload
        n = C.c_uint64()
        self._enter()
        self._check(self.lib.dlv_ccl26_dev(self.ctx, self._dev(mask, torch.uint8, "mask"), Z, Y, X,
                                           C.c_void_p(labels.data_ptr()), C.byref(n)))
        self._leave()
        return labels, int(n.value)

    def _byte_volume(self, what: str, mask):
        """the tensor checks of a uint8 (Z,Y,X) mask in HBM -> (Z, Y, X)"""
        torch = self.torch
        if not isinstance(mask, torch.Tensor) or mask.device != self.device:
            raise ValueError(f"{what}: mask: expected a torch tensor on {self.device}, got {type(mask).__name__} on "
                             f"{getattr(mask, 'device', None)}")
        if mask.dtype != torch.uint8 or mask.dim() != 3 or not mask.is_contiguous() or mask.numel() == 0:
            raise ValueError(f"{what}: mask: expected a contiguous, non-empty 3-D uint8 tensor, got {mask.dtype} of shape "
                             f"{tuple(mask.shape)}")
        return tuple(int(v) for v in mask.shape)

    def fill_holes(self, mask, fill_value: int = 2):
        """Exact hole filling of a uint8 (Z,Y,X) mask in HBM, in place (dlv_fill_holes_u8_dev): every voxel of every background
        component that reaches no face of the volume (6-connected; scipy.ndimage.binary_fill_holes(mask != 0)) becomes fill_value,
        no other byte is written.  The mask must not hold fill_value already.  -> (voxels_filled, holes)."""
        Z, Y, X = self._byte_volume("fill_holes", mask)
        if isinstance(fill_value, bool) or not isinstance(fill_value, (int, np.integer)) or not 1 <= int(fill_value) <= 255:
            raise ValueError(f"fill_holes: fill_value = {fill_value!r}: expected an integer 1..255")
        voxels, holes = C.c_uint64(), C.c_uint64()
        self._enter()
        try:
            self._check(self.lib.dlv_fill_holes_u8_dev(self.ctx, C.c_void_p(mask.data_ptr()), Z, Y, X, int(fill_value), C.byref(voxels),
                                                       C.byref(holes)))
        finally:
            self._leave()
        return int(voxels.value), int(holes.value)

    def cc_count_marked(self, labels, mask, n: int, value: int):
        """Per label 0..n the voxels whose mask byte equals `value` (dlv_cc_count_marked_dev): on the labels of a filled mask, the
        voxels fill_holes gave each component.  labels: int32 (uint32 payload) (Z,Y,X) in HBM, mask: uint8 of the same shape.
        -> int32 tensor (uint32 payload) of n+1 in HBM, like cc_counts."""
        torch = self.torch
        shape = self._label_volume("cc_count_marked", labels)
        if self._byte_volume("cc_count_marked", mask) != shape:
            raise ValueError(f"cc_count_marked: mask of shape {tuple(mask.shape)}, the labels are {shape}")
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= 255:
            raise ValueError(f"cc_count_marked: value = {value!r}: expected an integer 0..255")
        n = int(n)
        if n < 0:
            raise ValueError(f"cc_count_marked: n = {n}")
        counts = torch.empty(n + 1, dtype=torch.int32, device=self.device)
        self._enter()
        try:
            self._check(self.lib.dlv_cc_count_marked_dev(self.ctx, C.c_void_p(labels.data_ptr()), C.c_void_p(mask.data_ptr()),
                                                         int(labels.numel()), n, int(value), C.c_void_p(counts.data_ptr())))
        finally:
            self._leave()
        return counts

    def ccl_ran(self) -> dict:
        """what the last dlv_ccl26_dev of this context launched (include/delivr_hip_diag.h: dlv_ccl_ran) - tests"""
        out = _lib.CclRan()
        self._check(self.lib.dlv_diag_ccl_ran(self.ctx, C.byref(out)))
        return {name: int(getattr(out, name)) for name, _ in out._fields_}

    def cc_stats(self, labels, n: int) -> dict:
        """cc3d.statistics(no_slice_conversion=True) layout (count_blobs.py:85)."""
        Z, Y, X = (int(v) for v in labels.shape)
        counts = np.zeros(n + 1, dtype=np.uint32)
        bbox = np.zeros((n + 1, 6), dtype=np.uint16)
        cent = np.zeros((n + 1, 3), dtype=np.float64)
        self._enter()
        self._check(self.lib.dlv_cc_stats_dev(self.ctx, C.c_void_p(labels.data_ptr()), Z, Y, X, n,
                                              counts.ctypes.data_as(C.c_void_p), bbox.ctypes.data_as(C.c_void_p),
                                              cent.ctypes.data_as(C.c_void_p)))
        self._leave()
        return {"voxel_counts": counts, "bounding_boxes": bbox, "centroids": cent}

    def cc_stats_raw(self, labels, n: int) -> dict:
        """Accumulators behind cc_stats (dlv_cc_stats_raw_dev): counts u32, bbmin/bbmax u32 (n+1,3), sums u64 (n+1,3)."""
        Z, Y, X = (int(v) for v in labels.shape)
        counts = np.zeros(n + 1, dtype=np.uint32)
        bbmin = np.zeros((n + 1, 3), dtype=np.uint32)
        bbmax = np.zeros((n + 1, 3), dtype=np.uint32)
        sums = np.zeros((n + 1, 3), dtype=np.uint64)
        self._enter()
        self._check(self.lib.dlv_cc_stats_raw_dev(self.ctx, C.c_void_p(labels.data_ptr()), Z, Y, X, n,
                                                  counts.ctypes.data_as(C.c_void_p), bbmin.ctypes.data_as(C.c_void_p),
                                                  bbmax.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p)))
        self._leave()
        return {"counts": counts, "bbmin": bbmin, "bbmax": bbmax, "sums": sums}

    def seam_pairs(self, plane_a, plane_b) -> np.ndarray:
        """Unique (label in plane_a, label in plane_b) pairs that are 26-adjacent across a slab seam; (k,2) uint32,
        sorted (dlv_seam_pairs_dev: count pass, then emit pass)."""
        torch = self.torch
        Y, X = (int(v) for v in plane_a.shape)
        a = self._dev(plane_a, torch.int32, "plane_a")
        b = self._dev(plane_b, torch.int32, "plane_b")
        cnt = C.c_uint64()
        self._enter()
        self._check(self.lib.dlv_seam_pairs_dev(self.ctx, a, b, Y, X, None, 0, C.byref(cnt)))
        k = int(cnt.value)
        if k == 0:
            self._leave()
            return np.zeros((0, 2), dtype=np.uint32)
        pairs = torch.empty((k, 2), dtype=torch.int32, device=self.device)
        self._check(self.lib.dlv_seam_pairs_dev(self.ctx, a, b, Y, X, C.c_void_p(pairs.data_ptr()), k, C.byref(cnt)))
        self._leave()
        assert int(cnt.value) == k
        return np.unique(pairs.cpu().numpy().view(np.uint32), axis=0)

    def relabel(self, labels, lut: np.ndarray) -> None:
        """labels[i] = lut[labels[i]] in place (dlv_relabel_u32_dev); lut: uint32 (n_local+1,), lut[0] = 0."""
        torch = self.torch
        lut_dev = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.uint32).view(np.int32)).to(self.device)
        self._enter()
        self._check(self.lib.dlv_relabel_u32_dev(self.ctx, C.c_void_p(labels.data_ptr()), int(labels.numel()),
                                                 C.c_void_p(lut_dev.data_ptr()), int(lut_dev.numel())))
        self._leave()
        self.sync()

    def cc_counts(self, labels, n: int):
        """Voxels per label 0..n of a label volume in HBM (dlv_cc_counts_dev) -> int32 tensor (uint32 payload) of n+1 in HBM."""
        torch = self.torch
        ptr = self._dev(labels, torch.int32, "labels")
        counts = torch.empty(int(n) + 1, dtype=torch.int32, device=self.device)
        self._enter()
        self._check(self.lib.dlv_cc_counts_dev(self.ctx, ptr, int(labels.numel()), int(n), C.c_void_p(counts.data_ptr())))
        self._leave()
        return counts

    def cc_size_filter(self, labels, n: int, min_size: int, max_size: int, counts=None) -> int:
        """Size filter in place (dlv_cc_size_filter_dev): labels with min_size <= voxels <= max_size (inclusive, negative = no
        bound) are renumbered 1..K in their order, the others become 0 -> K.  counts: the voxel counts of the labels 0..n when they
        are not those of `labels` alone (a slab of a sharded run passes the sums over all slabs); a device tensor or an array."""
        torch = self.torch
        lo, hi = int(min_size), int(max_size)
        if lo >= 0 and hi >= 0 and lo > hi:
            raise ValueError(f"size filter: min_size {lo} > max_size {hi}")
        ptr = self._dev(labels, torch.int32, "labels")
        if lo < 0 and hi < 0:
            return int(n)
        if counts is None:
            counts = self.cc_counts(labels, n)
        elif not isinstance(counts, torch.Tensor):
            counts = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32)).to(self.device)
        if counts.device != self.device or counts.dtype != torch.int32 or not counts.is_contiguous() or counts.numel() != int(n) + 1:
            raise ValueError(f"counts: expected {int(n) + 1} contiguous int32 values (uint32 payload) on {self.device}")
        kept = C.c_uint64()
        self._enter()
        self._check(self.lib.dlv_cc_size_filter_dev(self.ctx, ptr, int(labels.numel()), int(n), C.c_void_p(counts.data_ptr()),
                                                    lo, hi, C.byref(kept)))
        self._leave()
        return int(kept.value)

    def _label_volume(self, what: str, labels, *raw):
        """the tensor checks of a label volume in HBM, and of the raw volume(s) given beside it -> (Z, Y, X)"""
        torch = self.torch
        for name, t, dtypes in (("labels", labels, (torch.int32,)),) + tuple(("raw", r, (torch.uint16, torch.int16)) for r in raw):
            if not isinstance(t, torch.Tensor) or t.device != self.device:
                raise ValueError(f"{what}: {name}: expected a torch tensor on {self.device}, got {type(t).__name__} on "
                                 f"{getattr(t, 'device', None)}")
            if t.dtype not in dtypes or t.dim() != 3:
                raise ValueError(f"{what}: {name}: expected a 3-D tensor of {' / '.join(str(d) for d in dtypes)}, got "
                                 f"{t.dim()}-D {t.dtype}")
        if not labels.is_contiguous() or labels.numel() == 0:
            raise ValueError(f"{what}: labels of shape {tuple(labels.shape)} must be contiguous and not empty")
        return tuple(int(v) for v in labels.shape)

    @staticmethod
    def _raw_pitches(what: str, raw, shape):
        """the raw volume (a tensor: _label_volume checked) holds a label volume of `shape` -> (pitch_y, pitch_z)"""
        Z, Y, X = shape
        if any(r < v for r, v in zip(raw.shape, (Z, Y, X))):
            raise ValueError(f"{what}: raw of shape {tuple(raw.shape)} is smaller than the labels {(Z, Y, X)}")
        pitch_z, pitch_y, pitch_x = (int(s) for s in raw.stride())
        if pitch_x != 1 or pitch_y < X or pitch_z < Y * pitch_y:
            raise ValueError(f"{what}: raw with strides {tuple(raw.stride())} is not a (padded) volume with a contiguous last axis")
        return pitch_y, pitch_z

    def _labels_under_raw(self, what: str, labels, raw, n):
        """the checks cc_intensity and cc_quantiles share -> (Z, Y, X, pitch_y, pitch_z, n)"""
        Z, Y, X = self._label_volume(what, labels, raw)
        pitch_y, pitch_z = self._raw_pitches(what, raw, (Z, Y, X))
        n = int(n)
        if n < 0:
            raise ValueError(f"{what}: n = {n}")
        return Z, Y, X, pitch_y, pitch_z, n

    def cc_quantiles(self, labels, raw, n: int, levels=(25, 50, 75)):
        """Per-label order statistics of the raw volume under a label volume (dlv_cc_quantiles_dev).  labels, raw: as for
        cc_intensity.  levels: 1..8 integers 0..100 in per cent, strictly increasing; with a label's m raw values sorted ascending,
        level p reads v[(p * (m - 1)) // 100] - the lower quantile, a value the label holds (50: the lower median, 0 / 100: minimum /
        maximum).  -> (uint16 array (n+1, len(levels)), uint32 array (n+1,) of the voxels measured per label); row 0 and a label
        without a voxel read 0 with a count of 0."""
        Z, Y, X, pitch_y, pitch_z, n = self._labels_under_raw("cc_quantiles", labels, raw, n)
        levels = list(levels)
        if (not 1 <= len(levels) <= 8 or any(isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 0 <= int(p) <= 100 for p in levels)
                or any(int(b) <= int(a) for a, b in zip(levels, levels[1:]))):
            raise ValueError(f"cc_quantiles: levels = {levels!r}: expected 1..8 integers 0..100, strictly increasing")
        values = np.zeros((n + 1, len(levels)), dtype=np.uint16)
        counts = np.zeros(n + 1, dtype=np.uint32)
        self._enter()
        self._check(self.lib.dlv_cc_quantiles_dev(self.ctx, C.c_void_p(labels.data_ptr()), C.c_void_p(raw.data_ptr()), Z, Y, X,
                                                  pitch_y, pitch_z, n, len(levels), (C.c_int * len(levels))(*(int(p) for p in levels)),
                                                  values.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)))
        self._leave()
        return values, counts

    def cc_intensity(self, labels, raw, n: int) -> dict:
        """Per-label statistics of the raw volume under a label volume (dlv_cc_intensity_dev).  labels: int32 (uint32 payload)
        (Z,Y,X) in HBM; raw: uint16 (or int16-viewed) (Zr,Yr,Xr) in HBM with Zr >= Z, Yr >= Y, Xr >= X, contiguous in its last
        axis - voxel (z,y,x) of the labels is raw[z,y,x], the pitches come from raw's strides (the padded network input, or a view
        into it).  -> {"intensity_sum", "intensity_sumsq": uint64, "intensity_min", "intensity_max": uint16}, n+1 rows each; a label
        without a voxel - and row 0 - reads 0, 0, 0xFFFF, 0."""
        Z, Y, X, pitch_y, pitch_z, n = self._labels_under_raw("cc_intensity", labels, raw, n)
        out = {"intensity_sum": np.zeros(n + 1, dtype=np.uint64), "intensity_sumsq": np.zeros(n + 1, dtype=np.uint64),
               "intensity_min": np.zeros(n + 1, dtype=np.uint16), "intensity_max": np.zeros(n + 1, dtype=np.uint16)}
        self._enter()
        self._check(self.lib.dlv_cc_intensity_dev(self.ctx, C.c_void_p(labels.data_ptr()), C.c_void_p(raw.data_ptr()), Z, Y, X,
                                                  pitch_y, pitch_z, n, *(a.ctypes.data_as(C.c_void_p) for a in out.values())))
        self._leave()
        return out

    def cc_confidence(self, labels, prob, n: int) -> dict:
        """Per-label statistics of the network's probabilities under a label volume (dlv_cc_confidence_dev).  labels: int32
        (uint32 payload) (Z,Y,X) in HBM; prob: float32 of the same shape in HBM, contiguous (the volume finalize leaves in its
        prob tensor, network_output.npy).  Every probability is taken as q = rint(clamp(p, 0, 1) * 2^24) (NaN: 0).  ->
        {"confidence_sum": uint64, "confidence_min_q", "confidence_max_q": uint32, "confidence_peak_index": uint64}, n+1 rows each;
        the peak is the linear index in this volume of the voxel of largest q, the first in raster order on a tie.  A label without
        a voxel - and row 0 - reads 0, 0xFFFFFFFF, 0 and 2^64 - 1."""
        torch = self.torch
        Z, Y, X = self._label_volume("cc_confidence", labels)
        if not isinstance(prob, torch.Tensor) or prob.device != self.device:
            raise ValueError(f"cc_confidence: prob: expected a torch tensor on {self.device}, got {type(prob).__name__} on "
                             f"{getattr(prob, 'device', None)}")
        if prob.dtype != torch.float32 or tuple(prob.shape) != (Z, Y, X) or not prob.is_contiguous():
            raise ValueError(f"cc_confidence: prob: expected a contiguous float32 tensor of the labels' shape {(Z, Y, X)}, got "
                             f"{prob.dtype} of shape {tuple(prob.shape)}")
        n = int(n)
        if n < 0:
            raise ValueError(f"cc_confidence: n = {n}")
        out = {"confidence_sum": np.zeros(n + 1, dtype=np.uint64), "confidence_min_q": np.zeros(n + 1, dtype=np.uint32),
               "confidence_max_q": np.zeros(n + 1, dtype=np.uint32), "confidence_peak_index": np.zeros(n + 1, dtype=np.uint64)}
        self._enter()
        self._check(self.lib.dlv_cc_confidence_dev(self.ctx, C.c_void_p(labels.data_ptr()), C.c_void_p(prob.data_ptr()), Z, Y, X, n,
                                                   *(a.ctypes.data_as(C.c_void_p) for a in out.values())))
        self._leave()
        return out

    def cc_shell(self, labels, radius: int, raw=None):
        """The background shell of every component (dlv_cc_shell_dev): the labels are expanded into the background by `radius`
        (1..16) synchronous steps of a 26-neighbourhood minimum - a voxel goes to the smallest label among the cells nearest to
        it in Chebyshev distance - and the expanded voxels that are background in `labels` and not 0 in `raw` are the shell.
        labels, raw: as for cc_intensity; raw None: no raw condition (labels + shell are then the expanded labels).  -> int32
        tensor (uint32 payload) of the labels' shape in HBM; cc_intensity / cc_counts on it measure the shells.  Needs one more
        volume of that size while it runs when radius > 1."""
        torch = self.torch
        Z, Y, X = self._label_volume("cc_shell", labels, *(() if raw is None else (raw,)))
        pitch_y, pitch_z = (0, 0) if raw is None else self._raw_pitches("cc_shell", raw, (Z, Y, X))
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= 16:
            raise ValueError(f"cc_shell: radius = {radius!r}: expected an integer 1..16")
        radius = int(radius)
        shell = torch.empty((Z, Y, X), dtype=torch.int32, device=self.device)
        scratch = torch.empty((Z, Y, X), dtype=torch.int32, device=self.device) if radius > 1 else None
        self._enter()
        self._check(self.lib.dlv_cc_shell_dev(self.ctx, C.c_void_p(labels.data_ptr()), C.c_void_p(raw.data_ptr()) if raw is not None else None,
                                              Z, Y, X, pitch_y, pitch_z, radius, C.c_void_p(shell.data_ptr()),
                                              C.c_void_p(scratch.data_ptr()) if scratch is not None else None))
        self._leave()  # (torch's stream now waits for the sweeps: the scratch volume freed here is not reused before them)
        return shell

    def cc_shape(self, labels, n: int, keep=None, z_abs0: int = 0) -> dict:
        """Per-label shape accumulators of a label volume (dlv_cc_shape_dev).  labels: int32 (uint32 payload) (Zb,Y,X) in HBM,
        contiguous.  keep: (first, planes) - the planes of `labels` that are measured (default: all); the others only serve as
        neighbours (a slab extended by its neighbours' planes).  z_abs0: the absolute z of the buffer's first plane.
        -> {"shape_counts": uint32 (n+1), "shape_sums": uint64 (n+1,3) = sum z, y, x, "shape_moments": uint64 (n+1,6) = sum zz,
        yy, xx, zy, zx, yx, "shape_faces": uint64 (n+1,3) = exposed faces per axis z, y, x, "shape_surface_voxels": uint32 (n+1)};
        row 0 and a label without a measured voxel are all zero, so slabs add up (hostlogic.merge_shape)."""
        Z, Y, X = self._label_volume("cc_shape", labels)
        first, planes = (0, Z) if keep is None else (int(keep[0]), int(keep[1]))
        if first < 0 or planes < 1 or first + planes > Z:
            raise ValueError(f"cc_shape: keep = {keep!r} does not select planes of the {Z} in the buffer")
        n, z_abs0 = int(n), int(z_abs0)
        if n < 0 or z_abs0 < 0:
            raise ValueError(f"cc_shape: n = {n}, z_abs0 = {z_abs0}")
        out = {"shape_counts": np.zeros(n + 1, dtype=np.uint32), "shape_sums": np.zeros((n + 1, 3), dtype=np.uint64),
               "shape_moments": np.zeros((n + 1, 6), dtype=np.uint64), "shape_faces": np.zeros((n + 1, 3), dtype=np.uint64),
               "shape_surface_voxels": np.zeros(n + 1, dtype=np.uint32)}
        self._enter()
        self._check(self.lib.dlv_cc_shape_dev(self.ctx, C.c_void_p(labels.data_ptr()), Z, Y, X, first, planes, z_abs0, n,
                                              *(a.ctypes.data_as(C.c_void_p) for a in out.values())))
        self._leave()
        return out

    def cc_depth(self, labels, n: int, spacing=(1, 1, 1), return_map: bool = False) -> dict:
        """Per-label depth from the exact label-wise Euclidean distance map (dlv_cc_depth_dev).  labels: int32 (uint32 payload)
        (Z,Y,X) in HBM, contiguous, not modified.  spacing: (wz, wy, wx), integers 1..64.  D2 of a voxel of a label 1..n is its
        squared distance, in spacing units, to the nearest voxel of another label, the outside of the volume counting as
        background; 0 elsewhere.  -> {"depth_max_sq": uint32, "depth_sum_sq": uint64, "depth_peak_index": uint64}, n+1 rows each:
        the largest D2 of the label, the sum over its voxels, and the linear index of the voxel that holds the largest, the first
        in raster order on a tie.  Row 0 and a label without a voxel read 0, 0 and 2^64 - 1.  return_map: the dict also holds
        "depth_map", the D2 volume in HBM (int32 tensor, uint32 payload).  Needs two more volumes of the labels' size while it
        runs; the one that is not returned is freed."""
        torch = self.torch
        Z, Y, X = self._label_volume("cc_depth", labels)
        spacing = tuple(spacing) if isinstance(spacing, (tuple, list)) else (spacing,)
        if len(spacing) != 3 or any(isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 1 <= int(w) <= 64 for w in spacing):
            raise ValueError(f"cc_depth: spacing = {spacing!r}: expected three integers 1..64 (wz, wy, wx)")
        n = int(n)
        if n < 0:
            raise ValueError(f"cc_depth: n = {n}")
        work_a = torch.empty((Z, Y, X), dtype=torch.int32, device=self.device)
        work_b = torch.empty((Z, Y, X), dtype=torch.int32, device=self.device)
        out = {"depth_max_sq": np.zeros(n + 1, dtype=np.uint32), "depth_sum_sq": np.zeros(n + 1, dtype=np.uint64),
               "depth_peak_index": np.zeros(n + 1, dtype=np.uint64)}
        self._enter()
        try:
            self._check(self.lib.dlv_cc_depth_dev(self.ctx, C.c_void_p(labels.data_ptr()), Z, Y, X, n, *(int(w) for w in spacing),
                                                  C.c_void_p(work_a.data_ptr()), C.c_void_p(work_b.data_ptr()),
                                                  *(a.ctypes.data_as(C.c_void_p) for a in out.values())))
        finally:
            self._leave()
        if return_map:
            out["depth_map"] = work_a
        return out

    def cc_split(self, labels, n: int, depth: int, min_core: int = 1):
        """Fused cells split by their erosion cores, in place (dlv_cc_split_dev).  labels: int32 (uint32 payload) (Z,Y,X) in HBM,
        contiguous, labels 0..n.  The labels are eroded `depth` (1..16) times with the 6 face neighbours; what is left are the
        cores (26-connected; those of fewer than `min_core` voxels are dropped).  A label with two or more cores is divided among
        them: every voxel goes to the core nearest to it in 26-steps through its own label, to the smallest core label on a tie.
        The pieces and the labels that stay whole are renumbered 1..K in raster order of their first voxel, as ccl26 numbers.
        -> (K, parent: uint32 ndarray of K+1 with parent[j] = the old label of piece j and parent[0] = 0, the number of labels
        that were split).  Needs two more volumes of the labels' size while it runs."""
        Z, Y, X = self._label_volume("cc_split", labels)
        if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 1 <= int(depth) <= 16:
            raise ValueError(f"cc_split: depth = {depth!r}: expected an integer 1..16")
        if isinstance(min_core, bool) or not isinstance(min_core, (int, np.integer)) or int(min_core) < 1:
            raise ValueError(f"cc_split: min_core = {min_core!r}: expected an integer >= 1")
        n = int(n)
        if n < 0:
            raise ValueError(f"cc_split: n = {n}")
        return self._split_call(labels, n, lambda *tail: self.lib.dlv_cc_split_dev(
            self.ctx, C.c_void_p(labels.data_ptr()), Z, Y, X, n, int(depth), int(min_core), *tail))

    def _split_call(self, labels, n: int, entry):
        """The call of cc_split / cc_split_depth: entry(work_a, work_b, &K, &n_split, parent, cap) -> rc is the library's entry with
        its leading arguments bound.  The parent table starts at 2 n + 2 rows; an entry that finds it too small reports K and leaves
        the labels untouched, and is called once more with K + 1 rows."""
        torch = self.torch
        work_a = torch.empty(tuple(labels.shape), dtype=torch.int32, device=self.device)
        work_b = torch.empty(tuple(labels.shape), dtype=torch.int32, device=self.device)
        k, n_split = C.c_uint64(), C.c_uint64()
        cap = 2 * n + 2
        self._enter()
        try:
            for attempt in (0, 1):
                parent = torch.empty(cap, dtype=torch.int32, device=self.device)
                k.value = 0
                rc = entry(C.c_void_p(work_a.data_ptr()), C.c_void_p(work_b.data_ptr()), C.byref(k), C.byref(n_split),
                           C.c_void_p(parent.data_ptr()), cap)
                if rc != 0 and attempt == 0 and int(k.value) + 1 > cap:  # (the table was too small: K is known now, the labels untouched)
                    cap = int(k.value) + 1
                    continue
                self._check(rc)
                break
        finally:
            self._leave()
        K = int(k.value)
        return K, parent[:K + 1].cpu().numpy().view(np.uint32), int(n_split.value)

    def cc_split_depth(self, labels, n: int, spacing, core_d2: int = 0, fraction: int = 0, min_core: int = 1):
        """Fused cells split by their Euclidean depth cores, in place (dlv_cc_split_depth_dev): cc_split for stacks whose voxels
        are not cubes.  labels: int32 (uint32 payload) (Z,Y,X) in HBM, contiguous, labels 0..n, no two different labels
        26-adjacent (what ccl26, fill_holes and cc_size_filter give).  spacing: (wz, wy, wx), integers 1..64.  With D2 the exact
        squared distance of a voxel to the outside of its label in spacing units (cc_depth) and m(l) the largest D2 of label l,
        the cores are the voxels with D2 >= max(core_d2, ceil(fraction^2 * m(l) / 10000), 1): at least sqrt(core_d2) from the
        outside, and at least `fraction` (0..99) per cent of the cell's inscribed radius; one of the two must be above 0.  From
        there on as cc_split: cores 26-connected, those of fewer than `min_core` voxels dropped, a label with two or more cores
        divided among them, all renumbered 1..K in raster order of their first voxel.  -> (K, parent: uint32 ndarray of K+1, the
        number of labels that were split).  Needs two more volumes of the labels' size while it runs."""
        Z, Y, X = self._label_volume("cc_split_depth", labels)
        spacing = tuple(spacing) if isinstance(spacing, (tuple, list)) else (spacing,)
        if len(spacing) != 3 or any(isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 1 <= int(w) <= 64 for w in spacing):
            raise ValueError(f"cc_split_depth: spacing = {spacing!r}: expected three integers 1..64 (wz, wy, wx)")
        if isinstance(core_d2, bool) or not isinstance(core_d2, (int, np.integer)) or not 0 <= int(core_d2) <= 2**32 - 1:
            raise ValueError(f"cc_split_depth: core_d2 = {core_d2!r}: expected an integer 0..2^32 - 1")
        if isinstance(fraction, bool) or not isinstance(fraction, (int, np.integer)) or not 0 <= int(fraction) <= 99:
            raise ValueError(f"cc_split_depth: fraction = {fraction!r}: expected an integer 0..99")
        if int(core_d2) == 0 and int(fraction) == 0:
            raise ValueError("cc_split_depth: core_d2 and fraction are both 0: no core is defined")
        if isinstance(min_core, bool) or not isinstance(min_core, (int, np.integer)) or int(min_core) < 1:
            raise ValueError(f"cc_split_depth: min_core = {min_core!r}: expected an integer >= 1")
        n = int(n)
        if n < 0:
            raise ValueError(f"cc_split_depth: n = {n}")
        return self._split_call(labels, n, lambda *tail: self.lib.dlv_cc_split_depth_dev(
            self.ctx, C.c_void_p(labels.data_ptr()), Z, Y, X, n, *(int(w) for w in spacing), int(core_d2), int(fraction), int(min_core), *tail))

    def cc_runs_encode(self, labels) -> dict:
        """The run-length coding of a label volume in HBM (dlv_cc_runs_count_dev, dlv_cc_runs_emit_dev; the format and the numpy
        reference: label_runs.py).  labels: int32 (uint32 payload) (Z,Y,X) in HBM, contiguous, X <= 65536.  -> {"row_start": uint64
        (Z*Y + 1), "x0", "x1": uint16 (R), "label": uint32 (R), "shape": (Z, Y, X)} on the host - label_runs.encode_runs' dict."""
        torch = self.torch
        Z, Y, X = self._label_volume("cc_runs_encode", labels)
        row_start = torch.empty(Z * Y + 1, dtype=torch.int64, device=self.device)  # uint64 payload
        n_runs = C.c_uint64()
        self._enter()
        try:
            self._check(self.lib.dlv_cc_runs_count_dev(self.ctx, C.c_void_p(labels.data_ptr()), Z, Y, X, C.c_void_p(row_start.data_ptr()),
                                                       C.byref(n_runs)))
            R = int(n_runs.value)
            x0 = torch.empty(R, dtype=torch.int16, device=self.device)
            x1 = torch.empty(R, dtype=torch.int16, device=self.device)
            label = torch.empty(R, dtype=torch.int32, device=self.device)
            self._check(self.lib.dlv_cc_runs_emit_dev(self.ctx, C.c_void_p(labels.data_ptr()), Z, Y, X, C.c_void_p(row_start.data_ptr()), R,
                                                      *(C.c_void_p(t.data_ptr()) if R else None for t in (x0, x1, label))))
        finally:
            self._leave()
        return {"row_start": row_start.cpu().numpy().view(np.uint64), "x0": x0.cpu().numpy().view(np.uint16),
                "x1": x1.cpu().numpy().view(np.uint16), "label": label.cpu().numpy().view(np.uint32), "shape": (Z, Y, X)}

    def cc_runs_decode(self, runs: dict, z0: int = 0, z1: Optional[int] = None, out=None):
        """The planes [z0, z1) of the label volume a run-length coding holds, decoded into HBM (dlv_cc_runs_decode_dev).  runs: the
        dict of cc_runs_encode / label_runs.load_runs (validated there: the kernel clamps what it reads, it does not judge it).
        Only the rows' slice of row_start and their runs are uploaded.  out: an int32 tensor (z1 - z0, Y, X) in HBM to decode into
        (it need not be cleared).  -> int32 tensor (uint32 payload) (z1 - z0, Y, X), every voxel written."""
        torch = self.torch
        Z, Y, X = (int(v) for v in runs["shape"])
        z0, z1 = int(z0), Z if z1 is None else int(z1)
        if not 0 <= z0 < z1 <= Z:
            raise ValueError(f"cc_runs_decode: planes [{z0}, {z1}) do not lie in the {Z} planes of the coding")
        rs = np.ascontiguousarray(runs["row_start"][z0 * Y:z1 * Y + 1], dtype=np.uint64)
        a, b = int(rs[0]), int(rs[-1])
        if len(rs) != (z1 - z0) * Y + 1 or not a <= b <= min(len(runs[k]) for k in ("x0", "x1", "label")):
            raise ValueError("cc_runs_decode: row_start does not match the shape and the run arrays")

        def dev(arr, np_dtype, as_int):  # (unsigned payloads in torch's signed types)
            return torch.from_numpy(np.ascontiguousarray(arr, dtype=np_dtype).view(as_int)).to(self.device)

        rs_dev = dev(rs, np.uint64, np.int64)
        x0, x1 = dev(runs["x0"][a:b], np.uint16, np.int16), dev(runs["x1"][a:b], np.uint16, np.int16)
        label = dev(runs["label"][a:b], np.uint32, np.int32)
        if out is None:
            out = torch.empty((z1 - z0, Y, X), dtype=torch.int32, device=self.device)
        elif self._label_volume("cc_runs_decode", out) != (z1 - z0, Y, X):
            raise ValueError(f"cc_runs_decode: out of shape {tuple(out.shape)}, the planes [{z0}, {z1}) are {(z1 - z0, Y, X)}")
        self._enter()
        try:
            self._check(self.lib.dlv_cc_runs_decode_dev(self.ctx, C.c_void_p(rs_dev.data_ptr()), (z1 - z0) * Y, X,
                                                        *(C.c_void_p(t.data_ptr()) if b > a else None for t in (x0, x1, label)), b - a,
                                                        C.c_void_p(out.data_ptr())))
        finally:
            self._leave()  # (torch's stream now waits for the kernel: the uploaded runs freed here are not reused before it)
        return out

    def cc_overlap(self, labels_a, n_a: int, labels_b, n_b: int, settings=None) -> dict:
        """The overlap table of two label volumes in HBM (dlv_cc_overlap_count_dev, dlv_cc_overlap_dev; the numpy statement:
        compare_cells.overlap_table_np).  labels_a, labels_b: int32 (uint32 payload) (Z,Y,X) in HBM, contiguous, of one shape.  A
        voxel takes part when 1 <= a <= n_a and 1 <= b <= n_b.  -> {"a", "b": uint32 (P), "voxels": uint64 (P), "segments": S}: the
        P pairs of labels that share voxels, sorted by (a, b) and unique, with the voxels they share; S = the stretches of one pair
        inside the rows, which sized the table.  The table (32 bytes per min(S, n_a * n_b), rounded up to a power of two) and the
        outputs (16 bytes each) must fit the HBM budget (streaming.hbm_budget_bytes of `settings`): MemoryError names the sizes."""
        torch = self.torch
        shape = self._label_volume("cc_overlap", labels_a)
        if self._label_volume("cc_overlap", labels_b) != shape:
            raise ValueError(f"cc_overlap: labels_a of shape {shape}, labels_b of shape {tuple(labels_b.shape)}")
        Z, Y, X = shape
        n_a, n_b = int(n_a), int(n_b)
        if n_a < 0 or n_b < 0:
            raise ValueError(f"cc_overlap: n_a = {n_a}, n_b = {n_b}")
        empty = {"a": np.zeros(0, dtype=np.uint32), "b": np.zeros(0, dtype=np.uint32), "voxels": np.zeros(0, dtype=np.uint64), "segments": 0}
        pa, pb = C.c_void_p(labels_a.data_ptr()), C.c_void_p(labels_b.data_ptr())
        s, p = C.c_uint64(), C.c_uint64()
        self._enter()
        try:
            self._check(self.lib.dlv_cc_overlap_count_dev(self.ctx, pa, pb, Z, Y, X, n_a, n_b, C.byref(s)))
            S = int(s.value)
            bound = min(S, n_a * n_b)
            if bound == 0:
                return empty
            cap = 1 << (2 * bound - 1).bit_length()  # the power of two >= 2 * bound
            from .streaming import hbm_budget_bytes

            need, budget = cap * 16 + 2 * bound * 8, hbm_budget_bytes(self, settings)
            if need > budget:
                raise MemoryError(f"delivr_cfos_amd (DLV_ENOMEM): cc_overlap needs a pair table of {cap} slots ({cap * 16 / 2**30:.2f} GiB) and "
                                  f"outputs of {bound} pairs ({bound * 16 / 2**30:.2f} GiB) for {S} pair segments of {n_a} x {n_b} labels, "
                                  f"the HBM budget is {budget / 2**30:.2f} GiB; compare a crop, or raise settings['mi355x']['hbm_budget_gb']")
            table = torch.empty(2 * cap, dtype=torch.int64, device=self.device)  # uint64 payloads
            keys = torch.empty(bound, dtype=torch.int64, device=self.device)
            voxels = torch.empty(bound, dtype=torch.int64, device=self.device)
            self._check(self.lib.dlv_cc_overlap_dev(self.ctx, pa, pb, Z, Y, X, n_a, n_b, S, C.c_void_p(table.data_ptr()), cap,
                                                    C.c_void_p(keys.data_ptr()), C.c_void_p(voxels.data_ptr()), bound, C.byref(p)))
        finally:
            self._leave()
        P = int(p.value)
        key = keys[:P].cpu().numpy().view(np.uint64)
        vox = voxels[:P].cpu().numpy().view(np.uint64)
        order = np.argsort(key, kind="stable")  # (the device order is unspecified)
        key = key[order]
        return {"a": (key >> np.uint64(32)).astype(np.uint32), "b": (key & np.uint64(0xFFFFFFFF)).astype(np.uint32),
                "voxels": np.ascontiguousarray(vox[order]), "segments": S}

    def cc_neighbours(self, labels, n: int, spacing=(1, 1, 1), radius_sq: int = 1, settings=None) -> dict:
        """The neighbour table of a label volume in HBM (dlv_cc_neighbours_count_dev, dlv_cc_neighbours_dev; the numpy statement:
        tests/helpers/neighbour_reference.py).  labels: int32 (uint32 payload) (Z,Y,X) in HBM, contiguous, not modified.  A voxel
        takes part when 1 <= label <= n.  spacing: (wz, wy, wx), integers 1..64; radius_sq: an integer >= 1, in spacing units.
        -> {"a", "b": uint32 (P), "gap_sq": uint32 (P), "segments": S}: the P pairs of labels a < b whose cells come within
        sqrt(radius_sq) of each other, sorted by (a, b) and unique, with the exact smallest squared distance between a voxel of one
        and a voxel of the other; S = the segments of the scan, which sized the table.  ValueError for a reach
        floor(sqrt(radius_sq) / w) above hostlogic.NEIGHBOUR_MAX_REACH voxels on an axis.  The table (32 bytes per
        min(S, n (n - 1) / 2), rounded up to a power of two) and the outputs (12 bytes each) must fit the HBM budget
        (streaming.hbm_budget_bytes of `settings`): MemoryError names the sizes."""
        from .hostlogic import neighbour_reach

        torch = self.torch
        Z, Y, X = self._label_volume("cc_neighbours", labels)
        spacing = tuple(spacing) if isinstance(spacing, (tuple, list)) else (spacing,)
        if len(spacing) != 3 or any(isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 1 <= int(w) <= 64 for w in spacing):
            raise ValueError(f"cc_neighbours: spacing = {spacing!r}: expected three integers 1..64 (wz, wy, wx)")
        if isinstance(radius_sq, bool) or not isinstance(radius_sq, (int, np.integer)) or int(radius_sq) < 1:
            raise ValueError(f"cc_neighbours: radius_sq = {radius_sq!r}: expected an integer >= 1")
        n, r2 = int(n), int(radius_sq)
        if n < 0:
            raise ValueError(f"cc_neighbours: n = {n}")
        neighbour_reach(r2, spacing, "cc_neighbours: radius_sq")  # (ValueError that names the axis)
        empty = {"a": np.zeros(0, dtype=np.uint32), "b": np.zeros(0, dtype=np.uint32), "gap_sq": np.zeros(0, dtype=np.uint32), "segments": 0}
        head = (self.ctx, C.c_void_p(labels.data_ptr()), Z, Y, X, n, *(int(w) for w in spacing), r2)
        s, p = C.c_uint64(), C.c_uint64()
        self._enter()
        try:
            self._check(self.lib.dlv_cc_neighbours_count_dev(*head, C.byref(s)))
            S = int(s.value)
            bound = min(S, n * (n - 1) // 2)
            if bound == 0:
                return empty
            cap = 1 << (2 * bound - 1).bit_length()  # the power of two >= 2 * bound
            from .streaming import hbm_budget_bytes

            need, budget = cap * 16 + bound * 12, hbm_budget_bytes(self, settings)
            if need > budget:
                raise MemoryError(f"delivr_cfos_amd (DLV_ENOMEM): cc_neighbours needs a pair table of {cap} slots ({cap * 16 / 2**30:.2f} GiB) "
                                  f"and outputs of {bound} pairs ({bound * 12 / 2**30:.2f} GiB) for {S} segments of {n} labels, the HBM "
                                  f"budget is {budget / 2**30:.2f} GiB; take a smaller radius, or raise settings['mi355x']['hbm_budget_gb']")
            table = torch.empty(2 * cap, dtype=torch.int64, device=self.device)  # uint64 payloads
            keys = torch.empty(bound, dtype=torch.int64, device=self.device)
            gaps = torch.empty(bound, dtype=torch.int32, device=self.device)  # uint32 payloads
            self._check(self.lib.dlv_cc_neighbours_dev(*head, S, C.c_void_p(table.data_ptr()), cap, C.c_void_p(keys.data_ptr()),
                                                       C.c_void_p(gaps.data_ptr()), bound, C.byref(p)))
        finally:
            self._leave()
        P = int(p.value)
        key = keys[:P].cpu().numpy().view(np.uint64)
        gap = gaps[:P].cpu().numpy().view(np.uint32)
        order = np.argsort(key, kind="stable")  # (the device order is unspecified)
        key = key[order]
        return {"a": (key >> np.uint64(32)).astype(np.uint32), "b": (key & np.uint64(0xFFFFFFFF)).astype(np.uint32),
                "gap_sq": np.ascontiguousarray(gap[order]), "segments": S}

    # ---- blob painting -----------------------------------------------------------------------------
    def edt_u16(self, stack, sampling_zyx):
        """blob_depthmap.py:160-170: exact Euclidean distance (units of `sampling_zyx`) of every non-zero voxel of the
        uint16 stack to the nearest zero voxel, the stack surrounded by zeros; truncated to uint16 (dlv_edt_u16_dev)."""
        torch = self.torch
        Z, Y, X = (int(v) for v in stack.shape)
        out = torch.empty((Z, Y, X), dtype=torch.uint16, device=self.device)
        samp = (C.c_double * 3)(*[float(v) for v in sampling_zyx])
        self._enter()
        self._check(self.lib.dlv_edt_u16_dev(self.ctx, self._dev(stack, torch.uint16, "stack"), Z, Y, X, samp,
                                             C.c_void_p(out.data_ptr())))
        self._leave()
        return out

    def paint_boxes(self, bin_img, boxes: np.ndarray, values):
        """blob_highlighter.py:108-125 / :150-158 on the device.  bin_img: uint8 (Z,Y,X) in HBM; boxes (n,6) int32
        half-open slices in painting order; values: list of (n,) uint8 / uint16 arrays (one image per array).
        Returns the list of painted images (HBM tensors)."""
        torch = self.torch
        Z, Y, X = (int(v) for v in bin_img.shape)
        boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 6)
        n = int(boxes.shape[0])
        owner = torch.empty((Z, Y, X), dtype=torch.int32, device=self.device)
        boxes_dev = torch.from_numpy(boxes).to(self.device) if n else None
        self._enter()
        self._check(self.lib.dlv_paint_owner_dev(
            self.ctx, self._dev(bin_img, torch.uint8, "bin_img"), Z, Y, X,
            C.c_void_p(boxes_dev.data_ptr()) if n else None, boxes.ctypes.data_as(C.c_void_p) if n else None, n,
            C.c_void_p(owner.data_ptr())))
        outs = []
        for val in values:
            val = np.ascontiguousarray(val)
            if val.dtype not in (np.uint8, np.uint16) or val.shape != (n,):
                raise TypeError("values: (n_boxes,) uint8 or uint16 arrays")
            tdt = torch.uint8 if val.dtype == np.uint8 else torch.uint16
            vdev = torch.from_numpy(val if n else np.zeros(1, val.dtype)).to(self.device)
            out = torch.empty((Z, Y, X), dtype=tdt, device=self.device)
            self._check(self.lib.dlv_paint_apply_dev(self.ctx, C.c_void_p(owner.data_ptr()), C.c_void_p(bin_img.data_ptr()),
                                                     Z * Y * X, C.c_void_p(vdev.data_ptr()), val.dtype.itemsize,
                                                     C.c_void_p(out.data_ptr())))
            outs.append(out)
        self._leave()
        self.sync()
        return outs

    def _paint_luts(self, what: str, rgb, u16):
        """the look-up tables of paint_labels / paint_runs in HBM -> (n_lut, packed r | g << 8 | b << 16 int32 tensor or None, uint16
        tensor or None)"""
        torch = self.torch
        if rgb is None and u16 is None:
            raise ValueError(f"{what}: neither rgb nor u16 is given")
        n_lut, rgb_dev, u16_dev = None, None, None
        if rgb is not None:
            rgb = np.asarray(rgb)
            if rgb.dtype != np.uint8 or rgb.ndim != 2 or rgb.shape[1] != 3 or rgb.shape[0] < 1:
                raise TypeError(f"{what}: rgb: expected an (n_lut, 3) uint8 array, got {rgb.dtype} of shape {rgb.shape}")
            n_lut = int(rgb.shape[0])
            wide = rgb.astype(np.uint32)
            packed = np.ascontiguousarray(wide[:, 0] | (wide[:, 1] << 8) | (wide[:, 2] << 16))
            rgb_dev = torch.from_numpy(packed.view(np.int32)).to(self.device)
        if u16 is not None:
            u16 = np.ascontiguousarray(u16)
            if u16.dtype != np.uint16 or u16.ndim != 1 or u16.shape[0] < 1:
                raise TypeError(f"{what}: u16: expected an (n_lut,) uint16 array, got {u16.dtype} of shape {u16.shape}")
            if n_lut is not None and int(u16.shape[0]) != n_lut:
                raise ValueError(f"{what}: rgb holds {n_lut} entries, u16 {int(u16.shape[0])}")
            n_lut = int(u16.shape[0])
            u16_dev = torch.from_numpy(u16.view(np.int16).copy()).to(self.device)
        return n_lut, rgb_dev, u16_dev

    def _paint_planes(self, shape, rgb_dev, u16_dev):
        """the output planes of one paint call (not cleared: the kernels write every element) and their pointers, NULL where a
        table is absent"""
        torch = self.torch
        chans = tuple(torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(3)) if rgb_dev is not None else None
        gray = torch.empty(shape, dtype=torch.uint16, device=self.device) if u16_dev is not None else None
        ptrs = [C.c_void_p(t.data_ptr()) for t in chans] if chans else [None, None, None]
        ptrs.append(C.c_void_p(gray.data_ptr()) if gray is not None else None)
        result = tuple(x for x in (chans, gray) if x is not None)
        return ptrs, (result[0] if len(result) == 1 else result)

    def paint_labels(self, labels, rgb=None, u16=None):
        """Every voxel painted with the value of the cell whose label it carries, out[v] = lut[labels[v]] (dlv_paint_labels_dev;
        blob_highlighter's "labels" mode).  labels: int32 (uint32 payload) (Z,Y,X) in HBM, contiguous.  rgb: (n_lut, 3) uint8,
        u16: (n_lut,) uint16, indexed by label - either or both, written in one pass; label 0 and labels >= n_lut paint 0.
        -> (r, g, b) uint8 tensors for rgb, a uint16 tensor for u16, ((r, g, b), image) for both - in HBM."""
        Z, Y, X = self._label_volume("paint_labels", labels)
        n_lut, rgb_dev, u16_dev = self._paint_luts("paint_labels", rgb, u16)
        ptrs, result = self._paint_planes((Z, Y, X), rgb_dev, u16_dev)
        self._enter()
        try:
            self._check(self.lib.dlv_paint_labels_dev(self.ctx, C.c_void_p(labels.data_ptr()), Z, Y, X, n_lut,
                                                      C.c_void_p(rgb_dev.data_ptr()) if rgb_dev is not None else None,
                                                      C.c_void_p(u16_dev.data_ptr()) if u16_dev is not None else None, *ptrs))
        finally:
            self._leave()
        return result

    def paint_runs(self, runs: dict, z0: int = 0, z1: Optional[int] = None, rgb=None, u16=None):
        """paint_labels for the planes [z0, z1) of the label volume a run-length coding holds, straight from the runs: the label
        volume is never built (dlv_paint_runs_dev).  runs: the dict of cc_runs_encode / label_runs.load_runs (validated there: the
        kernel clamps what it reads, it does not judge it).  Only the rows' slice of row_start and their runs are uploaded, as
        cc_runs_decode does.  -> the planes of paint_labels, (z1 - z0, Y, X) each, every element written."""
        torch = self.torch
        Z, Y, X = (int(v) for v in runs["shape"])
        z0, z1 = int(z0), Z if z1 is None else int(z1)
        if not 0 <= z0 < z1 <= Z:
            raise ValueError(f"paint_runs: planes [{z0}, {z1}) do not lie in the {Z} planes of the coding")
        rs = np.ascontiguousarray(runs["row_start"][z0 * Y:z1 * Y + 1], dtype=np.uint64)
        a, b = int(rs[0]), int(rs[-1])
        if len(rs) != (z1 - z0) * Y + 1 or not a <= b <= min(len(runs[k]) for k in ("x0", "x1", "label")):
            raise ValueError("paint_runs: row_start does not match the shape and the run arrays")
        n_lut, rgb_dev, u16_dev = self._paint_luts("paint_runs", rgb, u16)

        def dev(arr, np_dtype, as_int):  # (unsigned payloads in torch's signed types)
            return torch.from_numpy(np.ascontiguousarray(arr, dtype=np_dtype).view(as_int)).to(self.device)

        rs_dev = dev(rs, np.uint64, np.int64)
        x0, x1 = dev(runs["x0"][a:b], np.uint16, np.int16), dev(runs["x1"][a:b], np.uint16, np.int16)
        label = dev(runs["label"][a:b], np.uint32, np.int32)
        ptrs, result = self._paint_planes((z1 - z0, Y, X), rgb_dev, u16_dev)
        self._enter()
        try:
            self._check(self.lib.dlv_paint_runs_dev(self.ctx, C.c_void_p(rs_dev.data_ptr()), (z1 - z0) * Y, X,
                                                    *(C.c_void_p(t.data_ptr()) if b > a else None for t in (x0, x1, label)), b - a,
                                                    n_lut, C.c_void_p(rgb_dev.data_ptr()) if rgb_dev is not None else None,
                                                    C.c_void_p(u16_dev.data_ptr()) if u16_dev is not None else None, *ptrs))
        finally:
            self._leave()  # (torch's stream now waits for the kernel: the uploaded runs freed here are not reused before it)
        return result

    # ---- atlas-space heat map ----------------------------------------------------------------------
    def heatmap(self, cells_xyz: np.ndarray, shape_zyx, sigma: float = 2.25):
        """create_heatmap (cells_to_atlas.py:174-200) on the device: float32 (Z,Y,X) tensor in HBM."""
        torch = self.torch
        Z, Y, X = (int(v) for v in shape_zyx)
        xyz = np.ascontiguousarray(cells_xyz, dtype=np.int32).reshape(-1, 3)
        n = int(xyz.shape[0])
        heat = torch.empty((Z, Y, X), dtype=torch.float32, device=self.device)
        tmp = torch.empty_like(heat)
        xyz_dev = torch.from_numpy(xyz).to(self.device) if n else None
        # scipy.ndimage._filters._gaussian_kernel1d, order 0
        radius = int(4.0 * float(sigma) + 0.5)
        x = np.arange(-radius, radius + 1)
        phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
        phi = phi / phi.sum()
        w = np.ascontiguousarray(phi[radius:], dtype=np.float64)
        self._enter()
        self._check(self.lib.dlv_heatmap_counts_dev(self.ctx, C.c_void_p(xyz_dev.data_ptr()) if n else None, n, Z, Y, X,
                                                    C.c_void_p(heat.data_ptr())))
        self._check(self.lib.dlv_gauss_blur_f32_dev(self.ctx, C.c_void_p(heat.data_ptr()), Z, Y, X,
                                                    w.ctypes.data_as(C.c_void_p), radius, C.c_void_p(tmp.data_ptr())))
        self._leave()
        return heat

    # ---- resamplers --------------------------------------------------------------------------------
    def block_mean_u16(self, vol, factors):
        torch = self.torch
        Z, Y, X = (int(v) for v in vol.shape)
        fz, fy, fx = (int(f) for f in factors)
        out = torch.empty((-(-Z // fz), -(-Y // fy), -(-X // fx)), dtype=torch.uint16, device=self.device)
        self._enter()
        self._check(self.lib.dlv_block_mean_u16_dev(self.ctx, self._dev(vol, torch.uint16, "vol"), Z, Y, X, fz, fy, fx,
                                                    self._dev(out, torch.uint16, "out")))
        self._leave()
        return out

    def zoom_spline2_u8(self, mask, out_shape):
        torch = self.torch
        iz, iy, ix = (int(v) for v in mask.shape)
        oz, oy, ox = (int(v) for v in out_shape)
        out = torch.empty((oz, oy, ox), dtype=torch.uint8, device=self.device)
        self._enter()
        self._check(self.lib.dlv_zoom_spline2_u8_dev(self.ctx, self._dev(mask, torch.uint8, "mask"), iz, iy, ix,
                                                     self._dev(out, torch.uint8, "out"), oz, oy, ox))
        self._leave()
        return out

    def mask_pad_u16(self, raw, mask, padded_shape, threshold=0):
        torch = self.torch
        Z, Y, X = (int(v) for v in raw.shape)
        Zp, Yp, Xp = (int(v) for v in padded_shape)
        out = torch.empty((Zp, Yp, Xp), dtype=torch.uint16, device=self.device)
        self._enter()
        self._check(self.lib.dlv_mask_pad_u16_dev(
            self.ctx, self._dev(raw, torch.uint16, "raw"),
            self._dev(mask, torch.uint8, "mask") if mask is not None else None, int(threshold), Z, Y, X,
            self._dev(out, torch.uint16, "out"), Zp, Yp, Xp))
        self._leave()
        return out

    def trilinear_u16(self, vol, out_shape):
        torch = self.torch
        iz, iy, ix = (int(v) for v in vol.shape)
        oz, oy, ox = (int(v) for v in out_shape)
        out = torch.empty((oz, oy, ox), dtype=torch.uint16, device=self.device)
        self._enter()
        self._check(self.lib.dlv_trilinear_u16_dev(self.ctx, self._dev(vol, torch.uint16, "vol"), iz, iy, ix,
                                                   self._dev(out, torch.uint16, "out"), oz, oy, ox))
        self._leave()
        return out

    def affine_warp_u16(self, vol, matrix34, out_shape):
        """uint16 (Z,Y,X) in HBM resampled through a 3x4 affine map (output voxel index -> input voxel index, index
        space, zero outside, trilinear, round half up) - the north-star's atlas-space warp (dlv_affine_warp_u16_dev)."""
        torch = self.torch
        iz, iy, ix = (int(v) for v in vol.shape)
        oz, oy, ox = (int(v) for v in out_shape)
        m = np.ascontiguousarray(np.asarray(matrix34, dtype=np.float64).reshape(12))
        out = torch.empty((oz, oy, ox), dtype=torch.uint16, device=self.device)
        self._enter()
        self._check(self.lib.dlv_affine_warp_u16_dev(self.ctx, self._dev(vol, torch.uint16, "vol"), iz, iy, ix,
                                                     m.ctypes.data_as(C.POINTER(C.c_double)),
                                                     self._dev(out, torch.uint16, "out"), oz, oy, ox))
        self._leave()
        return out

    # ---- kernel timer ------------------------------------------------------------------------------
    # ---- fp16 range guard: per-block output shift (dlv_unet_set_conv_shift) ----------------------------------------
    def set_conv_shift(self, layer: int, shift: int) -> None:
        """conv block `layer` (0..17) stores its raw output 2^-shift times smaller (16-bit paths only; InstanceNorm removes the
        factor exactly)"""
        self._enter()
        self._check(self.lib.dlv_unet_set_conv_shift(self.ctx, int(layer), int(shift)))
        self._leave()

    def conv_shifts(self):
        out = []
        for i in range(_lib.N_CONV):
            v = C.c_int()
            self._check(self.lib.dlv_unet_get_conv_shift(self.ctx, i, C.byref(v)))
            out.append(v.value)
        return out

    def note_conv_shifts(self, shifts) -> None:
        """the blob this engine received by broadcast was packed with these per-block shifts (no repack)"""
        arr = (C.c_int * _lib.N_CONV)(*[int(v) for v in shifts])
        self._check(self.lib.dlv_unet_note_conv_shifts(self.ctx, arr))

    def range_report(self):
        """(layer the last DLV_ERANGE named or -1, [|mean| + 8 sigma of every conv block's raw output where it exceeded 4096])"""
        layer = C.c_int()
        peaks = (C.c_float * _lib.N_CONV)()
        self._check(self.lib.dlv_range_report(self.ctx, C.byref(layer), peaks))
        return layer.value, [float(v) for v in peaks]

    def range_recover(self) -> int:
        """dlv_range_recover: the library's own next step after DLV_ERANGE (what range_guard.next_shifts decides, applied);
        -> number of conv blocks whose shift changed; raises DelivrHipError(DLV_ERANGE) when nothing is left to try"""
        n = C.c_int()
        self._enter()
        try:
            self._check(self.lib.dlv_range_recover(self.ctx, C.byref(n)))
        finally:
            self._leave()
        return n.value

    def set_lanes(self, lanes: int):
        self._check(self.lib.dlv_set_lanes(self.ctx, int(lanes)))

    def prof_enable(self, on: bool = True):
        self._check(self.lib.dlv_prof_enable(self.ctx, 1 if on else 0))

    def prof_reset(self):
        self._check(self.lib.dlv_prof_reset(self.ctx))

    def prof_report(self) -> Dict[str, dict]:
        ent = (_lib.ProfEntry * _lib.PROF_MAX)()
        n = C.c_int()
        self._check(self.lib.dlv_prof_report(self.ctx, ent, _lib.PROF_MAX, C.byref(n)))
        out = {}
        for i in range(min(n.value, _lib.PROF_MAX)):
            e = ent[i]
            out[e.name.decode()] = {"launches": e.launches, "total_ms": e.total_ms, "flops": e.flops, "bytes": e.bytes}
        return out


def _tensor_view(torch, ptr: int, nbytes: int, device):
    """uint8 torch view of library-owned HBM (no copy) via __cuda_array_interface__."""

    class _Holder:
        pass

    h = _Holder()
    h.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(h, device=device)
