"""float64 references of single layers of the 16-bit MFMA path (tests/test_gpu_conv_kernels.py, tests/test_gpu_layer_kernels.py).

TEST INFRASTRUCTURE ONLY, like the rest of ``oracle/``.  Each reference works on the operands the kernel receives - inputs
and weights rounded to the 16-bit format with torch's ``.half()`` / ``.bfloat16()`` - and does the arithmetic in float64 on
the CPU.  ``fmt=None`` skips the rounding: then the references equal the oracle U-Net's own layers run in float64
(tests/test_layer_ref_cpu.py).

Every conv-block reference returns a dict (the references of the layers without an InstanceNorm of their own - deconv,
norm_pool, replicate_pad, final_logits - say what they return):
  raw    conv output including every bias term (what torch's modules compute)
  drop   the per-channel constant (B, C) a kernel may leave out of its stored raw output: the conv bias (z-reg conv) or the
         folded conv's interior up-sampling bias term  sum_taps Wc_up * b_up  (upconv.hip); see ``stored_raw``
  mean, var   InstanceNorm statistics of ``raw`` (biased variance) per (sample, channel)
  scale, shift  InstanceNorm affine: normalised = raw * scale + shift
  out    Mish(InstanceNorm(raw))
"""
from __future__ import annotations

from typing import Optional

EPS = 1e-5


def round16(t, fmt: Optional[str]):
    """float64 copy of t rounded to fp16 ("fp16"/"f16"), bf16 ("bf16") or not at all (None)."""
    if fmt is None:
        return t.double()
    if fmt in ("fp16", "f16"):
        return t.half().double()
    if fmt == "bf16":
        return t.bfloat16().double()
    raise ValueError(fmt)


def mish(x):
    import torch

    return x * torch.tanh(torch.nn.functional.softplus(x))


def activate(raw, ss, fmt: Optional[str]):
    """what a consumer sees of a raw tensor awaiting scale/shift ss (B, C, 2): round16(mish(round16(raw) * sc + sh))."""
    r = round16(raw, fmt)
    ss = ss.double()
    return round16(mish(r * ss[:, :, 0, None, None, None] + ss[:, :, 1, None, None, None]), fmt)


def _norm(raw, gamma, beta, drop):
    gamma, beta = gamma.double(), beta.double()
    mean = raw.mean(dim=(2, 3, 4))
    var = ((raw - mean[:, :, None, None, None]) ** 2).mean(dim=(2, 3, 4))
    scale = gamma[None, :] / (var + EPS).sqrt()
    shift = beta[None, :] - mean * scale
    out = mish(raw * scale[:, :, None, None, None] + shift[:, :, None, None, None])
    return {"raw": raw, "drop": drop, "mean": mean, "var": var, "scale": scale, "shift": shift, "out": out}


def stored_raw(ref, raw_scale: float, drops: bool):
    """the raw output as a kernel stores it: raw_scale * (raw - drop) where the kernel drops the constant."""
    r = ref["raw"] - ref["drop"][:, :, None, None, None] if drops else ref["raw"]
    return r * raw_scale


def conv_block(x1, weight, bias, gamma, beta, fmt: Optional[str], ss1=None, x2=None):
    """Conv3d(k3, pad 1) + InstanceNorm + Mish on cat[x1, x2].  ss1 (B, c1, 2): x1 is raw and activated on load."""
    import torch
    import torch.nn.functional as F

    a1 = activate(x1, ss1, fmt) if ss1 is not None else round16(x1, fmt)
    xin = a1 if x2 is None else torch.cat([a1, round16(x2, fmt)], dim=1)
    raw = F.conv3d(xin, round16(weight, fmt), bias.double(), padding=1)
    return _norm(raw, gamma, beta, bias.double()[None, :].expand(raw.shape[0], -1))


def folded_upcat(skip, coarse, w_conv, b_conv, w_up, b_up, gamma, beta, fmt: Optional[str], ss_skip=None):
    """The first conv of an UpCat block written the plain way: u = ConvTranspose3d(coarse), Conv3d(cat[skip, u]).
    coarse is the ACTIVATED coarse tensor (rounded to the format, as the kernel receives it); the up-half weights are the
    checkpoint's (the kernel folds them in fp32 and rounds the product once).  drop = conv bias + the interior term
    sum_taps Wc_up * b_up, the constant the folded kernel leaves out."""
    import torch
    import torch.nn.functional as F

    cs = skip.shape[1]
    s = activate(skip, ss_skip, fmt) if ss_skip is not None else round16(skip, fmt)
    u = F.conv_transpose3d(round16(coarse, fmt), w_up.double(), b_up.double(), stride=2)
    w = w_conv.double()
    wr = torch.cat([round16(w[:, :cs], fmt), w[:, cs:]], dim=1)
    raw = F.conv3d(torch.cat([s, u], dim=1), wr, b_conv.double(), padding=1)
    const = torch.einsum("oct,c->o", w[:, cs:].reshape(w.shape[0], -1, 27), b_up.double())
    return _norm(raw, gamma, beta, (b_conv.double() + const)[None, :].expand(raw.shape[0], -1))


def stem(vol, weight, bias, gamma, beta, fmt: Optional[str], w_scale: float = 1.0, flip_dim: Optional[int] = None):
    """Conv3d(1 -> C) + InstanceNorm + Mish of B uint16 windows (B, D, H, W) (an int tensor), flipped along flip_dim (2 = z,
    3 = y, 4 = x of the (B, 1, D, H, W) input).  The MFMA stem splits a voxel into its low and high byte (exact in both
    formats) and multiplies them with round16(w * w_scale) and round16(256 * w * w_scale): w_scale is the format's
    STEM_SCALE times 2^-shift; the result is divided by w_scale again here (raw in the module's units)."""
    import torch.nn.functional as F

    v = vol.long()[:, None]
    if flip_dim is not None:
        v = v.flip(flip_dim)
    lo, hi = (v & 255).double(), (v >> 8).double()
    w = weight.double()
    raw = (F.conv3d(lo, round16(w * w_scale, fmt), padding=1) + F.conv3d(hi, round16(256.0 * w * w_scale, fmt), padding=1)) / w_scale
    raw = raw + bias.double()[None, :, None, None, None]
    return _norm(raw, gamma, beta, bias.double()[None, :].expand(raw.shape[0], -1))


# ---------------------------------------------------------------------------------------------------
# the other layers of the 16-bit forward (tests/test_gpu_layer_kernels.py): no InstanceNorm of their own, so each returns what
# its check needs instead of the dict above
# ---------------------------------------------------------------------------------------------------
def deconv(x, w, b, fmt: Optional[str], ss=None):
    """ConvTranspose3d(k2, s2) of x (B, Cin, D, H, W) with w (Cin, Cout, 2, 2, 2) and bias b.  ss (B, Cin, 2): x is raw and goes
    through ``activate`` first.  Returns {"raw": the output with its bias, "x": the operand the kernel multiplies, "abs": the
    same transposed conv of |x| and |w| without bias (the sum of absolute products the fp32 accumulation error scales with)}."""
    import torch.nn.functional as F

    a = activate(x, ss, fmt) if ss is not None else round16(x, fmt)
    w16 = round16(w, fmt)
    return {"raw": F.conv_transpose3d(a, w16, b.double(), stride=2), "x": a, "abs": F.conv_transpose3d(a.abs(), w16.abs(), None, stride=2)}


def norm_pool(raw, ss, fmt: Optional[str], fmt_out: Optional[str], pool: bool):
    """The InstanceNorm + Mish pass over a stored raw tensor: y = round16(raw, fmt) * sc + sh, act = mish(y).  Returns {"y", "act"
    (both unrounded float64), "out": round16(act, fmt_out), and with pool "pooled_act": MaxPool3d(2) of act (odd sizes drop the
    last plane / row / column) and "pooled": round16 of it to fmt_out (rounding is monotone: the maximum of the rounded values)}."""
    import torch.nn.functional as F

    s = ss.double()
    y = round16(raw, fmt) * s[:, :, 0, None, None, None] + s[:, :, 1, None, None, None]
    act = mish(y)
    r = {"y": y, "act": act, "out": round16(act, fmt_out)}
    if pool:
        r["pooled_act"] = F.max_pool3d(act, 2)
        r["pooled"] = round16(r["pooled_act"], fmt_out)
    return r


def replicate_pad(u, skip_shape):
    """UpCat's padding of an up-sampled tensor to the skip tensor's (D, H, W): the edge value once more at the far end of every
    dimension that is a voxel short."""
    import torch.nn.functional as F

    pad = []
    for have, want in zip(reversed(u.shape[2:]), reversed(tuple(skip_shape))):
        if want - have not in (0, 1):
            raise ValueError(f"skip shape {tuple(skip_shape)} against {tuple(u.shape[2:])}")
        pad += [0, want - have]
    return F.pad(u, pad, mode="replicate") if any(pad) else u


def final_logits(raw, ss, w, b, fmt: Optional[str]):
    """The final Conv3d(32 -> 1, k1) on the raw output of the last block, activated on load in fp32 (no 16-bit rounding of the
    activation; w (1, 32, 1, 1, 1) and b stay fp32).  Returns {"logits" (B, D, H, W), "y", "m" = mish(y)} (B, 32, D, H, W)."""
    s = ss.double()
    y = round16(raw, fmt) * s[:, :, 0, None, None, None] + s[:, :, 1, None, None, None]
    m = mish(y)
    wc = w.double().reshape(1, -1, 1, 1, 1)
    return {"logits": (m * wc).sum(dim=1) + b.double().reshape(()), "y": y, "m": m}
