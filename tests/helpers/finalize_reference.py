"""The finalize step (csrc/finalize.hip) stated with numpy and scipy alone, slab semantics included, and the inputs and cases of
tests/test_gpu_finalize_kernels.py (tests/test_finalize_reference_cpu.py checks both without a GPU).

    mean = acc / cnt (float32; no count map: acc is the mean);  fg = 1 / (1 + exp(-mean)) >= threshold, in float32
    keep = binary_erosion(raw > 0, iterations=radius, border_value=1), evaluated per z-block
    out  = fg & keep on the unpadded (nz, Y, X) planes

The z-blocks sit at ABSOLUTE multiples of `zblock` and are clipped to the planes [z_abs0, z_abs0 + nz) the buffers hold; whatever
lies outside a clipped block counts as foreground.  Radius 0 means no erosion (keep = raw > 0): scipy's iterations=0 means "repeat
until nothing changes" instead, so orc.l1_distance_keep states that one radius."""
import functools
from collections import namedtuple

import numpy as np

from oracle import delivr_oracle as orc

BAND = 1e-6                   # no voxel's fp64 sigmoid lies this close to a threshold (make_sums redraws those that do)
THRESHOLDS = (0.5, 0.3, 0.9)  # the thresholds of the GPU cases


def zblocks(nz, zblock, z_abs0=0):
    """[(lo, hi)]: local plane ranges of the z-blocks (absolute multiples of zblock, clipped to [z_abs0, z_abs0 + nz)); zblock <= 0:
    one block"""
    if zblock <= 0:
        return [(0, nz)]
    out = []
    for b in range(z_abs0 // zblock, (z_abs0 + nz - 1) // zblock + 1):
        lo, hi = max(b * zblock, z_abs0), min((b + 1) * zblock, z_abs0 + nz)
        out.append((lo - z_abs0, hi - z_abs0))
    return out


def eroded_keep(raw, stack_zyx, radius, zblock, z_abs0=0):
    """uint8 (nz, Y, X): raw[:nz, :Y, :X] > 0 eroded per z-block - scipy itself for radius >= 1"""
    nz, Y, X = (int(v) for v in stack_zyx)
    fg = (np.asarray(raw)[:nz, :Y, :X] > 0).astype(np.uint8)
    keep = np.empty((nz, Y, X), dtype=np.uint8)
    for lo, hi in zblocks(nz, zblock, z_abs0):
        keep[lo:hi] = orc.erode_l1(fg[lo:hi], radius) if radius >= 1 else orc.l1_distance_keep(fg[lo:hi], 0)
    return keep


def mean32(acc, cnt, stack_zyx):
    """float32 (nz, Y, X): acc / cnt as orc.finalize forms it (x/0 = +-inf, 0/0 = NaN)"""
    nz, Y, X = (int(v) for v in stack_zyx)
    s = np.asarray(acc, dtype=np.float32)[:nz, :Y, :X]
    if cnt is None:
        return s
    with np.errstate(divide="ignore", invalid="ignore"):
        return (s / np.asarray(cnt)[:nz, :Y, :X]).astype(np.float32)


def sigmoid64(m32):
    """the fp64 sigmoid of a float32 mean (NaN where the mean is NaN)"""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-m32.astype(np.float64)))


def finalize_reference(acc, cnt, raw, stack_zyx, threshold, radius, zblock, z_abs0=0):
    """-> (uint8 mask (nz, Y, X), fp64 sigmoid of the float32 mean (nz, Y, X)).  acc / cnt / raw may be padded ((>= nz, Yp, Xp)):
    only [:nz, :Y, :X] is read.  The decision is orc.finalize's: float32 division, 1 / (1 + exp(-m)) in float32, >=."""
    m32 = mean32(acc, cnt, stack_zyx)
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-m32))
    assert sig.dtype == np.float32
    fg = (sig >= np.float32(threshold)).astype(np.uint8)
    return fg * eroded_keep(raw, stack_zyx, radius, zblock, z_abs0), sigmoid64(m32)


def ulp_distance(got32, want64):
    """float32 units in the last place between got32 and want64 rounded to float32, for non-negative finite values"""
    a = np.ascontiguousarray(got32, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(want64.astype(np.float32)).view(np.int32).astype(np.int64)
    return np.abs(a - b)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def in_band(acc, cnt, thresholds=THRESHOLDS):
    """voxels whose fp64 sigmoid - of acc / cnt or of acc alone - lies within BAND of one of the thresholds"""
    bad = np.zeros(acc.shape, dtype=bool)
    for m in (mean32(acc, cnt, acc.shape), acc):
        s = sigmoid64(m)
        for t in thresholds:
            bad |= np.abs(s - np.float64(np.float32(t))) <= BAND
            bad |= np.abs(s - t) <= BAND
    return bad


def make_sums(shape, seed, thresholds=THRESHOLDS):
    """-> (acc float32, cnt uint8 in 1..8), both `shape`: mean logits ~ N(0, 2) drawn per voxel (no two planes alike), acc = mean *
    cnt.  A voxel whose sigmoid lies within BAND of a threshold is redrawn - with or without the count map, so one pair serves
    both - until none is left: no voxel is ever masked out of a comparison."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(1, 9, size=shape).astype(np.uint8)
    acc = (rng.normal(0.0, 2.0, size=shape) * cnt).astype(np.float32)
    for _ in range(100):
        bad = in_band(acc, cnt, thresholds)
        if not bad.any():
            break
        acc[bad] = (rng.normal(0.0, 2.0, size=int(bad.sum())) * cnt[bad]).astype(np.float32)
    assert not in_band(acc, cnt, thresholds).any()
    return acc, cnt


def shares(keep, raw_fg):
    """(kept, removed) shares of the foreground voxels of raw"""
    n = int(raw_fg.sum())
    kept = int(keep[raw_fg].sum())
    return (kept / n, (n - kept) / n) if n else (0.0, 0.0)


def place_zeros(shape, radius, zblock, z_abs0, seed, corner=False):
    """few zeros at random voxels (corner: voxel (0, 0, 0) first, which leaves the far planes of a stack no deeper than the radius
    their share): as many (1, 2, 3, 4, 6, 9, ... of one fixed random order) as it takes for the reference to remove at
    least 10 % of the foreground (radius 0 removes no foreground: a tenth of the voxels then)"""
    Z, Y, X = shape
    order = np.random.default_rng(seed).permutation(Z * Y * X)
    if corner:
        order = np.concatenate([[0], order[order != 0]])
    n = 1 if radius else max(1, order.size // 10)
    while True:
        raw = np.ones(shape, dtype=np.uint16)
        raw.ravel()[order[:n]] = 0
        if not radius or shares(eroded_keep(raw, shape, radius, zblock, z_abs0), raw > 0)[1] >= 0.10 or n >= order.size // 4:
            return [tuple(int(v) for v in np.unravel_index(i, shape)) for i in order[:n]]
        n = max(n + 1, n * 3 // 2)


Case = namedtuple("Case", "name shape radius pad zblock z_abs0 threshold cnt zeros switches exempt seed")


def case(name, shape, radius=30, pad=(0, 0), zblock=0, z_abs0=None, threshold=0.5, cnt=True, zeros="auto", switches=(), exempt=False,
         seed=0):
    """shape (Z, Y, X); pad: (Yp - Y, Xp - X); z_abs0 None: HipEngine.finalize, else finalize_slab at that plane; zeros: "auto"
    (place_zeros), "corner" (the same, voxel (0, 0, 0) first), "rows" (one zero per row at row_zeros(X), "rows_y": in the first row
    of every plane only, "rows_z": in the even planes only), "none", "all" or a list of (z, y, x); exempt: the kept / removed shares are
    not asserted (an all-or-nothing case)"""
    zeros = zeros if isinstance(zeros, str) else tuple(tuple(p) for p in zeros)
    return Case(name, tuple(shape), radius, tuple(pad), zblock, z_abs0, threshold, cnt, zeros, tuple(switches), exempt, seed)


def row_zeros(X):
    """x of the single zero of row i (cyclic): both ends of the first chunk, of the 64-voxel window and of the row"""
    return sorted({0, 7, 8, 63, 64, X - 8, X - 1} & set(range(X)))


Inputs = namedtuple("Inputs", "acc cnt raw mask sig keep")


@functools.lru_cache(maxsize=None)
def build(c, raw_pad=0):
    """the inputs of a case (padded: acc NaN, cnt 0 and raw `raw_pad` in the padding) and its reference: Inputs(acc, cnt or None,
    raw, mask, fp64 sigmoid, keep), computed once per case and read-only.  Asserts the kept and removed shares on the reference
    unless the case is exempt."""
    Z, Y, X = c.shape
    Yp, Xp = Y + c.pad[0], X + c.pad[1]
    z_abs0 = c.z_abs0 or 0
    a, n = make_sums(c.shape, c.seed + 1)
    raw_in = np.random.default_rng(c.seed + 2).integers(1, 65536, size=c.shape).astype(np.uint16)
    if c.zeros in ("auto", "corner"):
        zeros = place_zeros(c.shape, c.radius, c.zblock, z_abs0, c.seed + 3, corner=c.zeros == "corner")
    elif c.zeros in ("rows", "rows_y", "rows_z"):
        xs = row_zeros(X)
        rows = [(z, y) for z in range(Z) for y in range(Y) if (c.zeros != "rows_y" or y == 0) and (c.zeros != "rows_z" or z % 2 == 0)]
        zeros = [(z, y, xs[i % len(xs)]) for i, (z, y) in enumerate(rows)]
    elif c.zeros == "none":
        zeros = []
    elif c.zeros == "all":
        raw_in[:] = 0
        zeros = []
    else:
        zeros = list(c.zeros)
    for z, y, x in zeros:
        raw_in[z, y, x] = 0
    acc = np.full((Z, Yp, Xp), np.nan, dtype=np.float32)
    cnt = np.zeros((Z, Yp, Xp), dtype=np.uint8)
    raw = np.full((Z, Yp, Xp), raw_pad, dtype=np.uint16)
    acc[:, :Y, :X], cnt[:, :Y, :X], raw[:, :Y, :X] = a, n, raw_in
    cnt = cnt if c.cnt else None
    mask, sig = finalize_reference(acc, cnt, raw, c.shape, c.threshold, c.radius, c.zblock, z_abs0)
    keep = eroded_keep(raw, c.shape, c.radius, c.zblock, z_abs0)
    if not c.exempt:
        kept, removed = shares(keep, raw_in > 0)
        assert kept >= 0.05 and removed >= 0.05, (c.name, kept, removed)
    for a in (acc, cnt, raw, mask, sig, keep):
        if a is not None:
            a.setflags(write=False)
    return Inputs(acc, cnt, raw, mask, sig, keep)


# (acc, cnt, foreground at threshold 0.5 with the count map, ... without it: acc is the mean then)
PLANTED = (
    (np.float32(0.0), 3, True, True),       # +0 -> sigmoid exactly 0.5 -> >= 0.5
    (np.float32(-0.0), 3, True, True),      # -0 likewise
    (np.float32(0.0), 0, False, True),      # 0 / 0 = NaN -> background
    (np.float32(2.5), 0, True, True),       # x / 0 = +inf -> 1
    (np.float32(-2.5), 0, False, False),    # -inf -> 0
    (np.float32(1000.0), 1, True, True),    # what skipped windows contribute, and its mirror image
    (np.float32(-1000.0), 1, False, False),
)


def plant_decision(c, inp):
    """the inputs of a case with the PLANTED sums and counts written over the first voxels the erosion keeps, one per entry, and
    the reference of that -> (Inputs, [(z, y, x)])"""
    Z, Y, X = c.shape
    where = [tuple(int(v) for v in p) for p in np.argwhere(inp.keep > 0)[:: max(1, int(inp.keep.sum()) // len(PLANTED))][:len(PLANTED)]]
    assert len(where) == len(PLANTED)
    acc, cnt = inp.acc.copy(), None if inp.cnt is None else inp.cnt.copy()
    for p, (a, n, _, _) in zip(where, PLANTED):
        acc[p] = a
        if cnt is not None:
            cnt[p] = n
    mask, sig = finalize_reference(acc, cnt, inp.raw, c.shape, c.threshold, c.radius, c.zblock, c.z_abs0 or 0)
    return Inputs(acc, cnt, inp.raw, mask, sig, inp.keep), where


def expected_ran(c):
    """the launch record (dlv_finalize_ran) a case must give with 16-byte aligned buffers: the dispatch of finalize_impl restated"""
    Z, Y, X = c.shape
    Xp = X + c.pad[1]
    split, two = "erode_xy_split" in c.switches, "erode_z_two_sweeps" in c.switches
    cap, nchunk = c.radius + 1, (X + 7) // 8
    ran = dict(xy_form=0, nc=0, y_v=0, z_form=0, z_v=4 if X % 4 == 0 else 1, nblk=0, zphase=0, raw_vec=int(Xp % 8 == 0),
               dist_vec=int(X % 8 == 0), acc_vec=0)
    if cap <= 57 and nchunk <= 1024 and not split:
        ran["nc"] = 1 if nchunk <= 256 else 2 if nchunk <= 512 else 4
    else:
        ran["xy_form"], ran["y_v"] = (1 if cap <= 57 else 2), ran["z_v"]
        if cap > 57:
            ran["raw_vec"] = ran["dist_vec"] = 0
    ran["z_form"] = 0 if c.radius <= 31 and not two else 1
    ran["acc_vec"] = int(ran["z_form"] == 0 and ran["z_v"] == 4 and Xp % 4 == 0)
    if c.z_abs0 is None:
        zb = c.zblock if 0 < c.zblock <= Z else Z
    else:
        zb = c.zblock if c.zblock > 0 else 0x3FFFFFFF
        ran["zphase"] = c.z_abs0 % zb
    ran["nblk"] = -(-(Z + ran["zphase"]) // zb)
    return ran


# ---- the cases of tests/test_gpu_finalize_kernels.py --------------------------------------------------------------------------
XY_CHUNK_X = (2048, 2049, 4096, 4097, 8192, 8193, 2056, 4104, 4099)
XY_SMALL_X = (24, 13, 8, 7, 1)
XY_ROWS_Y = (1, 2, 3, 6)
WINDOW_X = tuple(range(57, 131, 9)) + (130, 200)  # X % 8 = 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 0
Z_RADII = ((0, ()), (1, ()), (30, ()), (31, ()), (32, ()), (1, ("erode_z_two_sweeps",)), (30, ("erode_z_two_sweeps",)))
SPLIT = ("erode_xy_split",)
TWO = ("erode_z_two_sweeps",)


def z_depths(radius):
    return sorted({z for z in (1, 2, 3, 5, radius, radius + 1, 2 * radius + 3, 150) if z >= 1})


def z_blocks_of(radius, Z):
    """zblock = 1, 2, radius - 1, radius, radius + 1, a non-divisor of Z, > Z"""
    nondiv = next(b for b in range(radius + 2, Z) if Z % b)
    return sorted({b for b in (1, 2, radius - 1, radius, radius + 1, nondiv, Z + 7) if b >= 1})


# (zblock, radius, [(z_abs0, nz)]): phases 0, 1 and zblock - 1; slabs shorter than a block, slabs that begin and end inside one
SLABS = (
    (10, 3, ((20, 25), (21, 4), (29, 12), (11, 29), (9, 1), (30, 7))),
    (40, 30, ((40, 50), (41, 20), (79, 45), (1, 100))),
    (40, 32, ((80, 45), (41, 90), (39, 43), (85, 12))),
)


def window_cases(X):
    """rows with one zero each (row_zeros) at radius 56 (cap 57: the last on the bit-window kernels) and 57 (the log-step kernel):
    alone (one row per plane, one plane per z-block), with a zero-free second row behind the y scan, with a zero-free second plane
    behind the z scan, and all of it through the separate x pass too.  The x distance stays the binding one in each."""
    n = len(row_zeros(X))
    small = X == 57  # the reference can keep (next to) nothing of a row this short
    out = []
    for r, sw, tag in ((56, (), ""), (57, (), ""), (56, SPLIT, "split_")):
        out.append(case(f"{tag}x_alone_r{r}", (n, 1, X), r, zblock=1, zeros="rows", switches=sw, exempt=small))
        out.append(case(f"{tag}y_scan_r{r}", (n, 2, X), r, zblock=1, zeros="rows_y", switches=sw, exempt=small))
        out.append(case(f"{tag}z_scan_r{r}", (2 * n, 1, X), r, zblock=2, zeros="rows_z", switches=sw, exempt=small))
    return out


def logstep_zeros(X, radius):
    return [(0, 0, 0)] if radius > 200 else [(0, 0, 0), (2, 3, X - 1)]


def all_cases():
    """every case of the GPU module, by family (the GPU tests and the CPU checks of the helper walk the same table)"""
    f = {}
    f["xy_chunks"] = [case(f"X{X}", (2, 3, X), 30) for X in XY_CHUNK_X]
    f["xy_small"] = [case(f"X{X}", (4, 6, X), 3) for X in XY_SMALL_X]
    f["xy_rows"] = [case(f"Y{Y}_X{X}", (3, Y, X), 3) for Y in XY_ROWS_Y for X in (24, 13)]
    f["xy_padding"] = [case("X16_Xp19", (3, 4, 16), 3, pad=(0, 3)), case("X13_Xp16", (3, 4, 13), 3, pad=(0, 3))]
    f["windows"] = [c._replace(name=f"X{X}_{c.name}") for X in WINDOW_X for c in window_cases(X)]
    f["split"] = [case(f"split_X{X}", (3, 4, X), 3, switches=SPLIT) for X in (24, 13)] + \
                 [case(f"unswitched_X{X}", (3, 5, X), 30) for X in (8193, 8200)]
    f["logstep"] = [case(f"r{r}_X{X}", (3, 4, X), r, zeros=logstep_zeros(X, r)) for r in (57, 100, 253) for X in (300, 301)]
    f["z_depth"] = [case(f"X{X}_r{r}{'_two' if sw else ''}_Z{Z}", (Z, 5, X), r, switches=sw, zeros="corner", exempt=r == 0 or (Z <= 5 and r >= 30))
                    for X in (8, 7) for r, sw in Z_RADII for Z in z_depths(r)]
    f["z_blocks"] = [case(f"X{X}_r{r}{'_two' if sw else ''}_zb{b}", (2 * r + 3, 5, X), r, zblock=b, switches=sw)
                     for X in (8, 7) for r, sw in ((3, ()), (30, ()), (32, ()), (3, TWO)) for b in z_blocks_of(r, 2 * r + 3)]
    f["z_slabs"] = [case(f"X{X}_r{r}{'_two' if sw else ''}_zb{b}_at{z0}_nz{nz}", (nz, 5, X), r, zblock=b, z_abs0=z0, switches=sw,
                         exempt=r >= 30 and nz <= 20)
                    for X in (8, 7) for b, r, slabs in SLABS for sw in ((), TWO) for z0, nz in slabs if not (sw and r > 31)]
    f["acc_unaligned"] = [case(f"X8_Xp{8 + p}_r3", (9, 5, 8), 3, pad=(0, p)) for p in (2, 4)] + \
                         [case("X8_Xp10_r31", (70, 5, 8), 31, pad=(0, 2), zeros="corner")]
    f["padding"] = [case("X16_Xp19", (3, 5, 16), 3, pad=(2, 3)), case("X13_Xp16", (3, 5, 13), 3, pad=(1, 3)),
                    case("X2056_Xp2064", (2, 3, 2056), 30, pad=(1, 8)), case("X24_Xp27_two", (3, 5, 24), 3, pad=(1, 3), switches=TWO),
                    case("X300_r57", (3, 4, 300), 57, pad=(1, 4), zeros=logstep_zeros(300, 57))]
    f["decision"] = [case(f"X{X}{'_two' if sw else ''}_t{t}_{'cnt' if cnt else 'nocnt'}", (4, 6, X), 1, threshold=t, cnt=cnt, switches=sw)
                     for X in (24, 23) for sw in ((), TWO) for t in THRESHOLDS for cnt in (True, False)]
    f["guards"] = [case(f"X{X}", (3, 4, X), 3 if X < 100 else 30) for X in (13, 16, 2056)]
    return f


def coverage(records):
    """what the issue wants the asserted launch records to cover, as a set of missing items"""
    want = {("xy", 0, nc) for nc in (1, 2, 4)} | {("xy", f, v) for f in (1, 2) for v in (4, 1)} | {("z", f, v) for f in (0, 1) for v in (4, 1)}
    want |= {(k, v) for k in ("raw_vec", "dist_vec", "acc_vec") for v in (0, 1)} | {"zphase"}
    seen = set()
    for r in records:
        seen.add(("xy", r["xy_form"], r["nc"] if r["xy_form"] == 0 else r["y_v"]))
        seen.add(("z", r["z_form"], r["z_v"]))
        seen |= {(k, r[k]) for k in ("raw_vec", "dist_vec", "acc_vec")}
        if r["zphase"]:
            seen.add("zphase")
    return want - seen
