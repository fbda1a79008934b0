"""Masks for the per-path tests of the 26-connected labelling (tests/test_ccl_cases_cpu.py pins the reference on them,
tests/test_gpu_ccl_kernels.py judges csrc/ccl.hip by it), and a second reference that uses nothing third-party: a plain flood
fill over the 26 neighbours that numbers the components by their first voxel in raster order.

Every builder returns a read-only uint8 mask; those whose number of components is known by construction return it beside the
mask."""
import itertools

import numpy as np

OFFSETS26 = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
# the 13 neighbours (dz, dy, dx) that precede a voxel in raster order: what every merge kernel unites a voxel with
PRECEDING13 = [o for o in OFFSETS26 if o < (0, 0, 0)]
assert len(PRECEDING13) == 13

GROUP_VOXELS = 1024 * 4096  # voxels of one group of the two-level scan: 1024 blocks of 4096 (csrc/dev_scan.h: SCAN_GROUP, csrc/ccl.hip: RCHUNK)


def _done(mask):
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    mask.setflags(write=False)
    return mask


def flood_fill26(mask: np.ndarray):
    """26-connected components of mask != 0 -> (uint32 labels 1..n in C-raster order of each component's first voxel, n)"""
    Z, Y, X = mask.shape
    pad = np.zeros((Z + 2, Y + 2, X + 2), dtype=bool)
    pad[1:-1, 1:-1, 1:-1] = mask != 0
    todo = pad.ravel().copy()
    sy, sz = X + 2, (Y + 2) * (X + 2)
    steps = [dz * sz + dy * sy + dx for dz, dy, dx in OFFSETS26]
    out = np.zeros(pad.size, dtype=np.uint32)
    n = 0
    for start in np.flatnonzero(todo):  # raster order
        if not todo[start]:
            continue
        n += 1
        todo[start] = False
        out[start] = n
        stack = [int(start)]
        while stack:
            i = stack.pop()
            for s in steps:
                j = i + s
                if todo[j]:
                    todo[j] = False
                    out[j] = n
                    stack.append(j)
    return out.reshape(pad.shape)[1:-1, 1:-1, 1:-1].copy(), n


def pair_volume(X: int, xs, twin: bool = False):
    """K blocks of three planes (3, X), one pair of voxels each: A at (z0 + 1, 1, x) for x in xs, B at one of the 13 preceding
    offsets (a pair whose B lies outside the row is left out).  Blocks are two planes apart from the next block's voxels, so the
    volume has K components of 2 voxels, in raster order block by block.
    twin: only the offsets with dx = +-1, stretched to dx = +-2 - B no longer touches A: two components per block.
    -> (mask (3 K, 3, X), number of components, K)"""
    pairs = []
    for x in xs:
        for dz, dy, dx in PRECEDING13:
            if twin:
                if dx == 0:
                    continue
                dx *= 2
            if 0 <= x + dx < X:
                pairs.append((x, dz, dy, dx))
    K = len(pairs)
    mask = np.zeros((3 * K, 3, X), dtype=np.uint8)
    for k, (x, dz, dy, dx) in enumerate(pairs):
        mask[3 * k + 1, 1, x] = 1
        mask[3 * k + 1 + dz, 1 + dy, x + dx] = 1
    assert int(mask.sum()) == 2 * K
    return _done(mask), (2 * K if twin else K), K


def random_mask(shape, density: float, seed: int):
    rng = np.random.default_rng([seed, int(round(density * 1000)), *shape])
    return _done(rng.random(shape) < density)


def comb(shape):
    """every second column x = 0, 2, 4, ... over all rows but the last, which is full: the teeth meet in the last row of a plane
    only, after each has been united along its own length -> 1 component"""
    mask = np.zeros(shape, dtype=np.uint8)
    mask[:, :, ::2] = 1
    mask[:, -1, :] = 1
    return _done(mask), 1


def snake(shape):
    """one-voxel-wide path: in every second plane the rows y = 0, 2, 4, ... joined by one connector voxel at alternating ends
    (x = X - 1, 0, X - 1, ...); the planes between hold one voxel, under the end of the path above it -> 1 component"""
    Z, Y, X = shape
    mask = np.zeros(shape, dtype=np.uint8)
    mask[::2, ::2, :] = 1
    ends = [X - 1 if (y // 2) % 2 == 0 else 0 for y in range(1, Y, 2)]
    for y, x in zip(range(1, Y, 2), ends):
        if y + 1 < Y:
            mask[::2, y, x] = 1
    last_row = (Y - 1) // 2 * 2
    x_end = X - 1 if (last_row // 2) % 2 == 0 else 0  # the far end of the last row (row 0 runs from x = 0 to X - 1, row 2 back, ...)
    mask[1::2, last_row, x_end] = 1
    return _done(mask), 1


def checkerboard(shape):
    """(x + y + z) % 2 == 0: no two voxels share a face, every voxel touches others over edges -> 1 component (shape >= 2 in two
    axes), with as many unions per voxel as the neighbourhood allows"""
    z, y, x = np.indices(shape)
    return _done((x + y + z) % 2 == 0), 1


def lattice2(shape):
    """pitch-2 lattice: every voxel with even z, y and x, none touching another -> ceil(Z/2) ceil(Y/2) ceil(X/2) components"""
    mask = np.zeros(shape, dtype=np.uint8)
    mask[::2, ::2, ::2] = 1
    Z, Y, X = shape
    return _done(mask), ((Z + 1) // 2) * ((Y + 1) // 2) * ((X + 1) // 2)


def group_boundary_specks(shape):
    """nothing but the two voxels on either side of linear index GROUP_VOXELS (they lie in different planes: two components) - the
    first scan group is empty up to its very last voxel"""
    mask = np.zeros(int(np.prod(shape)), dtype=np.uint8)
    assert mask.size > GROUP_VOXELS
    mask[GROUP_VOXELS - 1] = 1
    mask[GROUP_VOXELS] = 1
    return _done(mask.reshape(shape)), 2


def nonempty_chunks(mask: np.ndarray) -> int:
    """16-voxel chunks (linear index) that hold foreground: what ccl_init_kernel lists"""
    flat = mask.ravel() != 0
    flat = np.concatenate([flat, np.zeros(-flat.size % 16, dtype=bool)])
    return int(flat.reshape(-1, 16).any(axis=1).sum())


# (builder, shape at an X that is a multiple of 16, shape at one that is not): the late-merge / contention cases
LATE_MERGE_CASES = {
    "comb": (comb, (6, 40, 64), (6, 40, 63)),
    "snake": (snake, (4, 16, 32), (4, 16, 31)),
    "checkerboard": (checkerboard, (5, 6, 32), (5, 6, 33)),
    "lattice2": (lattice2, (5, 7, 48), (5, 7, 45)),
}

RANDOM_DENSITIES = (0.05, 0.1, 0.3, 0.5, 0.9)
RANDOM_SEEDS = (0, 1, 2)
RANDOM_SHAPES_ROWS = ((5, 6, 16), (4, 5, 48), (6, 7, 64))   # X % 16 == 0: the row-window merge
RANDOM_SHAPES_VOXEL = ((5, 6, 15), (4, 5, 17), (3, 7, 33))  # the per-voxel merge
RANDOM_SHAPES_DEGENERATE = ((1, 1, 64), (1, 9, 32), (7, 1, 16), (1, 1, 1))

PAIR_XS = {32: (0, 15, 16, 31), 33: (0, 15, 16, 17, 32)}  # A's x: both sides of the 16-voxel chunk edges, and the row's ends


def seam_planes(Y: int, X: int, seed: int):
    """two label planes (uint32) with blobby random labels - 2 x 3 patches of one label, about half of them background, other labels
    in b than in a - and two label pairs that touch ONLY diagonally: a's corner voxel (0, 0) with b's (1, 1), and a's (Y - 1, X - 2)
    on the last row with b's (Y - 2, X - 1) on the last column.  -> (a, b, the two pairs)"""
    rng = np.random.default_rng([seed, Y, X])

    def blobs(first):
        coarse = rng.integers(first, first + 40, size=((Y + 1) // 2, (X + 2) // 3)).astype(np.uint32)
        coarse[rng.random(coarse.shape) < 0.5] = 0
        return np.repeat(np.repeat(coarse, 2, axis=0), 3, axis=1)[:Y, :X].copy()

    a, b = blobs(1), blobs(101)
    for p in (a, b):
        p[:3, :3] = 0
        p[Y - 3:, X - 3:] = 0
    a[0, 0], b[1, 1] = 901, 902
    a[Y - 1, X - 2], b[Y - 2, X - 1] = 903, 904
    for p in (a, b):
        p.setflags(write=False)
    return a, b, {(901, 902), (903, 904)}


def seam_pairs_brute(a: np.ndarray, b: np.ndarray):
    """every (label in a, label in b) over the 9 (dy, dx) neighbours, both non-zero -> (set of pairs, number of such neighbour pairs)"""
    Y, X = a.shape
    pairs, total = set(), 0
    for y in range(Y):
        for x in range(X):
            if not a[y, x]:
                continue
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < Y and 0 <= xx < X and b[yy, xx]:
                        pairs.add((int(a[y, x]), int(b[yy, xx])))
                        total += 1
    return pairs, total
