"""The reference of dlv_fill_holes_u8_dev (include/delivr_hip.h; INTEGRATION "Filling holes"), for tests/test_fill_holes_cpu.py and
tests/test_gpu_fill_holes.py: scipy.ndimage.binary_fill_holes(mask != 0) with its default structure, the volumes the tests share,
and `fill_by_gaps`, the restatement in plain Python of the way csrc/fill_holes.hip gets there (gaps of rows, union-find with an
"outside" node) - pinned against scipy on the host so that a difference on the device is the kernels' and not the method's."""
import numpy as np
from scipy import ndimage


def fill_reference(mask: np.ndarray):
    """(filled bool volume, voxels_filled, holes): holes = the 6-connected components of what the fill added"""
    fg = np.asarray(mask) != 0
    filled = ndimage.binary_fill_holes(fg)
    added = filled & ~fg
    return filled, int(added.sum()), int(ndimage.label(added)[1])


def expected_bytes(mask: np.ndarray, fill_value: int) -> np.ndarray:
    """the mask after dlv_fill_holes_u8_dev: hole voxels == fill_value, every other byte as before"""
    filled = fill_reference(mask)[0]
    out = np.array(mask, dtype=np.uint8)
    out[filled & (out == 0)] = fill_value
    return out


def label26(mask: np.ndarray):
    """26-connected components of mask != 0 -> (uint32 labels 1..n in C-raster order of each component's first voxel, n) - the
    numbering of dlv_ccl26_dev (scipy numbers in the same order: by the first voxel it meets)"""
    lab, n = ndimage.label(np.asarray(mask) != 0, structure=np.ones((3, 3, 3), dtype=bool))
    return lab.astype(np.uint32), int(n)


def ball(shape, centre, radius) -> np.ndarray:
    """the voxels within Euclidean distance `radius` of `centre`, as a bool volume"""
    zz, yy, xx = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return (zz - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (xx - centre[2]) ** 2 <= radius * radius


def shell(shape, centre, radius, wall=2) -> np.ndarray:
    """a hollow ball: the ball of `radius` without the ball of radius - wall"""
    return ball(shape, centre, radius) & ~ball(shape, centre, radius - wall)


def three_hollow_balls(X: int = 83) -> np.ndarray:
    """(21, 23, X): radii 8, 8, 9, walls 2 thick; the balls straddle the 16-voxel chunks of a row.  3269 voxels in 3 holes"""
    shape = (21, 23, X)
    return shell(shape, (10, 11, 12), 8) | shell(shape, (10, 11, 40), 8) | shell(shape, (10, 11, 66), 9)


def cube_shell(kink: int = 0) -> np.ndarray:
    """(9, 9, 17).  kink 0: a 7^3 cube shell around a 5^3 cavity.  kink 1: the wall towards +x is 3 thick and a tunnel leaves the
    cavity at [4,4,7], then goes on at [4,5,8], [4,5,9]: it turns over an edge, so the cavity is sealed.  kink 2: [4,4,8] cleared
    as well: the tunnel is face-connected and opens the cavity"""
    m = np.zeros((9, 9, 17), dtype=bool)
    m[1:8, 1:8, 1:(10 if kink else 8)] = True
    m[2:7, 2:7, 2:7] = False
    if kink:
        m[4, 4, 7] = m[4, 5, 8] = m[4, 5, 9] = False
    if kink == 2:
        m[4, 4, 8] = False
    return m


def cup(face: int) -> np.ndarray:
    """(9, 9, 9): a 7^3 cube shell pushed against face 0..5 (z0, z1, y0, y1, x0, x1) of the volume with the wall on that face taken
    away: the cavity is open to the outside, nothing is filled"""
    axis, far = divmod(face, 2)
    m = np.zeros((9, 9, 9), dtype=bool)
    outer = [slice(1, 8)] * 3
    inner = [slice(2, 7)] * 3
    outer[axis] = slice(2, 9) if far else slice(0, 7)
    inner[axis] = slice(3, 9) if far else slice(0, 6)
    m[tuple(outer)] = True
    m[tuple(inner)] = False
    return m


def nested() -> np.ndarray:
    """(25, 25, 40): a shell of radius 11 (wall 2) around a shell of radius 5 (wall 2) at (12, 12, 14), and a solid ball of radius 3
    at (12, 12, 32).  2679 voxels filled; 3 components before, 2 after: the inner shell is swallowed"""
    shape = (25, 25, 40)
    return shell(shape, (12, 12, 14), 11) | shell(shape, (12, 12, 14), 5) | ball(shape, (12, 12, 32), 3)


def dense_random(shape, p: float, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).random(shape) < p


def random_hollow_balls(seed: int = 1, shape=(40, 48, 150), count: int = 60, knock_out: float = 0.03) -> np.ndarray:
    """`count` balls of radius 2..7, 70 % of them hollow with walls 2 thick, then `knock_out` of the foreground cleared: most
    shells leak through a missing voxel, some only over an edge"""
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, dtype=bool)
    for _ in range(count):
        r = int(rng.integers(2, 8))
        c = tuple(int(rng.integers(0, s)) for s in shape)
        m |= shell(shape, c, r) if (rng.random() < 0.7 and r > 2) else ball(shape, c, r)
    fg = np.flatnonzero(m)
    m.ravel()[rng.choice(fg, size=int(len(fg) * knock_out), replace=False)] = False
    return m


def checkerboard(shape=(16, 16, 64), planes: bool = True) -> np.ndarray:
    """planes: (z + y + x) even - every row has X / 2 gaps of one voxel, and a background voxel that is not on a face of the volume
    has six foreground face neighbours: it is a hole of its own (6076 of them in the default shape).  Not planes: (y + x) even in
    every plane - the same rows, but every background voxel reaches both z faces along its column: nothing is filled"""
    zz, yy, xx = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return ((zz if planes else 0 * zz) + yy + xx) % 2 == 0


def boxed_checkerboard(shape=(16, 16, 64), planes: bool = True) -> np.ndarray:
    """the checkerboard inside a solid box wall one voxel thick: every background voxel inside is filled"""
    m = checkerboard(shape, planes)
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = (True,) * 6
    return m


# ---- the method of csrc/fill_holes.hip in plain Python ---------------------------------------------------------------------------
def row_gaps(row: np.ndarray):
    """(first, last, [(x0, x1), ...]) of one row: its foreground extent and its gaps - the background stretches with foreground on
    both sides; (None, None, []) for a row without foreground"""
    fg = np.flatnonzero(row)
    if not len(fg):
        return None, None, []
    cut = np.flatnonzero(np.diff(fg) > 1)
    return int(fg[0]), int(fg[-1]), [(int(fg[k]) + 1, int(fg[k + 1]) - 1) for k in cut]


def fill_by_gaps(mask: np.ndarray):
    """(filled bool volume, voxels_filled, holes, gaps) the way the device works: node 0 is the outside, a gap joins the outside
    through a neighbour row (z +- 1 or y +- 1) that lies outside the volume or whose extent does not cover it, and joins the
    overlapping gaps of the two neighbour rows that precede it; the gaps whose root is not 0 are written"""
    fg = np.asarray(mask) != 0
    Z, Y, X = fg.shape
    ext, start, gaps = {}, {}, []
    for z in range(Z):
        for y in range(Y):
            first, last, g = row_gaps(fg[z, y])
            ext[z, y] = (first, last)
            start[z, y] = (len(gaps), len(gaps) + len(g))
            gaps += [(z, y, a, b) for a, b in g]
    parent = list(range(len(gaps) + 1))

    def find(i):
        while parent[i] != i:
            i = parent[i]
        return i

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for g, (z, y, a, b) in enumerate(gaps):
        for k, (dz, dy) in enumerate(((-1, 0), (0, -1), (0, 1), (1, 0))):
            zz, yy = z + dz, y + dy
            if not (0 <= zz < Z and 0 <= yy < Y):
                union(g + 1, 0)
                continue
            first, last = ext[zz, yy]
            if first is None or not (first <= a and b <= last):
                union(g + 1, 0)
            if k < 2:
                for j in range(*start[zz, yy]):
                    if gaps[j][2] <= b and a <= gaps[j][3]:
                        union(g + 1, j + 1)
    filled = fg.copy()
    voxels = holes = 0
    for g, (z, y, a, b) in enumerate(gaps):
        root = find(g + 1)
        if root:
            filled[z, y, a:b + 1] = True
            voxels += b - a + 1
            holes += root == g + 1
    return filled, voxels, holes, len(gaps)
