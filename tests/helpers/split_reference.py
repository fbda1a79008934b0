"""numpy restatement of dlv_cc_split_dev's definition (include/delivr_hip.h; INTEGRATION "Splitting fused cells"), for
tests/test_split_cpu.py and tests/test_gpu_split.py: padded shifted views for the erosion and the growth, a plain flood fill for
the labelling - nothing third-party.  `grow_direct` is the second form for tiny volumes: a breadth-first search per voxel through
the voxel's own label, which takes the smallest core label at the minimal 26-step distance."""
import itertools

import numpy as np

NONE = np.uint32(0xFFFFFFFF)
OFFSETS26 = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]


def label26(mask: np.ndarray):
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


def erode6(mask: np.ndarray, depth: int) -> np.ndarray:
    """C_depth: `depth` steps with the 6 face neighbours, outside the volume counting as background"""
    C = mask != 0
    Z, Y, X = C.shape
    for _ in range(depth):
        P = np.pad(C, 1, constant_values=False)
        C = (P[1:-1, 1:-1, 1:-1] & P[:-2, 1:-1, 1:-1] & P[2:, 1:-1, 1:-1] & P[1:-1, :-2, 1:-1] & P[1:-1, 2:, 1:-1]
             & P[1:-1, 1:-1, :-2] & P[1:-1, 1:-1, 2:])
    return C


def core_labels(L: np.ndarray, depth: int, min_core: int = 1):
    """(Q, M): the cores of L labelled 1..M; with min_core > 1 those of fewer voxels removed and the rest renumbered in order"""
    Q, M = label26(erode6(L, depth))
    if min_core > 1 and M:
        sizes = np.bincount(Q.ravel(), minlength=M + 1)
        keep = sizes >= min_core
        keep[0] = False
        lut = np.where(keep, np.cumsum(keep), 0).astype(np.uint32)
        Q, M = lut[Q], int(keep.sum())
    return Q.astype(np.uint32), M


def grow(L: np.ndarray, Q: np.ndarray):
    """(G, steps): the fixed point of the synchronous growth of Q inside the labels of L, and the number of steps that changed a
    voxel"""
    Z, Y, X = L.shape
    G = Q.astype(np.uint32)
    PL = np.pad(L.astype(np.int64), 1, constant_values=-1)  # (outside the volume: a label nobody has)
    steps = 0
    while True:
        PG = np.pad(np.where(G == 0, NONE, G), 1, constant_values=NONE)
        m = np.full(L.shape, NONE, dtype=np.uint32)
        for dz, dy, dx in itertools.product(range(3), repeat=3):
            same = PL[dz:dz + Z, dy:dy + Y, dx:dx + X] == L
            np.minimum(m, np.where(same, PG[dz:dz + Z, dy:dy + Y, dx:dx + X], NONE), out=m)
        nxt = np.where(G != 0, G, np.where((L != 0) & (m != NONE), m, 0)).astype(np.uint32)
        if np.array_equal(nxt, G):
            return G, steps
        G = nxt
        steps += 1


def grow_direct(L: np.ndarray, Q: np.ndarray) -> np.ndarray:
    """G voxel by voxel: breadth-first through the voxel's own label, the smallest core label in the first level that holds one"""
    Z, Y, X = L.shape
    G = np.zeros(L.shape, dtype=np.uint32)
    for v in zip(*np.nonzero(L)):
        seen = {v}
        level = [v]
        while level:
            hit = [int(Q[u]) for u in level if Q[u]]
            if hit:
                G[v] = min(hit)
                break
            nxt = []
            for z, y, x in level:
                for dz, dy, dx in OFFSETS26:
                    u = (z + dz, y + dy, x + dx)
                    if 0 <= u[0] < Z and 0 <= u[1] < Y and 0 <= u[2] < X and u not in seen and L[u] == L[v]:
                        seen.add(u)
                        nxt.append(u)
            level = nxt
    return G


def pieces(L: np.ndarray, G: np.ndarray, Q: np.ndarray, M: int, n: int):
    """(out, K, parent, n_split) from the grown cores: the keys, numbered in C-raster order of their first voxel"""
    L = L.astype(np.uint32)
    comp = np.zeros(M + 1, dtype=np.int64)
    comp[Q[Q != 0]] = L[Q != 0]
    if M:
        assert (L[Q != 0] == comp[Q[Q != 0]]).all()  # a core lies inside one label
    cores = np.bincount(comp[1:], minlength=n + 1)
    key = np.where(L == 0, 0, np.where((cores[L] >= 2) & (G != 0), G.astype(np.int64), M + L.astype(np.int64)))
    flat = key.ravel()
    keys, first = np.unique(flat, return_index=True)
    keys, first = keys[keys != 0], first[keys != 0]
    order = np.argsort(first)
    lut = {0: 0}
    parent = np.zeros(len(keys) + 1, dtype=np.uint32)
    Lf = L.ravel()
    for new, j in enumerate(order, 1):
        lut[int(keys[j])] = new
        parent[new] = Lf[first[j]]
    out = np.vectorize(lut.get, otypes=[np.uint32])(flat).reshape(L.shape) if len(keys) else np.zeros(L.shape, np.uint32)
    return out, len(keys), parent, int((cores[1:] >= 2).sum())


def split_reference(L: np.ndarray, n: int, depth: int, min_core: int = 1, direct: bool = False) -> dict:
    """The whole definition -> {"out": uint32 volume, "K", "parent": uint32 (K+1), "n_split", "M" (cores), "steps" (growth steps that
    changed a voxel; None with direct), "max_cores" (the most cores in one label)}"""
    L = np.asarray(L).astype(np.uint32)
    Q, M = core_labels(L, depth, min_core)
    if direct:
        G, steps = grow_direct(L, Q), None
    else:
        G, steps = grow(L, Q)
    out, K, parent, n_split = pieces(L, G, Q, M, n)
    comp = np.zeros(M + 1, dtype=np.int64)
    comp[Q[Q != 0]] = L[Q != 0]
    max_cores = int(np.bincount(comp[1:], minlength=n + 1).max()) if M else 0
    return {"out": out, "K": K, "parent": parent, "n_split": n_split, "M": M, "steps": steps, "max_cores": max_cores}


def ball(shape, centre, radius) -> np.ndarray:
    """the voxels within Euclidean distance `radius` of `centre`, as a bool volume"""
    zz, yy, xx = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return (zz - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (xx - centre[2]) ** 2 <= radius * radius
