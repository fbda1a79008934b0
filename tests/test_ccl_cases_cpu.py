"""The reference of tests/test_gpu_ccl_kernels.py checked before the kernels are judged by it: oracle.delivr_oracle.ccl26 (scipy)
against the plain flood fill of tests/helpers/ccl_cases.py on every mask builder at its small shape, and against the numbers of
components that the builders give by construction."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import delivr_oracle as orc


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = _helper("ccl_cases")


def _both(mask):
    """the two references agree on the whole label volume and on n -> (labels, n)"""
    lab, n = orc.ccl26(mask)
    ff, nff = cases.flood_fill26(mask)
    assert lab.dtype == np.uint32 and ff.dtype == np.uint32
    assert n == nff
    np.testing.assert_array_equal(lab, ff)
    assert ((lab != 0) == (mask != 0)).all()
    return lab, n


@pytest.mark.parametrize("twin", [False, True])
@pytest.mark.parametrize("X", sorted(cases.PAIR_XS))
def test_pair_volumes_have_one_component_per_pair_or_two_per_stretched_pair(X, twin):
    mask, n_want, K = cases.pair_volume(X, cases.PAIR_XS[X], twin=twin)
    assert mask.shape == (3 * K, 3, X)
    # 13 offsets per x, less those that leave the row: 5 with dx = -1 at x = 0, 4 with dx = +1 at x = X - 1; the twin has the 9
    # offsets with dx != 0, and dx = +-2 leaves the row at neither 15, 16 nor 17
    nx = len(cases.PAIR_XS[X])
    assert K == (9 * nx - 5 - 4 if twin else 13 * nx - 5 - 4)
    lab, n = _both(mask)
    assert n == n_want
    counts = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    assert (counts == (1 if twin else 2)).all()
    per_block = lab.reshape(K, -1).max(axis=1)  # raster order: block k holds label k + 1 (pairs), 2 k + 1 and 2 k + 2 (twins)
    np.testing.assert_array_equal(per_block, (np.arange(K) + 1) * (2 if twin else 1))


@pytest.mark.parametrize("shape", cases.RANDOM_SHAPES_ROWS + cases.RANDOM_SHAPES_VOXEL + cases.RANDOM_SHAPES_DEGENERATE)
def test_random_masks(shape):
    seen = set()
    for density in cases.RANDOM_DENSITIES:
        for seed in cases.RANDOM_SEEDS:
            mask = cases.random_mask(shape, density, seed)
            assert mask.shape == shape
            seen.add(mask.tobytes())
            _both(mask)
    assert len(seen) > 1 or shape == (1, 1, 1)


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("name", sorted(cases.LATE_MERGE_CASES))
def test_late_merge_masks_have_the_components_of_their_construction(name, which):
    build = cases.LATE_MERGE_CASES[name][0]
    shape = cases.LATE_MERGE_CASES[name][which]
    assert (shape[2] % 16 == 0) == (which == 1)
    mask, n_want = build(shape)
    assert mask.shape == shape
    lab, n = _both(mask)
    assert n == n_want
    if name == "lattice2":
        Z, Y, X = shape
        assert n == -(-Z // 2) * -(-Y // 2) * -(-X // 2) == int(mask.sum())
    else:
        assert n == 1


def test_snake_is_a_path():
    """one voxel wide: full rows two apart, one connector voxel between them at alternating ends, and the planes between the snake
    planes hold one voxel - without a connector, or without that voxel, the components fall apart"""
    mask, _ = cases.snake((4, 16, 32))
    plane = mask[0]
    assert (plane[::2] == 1).all() and plane[15].sum() == 0
    assert plane[1:15:2].sum(axis=1).tolist() == [1] * 7
    assert np.flatnonzero(plane[1:15:2].any(axis=0)).tolist() == [0, 31]
    assert [int(np.flatnonzero(r)[0]) for r in plane[1:15:2]] == [31, 0, 31, 0, 31, 0, 31]
    assert mask[1].sum() == 1 and mask[3].sum() == 1 and mask[1, 14, 0] == 1
    cut = mask.copy()
    cut[0, 5, 31] = 0
    assert orc.ccl26(cut)[1] == 2  # (rows 0 .. 4 of plane 0 reach the rest through this connector alone)
    cut[2, 5, 31] = 0
    assert orc.ccl26(cut)[1] == 3
    cut = mask.copy()
    cut[1] = 0
    assert orc.ccl26(cut)[1] == 2
    np.testing.assert_array_equal(mask[0], mask[2])


def test_group_boundary_specks_small():
    """the builder on a flat shape (the flood fill is too slow for the 17 x 512 x 512 of the GPU test): two voxels, two planes"""
    mask, n_want = cases.group_boundary_specks((2, 1, cases.GROUP_VOXELS))
    assert n_want == 2 and int(mask.sum()) == 2
    assert mask[0, 0, -1] == 1 and mask[1, 0, 0] == 1
    mask, _ = cases.group_boundary_specks((17, 512, 512))
    idx = np.flatnonzero(mask.ravel())
    np.testing.assert_array_equal(idx, [cases.GROUP_VOXELS - 1, cases.GROUP_VOXELS])
    z, y, x = np.unravel_index(idx, mask.shape)
    assert abs(int(y[0]) - int(y[1])) > 1  # not neighbours
    lab, n = orc.ccl26(mask)
    assert n == 2 and lab.ravel()[idx].tolist() == [1, 2]


def test_nonempty_chunks_counts_by_linear_index():
    mask = np.zeros((1, 3, 11), dtype=np.uint8)  # 33 voxels: chunks [0, 16), [16, 32), [32, 33)
    assert cases.nonempty_chunks(mask) == 0
    mask[0, 2, 10] = 1  # voxel 32
    assert cases.nonempty_chunks(mask) == 1
    mask[0, 1, 4] = mask[0, 1, 5] = 1  # voxels 15 and 16
    assert cases.nonempty_chunks(mask) == 3


@pytest.mark.parametrize("Y,X", [(5, 7), (16, 16), (9, 33)])
def test_seam_planes_hold_their_diagonal_only_pairs(Y, X):
    a, b, diagonal = cases.seam_planes(Y, X, seed=0)
    assert a.shape == b.shape == (Y, X) and a.dtype == b.dtype == np.uint32
    pairs, total = cases.seam_pairs_brute(a, b)
    assert diagonal <= pairs and total >= len(pairs) > len(diagonal)
    # diagonal only: the voxel straight below a's voxel, and its row and column neighbours, are background in b
    assert b[0, 0] == 0 and b[0, 1] == 0 and b[1, 0] == 0 and b[1, 1] == 902
    assert b[Y - 1, X - 2] == 0 and b[Y - 1, X - 1] == 0 and b[Y - 2, X - 2] == 0 and b[Y - 2, X - 1] == 904
    assert (a == 901).sum() == (b == 902).sum() == (a == 903).sum() == (b == 904).sum() == 1
