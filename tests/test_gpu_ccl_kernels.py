"""Every path of the 26-connected labelling (csrc/ccl.hip) alone against a reference: the row-window merge and the per-voxel merge
at the edges of the 16-voxel chunks, late merges and contention, the renumbering across scan groups, the mid-loop flush of
ccl_init_kernel, unaligned mask and label pointers, the seam kernel and the lookup-table kernels.

The reference of every labelling is oracle.delivr_oracle.ccl26, which tests/test_ccl_cases_cpu.py checks against a plain flood
fill and against the numbers of components the masks have by construction (tests/helpers/ccl_cases.py builds them).  Everything is
an integer: the whole label volume and n are compared for equality.  Each case also asserts, through HipEngine.ccl_ran()
(dlv_diag_ccl_ran: recorded at the launch sites of dlv_ccl26_dev), that it ran the path it is named for."""
import ctypes as C
import importlib.util
import os
from contextlib import contextmanager

import numpy as np
import pytest

from oracle import delivr_oracle as orc

pytestmark = pytest.mark.gpu

DEAD = 0xDEADBEEF
DEAD_I32 = DEAD - (1 << 32)


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = _helper("ccl_cases")


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


@contextmanager
def _switch(eng, name, value):
    eng.diag_set(name, value)
    try:
        yield
    finally:
        eng.diag_set(name, 0)


def _label(eng, mask):
    """HipEngine.ccl26 on an aligned copy of the mask -> (uint32 labels on the host, n, the launch record)"""
    import torch

    t = torch.from_numpy(np.array(mask, dtype=np.uint8)).cuda()
    assert t.data_ptr() % 16 == 0
    lab, n = eng.ccl26(t)
    assert lab.data_ptr() % 16 == 0
    return lab.cpu().numpy().view(np.uint32), n, eng.ccl_ran()


def _check(eng, mask, rows, n_want=None):
    """the labelling of `mask` equals the reference; it ran the row-window merge (rows) or the per-voxel merge, with 16-byte
    accesses and the list relabel, over the chunks and blocks numpy counts -> (labels, n, launch record)"""
    labels, n, ran = _label(eng, mask)
    ref, nref = orc.ccl26(mask)
    if n_want is not None:
        assert nref == n_want
    assert n == nref
    np.testing.assert_array_equal(labels, ref)
    blocks = -(-mask.size // 4096)
    assert ran["aligned"] == 1 and ran["merge_rows"] == int(rows) and ran["relabel"] == 0, ran
    assert ran["list_n"] == cases.nonempty_chunks(mask), ran
    assert ran["blocks"] == blocks and ran["groups"] == -(-blocks // 1024), ran
    assert ran["init_per"] % 256 == 0 and ran["init_per"] * ran["init_grid"] >= -(-mask.size // 16), ran
    return labels, n, ran


# ---- (a) links across the edge of a 16-voxel chunk ----------------------------------------------------------------------------
@pytest.mark.parametrize("X", [32, 33])
def test_pairs_linked_across_chunk_edges(eng, X):
    """One pair of voxels per three-plane block: A at x = 0, 15, 16, 31 (X = 32: the row-window merge, whose 18-bit windows take
    bit 0 and bit 17 from the neighbouring chunks) or 0, 15, 16, 17, 32 (X = 33: the per-voxel merge, chunks straddle rows), B at
    each of the 13 preceding offsets -> one label per block, in raster order; the twin with dx = +-2 -> two labels per block.
    Smallest shape: two 16-voxel chunks per row (X = 32) is the least at which a row has a chunk edge inside it and both a first
    and a last chunk; X = 33 is the least above it that is no multiple of 16."""
    rows = X % 16 == 0
    mask, n_want, K = cases.pair_volume(X, cases.PAIR_XS[X])
    labels, n, _ = _check(eng, mask, rows, n_want)
    assert n == K
    assert (np.bincount(labels.ravel())[1:] == 2).all()
    np.testing.assert_array_equal(labels.reshape(K, -1).max(axis=1), np.arange(K) + 1)
    np.testing.assert_array_equal(np.where(labels.reshape(K, -1) > 0, labels.reshape(K, -1), K + 1).min(axis=1), np.arange(K) + 1)

    twin, n_twin, Kt = cases.pair_volume(X, cases.PAIR_XS[X], twin=True)
    labels, n, _ = _check(eng, twin, rows, n_twin)
    assert n == 2 * Kt
    assert (np.bincount(labels.ravel())[1:] == 1).all()
    np.testing.assert_array_equal(labels.reshape(Kt, -1).max(axis=1), 2 * (np.arange(Kt) + 1))


# ---- (b) "the centre stands for all three" ------------------------------------------------------------------------------------
def _random_case(eng, shape, rows):
    for density in cases.RANDOM_DENSITIES:
        for seed in cases.RANDOM_SEEDS:
            _check(eng, cases.random_mask(shape, density, seed), rows)


@pytest.mark.parametrize("shape", cases.RANDOM_SHAPES_ROWS)
def test_random_masks_row_window_merge(eng, shape):
    """Random masks at densities 0.05 .. 0.9, three seeds each, through ccl_merge_list_kernel<true>: a voxel is united with the
    centre of a neighbour row, or with both diagonal voxels where the centre is background.  Smallest shape: X = 16, one chunk per
    row (no neighbouring chunk on either side); 48 and 64 give rows with inner chunks."""
    _random_case(eng, shape, rows=True)


@pytest.mark.parametrize("shape", cases.RANDOM_SHAPES_VOXEL)
def test_random_masks_per_voxel_merge(eng, shape):
    """The same masks' kin at X = 15, 17 and 33 through ccl_merge_list_kernel<false>: 16-voxel chunks that straddle rows.  Smallest
    shape: X = 15, one less than a chunk."""
    _random_case(eng, shape, rows=False)


@pytest.mark.parametrize("shape", cases.RANDOM_SHAPES_DEGENERATE)
def test_random_masks_degenerate_shapes(eng, shape):
    """One row, one plane, one column of rows, one voxel: no neighbour row above, below or in the plane before.  (1, 1, 1) is the
    smallest volume there is: one partial chunk, the per-voxel merge."""
    _random_case(eng, shape, rows=shape[2] % 16 == 0)


# ---- (c) late merges and contention -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [1, 2], ids=["rows", "voxel"])
@pytest.mark.parametrize("name", sorted(cases.LATE_MERGE_CASES))
def test_late_merges_and_contention(eng, name, which):
    """comb: every second column, joined by the last row alone - each tooth has its own root until then.  snake: a one-voxel-wide
    path through (4, 16, 32), the longest chain of parents a volume of its size can give.  checkerboard: one component in which no
    voxel has a face neighbour, every union is diagonal and all of them contend for one root.  lattice2: a root in every second
    voxel.  Each at an X that is a multiple of 16 (row-window merge) and at one that is not.  Smallest shapes: the issue's (6, 40,
    64) and (4, 16, 32) - more than one 4096-voxel block for the comb; the other two need two chunks per row and an odd Y."""
    build, shape = cases.LATE_MERGE_CASES[name][0], cases.LATE_MERGE_CASES[name][which]
    mask, n_want = build(shape)
    _check(eng, mask, shape[2] % 16 == 0, n_want)


# ---- (d) renumbering across scan groups ---------------------------------------------------------------------------------------
def _groups_lattice():
    return cases.lattice2((18, 512, 512))


def _groups_random():
    return cases.random_mask((17, 512, 512), 0.04, 0), None


def _groups_specks():
    return cases.group_boundary_specks((17, 512, 512))


@pytest.mark.parametrize("build", [_groups_lattice, _groups_random, _groups_specks], ids=["lattice", "random4pc", "boundary_specks"])
def test_renumbering_across_two_scan_groups(eng, build):
    """The two-level scan with two groups (dev_scan_sums / dev_scan_groups / dev_scan_apply, csrc/dev_scan.h): the labels of the second group start
    at the first group's total.  Smallest shape: a group is 1024 blocks of 4096 voxels = 4,194,304 voxels, so 17 planes of 512 x 512
    are the fewest whole planes with a second group (18 for the lattice: 589,824 labels, 1152 blocks).  boundary_specks: nothing
    but voxel 4,194,303 and voxel 4,194,304 - the second group starts at 1, not at 0."""
    mask, n_want = build()
    _, n, ran = _check(eng, mask, rows=True, n_want=n_want)
    assert ran["groups"] == 2, ran
    if build is _groups_lattice:
        assert n == 589824 and ran["blocks"] == 1152


# ---- (e) the mid-loop flush of ccl_init_kernel --------------------------------------------------------------------------------
def _flush_full_8():
    return np.ones((8, 64, 96), dtype=np.uint8)


def _flush_full_12():
    return np.ones((12, 64, 96), dtype=np.uint8)


def _flush_half_12():
    return cases.random_mask((12, 64, 96), 0.5, 0)


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("build", [_flush_full_8, _flush_full_12, _flush_half_12], ids=["full_8x64x96", "full_12x64x96", "half_12x64x96"])
def test_init_flush_inside_the_loop(eng, build, grid):
    """A workgroup of ccl_init_kernel that owns 2048 chunks or more empties its 2048-entry buffer inside its loop (fill > 2048 -
    256).  "ccl_init_grid" = 1 / 2 gives one or two workgroups the whole volume.  Smallest shape: 2048 chunks of foreground =
    32,768 voxels in one workgroup; (8, 64, 96) has 3072 chunks (one workgroup: 3072 each; two: 1536 each, which stays below the
    buffer - that combination checks the switch and the labels only), (12, 64, 96) has 4608 (4608 / 2304 each)."""
    mask = build()
    nch = mask.size // 16
    default_labels, default_n, default_ran = _check(eng, mask, rows=True)
    assert default_ran["init_grid"] == -(-nch // 256)
    with _switch(eng, "ccl_init_grid", grid):
        labels, n, ran = _check(eng, mask, rows=True)
    share = -(-nch // grid)  # chunks per workgroup, rounded up to whole iterations of 256 threads
    assert ran["init_grid"] == grid and ran["init_per"] == -(-share // 256) * 256, ran
    if not (build is _flush_full_8 and grid == 2):
        assert ran["init_per"] >= 2048, ran
    assert ran["list_n"] == default_ran["list_n"] == cases.nonempty_chunks(mask)
    if build is not _flush_half_12:
        assert ran["list_n"] == nch
    assert n == default_n
    np.testing.assert_array_equal(labels, default_labels)
    assert eng.ccl26(eng.to_device(np.array(mask)))[1] == n and eng.ccl_ran()["init_grid"] == default_ran["init_grid"]  # switched off again


# ---- (f) unaligned pointers, through the raw library call ---------------------------------------------------------------------
@pytest.mark.parametrize("simple", [0, 1], ids=["list", "ccl_simple"])
@pytest.mark.parametrize("shape", [(3, 5, 7), (4, 6, 32), (5, 9, 131)])
def test_unaligned_mask_and_label_pointers(eng, shape, simple):
    """A mask that starts 1 or 5 bytes past a 16-byte boundary and labels that start 4, 8 or 12 bytes past one (each also with the
    other pointer aligned): the scalar branch of mask_bits16, the scalar stores of ccl_relabel_list_kernel and, with "ccl_simple",
    ccl_relabel_kernel.  The label buffer is prefilled with 0xDEADBEEF: the background must come out 0 and the words before and
    after the view must keep the prefill.  Smallest shape: (3, 5, 7) = 105 voxels, six whole chunks and a partial one; (4, 6, 32)
    has X % 16 == 0 and must still take the per-voxel merge; (5, 9, 131) has more than one 4096-voxel block."""
    import torch

    Z, Y, X = shape
    nvox = Z * Y * X
    mask = cases.random_mask(shape, 0.3, 7)
    ref, nref = orc.ccl26(mask)
    assert 0 < nref and (ref == 0).any()
    mbuf = torch.zeros(nvox + 48, dtype=torch.uint8, device=eng.device)
    lbuf = torch.empty(nvox + 16, dtype=torch.int32, device=eng.device)
    assert mbuf.data_ptr() % 16 == 0 and lbuf.data_ptr() % 16 == 0
    mask_t = torch.from_numpy(np.array(mask).ravel()).to(eng.device)
    with _switch(eng, "ccl_simple", simple):
        for moff in (16, 17, 21):
            for lword in (4, 5, 6, 7):
                if moff % 16 == 0 and lword % 4 == 0:
                    continue
                mbuf.zero_()
                mbuf[moff:moff + nvox] = mask_t
                lbuf.fill_(DEAD_I32)
                n = C.c_uint64()
                eng._enter()
                eng._check(eng.lib.dlv_ccl26_dev(eng.ctx, C.c_void_p(mbuf.data_ptr() + moff), Z, Y, X, C.c_void_p(lbuf.data_ptr() + 4 * lword),
                                                 C.byref(n)))
                eng._leave()
                ran = eng.ccl_ran()
                assert ran["aligned"] == 0 and ran["merge_rows"] == 0 and ran["relabel"] == (2 if simple else 0), (moff, lword, ran)
                assert ran["list_n"] == cases.nonempty_chunks(mask)
                out = lbuf.cpu().numpy().view(np.uint32)
                assert (out[:lword] == DEAD).all() and (out[lword + nvox:] == DEAD).all(), (moff, lword)
                assert int(n.value) == nref
                np.testing.assert_array_equal(out[lword:lword + nvox].reshape(shape), ref, err_msg=f"mask +{moff % 16} B, labels +{4 * lword % 16} B")


# ---- (g) dlv_seam_pairs_dev, raw ----------------------------------------------------------------------------------------------
def _seam_raw(eng, a, b, Y, X, pairs, cap):
    cnt = C.c_uint64()
    eng._enter()
    eng._check(eng.lib.dlv_seam_pairs_dev(eng.ctx, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), Y, X,
                                          C.c_void_p(pairs.data_ptr()) if pairs is not None else None, cap, C.byref(cnt)))
    eng._leave()
    return int(cnt.value)


@pytest.mark.parametrize("Y,X", [(5, 7), (16, 16), (9, 33)])
def test_seam_pairs_raw_vs_brute_force(eng, Y, X):
    """seam_pairs_kernel without the host's np.unique: the set of emitted pairs equals a brute force over the 9 neighbours, label
    pairs that touch only diagonally at the plane's corner and at its edge included; the count-only pass and the emit pass return
    the same count; with cap below the count the count is still the full one and nothing is written past 2 * cap words.  Smallest
    plane: (5, 7) holds the two 3 x 3 diagonal-only corners side by side; (9, 33) is more than one 256-thread workgroup."""
    import torch

    a, b, diagonal = cases.seam_planes(Y, X, seed=1)
    want, total = cases.seam_pairs_brute(a, b)
    assert diagonal <= want
    a_t = torch.from_numpy(a.view(np.int32).copy()).to(eng.device)
    b_t = torch.from_numpy(b.view(np.int32).copy()).to(eng.device)
    count = _seam_raw(eng, a_t, b_t, Y, X, None, 0)
    assert len(want) <= count <= total  # (a voxel emits a pair again only when another label came between: never more than the neighbour pairs)
    buf = torch.full((2 * count + 8,), DEAD_I32, dtype=torch.int32, device=eng.device)
    assert _seam_raw(eng, a_t, b_t, Y, X, buf, count) == count
    out = buf.cpu().numpy().view(np.uint32)
    assert (out[2 * count:] == DEAD).all()
    assert {(int(p), int(q)) for p, q in out[:2 * count].reshape(-1, 2)} == want
    for cap in (count // 2, 1, 0):
        buf.fill_(DEAD_I32)
        assert _seam_raw(eng, a_t, b_t, Y, X, buf, cap) == count
        out = buf.cpu().numpy().view(np.uint32)
        assert (out[2 * cap:] == DEAD).all(), cap
        assert {(int(p), int(q)) for p, q in out[:2 * cap].reshape(-1, 2)} <= want, cap
    got = eng.seam_pairs(a_t, b_t)
    np.testing.assert_array_equal(got, np.array(sorted(want), dtype=np.uint32))


@pytest.mark.parametrize("name", ["comb", "snake"])
def test_streamed_labelling_in_four_slabs_equals_the_single_volume(eng, name, tmp_path):
    """streaming.ccl_streamed with 4 slabs: the seam pairs, the host's merge and the table relabel put the comb (whose teeth meet in
    the last row of every plane) and the snake (one plane per slab: every link crosses a seam) back together."""
    from delivr_cfos_amd import streaming

    build, shape = cases.LATE_MERGE_CASES[name][0], cases.LATE_MERGE_CASES[name][1]
    mask, n_want = build(shape)
    single, n_single, _ = _check(eng, mask, rows=True, n_want=n_want)
    made = []

    def create_output(n):
        made.append(np.zeros(shape, dtype=np.uint32))
        return made[-1]

    n, _stats = streaming.ccl_streamed(eng, np.array(mask), 4, str(tmp_path / "provisional.npy"), create_output)
    assert n == n_single == n_want and len(made) == 1
    np.testing.assert_array_equal(made[0], single)


# ---- (h) tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvox", [1, 3, 4, 5, 1023, 4099])
def test_relabel_table_vs_numpy(eng, nvox):
    """dlv_relabel_u32_dev (relabel_lut_kernel with head = 0) with a random permutation table against numpy: fewer voxels than one
    16-byte access (1, 3), exactly one (4), one and a tail (5), and more than the 1024 voxels of a workgroup's first pass with a
    tail of 3 (1023, 4099).  A pointer that is not 16-byte aligned is refused with the library's error."""
    import torch

    from delivr_cfos_amd._lib import DLV_EINVAL

    rng = np.random.default_rng(nvox)
    L = 37
    lut = np.concatenate([[0], rng.permutation(L) + 1]).astype(np.uint32)
    labels = rng.integers(0, L + 1, size=nvox).astype(np.uint32)
    labels[rng.integers(0, nvox)] = L  # the last row of the table is used
    buf = torch.full((nvox + 8,), DEAD_I32, dtype=torch.int32, device=eng.device)
    buf[:nvox] = torch.from_numpy(labels.view(np.int32)).to(eng.device)
    eng.relabel(buf[:nvox], lut)
    out = buf.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(out[:nvox], lut[labels])
    assert (out[nvox:] == DEAD).all()
    lut_dev = torch.from_numpy(lut.view(np.int32)).to(eng.device)
    before = buf.clone()
    rc = eng.lib.dlv_relabel_u32_dev(eng.ctx, C.c_void_p(buf.data_ptr() + 4), nvox, C.c_void_p(lut_dev.data_ptr()), L + 1)
    assert rc == DLV_EINVAL and b"16-byte aligned" in eng.lib.dlv_last_error(eng.ctx)
    eng.sync()
    assert torch.equal(buf, before)


@pytest.fixture(scope="module")
def many_labels():
    """a label volume made in numpy, not by the labelling: 1,100,000 labels with 0 .. 3 voxels each and some background, shuffled"""
    rng = np.random.default_rng(11)
    n = 1_100_000
    per = rng.integers(0, 4, size=n + 1)
    per[0] = 300_000
    per[n] = 2  # the last label is kept: n_kept counts the table's last row
    vol = np.repeat(np.arange(n + 1, dtype=np.uint32), per)
    rng.shuffle(vol)
    keep = per == 2
    keep[0] = False
    new = (np.cumsum(keep) * keep).astype(np.uint32)
    want = new[vol]
    for a in (vol, per, want):
        a.setflags(write=False)
    return n, vol, per, int(keep.sum()), want


@pytest.mark.parametrize("head", [0, 1, 3])
def test_size_filter_over_more_than_2_20_labels(eng, many_labels, head):
    """dlv_cc_size_filter_dev with bounds [2, 2] on 1,100,000 labels: its lookup table is the scan over n + 1 rows, and
    dev_scan_groups_kernel gives a thread more than one group (per > 1) only above 1024 groups of 1024 rows = 2^20 rows - 1,100,001
    rows are 1075 groups, per = 2.  head: the volume starts 16 - 4 * head bytes past a 16-byte boundary (relabel_lut_kernel with
    head > 0).  n_kept and the filtered volume equal numpy's cumulative sum over the kept flags."""
    import torch

    n, vol, per, n_kept_want, want = many_labels
    assert n + 1 > 1 << 20 and vol.max() == n
    buf = torch.full((vol.size + 8,), DEAD_I32, dtype=torch.int32, device=eng.device)
    assert buf.data_ptr() % 16 == 0
    first = (4 - head) % 4
    labels = buf[first:first + vol.size]
    assert (16 - labels.data_ptr() % 16) % 16 == 4 * head
    labels.copy_(torch.from_numpy(vol.view(np.int32).copy()).to(eng.device))
    aligned = torch.from_numpy(vol.view(np.int32).copy()).to(eng.device)
    counts = eng.cc_counts(aligned, n)
    np.testing.assert_array_equal(counts.cpu().numpy().view(np.uint32)[1:], per[1:])
    kept = eng.cc_size_filter(labels, n, 2, 2, counts=counts)
    assert kept == n_kept_want
    out = buf.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(out[first:first + vol.size], want)
    assert (out[:first] == DEAD).all() and (out[first + vol.size:] == DEAD).all()
