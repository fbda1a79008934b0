"""count_blobs' size filter on the device (dlv_cc_counts_dev / dlv_cc_size_filter_dev; settings["mi355x"]["size_filter"]).

The reference of every case is numpy on the labels dlv_ccl26_dev returned: bincount -> keep flags -> cumsum -> table look-up.
Everything compared is an integer: equality, no tolerance."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _expected(labels: np.ndarray, n: int, lo: int, hi: int):
    counts = np.bincount(labels.ravel(), minlength=n + 1)
    keep = (counts >= (lo if lo >= 0 else 0)) & (counts <= (hi if hi >= 0 else np.iinfo(np.int64).max))
    keep[0] = False
    lut = np.where(keep, np.cumsum(keep), 0).astype(np.uint32)
    return counts, keep, lut[labels], int(keep.sum())


@pytest.fixture(scope="module")
def eng():
    from delivr_cfos_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def _label(eng, mask):
    import torch

    lab, n = eng.ccl26(torch.from_numpy(mask).cuda())
    return lab.cpu().numpy().view(np.uint32), n


def _to_dev(labels):
    import torch

    return torch.from_numpy(labels.view(np.int32).copy()).cuda()


def _filtered(eng, labels, n, lo, hi):
    dev = _to_dev(labels)
    k = eng.cc_size_filter(dev, n, lo, hi)
    return dev.cpu().numpy().view(np.uint32), k


# ---- 1. odd geometry ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd(eng):
    """33 x 67 x 131 (x no multiple of 8, 289 641 voxels = 1 mod 4): boxes of 1-3 voxels per axis on a pitch-4 grid, so that
    the sizes run from 1 to 27 and no two cells touch"""
    rng = np.random.default_rng(5)
    shape = (33, 67, 131)
    mask = np.zeros(shape, dtype=np.uint8)
    for z in range(0, shape[0], 4):
        for y in range(0, shape[1], 4):
            ext = rng.integers(1, 4, size=(len(range(0, shape[2], 4)), 3))
            for (dz, dy, dx), x in zip(ext, range(0, shape[2], 4)):
                mask[z:z + dz, y:y + dy, x:x + dx] = 1
    labels, n = _label(eng, mask)
    assert mask.size % 4 == 1 and n == 9 * 17 * 33
    labels.setflags(write=False)
    mask.setflags(write=False)
    return mask, labels, n


@pytest.mark.parametrize("lo, hi", [(2, -1), (-1, 8), (4, 12), (-1, -1)])
def test_odd_geometry_equals_numpy_aligned_and_unaligned_and_the_relabelled_mask(eng, odd, lo, hi):
    import torch

    mask, labels, n = odd
    counts, keep, expected, k_ref = _expected(labels, n, lo, hi)
    assert counts[1:].min() == 1 and counts[1:].max() == 27
    if (lo, hi) != (-1, -1):
        assert 0 < k_ref < n
    dev = _to_dev(labels)
    assert dev.data_ptr() % 16 == 0
    got_counts = eng.cc_counts(dev, n)
    np.testing.assert_array_equal(got_counts.cpu().numpy().view(np.uint32), counts)
    k = eng.cc_size_filter(dev, n, lo, hi, counts=got_counts)
    assert k == k_ref
    filtered = dev.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(filtered, expected)
    # a volume that starts 4 bytes behind a 16-byte boundary: the plain path of both kernels, counts computed inside
    buf = torch.zeros(labels.size + 1, dtype=torch.int32, device="cuda")
    view = buf[1:]
    view.copy_(_to_dev(labels).reshape(-1))
    assert view.data_ptr() % 16 == 4
    np.testing.assert_array_equal(eng.cc_counts(view, n).cpu().numpy().view(np.uint32), counts)
    assert eng.cc_size_filter(view, n, lo, hi) == k_ref
    np.testing.assert_array_equal(view.cpu().numpy().view(np.uint32).reshape(labels.shape), expected)
    assert int(buf[0]) == 0
    # the cc3d identity: an order-preserving compaction IS the labelling of the mask without the dropped components
    relabelled, n2 = _label(eng, mask * keep[labels].astype(np.uint8))
    assert n2 == k_ref
    np.testing.assert_array_equal(filtered, relabelled)


# ---- 2. more labels than one scan block and than 2^16 ---------------------------------------------------------------
def test_more_than_2_to_16_labels_down_to_a_uint16_file(eng, tmp_path):
    from delivr_cfos_amd.count_blobs import count_blobs

    rng = np.random.default_rng(6)
    shape = (64, 96, 144)
    mask = np.zeros(shape, dtype=np.uint8)
    mask[::2, ::2, ::3] = 1
    mask[::2, ::2, 1::3] = rng.integers(0, 2, size=(32, 48, 48), dtype=np.uint8)  # singles or x-pairs
    labels, n = _label(eng, mask)
    assert n == 32 * 48 * 48 and n > 65536
    counts, keep, expected, k_ref = _expected(labels, n, 2, -1)
    assert 0 < k_ref < 65536
    got, k = _filtered(eng, labels, n, 2, -1)
    assert k == k_ref
    np.testing.assert_array_equal(got, expected)
    d = tmp_path / "in" / "brain" / "binary_segmentations"
    os.makedirs(d)
    np.save(str(d / "binaries.npy"), mask)
    settings = {"postprocessing": {"output_location": str(tmp_path / "post") + "/"}, "mi355x": {"size_filter": True}}
    assert count_blobs(settings, str(tmp_path / "in"), 0, "brain", (1, 1) + shape, 2, -1, engine=eng) == k_ref
    written = np.load(os.path.join(str(tmp_path / "post"), f"brain-{k_ref}-cc3d.npy"))
    assert written.dtype == np.uint16
    np.testing.assert_array_equal(written, expected)
    assert count_blobs.last_filter == {"min_size": 2, "max_size": -1, "n_before": n, "n_kept": k_ref,
                                       "voxels_removed": int(counts[1:][~keep[1:]].sum())}


# ---- 3. one giant component plus specks ---------------------------------------------------------------------------
def test_one_giant_component_beside_specks(eng):
    rng = np.random.default_rng(7)
    mask = np.zeros((34, 66, 100), dtype=np.uint8)
    mask[1:33, 1:65, 1:65] = 1  # 131 072 voxels behind one label: every lane of every wave adds to the same counter
    mask[::2, ::2, 67::2] = rng.integers(0, 2, size=(17, 33, 17), dtype=np.uint8)  # isolated voxels, some ahead of the block in raster order
    labels, n = _label(eng, mask)
    block = int(labels[1, 1, 1])
    counts, keep, expected, k_ref = _expected(labels, n, -1, 100)
    assert counts[block] == 32 * 64 * 64 and 1 < block < n and k_ref == n - 1
    got, k = _filtered(eng, labels, n, -1, 100)
    assert k == n - 1
    np.testing.assert_array_equal(got, expected)
    assert got[1, 1, 1] == 0 and np.array_equal(got[labels > block], labels[labels > block] - 1)  # the specks keep their order
    got, k = _filtered(eng, labels, n, 100, -1)
    assert k == 1
    np.testing.assert_array_equal(got, (labels == block).astype(np.uint32))


# ---- 4. edges ---------------------------------------------------------------------------------------------------
def test_empty_mask_everything_removed_and_min_above_max(eng, odd):
    from delivr_cfos_amd import _lib

    empty = np.zeros((9, 10, 11), dtype=np.uint8)
    labels, n = _label(eng, empty)
    assert n == 0
    dev = _to_dev(labels)
    np.testing.assert_array_equal(eng.cc_counts(dev, 0).cpu().numpy().view(np.uint32), [empty.size])
    assert eng.cc_size_filter(dev, 0, 1, -1) == 0
    assert not dev.any()
    _, labels, n = odd
    got, k = _filtered(eng, labels, n, 1000, -1)
    assert k == 0 and not got.any()
    dev = _to_dev(labels)
    with pytest.raises(ValueError):
        eng.cc_size_filter(dev, n, 5, 4)
    counts = eng.cc_counts(dev, n)
    kept = C.c_uint64()
    rc = eng.lib.dlv_cc_size_filter_dev(eng.ctx, C.c_void_p(dev.data_ptr()), labels.size, n, C.c_void_p(counts.data_ptr()), 5, 4, C.byref(kept))
    assert rc == _lib.DLV_EINVAL
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), labels)  # refused: untouched
    kept.value = 0  # both bounds negative through the C entry point itself: K = n, nothing touched
    rc = eng.lib.dlv_cc_size_filter_dev(eng.ctx, C.c_void_p(dev.data_ptr()), labels.size, n, C.c_void_p(counts.data_ptr()), -1, -1, C.byref(kept))
    assert rc == 0 and kept.value == n
    eng.sync()
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), labels)


# ---- 5. end to end ------------------------------------------------------------------------------------------------
def test_count_blobs_with_the_switch_on_writes_the_filtered_mask_and_off_the_whole_one(eng, tmp_path):
    from delivr_cfos_amd.count_blobs import count_blobs
    from oracle import delivr_oracle as orc

    rng = np.random.default_rng(11)
    mask = (rng.random((40, 64, 72)) < 0.05).astype(np.uint8)
    d = tmp_path / "in" / "brain" / "binary_segmentations"
    os.makedirs(d)
    np.save(str(d / "binaries.npy"), mask)
    lab_all, n_all = orc.ccl26(mask)
    sizes = np.bincount(lab_all.ravel(), minlength=n_all + 1)
    keep = (sizes >= 3) & (sizes <= 20)
    keep[0] = False
    erased = mask * keep[lab_all].astype(np.uint8)
    lab_ref, n_ref = orc.ccl26(erased)
    assert 1 < n_ref < n_all and sizes[1:].max() > 20  # both bounds remove something
    st_ref = orc.cc_stats(lab_ref, n_ref)

    post = str(tmp_path / "on")
    settings = {"postprocessing": {"output_location": post + "/"}, "mi355x": {"size_filter": True}}
    assert count_blobs(settings, str(tmp_path / "in"), 0, "brain", (1, 1) + mask.shape, 3, 20, engine=eng) == n_ref
    assert sorted(f for f in os.listdir(post) if f.endswith(".npy")) == [f"brain-{n_ref}-cc3d.npy"]
    labels = np.load(os.path.join(post, f"brain-{n_ref}-cc3d.npy"))
    assert labels.dtype == np.uint16 and np.array_equal(labels.astype(np.uint32), lab_ref)
    stats = pickle.load(open(os.path.join(post, "brain-stats.pickle"), "rb"))
    for key in ("voxel_counts", "bounding_boxes", "centroids"):
        np.testing.assert_array_equal(stats[key], st_ref[key])
    assert stats["voxel_counts"][0] == mask.size - int(erased.sum())  # the background row counts the removed voxels
    assert open(os.path.join(post, f"{mask.shape}_brain.csv")).read() == orc.cells_csv_text(st_ref, n_ref)
    assert count_blobs.last_filter == {"min_size": 3, "max_size": 20, "n_before": n_all, "n_kept": n_ref,
                                       "voxels_removed": int(mask.sum()) - int(erased.sum())}
    assert np.array_equal(np.load(str(d / "binaries.npy")), mask)  # step 2's output is not rewritten

    # the regression guard: same bounds, switch off - what the reference writes, the bounds ignored
    post = str(tmp_path / "off")
    settings = {"postprocessing": {"output_location": post + "/"}}
    assert count_blobs(settings, str(tmp_path / "in"), 0, "brain", (1, 1) + mask.shape, 3, 20, engine=eng) == n_all
    labels = np.load(os.path.join(post, f"brain-{n_all}-cc3d.npy"))
    assert np.array_equal(labels.astype(np.uint32), lab_all)
    st_all = orc.cc_stats(lab_all, n_all)
    stats = pickle.load(open(os.path.join(post, "brain-stats.pickle"), "rb"))
    for key in ("voxel_counts", "bounding_boxes", "centroids"):
        np.testing.assert_array_equal(stats[key], st_all[key])
    assert count_blobs.last_filter is None


# ---- 6. sharded ---------------------------------------------------------------------------------------------------
class _ThreadRanks:
    """The torch.distributed calls of count_blobs' sharded path between THREADS of this process (one HipEngine per thread,
    all on device 0): objects travel through a shared list between two barriers, seam planes through queues."""

    isend, irecv = "isend", "irecv"

    def __init__(self, world):
        import queue
        import threading

        self.world = world
        self.q = {(a, b): queue.Queue() for a in range(world) for b in range(world)}
        self.bar = threading.Barrier(world)
        self.box = [None] * world
        self.local = threading.local()

    def bind(self, rank):
        self.local.rank = rank

    def get_backend(self):
        return "threads"

    def get_rank(self):
        return self.local.rank

    def get_world_size(self):
        return self.world

    class P2POp:
        def __init__(self, op, tensor, peer, group=None):
            self.op, self.tensor, self.peer = op, tensor, peer

    class _Done:
        def wait(self):
            return None

    def batch_isend_irecv(self, ops):
        me = self.local.rank
        for o in ops:
            if o.op == "isend":
                self.q[(me, o.peer)].put(o.tensor.clone())
        for o in ops:
            if o.op == "irecv":
                o.tensor.copy_(self.q[(o.peer, me)].get(timeout=120))
        return [self._Done() for _ in ops]

    def _exchange(self, obj):
        self.box[self.local.rank] = obj
        self.bar.wait()
        got = list(self.box)
        self.bar.wait()
        return got

    def all_gather_object(self, out, obj, group=None):
        out[:] = self._exchange(obj)

    def gather_object(self, obj, out, dst=0, group=None):
        got = self._exchange(obj)
        if self.local.rank == dst:
            out[:] = got

    def broadcast_object_list(self, box, src=0, group=None):
        box[:] = self._exchange(list(box))[src]


def _seam_volume():
    """45 planes in three even slabs; one component above max_size and one inside the bounds, each across a seam"""
    rng = np.random.default_rng(13)
    m = (rng.random((45, 40, 56)) < 0.03).astype(np.uint8)
    m[:, 18:23, 28:33] = 0
    m[10:20, 20, 30] = 1   # 10 voxels across the seam at z = 15: above max_size
    m[29:31, 20, 30] = 1   # 2 voxels across the seam at z = 30: kept
    return m, 2, 8, 3


def _single_engine_reference(eng, m, lo, hi, world):
    from delivr_cfos_amd.count_blobs import _even_slabs

    assert _even_slabs(m.shape[0], world) == [(0, 15), (15, 30), (30, 45)]
    labels, n = _label(eng, m)
    counts, keep, expected, k_ref = _expected(labels, n, lo, hi)
    col = int(labels[10, 20, 30])
    assert counts[col] == 10 and not keep[col] and labels[14, 20, 30] == labels[15, 20, 30] == col
    assert keep[labels[29, 20, 30]] and labels[29, 20, 30] == labels[30, 20, 30]
    single = _to_dev(labels)
    assert eng.cc_size_filter(single, n, lo, hi) == k_ref
    st1 = eng.cc_stats(single, k_ref)
    np.testing.assert_array_equal(single.cpu().numpy().view(np.uint32), expected)
    last = {"min_size": lo, "max_size": hi, "n_before": n, "n_kept": k_ref, "voxels_removed": int(counts[1:][~keep[1:]].sum())}
    return expected, k_ref, st1, last


def _run_thread_ranks(fake, body):
    """body(rank, engine) on one thread per rank, one HipEngine each on device 0 -> the results in rank order"""
    import threading

    import torch
    from delivr_cfos_amd.engine import HipEngine

    results, errors = [None] * fake.world, []

    def rank_main(rank):
        try:
            fake.bind(rank)
            torch.cuda.set_device(0)
            e = HipEngine(0)
            results[rank] = body(rank, e)
            e.close()
        except BaseException as exc:  # noqa: BLE001
            errors.append((rank, repr(exc)))
            fake.bar.abort()

    ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(fake.world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errors, errors
    return results


def test_sharded_count_blobs_with_bounds_equals_the_single_engine_result(eng, tmp_path):
    from delivr_cfos_amd.count_blobs import _count_blobs_sharded, count_blobs
    from delivr_cfos_amd.hostlogic import CountOptions

    m, lo, hi, world = _seam_volume()
    expected, k_ref, st1, last = _single_engine_reference(eng, m, lo, hi, world)
    fake = _ThreadRanks(world)
    results = _run_thread_ranks(fake, lambda rank, e: _count_blobs_sharded(e, m, fake, str(tmp_path), "b", opts=CountOptions(bounds=(lo, hi))))
    assert all(r[0] == k_ref for r in results)
    assert results[1][1] is None and results[2][1] is None
    assert sorted(os.listdir(str(tmp_path))) == [f"b-{k_ref}-cc3d.npy"]
    written = np.load(os.path.join(str(tmp_path), f"b-{k_ref}-cc3d.npy"))
    assert written.dtype == np.uint16
    np.testing.assert_array_equal(written, expected)
    for key in ("voxel_counts", "bounding_boxes", "centroids"):
        np.testing.assert_array_equal(results[0][1][key], st1[key])
    assert count_blobs.last_filter == last


def test_count_blobs_under_torch_distributed_hands_the_bounds_to_the_sharded_path(eng, tmp_path, monkeypatch, capsys):
    """the public entry point with an initialised process group of three ranks (torch.distributed's calls replaced by the thread
    ranks): settings and min_size / max_size must reach the slabs - file, pickle, CSV and last_filter are the filtered ones"""
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs
    from oracle import delivr_oracle as orc

    m, lo, hi, world = _seam_volume()
    expected, k_ref, st1, last = _single_engine_reference(eng, m, lo, hi, world)
    d = tmp_path / "in" / "brain" / "binary_segmentations"
    os.makedirs(d)
    np.save(str(d / "binaries.npy"), m)
    post = str(tmp_path / "post")
    fake = _ThreadRanks(world)
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    for name in ("get_rank", "get_world_size", "get_backend", "P2POp", "isend", "irecv", "batch_isend_irecv", "all_gather_object",
                 "gather_object", "broadcast_object_list"):
        monkeypatch.setattr(dist, name, getattr(fake, name))
    for switch in (True, False):
        out = post + ("_on" if switch else "_off")
        settings = {"postprocessing": {"output_location": out + "/"}, "mi355x": {"size_filter": switch}}
        results = _run_thread_ranks(fake, lambda rank, e: count_blobs(settings, str(tmp_path / "in"), 0, "brain", (1, 1) + m.shape, lo, hi, engine=e))
        if switch:
            assert results == [k_ref] * world
            written = np.load(os.path.join(out, f"brain-{k_ref}-cc3d.npy"))
            assert written.dtype == np.uint16
            np.testing.assert_array_equal(written, expected)
            stats = pickle.load(open(os.path.join(out, "brain-stats.pickle"), "rb"))
            for key in ("voxel_counts", "bounding_boxes", "centroids"):
                np.testing.assert_array_equal(stats[key], st1[key])
            assert open(os.path.join(out, f"{m.shape}_brain.csv")).read() == orc.cells_csv_text(st1, k_ref)
            assert count_blobs.last_filter == last
            assert "size filter (min_size 2, max_size 8): kept" in capsys.readouterr().out
        else:  # the same ranks without the switch: the whole labelling, and the line that says the bounds are ignored
            n_all = last["n_before"]
            assert results == [n_all] * world
            assert os.path.isfile(os.path.join(out, f"brain-{n_all}-cc3d.npy"))
            assert count_blobs.last_filter is None
            assert "are ignored, as in the reference" in capsys.readouterr().out


# ---- 7. refusal ---------------------------------------------------------------------------------------------------
def test_a_mask_that_needs_the_streamed_path_is_refused_with_the_switch_on(eng, tmp_path):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask = (np.random.default_rng(17).random((24, 32, 40)) < 0.05).astype(np.uint8)
    d = tmp_path / "in" / "brain" / "binary_segmentations"
    os.makedirs(d)
    np.save(str(d / "binaries.npy"), mask)
    post = str(tmp_path / "post")
    settings = {"postprocessing": {"output_location": post + "/"}, "mi355x": {"size_filter": True, "hbm_budget_gb": 1e-4}}
    with pytest.raises(MemoryError, match=r"size_filter.*hbm_budget_gb"):
        count_blobs(settings, str(tmp_path / "in"), 0, "brain", (1, 1) + mask.shape, 3, -1, engine=eng)
    assert not [f for f in os.listdir(post) if "cc3d" in f or f.endswith((".npy", ".partial", ".tmp"))]
