"""Per-cell confidence on the device (dlv_cc_confidence_dev / HipEngine.cc_confidence; settings["mi355x"]["confidence_stats"] in
count_blobs).

The reference of every case is numpy on the labels and probabilities handed in: q = rint(clip(p, 0, 1) * 2^24) with NaN as 0, a
stable argsort by label, add / minimum / maximum.reduceat over the runs of equal labels in uint64, and the peak as the first voxel
in raster order that holds its label's maximum.  Everything compared is an integer - equality, no tolerance; the finished floats
are float64 equality with q / 2^24 and sum / (count * 2^24)."""
import importlib.util
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("confidence_sum", "confidence_min_q", "confidence_max_q", "confidence_peak_index")
DTYPES = (np.uint64, np.uint32, np.uint32, np.uint64)
NO_PEAK = np.uint64(2**64 - 1)
SHAPES = [(1, 1, 1), (3, 5, 7), (4, 6, 64), (2, 3, 2056), (2, 2, 2049)]


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _q(prob):
    p = np.asarray(prob, dtype=np.float32)
    return np.rint(np.clip(np.where(np.isnan(p), 0, p), 0, 1).astype(np.float32) * np.float32(2**24)).astype(np.uint32)


def _reference(labels: np.ndarray, prob: np.ndarray, n: int) -> dict:
    """the ABI's rows 0..n: absent labels - and row 0 - read 0, 0xFFFFFFFF, 0, 2^64 - 1; labels above n are left out"""
    assert labels.shape == prob.shape
    lab = labels.ravel()
    order = np.argsort(lab, kind="stable")  # (stable: inside a label the voxels stay in raster order)
    ls, qs = lab[order], _q(prob).ravel()[order].astype(np.uint64)
    starts = np.flatnonzero(np.r_[True, ls[1:] != ls[:-1]])
    present = ls[starts].astype(np.int64)
    sel = (present >= 1) & (present <= n)
    out = {"confidence_sum": np.zeros(n + 1, dtype=np.uint64), "confidence_min_q": np.full(n + 1, 0xFFFFFFFF, dtype=np.uint32),
           "confidence_max_q": np.zeros(n + 1, dtype=np.uint32), "confidence_peak_index": np.full(n + 1, NO_PEAK, dtype=np.uint64)}
    top = np.maximum.reduceat(qs, starts)
    at_top = qs == np.repeat(top, np.diff(np.r_[starts, len(ls)]))
    first = np.minimum.reduceat(np.where(at_top, order.astype(np.uint64), NO_PEAK), starts)  # argmax of (q, -index)
    out["confidence_sum"][present[sel]] = np.add.reduceat(qs, starts)[sel]
    out["confidence_min_q"][present[sel]] = np.minimum.reduceat(qs, starts)[sel].astype(np.uint32)
    out["confidence_max_q"][present[sel]] = top[sel].astype(np.uint32)
    out["confidence_peak_index"][present[sel]] = first[sel]
    return out


def _assert_same(got: dict, ref: dict, keys=KEYS):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


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


def _labels_dev(labels):
    import torch

    return torch.from_numpy(labels.view(np.int32).copy()).cuda()


def _prob_dev(prob):
    import torch

    return torch.from_numpy(np.array(prob, dtype=np.float32, order="C")).cuda()


HALF_K = np.array([0, 1, 2, 3, 2**20, 2**20 + 1, 2**21 - 2, 2**21 - 1], dtype=np.int64)  # both parities
SPECIAL = np.concatenate([np.array([0.0, 0.5, 1.0, 2.0**-30, -0.25, 1.5, np.nan, np.inf, -np.inf, -0.0], dtype=np.float32),
                          ((2 * HALF_K + 1).astype(np.float64) * 2.0**-25).astype(np.float32)])


def _probabilities(shape, rng):
    """name -> volume: random in [0, 1]; the special values sown over a random volume (cycled through, so that a volume of one voxel
    holds one of them); a constant"""
    size = int(np.prod(shape))
    rand = rng.random(shape, dtype=np.float32)
    rand.ravel()[rng.integers(0, size, size=max(size // 50, 1))] = 1.0  # (random() stays below 1)
    special = rng.random(shape, dtype=np.float32)
    where = rng.permutation(size)[:max(size // 3, 1)]
    special.ravel()[where] = SPECIAL[np.arange(len(where)) % len(SPECIAL)]
    return {"random": rand, "special": special, "constant": np.full(shape, 0.625, dtype=np.float32)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_loader_and_fold_path_against_numpy(eng, shape):
    rng = np.random.default_rng(sum(shape))
    probs = _probabilities(shape, rng)
    labellings = {}
    for density in (0.05, 0.4):
        labellings[f"ccl {density}"] = _label(eng, (rng.random(shape) < density).astype(np.uint8))
    labellings["one component"] = _label(eng, np.ones(shape, dtype=np.uint8))  # all 64 lanes of a wave hold one label
    assert labellings["one component"][1] == 1
    for lname, (labels, n) in labellings.items():
        lab_dev = _labels_dev(labels)
        for pname, prob in probs.items():
            prob_dev = _prob_dev(prob)
            ref = _reference(labels, prob, n)
            got = eng.cc_confidence(lab_dev, prob_dev, n)
            assert list(got) == list(KEYS)
            try:
                _assert_same(got, ref)
            except AssertionError as exc:
                raise AssertionError(f"{lname} / {pname}: {exc}") from None
            assert [int(got[k][0]) for k in KEYS] == [0, 0xFFFFFFFF, 0, 2**64 - 1]  # the background is not measured
            if pname == "constant" and n:  # every voxel ties: the peak is the cell's first voxel in raster order
                first = np.full(n + 1, labels.size, dtype=np.int64)
                np.minimum.at(first, labels.ravel().astype(np.int64), np.arange(labels.size))
                np.testing.assert_array_equal(got["confidence_peak_index"][1:], first[1:].astype(np.uint64))
                assert (got["confidence_min_q"][1:] == 0.625 * 2**24).all() and (got["confidence_max_q"][1:] == 0.625 * 2**24).all()
            np.testing.assert_array_equal(prob_dev.cpu().numpy().view(np.uint32), prob.view(np.uint32))  # read, never written
        np.testing.assert_array_equal(lab_dev.cpu().numpy().view(np.uint32), labels)
    # n below the largest label: the higher labels are ignored; n = 0: the background's row alone
    labels, n = labellings["ccl 0.4"]
    lab_dev, prob_dev = _labels_dev(labels), _prob_dev(probs["special"])
    whole = _reference(labels, probs["special"], n)
    for few in sorted({0, n // 2}):
        got = eng.cc_confidence(lab_dev, prob_dev, few)
        _assert_same(got, _reference(labels, probs["special"], few))
        _assert_same(got, {k: v[:few + 1] for k, v in whole.items()})
    assert {k: v.tolist() for k, v in eng.cc_confidence(lab_dev, prob_dev, 0).items()} == {
        "confidence_sum": [0], "confidence_min_q": [0xFFFFFFFF], "confidence_max_q": [0], "confidence_peak_index": [2**64 - 1]}


def test_volumes_4_bytes_past_a_16_byte_boundary_take_the_scalar_loads(eng):
    import torch

    shape = (4, 6, 64)
    rng = np.random.default_rng(21)
    labels, n = _label(eng, (rng.random(shape) < 0.3).astype(np.uint8))
    prob = _probabilities(shape, rng)["special"]
    lab_host = np.full(labels.size + 2, 0x7FFFFFF0, dtype=np.int32)  # guards: a label far above n
    lab_host[1:-1] = labels.view(np.int32).ravel()
    prob_host = np.full(prob.size + 2, 1.0, dtype=np.float32)  # guards: the largest probability there is
    prob_host[1:-1] = prob.ravel()
    lab_buf, prob_buf = torch.from_numpy(lab_host).cuda(), torch.from_numpy(prob_host).cuda()
    lab_view, prob_view = lab_buf[1:-1].view(shape), prob_buf[1:-1].view(shape)
    assert lab_view.data_ptr() % 16 == 4 and prob_view.data_ptr() % 16 == 4
    ref = _reference(labels, prob, n)
    _assert_same(eng.cc_confidence(lab_view, prob_view, n), ref)
    _assert_same(eng.cc_confidence(_labels_dev(labels), prob_view, n), ref)  # aligned labels over unaligned probabilities
    _assert_same(eng.cc_confidence(lab_view, _prob_dev(prob), n), ref)  # ... and the reverse
    np.testing.assert_array_equal(lab_buf.cpu().numpy(), lab_host)
    np.testing.assert_array_equal(prob_buf.cpu().numpy().view(np.uint32), prob_host.view(np.uint32))


def test_refused_arguments(eng):
    import ctypes as C

    import torch
    from delivr_cfos_amd import _lib

    shape = (3, 5, 7)
    labels, n = _label(eng, (np.random.default_rng(2).random(shape) < 0.3).astype(np.uint8))
    lab_dev, prob_dev = _labels_dev(labels), _prob_dev(np.full(shape, 0.5))
    out = [np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint64)]
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in out]
    lp, pp = C.c_void_p(lab_dev.data_ptr()), C.c_void_p(prob_dev.data_ptr())
    call = eng.lib.dlv_cc_confidence_dev
    assert call(eng.ctx, lp, pp, 3, 0, 7, n, *ptrs) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, None, 3, 5, 7, n, *ptrs) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, pp, 3, 5, 7, n, ptrs[0], ptrs[1], ptrs[2], None) == _lib.DLV_EINVAL
    assert call(eng.ctx, lp, pp, 3, 5, 7, 2**32 - 1, *ptrs) == _lib.DLV_EINVAL
    assert not any(a.any() for a in out)  # refused: nothing written
    assert call(eng.ctx, lp, pp, 3, 5, 7, n, *ptrs) == 0
    _assert_same(dict(zip(KEYS, out)), _reference(labels, np.full(shape, 0.5, dtype=np.float32), n))
    for bad in (prob_dev.double(), prob_dev[:2], prob_dev.reshape(-1), prob_dev.transpose(1, 2), prob_dev.cpu(), prob_dev.view(torch.int32)):
        with pytest.raises(ValueError):
            eng.cc_confidence(lab_dev, bad, n)
    with pytest.raises(ValueError):
        eng.cc_confidence(lab_dev.view(torch.float32), prob_dev, n)
    with pytest.raises(ValueError):
        eng.cc_confidence(lab_dev, prob_dev, -1)


# ---- slabs -------------------------------------------------------------------------------------------------------------------------
def test_z_slabs_merge_to_the_whole_volume_peak_ties_across_the_cut_included(eng):
    from delivr_cfos_amd.hostlogic import merge_confidence

    shape = (9, 6, 64)
    rng = np.random.default_rng(9)
    mask = (rng.random(shape) < 0.04).astype(np.uint8)
    mask[:, 1:4, 9:15] = 0  # (room around the two cells below: no speck joins them)
    mask[2:7, 3:6, 39:42] = 0
    mask[:, 2, 10:14] = 1  # a column through every plane: it crosses both cuts
    mask[3:6, 4, 40] = 1  # ... and one through the one-plane slab
    labels, n = _label(eng, mask)
    prob = rng.choice(np.array([0.5, 0.75, 1.0], dtype=np.float32), size=shape)  # three values: ties everywhere
    prob[:, 2, 10:14] = 0.875  # the long column's maximum sits in every slab: the first slab's voxel must win
    prob[3:6, 4, 40] = [0.5, 0.625, 0.625]  # the maximum in the middle slab and again below it
    lab_dev, prob_dev = _labels_dev(labels), _prob_dev(prob)
    whole = eng.cc_confidence(lab_dev, prob_dev, n)
    _assert_same(whole, _reference(labels, prob, n))
    column, short = int(labels[0, 2, 10]), int(labels[3, 4, 40])
    assert whole["confidence_peak_index"][column] == (0 * 6 + 2) * 64 + 10 and whole["confidence_peak_index"][short] == (4 * 6 + 4) * 64 + 40
    cuts = ((0, 4), (4, 5), (5, 9))
    parts = [(eng.cc_confidence(lab_dev[lo:hi], prob_dev[lo:hi], n), lo, 6 * 64) for lo, hi in cuts]
    for (part, lo, _), (_, hi) in zip(parts, cuts):
        _assert_same(part, _reference(labels[lo:hi], prob[lo:hi], n))  # a slab's peaks are indices inside the slab
    assert all((p[0]["confidence_peak_index"][1:] == NO_PEAK).any() for p in parts)  # every slab lacks some labels
    _assert_same(merge_confidence(parts), whole)
    _assert_same(merge_confidence([parts[2], None, parts[0], parts[1]]), whole)


# ---- count_blobs end to end ----------------------------------------------------------------------------------------------------------
STD_KEYS = {"voxel_counts", "bounding_boxes", "centroids"}
CONF_KEYS = ("confidence_sum", "confidence_min", "confidence_max", "confidence_mean", "confidence_peak")


def _brain_on_disk(tmp_path, mask, prob, raw=None):
    """step 2's output of the brain 'brain' - binaries.npy and, with prob, network_output.npy beside it - and with raw the padded
    raw volume -> (input folder, the probability file's path)"""
    d = tmp_path / "in" / "brain"
    os.makedirs(d / "binary_segmentations")
    np.save(str(d / "binary_segmentations" / "binaries.npy"), mask)
    prob_file = str(d / "binary_segmentations" / "network_output.npy")
    if prob is not None:
        np.save(prob_file, prob)
    if raw is not None:
        os.makedirs(d / "masked_niftis")
        np.save(str(d / "masked_niftis" / "x.npy"), raw[None, None])
    return str(tmp_path / "in"), prob_file


def _settings(path_in, post, **mi355x):
    s = {"postprocessing": {"output_location": post + "/"}, "blob_detection": {"input_location": path_in}}
    if mi355x:
        s["mi355x"] = mi355x
    return s


def _read(post, name):
    with open(os.path.join(post, name), "rb") as fh:
        return fh.read()


def _finished(labels, prob, n):
    """what count_blobs stores, from numpy alone"""
    ref = _reference(labels, prob, n)
    counts = np.bincount(labels.ravel(), minlength=n + 1)
    there = counts > 0
    there[0] = False
    Z, Y, X = labels.shape
    at = np.where(there, ref["confidence_peak_index"], 0).astype(np.int64)
    peak = np.stack([at // (Y * X), at // X % Y, at % X], axis=1)
    peak[~there] = -1
    mean = np.zeros(n + 1, dtype=np.float64)
    mean[there] = ref["confidence_sum"][there].astype(np.float64) / (counts[there].astype(np.float64) * 2.0**24)
    return {"voxel_counts": counts.astype(np.uint32), "confidence_sum": np.where(there, ref["confidence_sum"], 0).astype(np.uint64),
            "confidence_min": np.where(there, ref["confidence_min_q"], 0) / 2.0**24, "confidence_max": np.where(there, ref["confidence_max_q"], 0) / 2.0**24,
            "confidence_mean": mean, "confidence_peak": peak}


def _check_outputs(post, labels, prob, n, prob_file, more_keys=(), more_names=()):
    """pickle, table and last_confidence of a run with the key against numpy on the labels the run wrote"""
    from delivr_cfos_amd.count_blobs import count_blobs
    from delivr_cfos_amd.hostlogic import cell_confidence_csv_text

    ref = _finished(labels, prob, n)
    stats = pickle.loads(_read(post, "brain-stats.pickle"))
    assert set(stats) == STD_KEYS | set(CONF_KEYS) | set(more_keys)
    _assert_same(stats, ref, CONF_KEYS + ("voxel_counts",))
    assert stats["confidence_peak"].shape == (n + 1, 3) and stats["confidence_peak"][0].tolist() == [-1, -1, -1]
    assert n == 0 or (stats["confidence_min"][1:] >= 0.5).all()  # (the brain's cells lie where the probability is at least 0.5)
    assert _read(post, os.path.join("cell_confidence", "brain.csv")).decode() == cell_confidence_csv_text(ref, n)
    assert os.listdir(os.path.join(post, "cell_confidence")) == ["brain.csv"]
    assert "cell_confidence" in os.listdir(post) and all(name in os.listdir(post) for name in more_names)
    assert count_blobs.last_confidence == {"n": n, "prob_file": prob_file}
    return stats


@pytest.fixture(scope="module")
def brain():
    """32 x 48 x 40: probabilities as step 2 would leave them - the mask is prob >= 0.5 -, with plateaus (ties inside a cell) and a
    raw volume for the run beside intensity_stats"""
    rng = np.random.default_rng(17)
    shape = (32, 48, 40)
    prob = (rng.random(shape, dtype=np.float32) * np.float32(0.52)).astype(np.float32)  # 4 % of the voxels reach 0.5: specks
    blobs = rng.integers(2, [30, 46, 38], size=(60, 3))
    for z, y, x in blobs:
        prob[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] = np.float32(0.75)  # a plateau
        prob[z, y, x + 1] = prob[z + 1, y, x] = np.float32(0.96875)  # two equal peaks: the first in raster order counts
    prob[5:20, 10, 10] = 1.0
    mask = (prob >= 0.5).astype(np.uint8)
    raw = rng.integers(1, 65536, size=(32, 48, 64), dtype=np.uint16)
    for a in (mask, prob, raw):
        a.setflags(write=False)
    return mask, prob, raw


def test_count_blobs_fresh_run_adds_keys_and_table_and_a_run_without_the_key_nothing(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, prob, _ = brain
    path_in, prob_file = _brain_on_disk(tmp_path, mask, prob)
    stack = (1, 1) + mask.shape
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    n = count_blobs(_settings(path_in, on, confidence_stats=True), path_in, 0, "brain", stack, engine=eng)
    labels = np.load(os.path.join(on, f"brain-{n}-cc3d.npy")).astype(np.uint32)
    stats_on = _check_outputs(on, labels, prob, n, prob_file)
    assert "confidence_s" in count_blobs.last_timings
    assert sorted(os.listdir(on)) == sorted([f"{mask.shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle", "cell_confidence"])
    column = int(labels[5, 10, 10])
    assert stats_on["confidence_max"][column] == 1.0 and stats_on["confidence_peak"][column].tolist() == [5, 10, 10]
    for flag in ({}, {"confidence_stats": False}):
        post = off + str(len(flag))
        assert count_blobs(_settings(path_in, post, **flag), path_in, 0, "brain", stack, engine=eng) == n
        assert count_blobs.last_confidence is None and "confidence_s" not in count_blobs.last_timings
        assert sorted(os.listdir(post)) == sorted([f"{mask.shape}_brain.csv", f"brain-{n}-cc3d.npy", "brain-stats.pickle"])
        stats_off = pickle.loads(_read(post, "brain-stats.pickle"))
        assert set(stats_off) == STD_KEYS
        for name in (f"brain-{n}-cc3d.npy", f"{mask.shape}_brain.csv"):
            assert _read(on, name) == _read(post, name), name
        for k in STD_KEYS:
            np.testing.assert_array_equal(stats_on[k], stats_off[k])
    assert np.array_equal(np.load(prob_file).view(np.uint32), prob.view(np.uint32))  # the probabilities are read, never written


def test_count_blobs_with_split_and_size_filter_measures_the_final_labels(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, prob, _ = brain
    path_in, prob_file = _brain_on_disk(tmp_path, mask, prob)
    post = str(tmp_path / "post")
    n = count_blobs(_settings(path_in, post, confidence_stats=True, split_fused=1, size_filter=True), path_in, 0, "brain",
                    (1, 1) + mask.shape, 2, 40, engine=eng)
    assert count_blobs.last_filter["n_kept"] == n and 1 < n < count_blobs.last_filter["n_before"]
    labels = np.load(os.path.join(post, f"brain-{n}-cc3d.npy")).astype(np.uint32)
    stats = _check_outputs(post, labels, prob, n, prob_file, more_keys=("split_parent", "split_siblings", "split_depth"))
    assert stats["voxel_counts"][1:].min() >= 2 and stats["voxel_counts"][1:].max() <= 40


def test_count_blobs_with_a_run_length_label_file_fresh_and_from_the_cached_runs(eng, tmp_path, brain):
    from delivr_cfos_amd import label_runs
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, prob, _ = brain
    path_in, prob_file = _brain_on_disk(tmp_path, mask, prob)
    stack = (1, 1) + mask.shape
    fresh = str(tmp_path / "fresh")
    n = count_blobs(_settings(path_in, fresh, confidence_stats=True, label_file="runs"), path_in, 0, "brain", stack, engine=eng)
    labels = label_runs.load_labels(os.path.join(fresh, label_runs.runs_name("brain", n))).astype(np.uint32)
    ref_stats = _check_outputs(fresh, labels, prob, n, prob_file, more_names=(label_runs.runs_name("brain", n),))
    # a run file and a pickle of a run without the key: the runs are decoded in HBM, the pickle is completed
    cached = str(tmp_path / "cached")
    assert count_blobs(_settings(path_in, cached, label_file="runs"), path_in, 0, "brain", stack, engine=eng) == n
    before = pickle.loads(_read(cached, "brain-stats.pickle"))
    runs_bytes = _read(cached, label_runs.runs_name("brain", n))
    assert set(before) == STD_KEYS and "cell_confidence" not in os.listdir(cached)
    assert count_blobs(_settings(path_in, cached, confidence_stats=True, label_file="runs"), path_in, 0, "brain", stack, engine=eng) == n
    stats = _check_outputs(cached, labels, prob, n, prob_file)
    assert _read(cached, label_runs.runs_name("brain", n)) == runs_bytes
    for k in STD_KEYS:
        np.testing.assert_array_equal(stats[k], before[k])
    for k in CONF_KEYS:
        np.testing.assert_array_equal(stats[k], ref_stats[k])


def test_count_blobs_completes_a_cached_pickle_beside_cached_dense_labels(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, prob, _ = brain
    path_in, prob_file = _brain_on_disk(tmp_path, mask, prob)
    stack = (1, 1) + mask.shape
    post = str(tmp_path / "post")
    n = count_blobs(_settings(path_in, post), path_in, 0, "brain", stack, engine=eng)
    label_bytes, csv_bytes = _read(post, f"brain-{n}-cc3d.npy"), _read(post, f"{mask.shape}_brain.csv")
    before = pickle.loads(_read(post, "brain-stats.pickle"))
    before["a_users_entry"] = np.arange(5)  # an entry count_blobs knows nothing about survives the completion
    with open(os.path.join(post, "brain-stats.pickle"), "wb") as fh:
        pickle.dump(before, fh, protocol=pickle.HIGHEST_PROTOCOL)
    assert count_blobs(_settings(path_in, post, confidence_stats=True), path_in, 0, "brain", stack, engine=eng) == n
    labels = np.load(os.path.join(post, f"brain-{n}-cc3d.npy")).astype(np.uint32)
    stats = _check_outputs(post, labels, prob, n, prob_file, more_keys=("a_users_entry",))
    for k in before:
        assert stats[k].dtype == before[k].dtype
        np.testing.assert_array_equal(stats[k], before[k])
    assert _read(post, f"brain-{n}-cc3d.npy") == label_bytes and _read(post, f"{mask.shape}_brain.csv") == csv_bytes
    # a third run finds the keys: nothing is measured again, the pickle keeps its bytes
    pickle_bytes = _read(post, "brain-stats.pickle")
    assert count_blobs(_settings(path_in, post, confidence_stats=True), path_in, 0, "brain", stack, engine=eng) == n
    assert _read(post, "brain-stats.pickle") == pickle_bytes and "confidence_s" not in count_blobs.last_timings


def test_count_blobs_together_with_intensity_stats(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, prob, raw = brain
    path_in, prob_file = _brain_on_disk(tmp_path, mask, prob, raw)
    stack = (1, 1) + mask.shape
    both, alone = str(tmp_path / "both"), str(tmp_path / "alone")
    n = count_blobs(_settings(path_in, both, confidence_stats=True, intensity_stats=True), path_in, 0, "brain", stack, engine=eng)
    assert {"intensity_s", "confidence_s"} <= set(count_blobs.last_timings)
    labels = np.load(os.path.join(both, f"brain-{n}-cc3d.npy")).astype(np.uint32)
    intensity_keys = ("intensity_sum", "intensity_sumsq", "intensity_min", "intensity_max", "intensity_mean")
    stats = _check_outputs(both, labels, prob, n, prob_file, more_keys=intensity_keys, more_names=("cell_intensity",))
    assert count_blobs.last_intensity == {"n": n, "raw_file": os.path.join(path_in, "brain", "masked_niftis", "x.npy")}
    assert count_blobs(_settings(path_in, alone, intensity_stats=True), path_in, 0, "brain", stack, engine=eng) == n
    assert count_blobs.last_confidence is None
    only = pickle.loads(_read(alone, "brain-stats.pickle"))
    assert set(only) == STD_KEYS | set(intensity_keys)
    for k in only:
        np.testing.assert_array_equal(stats[k], only[k])
    assert _read(both, os.path.join("cell_intensity", "brain.csv")) == _read(alone, os.path.join("cell_intensity", "brain.csv"))


def test_a_missing_or_wrong_probability_file_raises_before_any_file_is_written(eng, tmp_path, brain):
    from delivr_cfos_amd.count_blobs import count_blobs

    mask, prob, _ = brain
    path_in, prob_file = _brain_on_disk(tmp_path, mask, None)
    post = str(tmp_path / "post")
    os.makedirs(post)
    open(os.path.join(post, "kept.txt"), "w").close()
    stack = (1, 1) + mask.shape
    settings = _settings(path_in, post, confidence_stats=True)
    with pytest.raises(FileNotFoundError, match="SAVE_ACTIVATED_OUTPUT"):
        count_blobs(settings, path_in, 0, "brain", stack, engine=eng)
    assert os.listdir(post) == ["kept.txt"]
    for wrong, pattern in ((prob.astype(np.float64), "float64"), (prob[:, :, :39], r"\(32, 48, 39\).*\(32, 48, 40\)"),
                           (np.asfortranarray(prob), "C-ordered"), (prob.astype(">f4"), "SAVE_ACTIVATED_OUTPUT")):
        np.save(prob_file, wrong)
        with pytest.raises(ValueError, match=pattern):
            count_blobs(settings, path_in, 0, "brain", stack, engine=eng)
        assert os.listdir(post) == ["kept.txt"]
    np.save(prob_file, prob)
    with pytest.raises(MemoryError, match=r"confidence_stats.*hbm_budget_gb"):
        count_blobs(_settings(path_in, post, confidence_stats=True, hbm_budget_gb=1e-4), path_in, 0, "brain", stack, engine=eng)
    assert os.listdir(post) == ["kept.txt"]
    with pytest.raises(ValueError, match="confidence_stats"):
        count_blobs(_settings(path_in, post, confidence_stats=1), path_in, 0, "brain", stack, engine=eng)
    assert os.listdir(post) == ["kept.txt"] and count_blobs.last_confidence is None


def test_count_blobs_under_torch_distributed_equals_the_single_engine_result(eng, tmp_path, brain, monkeypatch):
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs

    ranks = _helper("thread_ranks")
    mask, prob, _ = brain
    path_in, prob_file = _brain_on_disk(tmp_path, mask, prob)
    stack = (1, 1) + mask.shape
    single = str(tmp_path / "single")
    n = count_blobs(_settings(path_in, single, confidence_stats=True), path_in, 0, "brain", stack, engine=eng)
    labels = np.load(os.path.join(single, f"brain-{n}-cc3d.npy")).astype(np.uint32)
    ref = _check_outputs(single, labels, prob, n, prob_file)
    assert len(np.unique(labels[9:11, 10, 10])) == 1 and labels[9, 10, 10] != 0  # a cell across the first cut (32 planes over 3 ranks: 10 | 11 | 11)
    fake = ranks.ThreadRanks(3)
    fake.patch(monkeypatch, dist)
    post = str(tmp_path / "sharded")
    settings = _settings(path_in, post, confidence_stats=True)
    results = ranks.run_thread_ranks(fake, lambda rank, e: count_blobs(settings, path_in, 0, "brain", stack, engine=e))
    assert results == [n] * 3
    np.testing.assert_array_equal(np.load(os.path.join(post, f"brain-{n}-cc3d.npy")), labels)
    stats = _check_outputs(post, labels, prob, n, prob_file)
    for key in ref:
        np.testing.assert_array_equal(stats[key], ref[key])
    for name in (f"{mask.shape}_brain.csv", os.path.join("cell_confidence", "brain.csv")):
        assert _read(post, name) == _read(single, name), name
