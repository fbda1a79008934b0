"""The run-length label file on the host (delivr_cfos_amd/label_runs.py), its settings key (hostlogic.label_file_format) and
count_blobs' refusal of it under torch.distributed.  No GPU.  Every comparison is integer equality."""
import importlib.util
import os
import threading

import numpy as np
import pytest

from delivr_cfos_amd import label_runs as lr


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _volume(shape=(3, 4, 19), seed=3):
    """sparse runs, touching runs of different labels, a run at either end of a row, an empty and a full row"""
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, dtype=np.uint32)
    flat = v.reshape(-1, shape[2])
    for row in flat[2:]:
        x = int(rng.integers(0, 3))
        while x < shape[2]:
            n = int(rng.integers(1, 5))
            row[x:x + n] = rng.integers(1, 9)
            x += n + int(rng.integers(0, 4))
    flat[1] = 7
    assert not flat[0].any() and flat[:, 0].any() and flat[:, -1].any()
    assert ((flat[:, 1:] != flat[:, :-1]) & (flat[:, 1:] != 0) & (flat[:, :-1] != 0)).any()  # two runs touch
    return v


def _loop_encode(v):
    """the definition, voxel by voxel"""
    Z, Y, X = v.shape
    row_start, x0, x1, label = [0], [], [], []
    for z in range(Z):
        for y in range(Y):
            row = v[z, y]
            for x in range(X):
                lab = int(row[x])
                if lab != 0 and (x == 0 or lab != int(row[x - 1])):
                    x0.append(x)
                    label.append(lab)
                if lab != 0 and (x == X - 1 or lab != int(row[x + 1])):
                    x1.append(x)
            row_start.append(len(x0))
    return (np.array(row_start, dtype=np.uint64), np.array(x0, dtype=np.uint16), np.array(x1, dtype=np.uint16),
            np.array(label, dtype=np.uint32))


def _assert_runs_equal(got, want):
    assert tuple(got["shape"]) == tuple(want["shape"])
    for key, dtype in lr.ARRAYS:
        assert got[key].dtype == dtype, key
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def test_encode_runs_against_a_double_loop():
    v = _volume()
    runs = lr.encode_runs(v)
    assert runs["shape"] == (3, 4, 19)
    for (key, dtype), want in zip(lr.ARRAYS, _loop_encode(v)):
        assert runs[key].dtype == dtype and runs[key].shape == want.shape, key
        np.testing.assert_array_equal(runs[key], want, err_msg=key)
    assert len(runs["row_start"]) == 3 * 4 + 1 and int(runs["row_start"][-1]) == len(runs["label"]) > 12


def test_decode_inverts_encode_also_on_a_plane_range():
    v = _volume((5, 4, 19), seed=4)
    runs = lr.encode_runs(v)
    out = lr.decode_runs(runs)
    assert out.dtype == np.uint32
    np.testing.assert_array_equal(out, v)
    np.testing.assert_array_equal(lr.decode_runs(runs, 1, 4), v[1:4])
    np.testing.assert_array_equal(lr.decode_runs(runs, 4), v[4:])
    zeros = np.zeros((2, 3, 5), dtype=np.uint32)
    runs0 = lr.encode_runs(zeros)
    assert len(runs0["label"]) == 0 and not runs0["row_start"].any()
    np.testing.assert_array_equal(lr.decode_runs(runs0), zeros)
    wide = np.zeros((1, 2, 65536), dtype=np.uint32)
    wide[0, 0] = 2**32 - 2
    wide[0, 1, 65530:] = 3
    runs_w = lr.encode_runs(wide)
    assert runs_w["x1"].tolist() == [65535, 65535] and runs_w["x0"].tolist() == [0, 65530]
    np.testing.assert_array_equal(lr.decode_runs(runs_w), wide)
    with pytest.raises(ValueError, match="65536"):
        lr.encode_runs(np.zeros((1, 1, 65537), dtype=np.uint32))


def test_file_round_trip_and_the_dense_cache_lookup_does_not_see_it(tmp_path):
    from delivr_cfos_amd.count_blobs import load_cached_brain, load_cached_runs

    v = _volume()
    runs = lr.encode_runs(v)
    name = lr.runs_name("brain", 8)
    assert name == "brain-8-cc3d.runs" and ".npy" not in name
    path = str(tmp_path / name)
    lr.save_runs(path, runs, 8)
    assert os.listdir(str(tmp_path)) == [name]  # (no .partial left)
    got = lr.load_runs(path)
    assert got["n"] == 8
    _assert_runs_equal(got, runs)
    np.testing.assert_array_equal(lr.load_labels(path), v)
    np.testing.assert_array_equal(lr.load_labels(path, 1, 3), v[1:3])
    with open(path, "rb") as fh:  # five arrays back to back, readable with five np.load
        header = np.load(fh)
        parts = [np.load(fh) for _ in range(4)]
        assert fh.read() == b""
    assert header.dtype == np.uint64 and header.tolist() == [lr.MAGIC, 1, 3, 4, 19, 8, len(runs["label"]), 0]
    for (key, _), part in zip(lr.ARRAYS, parts):
        np.testing.assert_array_equal(part, runs[key])
    settings = {"postprocessing": {"output_location": str(tmp_path)}}
    assert load_cached_brain(settings, "brain") is False
    assert load_cached_runs(settings, "brain") == (path, 8)
    assert load_cached_runs(settings, "other") is False


def _corrupt(runs, rule):
    r = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in runs.items()}
    n, header = 8, None
    first = int(np.flatnonzero(np.diff(r["row_start"].astype(np.int64)) >= 2)[0])  # a row with two runs or more
    k = int(r["row_start"][first])
    if rule == "magic":
        header = {0: lr.MAGIC + 1}
    elif rule == "version":
        header = {1: 2}
    elif rule == "row_start length":
        r["row_start"] = r["row_start"][:-1]
    elif rule == "run count":
        header = {6: len(r["label"]) + 1}
    elif rule == "x1 length":
        r["x1"] = r["x1"][:-1]
    elif rule == "row_start decreases":
        r["row_start"][1] = r["row_start"][2] + 1  # (entry 2 is the one that goes down)
    elif rule == "row_start end":
        r["row_start"][-1] += 1
    elif rule == "x0 above x1":
        r["x0"][k], r["x1"][k] = 5, 4
    elif rule == "x1 beyond X":
        r["x1"][len(r["x1"]) - 1] = 19
    elif rule == "runs overlap":
        r["x0"][k + 1] = r["x1"][k]
    elif rule == "runs out of order":
        for key in ("x0", "x1"):
            r[key][k], r[key][k + 1] = r[key][k + 1], r[key][k]
    elif rule == "label zero":
        r["label"][k] = 0
    elif rule == "label above N":
        r["label"][k] = n + 1
    else:
        raise AssertionError(rule)
    return r, n, header


RULES = ("magic", "version", "row_start length", "run count", "x1 length", "row_start decreases", "row_start end", "x0 above x1",
         "x1 beyond X", "runs overlap", "runs out of order", "label zero", "label above N")


@pytest.mark.parametrize("rule", RULES)
def test_one_corrupted_file_per_validation_rule(tmp_path, rule):
    runs = lr.encode_runs(_volume())
    bad, n, header = _corrupt(runs, rule)
    path = str(tmp_path / "brain-8-cc3d.runs")
    head = np.array([lr.MAGIC, lr.VERSION, 3, 4, 19, n, len(runs["label"]), 0], dtype=np.uint64)
    for at, value in (header or {}).items():
        head[at] = value
    with open(path, "wb") as fh:
        np.lib.format.write_array(fh, head)
        for key, dtype in lr.ARRAYS:
            np.lib.format.write_array(fh, np.ascontiguousarray(bad[key], dtype=dtype))
    with pytest.raises(ValueError, match="brain-8-cc3d.runs"):
        lr.load_runs(path)
    with pytest.raises(ValueError):
        lr.load_labels(path)


def test_a_file_that_is_not_a_run_file_and_a_truncated_one(tmp_path):
    path = str(tmp_path / "brain-8-cc3d.runs")
    np.save(path + ".npy", np.zeros(8, dtype=np.uint32))
    os.replace(path + ".npy", path)
    with pytest.raises(ValueError, match="not a run-length label file"):
        lr.load_runs(path)
    runs = lr.encode_runs(_volume())
    lr.save_runs(path, runs, 8)
    size = os.path.getsize(path)
    with open(path, "r+b") as fh:
        fh.truncate(size - 3)
    with pytest.raises(ValueError, match="brain-8-cc3d.runs"):
        lr.load_runs(path)


def test_label_file_format_and_the_options_record():
    from delivr_cfos_amd.hostlogic import CountOptions, count_options, label_file_format

    assert label_file_format({}) == "dense" and label_file_format(None) == "dense" and label_file_format({"mi355x": {}}) == "dense"
    assert label_file_format({"mi355x": {"label_file": "dense"}}) == "dense"
    assert label_file_format({"mi355x": {"label_file": "runs"}}) == "runs"
    for bad in ("rle", 1, True, "", "RUNS", ["runs"]):
        with pytest.raises(ValueError, match="label_file"):
            label_file_format({"mi355x": {"label_file": bad}})
        with pytest.raises(ValueError, match="label_file"):
            count_options({"mi355x": {"label_file": bad}}, -1, -1)
    assert CountOptions().label_file == "dense" and not CountOptions().runs_file
    assert count_options({}, -1, -1) == CountOptions()
    opts = count_options({"mi355x": {"label_file": "runs"}}, -1, -1)
    assert opts.label_file == "runs" and opts.runs_file and opts == CountOptions(label_file="runs")


def test_the_slab_streamed_path_and_oversized_decoded_labels_are_refused():
    from delivr_cfos_amd.hostlogic import CountOptions, check_hbm_budget

    opts, V = CountOptions(label_file="runs"), 2**30
    assert check_hbm_budget(opts, frozenset(), False, 5, V, 5 * V) is None
    with pytest.raises(MemoryError, match=r"label_file'\] = \"runs\".*slab-streamed labelling does not write run-length labels"):
        check_hbm_budget(opts, frozenset(), False, 5, V, 5 * V - 1)
    assert check_hbm_budget(CountOptions(), frozenset(), False, 5, V, 0) is None  # (the default is streamed as before)
    # a cached labelling: only a run file that is decoded counts
    assert check_hbm_budget(opts, frozenset(), True, 4, V, 0) is None
    assert check_hbm_budget(opts, frozenset(), True, 4, V, 4 * V, runs_decoded=True) is None
    with pytest.raises(MemoryError, match=r"label_file'\] = \"runs\" needs the cached labels in HBM \(4\.0 GiB\), the HBM budget is"):
        check_hbm_budget(opts, frozenset(), True, 4, V, 4 * V - 1, runs_decoded=True)


def test_two_ranks_raise_the_same_value_error_before_any_collective(tmp_path, monkeypatch):
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs

    ranks = _helper("thread_ranks")
    shape = (4, 6, 10)
    d = tmp_path / "in" / "brain" / "binary_segmentations"
    os.makedirs(d)
    np.save(str(d / "binaries.npy"), np.zeros(shape, dtype=np.uint8))
    post = str(tmp_path / "post")
    fake = ranks.ThreadRanks(2)
    fake.patch(monkeypatch, dist)
    settings = {"postprocessing": {"output_location": post + "/"}, "mi355x": {"label_file": "runs"}}
    caught = [None] * 2

    def rank_main(rank):
        fake.bind(rank)
        try:
            count_blobs(settings, str(tmp_path / "in"), 0, "brain", (1, 1) + shape, engine=object())  # (refused before the engine is used)
        except BaseException as exc:  # noqa: BLE001
            caught[rank] = exc

    ts = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not any(t.is_alive() for t in ts)  # nobody waits in a collective
    assert all(type(c) is ValueError for c in caught), caught
    assert len({str(c) for c in caught}) == 1 and "label_file" in str(caught[0]) and "torch.distributed" in str(caught[0])
    assert not os.path.exists(post)
