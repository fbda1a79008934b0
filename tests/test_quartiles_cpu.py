"""Host side of the per-cell intensity quartiles (settings["mi355x"]["intensity_quartiles"]), no GPU: the numpy reference of the
GPU tests pinned by hand-worked cells, hostlogic's finish / settings / table functions, and the refusal under torch.distributed."""
import importlib.util
import os
import threading

import numpy as np
import pytest


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# label -> (its raw values in storage order, the expected value at the levels 0, 25, 50, 75, 100)
#   m = 1: every index 0.  m = 2: (25, 50, 75) * 1 // 100 = 0, 0, 0.  m = 3: 0, 1, 1.  m = 4: 0, 1, 2.  m = 5: 1, 2, 3.
#   m = 100: 24, 49, 74.  m = 101: 25, 50, 75.
HAND_CELLS = {
    1: ([7], (7, 7, 7, 7, 7)),
    2: ([9, 3], (3, 3, 3, 3, 9)),
    3: ([5, 5, 1], (1, 1, 5, 5, 5)),                      # sorted 1 5 5
    4: ([8, 2, 2, 6], (2, 2, 2, 6, 8)),                   # sorted 2 2 6 8
    5: ([4, 4, 4, 0, 65535], (0, 4, 4, 4, 65535)),        # sorted 0 4 4 4 65535
    6: ([i // 2 for i in range(100)], (0, 12, 24, 37, 49)),         # pairs of ties: sorted[k] = k // 2
    7: ([1000 - i for i in range(101)], (900, 925, 950, 975, 1000)),  # stored descending: sorted[k] = 900 + k
    9: ([0], (0, 0, 0, 0, 0)),                            # a true 0 beside the absent label 8
}


def _hand_volume():
    rng = np.random.default_rng(3)
    voxels = [(lab, v) for lab, (vals, _) in HAND_CELLS.items() for v in vals]
    voxels += [(10, 123), (11, 5)]  # labels above n = 9: not measured
    voxels += [(0, int(v)) for v in rng.integers(0, 65536, size=40)]  # background
    voxels = [voxels[i] for i in rng.permutation(len(voxels))]
    size = 4 * 8 * 9
    assert len(voxels) <= size
    voxels += [(0, 77)] * (size - len(voxels))
    labels = np.array([l for l, _ in voxels], dtype=np.uint32).reshape(4, 8, 9)
    raw = np.array([v for _, v in voxels], dtype=np.uint16).reshape(4, 8, 9)
    return labels, raw


def test_the_reference_on_hand_worked_cells():
    ref = _helper("quantile_reference").quantile_reference
    labels, raw = _hand_volume()
    values, counts = ref(labels, raw, 9, (0, 25, 50, 75, 100))
    assert values.dtype == np.uint16 and values.shape == (10, 5) and counts.dtype == np.uint32 and counts.shape == (10,)
    for lab, (vals, expected) in HAND_CELLS.items():
        assert tuple(int(v) for v in values[lab]) == expected, lab
        assert int(counts[lab]) == len(vals)
    assert not values[0].any() and counts[0] == 0  # the background is not measured
    assert not values[8].any() and counts[8] == 0 and counts[9] == 1  # absent, against a true 0
    three, counts3 = ref(labels, raw, 9)  # the default levels are the quartiles
    np.testing.assert_array_equal(three, values[:, 1:4])
    np.testing.assert_array_equal(counts3, counts)
    few, counts_few = ref(labels, raw, 4, (0, 25, 50, 75, 100))  # a smaller n: the first rows
    np.testing.assert_array_equal(few, values[:5])
    np.testing.assert_array_equal(counts_few, counts[:5])
    for lab in (6, 7):  # ... and numpy's own lower percentile
        v = raw[labels == lab]
        assert [int(np.percentile(v, p, method="lower")) for p in (25, 50, 75)] == [int(x) for x in three[lab]]


def test_finish_quartiles_dtypes_row_0_absent_label_and_disagreeing_counts():
    from delivr_cfos_amd.hostlogic import QUARTILE_KEYS, QUARTILE_LEVELS, finish_quartiles

    assert QUARTILE_LEVELS == (25, 50, 75) and QUARTILE_KEYS == ("intensity_q25", "intensity_median", "intensity_q75")
    values = np.array([[9, 9, 9], [1, 2, 3], [0, 0, 0], [0, 0, 65535]], dtype=np.uint16)  # (row 0 is zeroed whatever it holds)
    counts = np.array([0, 5, 0, 4], dtype=np.uint32)
    voxel_counts = np.array([1000, 5, 0, 4], dtype=np.uint32)  # (row 0: the background's voxels, not compared)
    out = finish_quartiles(values, counts, voxel_counts)
    assert list(out) == list(QUARTILE_KEYS)
    assert all(a.dtype == np.uint16 and a.shape == (4,) for a in out.values())
    assert out["intensity_q25"].tolist() == [0, 1, 0, 0]
    assert out["intensity_median"].tolist() == [0, 2, 0, 0]
    assert out["intensity_q75"].tolist() == [0, 3, 0, 65535]
    assert values[0].tolist() == [9, 9, 9]  # the input is not modified
    with pytest.raises(RuntimeError, match="first label 2"):
        finish_quartiles(values, np.array([0, 5, 1, 3], dtype=np.uint32), voxel_counts)
    with pytest.raises(RuntimeError):
        finish_quartiles(values[:3], counts[:3], voxel_counts)
    with pytest.raises(RuntimeError):
        finish_quartiles(values[:, :2], counts, voxel_counts)


def test_finish_shell_quartiles_contrast_median():
    from delivr_cfos_amd.hostlogic import SHELL_QUARTILE_KEYS, finish_shell_quartiles

    values = np.array([[0, 0, 0], [10, 20, 30], [0, 0, 0], [1, 3, 3]], dtype=np.uint16)
    counts = np.array([0, 50, 0, 7], dtype=np.uint32)
    median = np.array([0, 30, 40, 100], dtype=np.uint16)
    out = finish_shell_quartiles(values, counts, counts.copy(), median)
    assert list(out) == list(SHELL_QUARTILE_KEYS)
    assert out["shell_q25"].tolist() == [0, 10, 0, 1] and out["shell_median"].tolist() == [0, 20, 0, 3]
    assert out["shell_q75"].tolist() == [0, 30, 0, 3] and out["shell_median"].dtype == np.uint16
    assert out["contrast_median"].dtype == np.float64
    assert out["contrast_median"].tolist() == [0.0, 30 / 20, 0.0, 100 / 3]  # 0.0 for a cell without a shell
    with pytest.raises(RuntimeError, match="first label 3"):
        finish_shell_quartiles(values, counts, np.array([0, 50, 0, 8], dtype=np.uint32), median)


def test_intensity_quartiles_enabled():
    from delivr_cfos_amd.hostlogic import intensity_quartiles_enabled

    assert intensity_quartiles_enabled({"mi355x": {"intensity_stats": True, "intensity_quartiles": True}}) is True
    assert intensity_quartiles_enabled({"mi355x": {"intensity_stats": True, "intensity_quartiles": False}}) is False
    assert intensity_quartiles_enabled({"mi355x": {"intensity_quartiles": False}}) is False
    assert intensity_quartiles_enabled({"mi355x": {"intensity_stats": True}}) is False
    assert intensity_quartiles_enabled({"mi355x": {}}) is False
    assert intensity_quartiles_enabled({}) is False and intensity_quartiles_enabled(None) is False
    for bad in (1, 0, "true", 1.0, [True]):
        with pytest.raises(ValueError, match="intensity_quartiles"):
            intensity_quartiles_enabled({"mi355x": {"intensity_stats": True, "intensity_quartiles": bad}})
    for without in ({"mi355x": {"intensity_quartiles": True}}, {"mi355x": {"intensity_quartiles": True, "intensity_stats": False}}):
        with pytest.raises(ValueError, match="needs settings.*intensity_stats"):
            intensity_quartiles_enabled(without)


def test_cell_quartiles_csv_text_exact():
    from delivr_cfos_amd.hostlogic import cell_quartiles_csv_text

    stats = {"voxel_counts": np.array([900, 5, 0, 4], dtype=np.uint32),
             "intensity_q25": np.array([0, 1, 0, 0], dtype=np.uint16),
             "intensity_median": np.array([0, 2, 0, 0], dtype=np.uint16),
             "intensity_q75": np.array([0, 3, 0, 65535], dtype=np.uint16)}
    assert cell_quartiles_csv_text(stats, 3) == "Blob,Size,Q25,Median,Q75\n1,5,1,2,3\n2,0,0,0,0\n3,4,0,0,65535\n"
    assert cell_quartiles_csv_text(stats, 0) == "Blob,Size,Q25,Median,Q75\n"
    shell = dict(stats, shell_voxels=np.array([0, 50, 0, 7], dtype=np.uint32), shell_q25=np.array([0, 10, 0, 1], dtype=np.uint16),
                 shell_median=np.array([0, 20, 0, 3], dtype=np.uint16), shell_q75=np.array([0, 30, 0, 3], dtype=np.uint16),
                 contrast_median=np.array([0.0, 0.1, 0.0, 0.0], dtype=np.float64))
    assert cell_quartiles_csv_text(shell, 3) == ("Blob,Size,Q25,Median,Q75,ShellSize,ShellQ25,ShellMedian,ShellQ75,ContrastMedian\n"
                                                 "1,5,1,2,3,50,10,20,30,0.1\n2,0,0,0,0,0,0,0,0,0.0\n3,4,0,0,65535,7,1,3,3,0.0\n")
    partial = {k: v for k, v in shell.items() if k != "shell_q75"}  # an incomplete set of shell keys: the cells' columns alone
    assert cell_quartiles_csv_text(partial, 3) == cell_quartiles_csv_text(stats, 3)
    with pytest.raises(ValueError):
        cell_quartiles_csv_text(stats, 4)


def test_count_blobs_under_torch_distributed_refuses_the_key_before_opening_any_file(tmp_path, monkeypatch):
    import torch.distributed as dist
    from delivr_cfos_amd.count_blobs import count_blobs

    ranks = _helper("thread_ranks")
    fake = ranks.ThreadRanks(2)
    fake.patch(monkeypatch, dist)
    path_in, post = str(tmp_path / "in"), str(tmp_path / "post")  # (neither exists: nothing may be opened or created)
    settings = {"postprocessing": {"output_location": post + "/"}, "blob_detection": {"input_location": path_in},
                "mi355x": {"intensity_stats": True, "intensity_quartiles": True}}
    caught = [None] * 2

    def rank_main(rank):
        fake.bind(rank)
        try:
            count_blobs(settings, path_in, 0, "brain", (1, 1, 8, 8, 8), engine=object())  # (refused before the engine is used)
        except BaseException as exc:  # noqa: BLE001
            caught[rank] = exc

    ts = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not any(t.is_alive() for t in ts)  # nobody waits in a collective
    assert all(type(c) is ValueError for c in caught), caught
    assert len({str(c) for c in caught}) == 1 and "intensity_quartiles" in str(caught[0]) and "torch.distributed" in str(caught[0])
    assert not os.path.exists(post) and not os.path.exists(path_in)
    assert count_blobs.last_quartiles is None
