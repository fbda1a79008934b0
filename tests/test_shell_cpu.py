"""Host side of settings["mi355x"]["background_shell"] (hostlogic.background_shell_radius / merge_shell / finish_shell and the extra
columns of cell_intensity_csv_text): no device.  Integers are compared for equality, the two float columns with the same numpy
expression on the integer results."""
import numpy as np
import pytest

from delivr_cfos_amd import hostlogic
from delivr_cfos_amd.hostlogic import (SHELL_KEYS, background_shell_radius, cell_intensity_csv_text, finish_intensity, finish_shell,
                                       merge_intensity, merge_shell)


def _settings(**mi355x):
    return {"mi355x": mi355x}


def test_background_shell_radius_accepts_off_and_1_to_16():
    for off in (None, {}, {"mi355x": None}, _settings(), _settings(background_shell=None), _settings(background_shell=False),
                _settings(background_shell=0), _settings(background_shell=0, intensity_stats=True),
                _settings(background_shell=False, intensity_stats=True)):
        assert background_shell_radius(off) == 0
    for r in range(1, 17):
        got = background_shell_radius(_settings(background_shell=r, intensity_stats=True))
        assert got == r and type(got) is int
    assert background_shell_radius(_settings(background_shell=np.int64(5), intensity_stats=True)) == 5


@pytest.mark.parametrize("value", [True, -1, 17, 100, 1.0, 2.5, 0.0, "3", "", [3], (1,), {"r": 1}])
def test_background_shell_radius_refuses_everything_else(value):
    with pytest.raises(ValueError, match="background_shell"):
        background_shell_radius(_settings(background_shell=value, intensity_stats=True))


def test_background_shell_radius_needs_intensity_stats():
    for other in ({}, {"intensity_stats": False}, {"intensity_stats": 0}, {"size_filter": True}):
        with pytest.raises(ValueError, match="intensity_stats"):
            background_shell_radius(_settings(background_shell=3, **other))
    # a bad value is reported as such, with or without the other key
    with pytest.raises(ValueError, match="1..16"):
        background_shell_radius(_settings(background_shell=17))


def _acc(sums, sumsqs, mins, maxs):
    return {"intensity_sum": np.array(sums, dtype=np.uint64), "intensity_sumsq": np.array(sumsqs, dtype=np.uint64),
            "intensity_min": np.array(mins, dtype=np.uint16), "intensity_max": np.array(maxs, dtype=np.uint16)}


def test_finish_shell_rows_dtypes_and_the_zero_conventions():
    # rows: background, a shell of 3 voxels, no shell, a shell of one voxel of 65535
    parts = _acc([0, 60, 0, 65535], [0, 1400, 0, 65535**2], [0xFFFF, 10, 0xFFFF, 65535], [0, 30, 0, 65535])
    counts = np.array([1000, 3, 0, 1], dtype=np.uint32)  # (row 0 of cc_counts: the voxels outside every shell)
    cells = np.array([0.0, 40.0, 7.5, 131070.0 / 3])
    out = finish_shell(parts, counts, cells)
    assert tuple(out) == SHELL_KEYS
    assert [out[k].dtype for k in SHELL_KEYS] == [np.uint32, np.uint64, np.uint64, np.uint16, np.uint16, np.float64, np.float64]
    assert all(len(out[k]) == 4 for k in SHELL_KEYS)
    assert out["shell_voxels"].tolist() == [0, 3, 0, 1]
    assert out["shell_sum"].tolist() == [0, 60, 0, 65535] and out["shell_sumsq"].tolist() == [0, 1400, 0, 65535**2]
    assert out["shell_min"].tolist() == [0, 10, 0, 65535] and out["shell_max"].tolist() == [0, 30, 0, 65535]
    np.testing.assert_array_equal(out["shell_mean"], np.array([0.0, np.float64(60) / np.float64(3), 0.0, 65535.0]))
    np.testing.assert_array_equal(out["contrast"], np.array([0.0, 40.0 / (np.float64(60) / np.float64(3)), 0.0, cells[3] / 65535.0]))
    assert all(int(np.asarray(out[k][0])) == 0 for k in SHELL_KEYS)  # row 0 all zeros
    # the inputs are not modified
    assert parts["intensity_min"].tolist() == [0xFFFF, 10, 0xFFFF, 65535] and counts[0] == 1000
    # N = 0: one row of zeros
    zero = finish_shell(_acc([0], [0], [0xFFFF], [0]), np.array([125], dtype=np.uint32), np.array([0.0]))
    assert {k: v.tolist() for k, v in zero.items()} == {k: [0] for k in SHELL_KEYS}


def test_finish_shell_raises_when_measured_and_counted_disagree():
    cells = np.zeros(3)
    with pytest.raises(RuntimeError, match=r"first label 2: 4 voxels counted, none measured"):
        finish_shell(_acc([0, 5, 0], [0, 25, 0], [0xFFFF, 5, 0xFFFF], [0, 5, 0]), np.array([9, 1, 4], dtype=np.uint32), cells)
    with pytest.raises(RuntimeError, match=r"first label 1: 0 voxels counted, some measured"):
        finish_shell(_acc([0, 5, 0], [0, 25, 0], [0xFFFF, 5, 0xFFFF], [0, 5, 0]), np.array([9, 0, 0], dtype=np.uint32), cells)
    with pytest.raises(RuntimeError, match="rows"):
        finish_shell(_acc([0, 5], [0, 25], [0xFFFF, 5], [0, 5]), np.array([9, 1, 0], dtype=np.uint32), cells)
    with pytest.raises(RuntimeError, match="rows"):
        finish_shell(_acc([0, 5, 0], [0, 25, 0], [0xFFFF, 5, 0xFFFF], [0, 5, 0]), np.array([9, 1, 0], dtype=np.uint32), np.zeros(2))


def test_slab_parts_merge_with_merge_intensity_and_a_sum_of_the_counts():
    a = (_acc([0, 10, 0, 7], [0, 100, 0, 49], [0xFFFF, 10, 0xFFFF, 7], [0, 10, 0, 7]), np.array([50, 1, 0, 1], dtype=np.uint32))
    b = (_acc([0, 2**40, 9, 0], [0, 2**50, 41, 0], [0xFFFF, 3, 4, 0xFFFF], [0, 65535, 5, 0]), np.array([60, 2**31, 2, 0], dtype=np.uint32))
    c = (_acc([0, 2**40, 0, 0], [0, 2**50, 0, 0], [0xFFFF, 1, 0xFFFF, 0xFFFF], [0, 9, 0, 0]), np.array([70, 2**31, 0, 0], dtype=np.uint32))
    merged, counts = merge_shell([a, None, b])
    assert counts.dtype == np.uint64 and counts.tolist() == [110, 2**31 + 1, 2, 1]
    ref = merge_intensity([a[0], b[0]])
    for k in ref:
        np.testing.assert_array_equal(merged[k], ref[k])
    assert merged["intensity_sum"].tolist() == [0, 2**40 + 10, 9, 7] and merged["intensity_min"].tolist() == [0xFFFF, 3, 4, 7]
    out = finish_shell(merged, counts, np.array([0.0, 1.0, 2.0, 3.0]))
    assert out["shell_voxels"].tolist() == [0, 2**31 + 1, 2, 1]
    np.testing.assert_array_equal(out["shell_mean"][1:], merged["intensity_sum"][1:].astype(np.float64) / counts[1:].astype(np.float64))
    # three slabs whose counts sum past uint32: refused, not wrapped
    with pytest.raises(RuntimeError, match="2\\^32"):
        finish_shell(*merge_shell([a, b, c]), np.zeros(4))
    with pytest.raises(ValueError):
        merge_shell([a, (b[0], b[1][:3])])
    with pytest.raises(ValueError):
        merge_shell([None, None])


def _cell_stats():
    counts = np.array([900, 2, 1, 3], dtype=np.uint32)
    stats = {"voxel_counts": counts}
    stats.update(finish_intensity(_acc([0, 100, 65535, 10], [0, 5200, 65535**2, 38], [0xFFFF, 40, 65535, 1], [0, 60, 65535, 5]), counts))
    return stats


def test_csv_text_without_the_shell_keys_is_unchanged_and_with_them_gains_seven_columns():
    stats = _cell_stats()
    plain = cell_intensity_csv_text(stats, 3)
    mean = stats["intensity_mean"]
    assert plain == ("Blob,Size,Min,Max,Sum,SumSq,Mean\n"
                     f"1,2,40,60,100,5200,{float(mean[1])!r}\n"
                     f"2,1,65535,65535,65535,{65535**2},{float(mean[2])!r}\n"
                     f"3,3,1,5,10,38,{float(mean[3])!r}\n")
    assert plain.splitlines()[1] == "1,2,40,60,100,5200,50.0"
    shell = finish_shell(_acc([0, 7, 0, 2**33], [0, 25, 0, 2**49], [0xFFFF, 3, 0xFFFF, 2], [0, 4, 0, 65535]),
                         np.array([800, 2, 0, 70000], dtype=np.uint32), mean)
    # some of the keys only (a pickle of another version): the text of today
    partial = dict(stats, **{k: shell[k] for k in SHELL_KEYS[:-1]})
    assert cell_intensity_csv_text(partial, 3) == plain
    full = dict(stats, **shell, shell_radius=3)
    text = cell_intensity_csv_text(full, 3)
    lines = text.splitlines()
    assert text.endswith("\n") and len(lines) == 4
    assert lines[0] == "Blob,Size,Min,Max,Sum,SumSq,Mean,ShellSize,ShellMin,ShellMax,ShellSum,ShellSumSq,ShellMean,Contrast"
    for got, old, row in zip(lines[1:], plain.splitlines()[1:], (1, 2, 3)):
        assert got == (f"{old},{int(shell['shell_voxels'][row])},{int(shell['shell_min'][row])},{int(shell['shell_max'][row])},"
                       f"{int(shell['shell_sum'][row])},{int(shell['shell_sumsq'][row])},{float(shell['shell_mean'][row])!r},"
                       f"{float(shell['contrast'][row])!r}")
    assert lines[1] == f"1,2,40,60,100,5200,50.0,2,3,4,7,25,3.5,{50.0 / 3.5!r}"
    assert lines[2].endswith(",0,0,0,0,0,0.0,0.0")  # a cell without a shell
    with pytest.raises(ValueError, match="shorter"):
        cell_intensity_csv_text(dict(full, contrast=shell["contrast"][:3]), 3)
    assert hostlogic.SHELL_MAX_RADIUS == 16
