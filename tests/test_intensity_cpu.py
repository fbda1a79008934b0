"""Host side of count_blobs' per-cell intensity statistics (settings["mi355x"]["intensity_stats"]): the switch, the merge of
per-slab accumulators, the finishing step and the table - pure numpy, no device."""
import numpy as np
import pytest

from delivr_cfos_amd import hostlogic as hl


def _part(sums, sqs, mins, maxs):
    return {"intensity_sum": np.array(sums, dtype=np.uint64), "intensity_sumsq": np.array(sqs, dtype=np.uint64),
            "intensity_min": np.array(mins, dtype=np.uint16), "intensity_max": np.array(maxs, dtype=np.uint16)}


ABSENT = (0, 0, 0xFFFF, 0)


@pytest.mark.parametrize("settings, expected", [
    (None, False), ({}, False), ({"mi355x": None}, False), ({"mi355x": {}}, False), ({"mi355x": {"intensity_stats": False}}, False),
    ({"mi355x": {"intensity_stats": 0}}, False), ({"mi355x": {"size_filter": True}}, False),
    ({"postprocessing": {"intensity_stats": True}}, False),
    ({"mi355x": {"intensity_stats": True}}, True), ({"mi355x": {"intensity_stats": 1}}, True),
    ({"mi355x": {"intensity_stats": True, "size_filter": False}}, True),
])
def test_intensity_stats_enabled_truth_table(settings, expected):
    assert hl.intensity_stats_enabled(settings) is expected


def test_merge_intensity_adds_sums_and_combines_extrema_over_absent_labels_and_empty_slabs():
    # labels 0..4: 1 in both slabs, 2 in the first only, 3 in the second only with a TRUE minimum of 65535, 4 nowhere
    a = _part([0, 10, 7, 0, 0], [0, 60, 49, 0, 0], [0xFFFF, 2, 7, 0xFFFF, 0xFFFF], [0, 6, 7, 0, 0])
    b = _part([0, 2**40, 0, 131070, 0], [0, 2**60, 0, 2 * 65535**2, 0], [0xFFFF, 1, 0xFFFF, 65535, 0xFFFF], [0, 65535, 0, 65535, 0])
    keep = {k: v.copy() for k, v in a.items()}
    m = hl.merge_intensity([a, None, b])
    assert {k: v.dtype for k, v in m.items()} == {"intensity_sum": np.uint64, "intensity_sumsq": np.uint64,
                                                  "intensity_min": np.uint16, "intensity_max": np.uint16}
    np.testing.assert_array_equal(m["intensity_sum"], [0, 10 + 2**40, 7, 131070, 0])
    np.testing.assert_array_equal(m["intensity_sumsq"], [0, 60 + 2**60, 49, 2 * 65535**2, 0])
    np.testing.assert_array_equal(m["intensity_min"], [0xFFFF, 1, 7, 65535, 0xFFFF])
    np.testing.assert_array_equal(m["intensity_max"], [0, 65535, 7, 65535, 0])
    assert [tuple(int(m[k][4]) for k in hl.INTENSITY_KEYS)] == [ABSENT]  # absent everywhere stays absent
    for k in keep:
        np.testing.assert_array_equal(a[k], keep[k])  # the parts are not written to
    one = hl.merge_intensity([None, b])
    for k in hl.INTENSITY_KEYS:
        np.testing.assert_array_equal(one[k], b[k])
    with pytest.raises(ValueError):
        hl.merge_intensity([None, None])
    with pytest.raises(ValueError):
        hl.merge_intensity([a, _part([0], [0], [0xFFFF], [0])])


def test_finish_intensity_row_zero_mean_and_both_mismatches():
    merged = _part([0, 10, 131070, 2**54 + 2], [0, 38, 2 * 65535**2, 5], [0xFFFF, 1, 65535, 0], [0, 5, 65535, 9])
    counts = np.array([1000, 3, 2, 3], dtype=np.uint32)
    keep = {k: v.copy() for k, v in merged.items()}
    out = hl.finish_intensity(merged, counts)
    assert set(out) == set(hl.INTENSITY_KEYS) | {"intensity_mean"}
    np.testing.assert_array_equal(out["intensity_min"], [0, 1, 65535, 0])  # row 0: 0xFFFF -> 0; label 2's true 65535 stays
    np.testing.assert_array_equal(out["intensity_max"], [0, 5, 65535, 9])
    np.testing.assert_array_equal(out["intensity_sum"], merged["intensity_sum"])
    np.testing.assert_array_equal(out["intensity_sumsq"], merged["intensity_sumsq"])
    assert out["intensity_mean"].dtype == np.float64
    expected = merged["intensity_sum"].astype(np.float64) / counts
    expected[0] = 0.0
    np.testing.assert_array_equal(out["intensity_mean"], expected)
    assert out["intensity_mean"][1] == 10 / 3 and out["intensity_mean"][2] == 65535.0
    for k in keep:
        np.testing.assert_array_equal(merged[k], keep[k])  # (the input keeps its 0xFFFF in row 0)
    # a label without voxels anywhere: absent and count 0 agree, the mean is 0.0
    merged = _part([0, 4, 0], [0, 16, 0], [0xFFFF, 4, 0xFFFF], [0, 4, 0])
    out = hl.finish_intensity(merged, np.array([7, 1, 0], dtype=np.uint32))
    np.testing.assert_array_equal(out["intensity_mean"], [0.0, 4.0, 0.0])
    assert out["intensity_min"][2] == 0xFFFF
    # a label whose voxels are all 0 in the raw volume is NOT absent: min 0, not 0xFFFF
    zero = _part([0, 0], [0, 0], [0xFFFF, 0], [0, 0])
    assert hl.finish_intensity(zero, np.array([5, 2], dtype=np.uint32))["intensity_mean"][1] == 0.0
    # counted but not measured, and measured but not counted: labels and raw volume of different brains
    with pytest.raises(RuntimeError, match="label 2"):
        hl.finish_intensity(merged, np.array([7, 1, 3], dtype=np.uint32))
    with pytest.raises(RuntimeError, match="label 1"):
        hl.finish_intensity(merged, np.array([7, 0, 0], dtype=np.uint32))
    with pytest.raises(RuntimeError):
        hl.finish_intensity(merged, np.array([7, 1], dtype=np.uint32))  # rows that do not match


def test_cell_intensity_csv_text_three_cells_written_out():
    stats = {"voxel_counts": np.array([99, 3, 1, 2], dtype=np.uint32),
             "intensity_min": np.array([0, 1, 65535, 0], dtype=np.uint16), "intensity_max": np.array([0, 5, 65535, 4], dtype=np.uint16),
             "intensity_sum": np.array([0, 10, 65535, 4], dtype=np.uint64),
             "intensity_sumsq": np.array([0, 42, 65535**2, 16], dtype=np.uint64),
             "intensity_mean": np.array([0.0, 10 / 3, 65535.0, 2.0])}
    text = hl.cell_intensity_csv_text(stats, 3)
    assert text == ("Blob,Size,Min,Max,Sum,SumSq,Mean\n"
                    "1,3,1,5,10,42,3.3333333333333335\n"
                    "2,1,65535,65535,65535,4294836225,65535.0\n"
                    "3,2,0,4,4,16,2.0\n")
    assert hl.cell_intensity_csv_text(stats, 0) == "Blob,Size,Min,Max,Sum,SumSq,Mean\n"
    assert hl.cell_intensity_csv_text(stats, 2).count("\n") == 3  # ALL n labels: the last one is not dropped
    with pytest.raises(ValueError):
        hl.cell_intensity_csv_text(stats, 4)
