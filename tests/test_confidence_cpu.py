"""Host side of count_blobs' per-cell confidence (settings["mi355x"]["confidence_stats"]): the key's parser, its rows in the measuring
plan and in the HBM check, the merge of slabs, the finished keys and the table's text - numpy only, no device."""
import numpy as np
import pytest

from delivr_cfos_amd import hostlogic as hl

ABSENT = (0, 0xFFFFFFFF, 0, 2**64 - 1)


def _part(rows):
    """rows: (sum, min_q, max_q, peak_index) per label 0..n -> HipEngine.cc_confidence's dict"""
    cols = list(zip(*rows))
    return {"confidence_sum": np.array(cols[0], dtype=np.uint64), "confidence_min_q": np.array(cols[1], dtype=np.uint32),
            "confidence_max_q": np.array(cols[2], dtype=np.uint32), "confidence_peak_index": np.array(cols[3], dtype=np.uint64)}


# ---- the key ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("settings, expected", [(None, False), ({}, False), ({"mi355x": None}, False), ({"mi355x": {}}, False),
                                                ({"mi355x": {"confidence_stats": False}}, False),
                                                ({"mi355x": {"confidence_stats": True}}, True)])
def test_the_key_is_a_bool(settings, expected):
    assert hl.confidence_stats_enabled(settings) is expected
    assert hl.count_options(settings, -1, -1).confidence is expected


@pytest.mark.parametrize("bad", [1, 0, "true", 1.0, [True], np.bool_(True)])
def test_anything_but_a_bool_is_refused(bad):
    with pytest.raises(ValueError, match="confidence_stats"):
        hl.confidence_stats_enabled({"mi355x": {"confidence_stats": bad}})
    with pytest.raises(ValueError, match="confidence_stats"):
        hl.count_options({"mi355x": {"confidence_stats": bad}}, -1, -1)


def test_the_scale_and_the_default_record():
    assert hl.CONFIDENCE_SCALE == 1 << 24
    assert hl.CountOptions().confidence is False


def test_quantise_confidence_is_the_definition():
    p = np.array([0.0, 0.5, 1.0, 2.0**-30, -0.25, 1.5, np.nan, np.inf, -np.inf, 3 * 2.0**-25, 5 * 2.0**-25], dtype=np.float32)
    assert hl.quantise_confidence(p).tolist() == [0, 1 << 23, 1 << 24, 0, 0, 1 << 24, 0, 1 << 24, 0, 2, 2]  # (1.5 -> 2, 2.5 -> 2: half to even)
    assert hl.quantise_confidence(p).dtype == np.uint32
    # the half-way values (2k + 1) * 2^-25, k < 2^21, of both parities: exact in float32, and k + 1/2 goes to the even neighbour
    k = np.array([0, 1, 2, 3, 2**20, 2**20 + 1, 2**21 - 2, 2**21 - 1], dtype=np.int64)
    half = ((2 * k + 1).astype(np.float64) * 2.0**-25).astype(np.float32)
    assert np.array_equal(half.astype(np.float64), (2 * k + 1) * 2.0**-25)
    assert hl.quantise_confidence(half).tolist() == [int(v + (v & 1)) for v in k]
    assert hl.quantise_confidence(np.float32(-0.0)).tolist() == 0 and hl.quantise_confidence(np.zeros((2, 3), np.float32)).shape == (2, 3)


# ---- the measuring plan -------------------------------------------------------------------------------------------------------------
def test_measuring_plan_group_is_complete_only_with_every_key():
    on = hl.CountOptions(confidence=True)
    assert "confidence" not in hl.RAW_GROUPS
    assert hl.measuring_plan(hl.CountOptions(), None) == frozenset()
    assert hl.measuring_plan(on, None) == {"confidence"}
    assert hl.measuring_plan(on, {"voxel_counts": 0}) == {"confidence"}
    full = {k: 0 for k in hl.CONFIDENCE_KEYS}
    assert set(hl.CONFIDENCE_KEYS) == {"confidence_sum", "confidence_min", "confidence_max", "confidence_mean", "confidence_peak"}
    assert hl.measuring_plan(on, full) == frozenset()
    for k in hl.CONFIDENCE_KEYS:
        assert hl.measuring_plan(on, {j: 0 for j in full if j != k}) == {"confidence"}, k
    assert hl.measuring_plan(hl.CountOptions(), full) == frozenset()  # (not asked for: nothing to take)
    both = hl.CountOptions(confidence=True, intensity=True)
    assert hl.measuring_plan(both, full) == {"cells"} and hl.measuring_plan(both, None) == {"cells", "confidence"}


# ---- the HBM check ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cached, base", [(False, 9), (True, 4)])
def test_hbm_row_fits_up_to_base_plus_4_bytes_per_voxel(cached, base):
    opts = hl.CountOptions(confidence=True)
    voxels = 1000
    hl.check_hbm_budget(opts, {"confidence"}, cached, base, voxels, voxels * (base + 4))  # fits exactly
    with pytest.raises(MemoryError, match=r"confidence_stats.*hbm_budget_gb") as exc:
        hl.check_hbm_budget(opts, {"confidence"}, cached, base, voxels, voxels * (base + 4) - 1)
    assert ("slab-streamed labelling does not measure" in str(exc.value)) == (not cached)
    hl.check_hbm_budget(opts, frozenset(), cached, base, voxels, voxels * base)  # nothing left to measure: no extra volume
    assert "confidence_stats" in hl._HBM_FRESH and "confidence_stats" in hl._HBM_CACHED
    for order in (hl._HBM_FRESH, hl._HBM_CACHED):
        assert order.index("confidence_stats") == order.index("intensity_quartiles") + 1


# ---- merge and finish ---------------------------------------------------------------------------------------------------------------
def test_merge_confidence_on_hand_made_slabs():
    plane = 6  # (Y, X) = (2, 3)
    # labels 1..4; slab A = planes [0, 2), slab B = planes [2, 3)
    a = _part([ABSENT, (10, 3, 7, 4), (5, 5, 5, 11), ABSENT, (9, 9, 9, 0)])
    b = _part([ABSENT, (20, 2, 7, 1), (6, 6, 6, 0), ABSENT, (0, 0, 0, 5)])
    want = _part([ABSENT, (30, 2, 7, 4), (11, 5, 6, 12), ABSENT, (9, 0, 9, 0)])  # 1: a tie in q, the smaller global index; 2: the larger q
    for order in ([(a, 0, plane), (b, 2, plane)], [(b, 2, plane), None, (a, 0, plane)]):
        got = hl.merge_confidence(order)
        for k, dt in zip(hl.CONFIDENCE_RAW_KEYS, (np.uint64, np.uint32, np.uint32, np.uint64)):
            assert got[k].dtype == dt
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    # a voxel of q = 0 in one slab beats the absent row of the other, whatever the order
    zero, none = _part([ABSENT, (0, 0, 0, 3)]), _part([ABSENT, ABSENT])
    for order in ([(zero, 1, plane), (none, 0, plane)], [(none, 0, plane), (zero, 1, plane)]):
        got = hl.merge_confidence(order)
        assert [int(got[k][1]) for k in hl.CONFIDENCE_RAW_KEYS] == [0, 0, 0, 9]
    with pytest.raises(ValueError, match="no slab"):
        hl.merge_confidence([None])
    with pytest.raises(ValueError, match="same labels"):
        hl.merge_confidence([(a, 0, plane), (zero, 2, plane)])


def test_finish_confidence_keys_values_and_the_inconsistency_errors():
    shape = (3, 2, 3)
    merged = _part([ABSENT, (3 << 23, 1 << 23, 1 << 24, 17), ABSENT, (1 << 22, 1 << 22, 1 << 22, 4)])
    counts = np.array([11, 2, 0, 1], dtype=np.uint32)
    out = hl.finish_confidence(merged, counts, shape)
    assert list(out) == list(hl.CONFIDENCE_KEYS)
    assert out["confidence_sum"].dtype == np.uint64 and out["confidence_sum"].tolist() == [0, 3 << 23, 0, 1 << 22]
    for k, want in (("confidence_min", [0.0, 0.5, 0.0, 0.25]), ("confidence_max", [0.0, 1.0, 0.0, 0.25]), ("confidence_mean", [0.0, 0.75, 0.0, 0.25])):
        assert out[k].dtype == np.float64 and out[k].tolist() == want, k
    assert out["confidence_peak"].dtype == np.int64 and out["confidence_peak"].tolist() == [[-1, -1, -1], [2, 1, 2], [-1, -1, -1], [0, 1, 1]]
    with pytest.raises(ValueError, match="first label 2"):  # voxels counted, no peak
        hl.finish_confidence(merged, np.array([11, 2, 5, 1]), shape)
    with pytest.raises(ValueError, match="first label 3"):  # a peak, no voxels
        hl.finish_confidence(merged, np.array([11, 2, 0, 0]), shape)
    with pytest.raises(ValueError, match="rows"):
        hl.finish_confidence(merged, counts[:3], shape)
    with pytest.raises(ValueError, match="outside the volume"):
        hl.finish_confidence(merged, counts, (3, 2, 2))  # index 17 >= 12


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_cell_confidence_csv_text():
    stats = {"voxel_counts": np.array([11, 2, 0, 1], dtype=np.uint32),
             **hl.finish_confidence(_part([ABSENT, (3 << 23, 1 << 23, 1 << 24, 17), ABSENT, (1, 1, 1, 4)]), [11, 2, 0, 1], (3, 2, 3))}
    text = hl.cell_confidence_csv_text(stats, 3)
    assert text == ("id,voxels,confidence_mean,confidence_min,confidence_max,peak_z,peak_y,peak_x\n"
                    "1,2,0.75,0.5,1.0,2,1,2\n"
                    "2,0,0.0,0.0,0.0,-1,-1,-1\n"
                    f"3,1,{2.0**-24!r},{2.0**-24!r},{2.0**-24!r},0,1,1\n")
    assert hl.cell_confidence_csv_text(stats, 0) == "id,voxels,confidence_mean,confidence_min,confidence_max,peak_z,peak_y,peak_x\n"
    with pytest.raises(ValueError, match="shorter"):
        hl.cell_confidence_csv_text(stats, 4)
