"""No-GPU checks of count_blobs' size filter: the switch and the validation of the bounds (hostlogic.size_filter_bounds)
and the two entry points in the ctypes bindings."""
import pytest

from delivr_cfos_amd.hostlogic import size_filter_bounds

ON = {"mi355x": {"size_filter": True}}


@pytest.mark.parametrize("settings", [None, {}, {"mi355x": {}}, {"mi355x": None}, {"mi355x": {"size_filter": False}},
                                      {"postprocessing": {"min_size": 8}}])
@pytest.mark.parametrize("bounds", [(-1, -1), (8, -1), (-1, 100), (8, 100), (100, 8)])
def test_switch_absent_or_false_means_no_filter_whatever_the_bounds(settings, bounds):
    assert size_filter_bounds(settings, *bounds) is None


@pytest.mark.parametrize("bounds, expected", [((8, 100), (8, 100)), ((8, -1), (8, -1)), ((-1, 100), (-1, 100)), ((-1, -1), (-1, -1)),
                                              ((-7, -2), (-1, -1)), ((0, 0), (0, 0)), ((5, 5), (5, 5))])
def test_switch_on_returns_the_bounds_negative_means_none(bounds, expected):
    assert size_filter_bounds(ON, *bounds) == expected
    assert all(isinstance(v, int) for v in size_filter_bounds(ON, *bounds))


def test_min_above_max_raises_with_the_switch_on_only():
    with pytest.raises(ValueError, match="min_size 9 > max_size 8"):
        size_filter_bounds(ON, 9, 8)
    assert size_filter_bounds(ON, 9, -1) == (9, -1)  # (a negative bound is no bound: nothing to compare)
    assert size_filter_bounds({"mi355x": {"size_filter": False}}, 9, 8) is None


def test_both_entry_points_are_bound():
    from delivr_cfos_amd import _lib

    for name in ("dlv_cc_counts_dev", "dlv_cc_size_filter_dev"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dlv_cc_counts_dev"][1]) == 5
    assert len(_lib.SIGNATURES["dlv_cc_size_filter_dev"][1]) == 8
