"""Host side of count_blobs' opt-in keys, no GPU: the options record (hostlogic.CountOptions / count_options), the one HBM check
(check_hbm_budget) and the plan of what a cached pickle still lacks (measuring_plan)."""
import inspect

import pytest

from delivr_cfos_amd.hostlogic import (CountOptions, background_shell_radius, check_hbm_budget, count_options, intensity_quartiles_enabled,
                                       intensity_stats_enabled, measuring_plan, shape_stats_enabled, size_filter_bounds,
                                       split_fused_settings)

ALL_GROUPS = {"cells", "shell", "cell_quartiles", "shell_quartiles", "shape"}
RAW = {"cells", "shell", "cell_quartiles", "shell_quartiles"}


# ---- the options record -------------------------------------------------------------------------------------------------------

def _from_the_parsers(settings, lo, hi):
    return CountOptions(bounds=size_filter_bounds(settings, lo, hi), intensity=intensity_stats_enabled(settings),
                        shell_radius=background_shell_radius(settings), quartiles=intensity_quartiles_enabled(settings),
                        shape=shape_stats_enabled(settings), split=split_fused_settings(settings))


@pytest.mark.parametrize("mi, lo, hi", [
    (None, -1, -1),
    ({}, 5, 9),  # the bounds are ignored without the switch
    ({"size_filter": False}, 5, 9),
    ({"size_filter": True}, 5, 9),
    ({"size_filter": True}, None, 9),
    ({"size_filter": True}, -1, -1),
    ({"intensity_stats": False}, -1, -1),
    ({"intensity_stats": True}, -1, -1),
    ({"intensity_stats": True, "background_shell": 0}, -1, -1),
    ({"intensity_stats": True, "background_shell": 1}, -1, -1),
    ({"intensity_stats": True, "background_shell": 16}, -1, -1),
    ({"intensity_stats": True, "intensity_quartiles": False}, -1, -1),
    ({"intensity_stats": True, "intensity_quartiles": True}, -1, -1),
    ({"shape_stats": False}, -1, -1),
    ({"shape_stats": True}, -1, -1),
    ({"split_fused": 0}, -1, -1),
    ({"split_fused": 3}, -1, -1),
    ({"split_fused": 3, "split_min_core": 4}, -1, -1),
    ({"size_filter": True, "intensity_stats": True, "background_shell": 2, "intensity_quartiles": True, "shape_stats": True,
      "split_fused": 2, "split_min_core": 2}, 3, 40),
])
def test_count_options_is_what_the_parsers_return(mi, lo, hi):
    settings = {} if mi is None else {"mi355x": mi}
    opts = count_options(settings, lo, hi)
    assert opts == _from_the_parsers(settings, lo, hi)
    with pytest.raises(Exception):  # (frozen)
        opts.shape = True


def test_count_options_written_out():
    assert count_options({}, 5, 9) == CountOptions() == CountOptions(None, False, 0, False, False, None)
    full = {"mi355x": {"size_filter": True, "intensity_stats": True, "background_shell": 2, "intensity_quartiles": True, "shape_stats": True,
                       "split_fused": 3}}
    assert count_options(full, 5, None) == CountOptions(bounds=(5, -1), intensity=True, shell_radius=2, quartiles=True, shape=True, split=(3, 1))


@pytest.mark.parametrize("mi, lo, hi, parser", [
    ({"background_shell": 2}, -1, -1, background_shell_radius),  # a shell without intensity_stats
    ({"intensity_quartiles": True}, -1, -1, intensity_quartiles_enabled),  # quartiles without intensity_stats
    ({"split_min_core": 2}, -1, -1, split_fused_settings),  # split_min_core without split_fused
    ({"size_filter": True}, 9, 5, lambda s: size_filter_bounds(s, 9, 5)),  # min_size > max_size with the filter on
])
def test_count_options_rejects_what_the_parsers_reject(mi, lo, hi, parser):
    settings = {"mi355x": mi}
    with pytest.raises(ValueError) as theirs:
        parser(settings)
    with pytest.raises(ValueError) as ours:
        count_options(settings, lo, hi)
    assert str(ours.value) == str(theirs.value)


# one bad value per parser that can refuse (shape_stats_enabled and intensity_stats_enabled, the last two of the order, take
# any value as a truth value: no pair with them has two bad keys)
_BAD = {"min_size": {"size_filter": True}, "background_shell": {"intensity_stats": True, "background_shell": 99},
        "intensity_quartiles": {"intensity_stats": True, "intensity_quartiles": "yes"}, "split_fused": {"split_fused": 17}}


@pytest.mark.parametrize("earlier, later", [("min_size", "background_shell"), ("background_shell", "intensity_quartiles"),
                                            ("intensity_quartiles", "split_fused")])
def test_with_two_bad_keys_the_earlier_parser_wins(earlier, later):
    for key in (earlier, later):  # each is bad on its own
        with pytest.raises(ValueError, match=key):
            count_options({"mi355x": _BAD[key]}, 9, 5)
    with pytest.raises(ValueError) as ei:
        count_options({"mi355x": {**_BAD[later], **_BAD[earlier]}}, 9, 5)
    assert earlier in str(ei.value) and later not in str(ei.value)


def test_derived_properties():
    assert not CountOptions().filter_active and not CountOptions(bounds=(-1, -1)).filter_active
    assert CountOptions(bounds=(3, -1)).filter_active and CountOptions(bounds=(-1, 0)).filter_active
    assert [CountOptions(shell_radius=r).shell_bytes_per_voxel for r in (0, 1, 2, 3, 16)] == [0, 4, 8, 8, 8]


def test_the_sharded_path_without_options_means_no_opt_in_key():
    import importlib

    module = importlib.import_module("delivr_cfos_amd.count_blobs")
    assert inspect.signature(module._count_blobs_sharded).parameters["opts"].default == CountOptions()
    for name, fn in inspect.getmembers(module, inspect.isfunction):  # one argument describes the options, nowhere more
        if fn.__module__ == module.__name__:
            loose = {"bounds", "shell_radius", "shape", "split", "quartiles", "cells", "shell", "cell_quartiles", "shell_quartiles", "own"}
            params = set(inspect.signature(fn).parameters)
            assert len(params & loose) + ("opts" in params) <= 1, name


# ---- the HBM check ------------------------------------------------------------------------------------------------------------

V = 8 * 8 * 8
PHRASES = {"intensity_stats": "slab-streamed", "shape_stats": "slab-streamed", "split_fused": "8 more bytes", "size_filter": "slab-streamed",
           "intensity_quartiles": "2 more bytes per voxel", "background_shell": "more bytes per voxel"}
ORDER = ("intensity_stats", "background_shell", "intensity_quartiles", "shape_stats", "split_fused", "size_filter")


def _shell_bpv(radius):
    return 0 if not radius else (4 if radius == 1 else 8)


def _parent_fresh(opts, base):
    """The conditions of the parent's _count_blobs_single for a fresh labelling, in their order: (key, the condition beside
    `not cached`, the bytes per voxel compared with the budget).  size_filter sat inside the slab-streamed branch
    (`need > budget`), after the five others."""
    s = _shell_bpv(opts.shell_radius)
    return [("intensity_stats", opts.intensity, base + 2),                  # raw_vol is not None and V * (base + 2) > budget
            ("background_shell", s != 0, base + 2 + s),                     # shell_bpv and V * (base + 2 + shell_bpv) > budget
            ("intensity_quartiles", opts.quartiles, base + 2 + s + 2),      # quartiles and V * (base + 2 + shell_bpv + 2) > budget
            ("shape_stats", opts.shape, base),                              # shape and need > budget
            ("split_fused", opts.split is not None, base + 8),              # split is not None and V * (base + 8) > budget
            ("size_filter", opts.bounds is not None and (opts.bounds[0] >= 0 or opts.bounds[1] >= 0), base)]  # need > budget: _filter_active


def _parent_cached(opts, measured):
    """... and for cached labels (`labels_dev is None`), from the measure_* locals - here the set `measured`."""
    s = _shell_bpv(opts.shell_radius)
    return [("shape_stats", "shape" in measured, 4),                                          # measure_shape and V * 4 > budget
            ("intensity_stats", bool(measured & RAW), 4 + 2),                                 # measure and V * (4 + 2) > budget
            ("background_shell", "shell" in measured, 4 + 2 + s),                             # measure_shell and V * (4 + 2 + shell_bpv) > budget
            ("intensity_quartiles", bool(measured & {"cell_quartiles", "shell_quartiles"}), 4 + 2 + s + 2)]  # (measure_quartiles or measure_shell_quartiles)


def _first_refused(table, budget, voxels=V):
    for key, applies, bpv in table:
        if applies and voxels * bpv > budget:
            return key, voxels * bpv
    return None, None


def _check(opts, measured, cached, base, budget, table, voxels=V):
    """check_hbm_budget against the parent's table: the same key refused (or none), the message with its parts"""
    key, need = _first_refused(table, budget, voxels)
    if key is None:
        assert check_hbm_budget(opts, measured, cached, base, voxels, budget) is None
        return None
    with pytest.raises(MemoryError) as ei:
        check_hbm_budget(opts, measured, cached, base, voxels, budget)
    msg = str(ei.value)
    assert msg.startswith("delivr_cfos_amd (DLV_ENOMEM): "), msg
    assert f"settings['mi355x']['{key}']" in msg and msg.endswith(f"; raise settings['mi355x']['hbm_budget_gb'] or switch {key} off"), msg
    assert not any(k in msg for k in ORDER if k != key), msg  # no other key, a later one least of all
    assert f"({need / 2**30:.1f} GiB)" in msg and f"the HBM budget is {budget / 2**30:.1f} GiB" in msg, msg
    if cached:
        assert "cached labels" in msg and "slab-streamed" not in msg, msg
    else:
        assert "cached labels" not in msg and PHRASES[key] in msg, msg
        assert ("slab-streamed" in msg) == (key in ("intensity_stats", "shape_stats", "split_fused", "size_filter")), msg
    if key == "split_fused":
        assert "8 more bytes" in msg and f"['split_fused'] = {opts.split[0]} " in msg, msg
    if key == "intensity_quartiles":
        assert "2 more bytes per voxel" in msg, msg
    if key == "background_shell":
        assert f"['background_shell'] = {opts.shell_radius} needs {_shell_bpv(opts.shell_radius)} more bytes per voxel" in msg, msg
    return key


def _base():
    from delivr_cfos_amd.streaming import ccl_bytes_per_voxel

    assert ccl_bytes_per_voxel() == 7
    return ccl_bytes_per_voxel()


@pytest.mark.parametrize("opts, key, extra", [
    (CountOptions(intensity=True), "intensity_stats", 2),
    (CountOptions(intensity=True, shell_radius=1), "background_shell", 2 + 4),
    (CountOptions(intensity=True, shell_radius=3), "background_shell", 2 + 8),
    (CountOptions(intensity=True, quartiles=True), "intensity_quartiles", 2 + 0 + 2),
    (CountOptions(intensity=True, shell_radius=1, quartiles=True), "intensity_quartiles", 2 + 4 + 2),
    (CountOptions(intensity=True, shell_radius=3, quartiles=True), "intensity_quartiles", 2 + 8 + 2),
    (CountOptions(shape=True), "shape_stats", 0),
    (CountOptions(split=(2, 1)), "split_fused", 8),
    (CountOptions(bounds=(3, -1)), "size_filter", 0),
])
def test_fresh_labelling_thresholds(opts, key, extra):
    base = _base()
    table, measured = _parent_fresh(opts, base), measuring_plan(opts, None)
    need = V * (base + extra)
    assert _check(opts, measured, False, base, need, table) is None  # (the comparison is >)
    assert _check(opts, measured, False, base, need - 1, table) == key


def test_fresh_labelling_every_key_at_every_budget():
    base = _base()
    seen = []
    for radius in (0, 1, 3):
        opts = CountOptions(bounds=(3, 40), intensity=True, shell_radius=radius, quartiles=True, shape=True, split=(2, 1))
        table, measured = _parent_fresh(opts, base), measuring_plan(opts, None)
        for bpv in sorted({b for _, _, b in table}):
            for budget in (V * bpv, V * bpv - 1):
                seen.append(_check(opts, measured, False, base, budget, table))
    for opts in (CountOptions(bounds=(3, 40), shape=True, split=(2, 1)), CountOptions(bounds=(3, 40), split=(2, 1)), CountOptions(bounds=(-1, 9))):
        table = _parent_fresh(opts, base)
        for budget in (V * (base + 8), V * (base + 8) - 1, V * base, V * base - 1, 0):
            seen.append(_check(opts, frozenset(measuring_plan(opts, None)), False, base, budget, table))
    assert set(seen) == {None} | set(ORDER)
    assert check_hbm_budget(CountOptions(), frozenset(), False, base, V, 0) is None  # no key, nothing to refuse: the labelling is streamed


@pytest.mark.parametrize("opts, measured, key, bpv", [
    (CountOptions(shape=True), {"shape"}, "shape_stats", 4),
    (CountOptions(intensity=True), {"cells"}, "intensity_stats", 4 + 2),
    (CountOptions(intensity=True, shell_radius=1), {"cells", "shell"}, "background_shell", 4 + 2 + 4),
    (CountOptions(intensity=True, shell_radius=3), {"shell"}, "background_shell", 4 + 2 + 8),
    (CountOptions(intensity=True, quartiles=True), {"cell_quartiles"}, "intensity_quartiles", 4 + 2 + 0 + 2),
    (CountOptions(intensity=True, shell_radius=1, quartiles=True), {"shell_quartiles"}, "intensity_quartiles", 4 + 2 + 4 + 2),
    (CountOptions(intensity=True, shell_radius=3, quartiles=True), set(ALL_GROUPS), "intensity_quartiles", 4 + 2 + 8 + 2),
])
def test_cached_labels_thresholds(opts, measured, key, bpv):
    measured = frozenset(measured)
    table = _parent_cached(opts, measured)
    assert _check(opts, measured, True, 4, V * bpv, table) is None
    assert _check(opts, measured, True, 4, V * bpv - 1, table) == key


def test_cached_labels_every_plan_at_every_budget():
    seen = []
    for radius in (0, 1, 3):
        opts = CountOptions(bounds=(3, 40), intensity=True, shell_radius=radius, quartiles=True, shape=True, split=(2, 1))
        for measured in (set(), {"shape"}, {"cells"}, {"shell"}, {"cell_quartiles"}, {"shell_quartiles"}, {"shell", "shell_quartiles"},
                         {"cells", "shape"}, set(RAW), set(ALL_GROUPS)):
            measured = frozenset(measured)
            table = _parent_cached(opts, measured)
            for bpv in (4, 6, 6 + _shell_bpv(radius), 8 + _shell_bpv(radius)):
                for budget in (V * bpv, V * bpv - 1):
                    seen.append(_check(opts, measured, True, 4, budget, table))
    assert set(seen) == {None, "shape_stats", "intensity_stats", "background_shell", "intensity_quartiles"}  # (never split_fused / size_filter)


def test_the_figures_of_a_large_volume():
    voxels, base = 2**30, _base()
    opts = CountOptions(intensity=True, shell_radius=3)
    table = _parent_fresh(opts, base)
    assert _check(opts, measuring_plan(opts, None), False, base, 10 * 2**30, table, voxels) == "background_shell"
    with pytest.raises(MemoryError, match=r"\(17\.0 GiB\), the HBM budget is 10\.0 GiB; raise"):
        check_hbm_budget(opts, measuring_plan(opts, None), False, base, voxels, 10 * 2**30)
    with pytest.raises(MemoryError, match=r"intensity_stats.*\(6\.0 GiB\), the HBM budget is 5\.5 GiB; raise"):
        check_hbm_budget(opts, frozenset({"shell"}), True, 4, voxels, 11 * 2**29)


# ---- the plan for a cached pickle ---------------------------------------------------------------------------------------------

CELL_KEYS = ("intensity_sum", "intensity_sumsq", "intensity_min", "intensity_max", "intensity_mean")
SHELL_KEYS = ("shell_voxels", "shell_sum", "shell_sumsq", "shell_min", "shell_max", "shell_mean", "contrast")
CELL_QUARTILE_KEYS = ("intensity_q25", "intensity_median", "intensity_q75")
SHELL_QUARTILE_KEYS = ("shell_q25", "shell_median", "shell_q75", "contrast_median")
SHAPE_KEYS = ("shape_sums", "shape_moments", "shape_faces", "shape_surface_voxels", "shape_covariance", "shape_axes", "shape_elongation",
              "shape_sphericity")
EVERYTHING_ON = CountOptions(intensity=True, shell_radius=2, quartiles=True, shape=True)


def _complete_stats():
    stats = {k: object() for k in ("voxel_counts", "bounding_boxes", "centroids") + CELL_KEYS + SHELL_KEYS + CELL_QUARTILE_KEYS
             + SHELL_QUARTILE_KEYS + SHAPE_KEYS}
    stats["shell_radius"] = 2
    return stats


def _without(key):
    stats = _complete_stats()
    del stats[key]
    return stats


def test_a_complete_pickle_measures_nothing():
    plan = measuring_plan(EVERYTHING_ON, _complete_stats())
    assert plan == set() and isinstance(plan, frozenset)


def test_one_missing_key_remeasures_its_group_alone():
    for keys, group in ((CELL_KEYS, "cells"), (SHELL_KEYS, "shell"), (CELL_QUARTILE_KEYS, "cell_quartiles"),
                        (SHELL_QUARTILE_KEYS, "shell_quartiles"), (SHAPE_KEYS, "shape")):
        for key in keys:
            assert measuring_plan(EVERYTHING_ON, _without(key)) == {group}, key
    assert measuring_plan(EVERYTHING_ON, _without("contrast")) == {"shell"}
    assert measuring_plan(EVERYTHING_ON, _without("intensity_mean")) == {"cells"}
    assert measuring_plan(EVERYTHING_ON, _without("contrast_median")) == {"shell_quartiles"}
    assert measuring_plan(EVERYTHING_ON, _without("voxel_counts")) == set()  # (not a key of any opt-in group)


def test_another_shell_radius_remeasures_the_shell_groups_and_not_the_cells():
    stats = _complete_stats()
    stats["shell_radius"] = 3
    assert measuring_plan(EVERYTHING_ON, stats) == {"shell", "shell_quartiles"}
    assert measuring_plan(EVERYTHING_ON, _without("shell_radius")) == {"shell", "shell_quartiles"}
    asked_for_3 = CountOptions(intensity=True, shell_radius=3, quartiles=True, shape=True)
    assert measuring_plan(asked_for_3, _complete_stats()) == {"shell", "shell_quartiles"}
    assert measuring_plan(asked_for_3, stats) == set()


def test_without_a_pickle_everything_asked_for_is_measured():
    assert measuring_plan(EVERYTHING_ON, None) == {"cells", "shell", "cell_quartiles", "shell_quartiles", "shape"}
    assert measuring_plan(EVERYTHING_ON, {}) == {"cells", "shell", "cell_quartiles", "shell_quartiles", "shape"}
    assert measuring_plan(EVERYTHING_ON, {"voxel_counts": 0, "bounding_boxes": 0, "centroids": 0}) == {"cells", "shell", "cell_quartiles",
                                                                                                    "shell_quartiles", "shape"}


def test_an_option_that_is_off_never_appears():
    assert measuring_plan(CountOptions(), None) == set()
    assert measuring_plan(CountOptions(bounds=(1, 2), split=(2, 1)), None) == set()
    assert measuring_plan(CountOptions(shape=True), None) == {"shape"}
    assert measuring_plan(CountOptions(intensity=True), None) == {"cells"}
    assert measuring_plan(CountOptions(intensity=True, quartiles=True, shape=True), None) == {"cells", "cell_quartiles", "shape"}  # no shell
    assert measuring_plan(CountOptions(intensity=True, shell_radius=2, shape=True), None) == {"cells", "shell", "shape"}  # no quartiles
    assert measuring_plan(CountOptions(intensity=True, shell_radius=2, quartiles=True), None) == {"cells", "shell", "cell_quartiles",
                                                                                                 "shell_quartiles"}  # no shape
    # ... and a pickle that lacks the keys of a switched-off group, or holds the shells of some radius, changes nothing
    assert measuring_plan(CountOptions(intensity=True), _without("shape_axes")) == set()
    assert measuring_plan(CountOptions(intensity=True, quartiles=True), _complete_stats()) == set()
    assert measuring_plan(CountOptions(intensity=True, quartiles=True), _without("shell_radius")) == set()
    assert measuring_plan(CountOptions(shape=True), _without("intensity_sum")) == set()
    assert measuring_plan(CountOptions(), {}) == set()
