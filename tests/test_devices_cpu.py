"""settings["mi355x"]["devices"] -> the devices run_inference shards one volume over (hostlogic.resolve_devices): pure host
logic, no GPU."""
import numpy as np
import pytest

from delivr_cfos_amd.hostlogic import resolve_devices


def _todays_choice(cuda_devices, device_count):
    """what run_inference picked before the setting existed: the first entry of cuda_devices, 0 when empty or not visible"""
    d = int(str(cuda_devices).split(",")[0]) if str(cuda_devices).strip() else 0
    return d if d < device_count else 0


@pytest.mark.parametrize("cuda_devices,setting,count,want", [
    ("0,1", "all", 2, [0, 1]),
    ("0,1", "all", 8, [0, 1]),
    ("3,1,2", "all", 4, [3, 1, 2]),
    (" 0, 1 ", "all", 2, [0, 1]),
    ("0,1", [0, 1, 2, 3], 4, [0, 1, 2, 3]),
    ("0,1", [3, 2], 4, [3, 2]),
    ("0,1", [0], 1, [0]),
    ("0,1", (1,), 2, [1]),
    ("0,1", [0, 0], 1, [0, 0]),
    ("0,1", [0, 0, 0], 1, [0, 0, 0]),
    ("0,1", [1, 0, 1], 2, [1, 0, 1]),
    ("0,1", [np.int64(1), np.int32(0)], 2, [1, 0]),
    ("0,1", [0] * 16, 1, [0] * 16),
    ("0,1", "first", 2, [0]),
    ("1,0", "first", 2, [1]),
    ("5", "first", 2, [0]),
    ("", "first", 2, [0]),
])
def test_valid_settings(cuda_devices, setting, count, want):
    got = resolve_devices(cuda_devices, setting, count)
    assert got == want and all(type(d) is int for d in got)


@pytest.mark.parametrize("cuda_devices", ["0,1", "1,0", "1", "3", "7,0", "", "  ", 0, 2])
@pytest.mark.parametrize("count", [1, 2, 4, 8])
def test_first_and_absent_equal_todays_choice(cuda_devices, count):
    want = [_todays_choice(cuda_devices, count)]
    assert resolve_devices(cuda_devices, None, count) == want
    assert resolve_devices(cuda_devices, "first", count) == want
    # inside a process group the default stays what it was (the rank then runs on its LOCAL_RANK)
    assert resolve_devices(cuda_devices, None, count, group_world=4) == want


def test_repeats_are_preserved_in_order():
    assert resolve_devices("0,1", [1, 1, 0, 1, 0], 2) == [1, 1, 0, 1, 0]
    assert resolve_devices("1,1,0", "all", 2) == [1, 1, 0]


@pytest.mark.parametrize("cuda_devices,setting,count,match", [
    ("0,1", "every", 2, "expected"),
    ("0,1", "ALL", 2, "expected"),
    ("0,1", "", 2, "expected"),
    ("0,1", [], 2, "empty"),
    ("0,1", (), 2, "empty"),
    ("", "all", 2, "empty"),
    ("0,x", "all", 2, "comma-separated"),
    ("0,1", [-1], 2, "not among"),
    ("0,1", [0, -1], 2, "not among"),
    ("0,1", [2], 2, "not among"),
    ("0,1", [0, 1], 1, "not among"),
    ("0,1", "all", 1, "not among"),
    ("0,-1", "all", 2, "not among"),
    ("0,1", [0.0, 1.0], 2, "integers"),
    ("0,1", ["0", "1"], 2, "integers"),
    ("0,1", [True, False], 2, "integers"),
    ("0,1", 2, 4, "expected"),
    ("0,1", {"0": 1}, 4, "expected"),
    ("0,1", [0] * 17, 1, "at most 16"),
])
def test_invalid_settings_raise(cuda_devices, setting, count, match):
    with pytest.raises(ValueError, match=match):
        resolve_devices(cuda_devices, setting, count)


def test_several_devices_inside_a_process_group_raise():
    with pytest.raises(ValueError, match="torch.distributed"):
        resolve_devices("0,1", [0, 1], 2, group_world=2)
    with pytest.raises(ValueError, match="torch.distributed"):
        resolve_devices("0,1", "all", 2, group_world=8)
    with pytest.raises(ValueError, match="torch.distributed"):
        resolve_devices("0", [0, 0], 1, group_world=2)
    # one device per rank is fine, and a group of one is no group
    assert resolve_devices("0,1", [1], 2, group_world=2) == [1]
    assert resolve_devices("0,1", [0, 1], 2, group_world=1) == [0, 1]
