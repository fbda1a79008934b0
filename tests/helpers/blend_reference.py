"""What a sliding-window pass leaves in its accumulator when every forwarded voxel has the same logit: numpy and float64 only,
no engine.  The window list is the oracle's (orc.window_list); everything else is counting.

A checkpoint with final_conv.weight = 0 and final_conv.bias = c gives every voxel of a forwarded window the logit c exactly, in
every format; a window whose maximum is at most the threshold is skipped and contributes -1000.  With act / skp = the number of
active / skipped windows that cover a voxel, a constant-weight pass repeated `rep` times leaves
    acc = rep * (c * act - 1000 * skp),   cnt = rep * (act + skp)
- small integers, the same in whatever order the windows are added.  With an importance map the sums of the map over the covering
windows take the place of the counts (W_act, W_skp: float64)."""
import numpy as np

from oracle import delivr_oracle as orc

# (shape, roi, overlap) of the blend tests, with the recipe of their volume in volume()
GEOMETRIES = {
    "A": ((48, 40, 40), (32, 32, 16), 0.25),  # 12 windows
    "B": ((50, 61, 70), (24, 40, 20), 0.5),   # 72 windows, a clamped last window along z and y, up to 18 windows per voxel
    "C": ((40, 70, 45), (19, 35, 21), 0.3),   # odd window, odd interval
    "D": ((32, 32, 48), (32, 32, 16), 0.6),   # interval 6: seven x starts, the last one clamped
    "E": ((96, 40, 40), (32, 32, 16), 0.5),   # x starts on the 8-voxel grid, rows of a multiple of 8
}


def volume(shape):
    """dense synthetic signal with the low half of z and the low half of x zeroed: windows that are skipped, windows that are
    not, and voxels covered by both kinds"""
    from delivr_cfos_amd.synth import synth_volume_np

    vol = synth_volume_np(shape, seed=31, dense=True)
    vol[: shape[0] // 2] = 0
    vol[:, :, : shape[2] // 2] = 0
    return vol


def _windows(vol, roi, overlap, win_range):
    wins = orc.window_list(vol.shape, roi, overlap)
    d, h, w = (min(int(r), int(n)) for r, n in zip(roi, vol.shape))
    wmax = np.array([vol[z:z + d, y:y + h, x:x + w].max() for z, y, x in wins], dtype=np.int32)
    lo, hi = (0, len(wins)) if win_range is None else win_range
    return wins, wmax, (d, h, w), range(int(lo), int(hi))


def expected(vol, roi, overlap, skip_threshold=0, win_range=None):
    """-> (act, skp, wins, wmax): int64 maps of how many active / skipped windows cover each voxel, the window list and the
    maximum of every window.  win_range = (lo, hi): only windows lo .. hi - 1 are counted (wins and wmax stay whole)."""
    wins, wmax, (d, h, w), picked = _windows(vol, roi, overlap, win_range)
    act = np.zeros(vol.shape, dtype=np.int64)
    skp = np.zeros(vol.shape, dtype=np.int64)
    for i in picked:
        z, y, x = wins[i]
        (skp if wmax[i] <= skip_threshold else act)[z:z + d, y:y + h, x:x + w] += 1
    return act, skp, wins, wmax


def expected_weighted(vol, roi, overlap, importance, skip_threshold=0, win_range=None):
    """-> (W_act, W_skp): float64 sums of the (d, h, w) importance map over the active / skipped windows that cover each voxel"""
    wins, wmax, (d, h, w), picked = _windows(vol, roi, overlap, win_range)
    imp = np.asarray(importance, dtype=np.float64)
    assert imp.shape == (d, h, w), (imp.shape, (d, h, w))
    w_act = np.zeros(vol.shape, dtype=np.float64)
    w_skp = np.zeros(vol.shape, dtype=np.float64)
    for i in picked:
        z, y, x = wins[i]
        (w_skp if wmax[i] <= skip_threshold else w_act)[z:z + d, y:y + h, x:x + w] += imp
    return w_act, w_skp


def constant_acc(act, skp, c, rep=1):
    """the accumulator of a constant-weight pass, as float32 (exact while |acc| < 2^24)"""
    acc = rep * (int(c) * act - 1000 * skp)
    assert np.abs(acc).max() < 2 ** 24
    return acc.astype(np.float32)


def constant_cnt(act, skp, rep=1):
    cnt = rep * (act + skp)
    assert cnt.max() <= 255
    return cnt.astype(np.uint8)
