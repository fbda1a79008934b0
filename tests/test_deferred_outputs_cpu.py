"""The deferred outputs of step 2 under one join: create_nifti_seg(defer_write=True) hands binaries.npy AND, with
FLAGS.SAVE_ACTIVATED_OUTPUT, network_output.npy to the engine's background workers, and the one hostio.wait_deferred() that
__main__ and a pipelined batch call between the steps covers both - count_blobs' confidence_stats reads the second file.  No
device: the engine and the writer are stand-ins, the queue and the join are hostio's own."""
import os
import threading

import numpy as np
import pytest

from delivr_cfos_amd import hostio


class _Engine:  # (hostio keys its workers by the engine object)
    pass


def test_wait_deferred_joins_every_submitted_file_and_reraises(tmp_path):
    eng, other = _Engine(), _Engine()
    first_done = threading.Event()

    def write(path, after=None):
        if after is not None:
            after.wait()
        with open(path + ".partial", "wb") as fh:
            fh.write(b"x" * 4096)
        os.replace(path + ".partial", path)

    a, b = str(tmp_path / "binaries.npy"), str(tmp_path / "network_output.npy")
    fut_a = hostio.submit_deferred(eng, write, a)
    fut_a.add_done_callback(lambda f: first_done.set())
    fut_b = hostio.submit_deferred(eng, write, b, first_done)  # (starts its write only once the first file is complete)
    hostio.wait_deferred(eng)
    assert fut_a.done() and fut_b.done() and sorted(os.listdir(tmp_path)) == ["binaries.npy", "network_output.npy"]
    # an error of the second file is raised by the join, after the first one was waited for; another engine's queue is not touched
    gate = threading.Event()

    def fail():
        raise OSError("no space left for network_output.npy")

    blocked = hostio.submit_deferred(other, write, str(tmp_path / "other.npy"), gate)
    fut_c = hostio.submit_deferred(eng, write, str(tmp_path / "c.npy"))
    hostio.submit_deferred(eng, fail)
    with pytest.raises(OSError, match="network_output"):
        hostio.wait_deferred(eng)
    assert fut_c.done() and not blocked.done()
    hostio.wait_deferred(eng)  # (the failed transfers are forgotten: the next join is clean)
    gate.set()
    hostio.wait_deferred()  # every engine
    assert blocked.done() and os.path.exists(str(tmp_path / "other.npy"))


def test_create_nifti_seg_defers_the_probabilities_with_the_mask(tmp_path, monkeypatch):
    import torch
    from delivr_cfos_amd.inference import inference

    shape = (4, 6, 8)
    mask = np.arange(np.prod(shape), dtype=np.uint8).reshape(shape) % 2
    prob = np.linspace(0, 1, int(np.prod(shape)), dtype=np.float32).reshape(shape)
    release = threading.Event()
    calls = []

    class Engine:
        def finalize(self, acc, cnt, raw, zyx, threshold, erode_iters, zblock, want_prob=False, out=None):
            assert want_prob and tuple(zyx) == shape
            return mask, prob

        def sync(self):
            pass

    def save_npy(engine, tensor, path, dtype, what="d2h", partial=False, synced=False):
        release.wait()  # (the files stream out behind the caller: nothing is written before the join lets them)
        calls.append((what, partial, synced))
        np.save(path + ".partial.npy", np.asarray(tensor, dtype=dtype))
        os.replace(path + ".partial.npy", path)

    monkeypatch.setattr(inference, "save_npy", save_npy)
    eng = Engine()
    out_mask, out_prob = str(tmp_path / "binaries.npy"), str(tmp_path / "network_output.npy")
    got = inference.create_nifti_seg(0.5, torch.zeros(shape), out_mask, out_prob, torch.zeros(shape, dtype=torch.int16), (1, 1) + shape,
                                     engine=eng, defer_write=True)
    assert got is mask and os.listdir(tmp_path) == []  # returned with both writes still pending
    release.set()
    hostio.wait_deferred(eng)  # the one join of __main__ / a pipelined batch
    assert sorted(calls) == [("d2h_mask", True, True), ("d2h_prob", True, True)]  # both as <name>.partial, renamed when complete
    assert sorted(os.listdir(tmp_path)) == ["binaries.npy", "network_output.npy"]
    assert np.array_equal(np.load(out_mask), mask) and np.load(out_prob).dtype == np.float32 and np.array_equal(np.load(out_prob), prob)
    # without SAVE_ACTIVATED_OUTPUT (no probability file) one transfer is queued
    calls.clear()
    eng.finalize = lambda *a, want_prob=False, **k: mask
    inference.create_nifti_seg(0.5, torch.zeros(shape), out_mask, None, torch.zeros(shape, dtype=torch.int16), (1, 1) + shape,
                               engine=eng, defer_write=True)
    hostio.wait_deferred(eng)
    assert calls == [("d2h_mask", True, True)]
