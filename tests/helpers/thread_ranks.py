"""torch.distributed's calls, as count_blobs' sharded path uses them, between THREADS of one process (one HipEngine per thread,
all on device 0): objects travel through a shared list between two barriers, seam planes through queues.  The thread-rank fake
of tests/test_gpu_size_filter.py, for test files that need it too."""
import queue
import threading


class ThreadRanks:
    isend, irecv = "isend", "irecv"
    PATCHED = ("get_rank", "get_world_size", "get_backend", "P2POp", "isend", "irecv", "batch_isend_irecv", "all_gather_object",
               "gather_object", "broadcast_object_list")

    def __init__(self, world):
        self.world = world
        self.q = {(a, b): queue.Queue() for a in range(world) for b in range(world)}
        self.bar = threading.Barrier(world)
        self.box = [None] * world
        self.local = threading.local()

    def patch(self, monkeypatch, dist):
        """make `dist` (torch.distributed) look like an initialised group of these ranks"""
        monkeypatch.setattr(dist, "is_available", lambda: True)
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        for name in self.PATCHED:
            monkeypatch.setattr(dist, name, getattr(self, name))

    def bind(self, rank):
        self.local.rank = rank

    def get_backend(self):
        return "threads"

    def get_rank(self):
        return self.local.rank

    def get_world_size(self):
        return self.world

    class P2POp:
        def __init__(self, op, tensor, peer, group=None):
            self.op, self.tensor, self.peer = op, tensor, peer

    class _Done:
        def wait(self):
            return None

    def batch_isend_irecv(self, ops):
        me = self.local.rank
        for o in ops:
            if o.op == "isend":
                self.q[(me, o.peer)].put(o.tensor.clone())
        for o in ops:
            if o.op == "irecv":
                o.tensor.copy_(self.q[(o.peer, me)].get(timeout=120))
        return [self._Done() for _ in ops]

    def _exchange(self, obj):
        self.box[self.local.rank] = obj
        self.bar.wait()
        got = list(self.box)
        self.bar.wait()
        return got

    def all_gather_object(self, out, obj, group=None):
        out[:] = self._exchange(obj)

    def gather_object(self, obj, out, dst=0, group=None):
        got = self._exchange(obj)
        if self.local.rank == dst:
            out[:] = got

    def broadcast_object_list(self, box, src=0, group=None):
        box[:] = self._exchange(list(box))[src]


def run_thread_ranks(fake, body):
    """body(rank, engine) on one thread per rank, one HipEngine each on device 0 -> the results in rank order"""
    import torch
    from delivr_cfos_amd.engine import HipEngine

    results, errors = [None] * fake.world, []

    def rank_main(rank):
        try:
            fake.bind(rank)
            torch.cuda.set_device(0)
            e = HipEngine(0)
            results[rank] = body(rank, e)
            e.close()
        except BaseException as exc:  # noqa: BLE001
            errors.append((rank, repr(exc)))
            fake.bar.abort()

    ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(fake.world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errors, errors
    return results
