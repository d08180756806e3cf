"""Small ncclAllToAll / ncclAllToAllv calls through the NCCL ABI take the LL kernel (kernels/alltoall_ll.hip):
one rank per process (placed by mp_util), no vendor library.  What shows the path is the communicator's
own account -- a2a_ll_count() rises by one per call while registration_exchanges() and pull_ll_count() do
not move, on tensors the communicator has never seen -- beside results compared byte for byte with numpy
slicing of every rank's data, 0xA5 guards on both sides of every receive buffer.  Every worker runs under
the collect() watchdog from its first call.

The edges run with MSCCLPP_AMD_A2A_LL_MAX_BYTES=4096, so they do not depend on the measured bound.

Not tested: a captured call whose scratch would have to grow (it takes the pull path).  The communicator
allocates 64 MiB of LL scratch at init and the rule is clamped to 1 MiB segments, which need at most
32 MiB at 8 ranks, so no call reaches that branch through the ABI."""
import multiprocessing as mp
import os
import traceback

import mp_util
import pytest

pytestmark = pytest.mark.gpu

VAR = "MSCCLPP_AMD_A2A_LL_MAX_BYTES"
GUARD, PAD = 0xA5, 64


def _spawn(target, n, *extra, timeout=240):
    import mscclpp_amd as m

    uid = m.Communicator.unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, n, uid, q) + extra) for r in range(n)]
    for p in procs:
        p.start()
    return mp_util.collect(procs, q, n, timeout)


def _setup(rank, n, uid, ll_max):
    os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "10000")
    os.environ.pop("MSCCLPP_AMD_NCCL_LIB_PATH", None)  # no vendor library
    os.environ.pop("MSCCLPP_NCCL_LIB_PATH", None)
    os.environ.pop(VAR, None)
    os.environ.pop("MSCCLPP_AMD_PULL_LL_MAX_BYTES", None)
    if ll_max is not None:
        os.environ[VAR] = ll_max
    import torch

    import mscclpp_amd as m

    dev, shared = mp_util.place_rank(rank, n)
    return torch, m, m.Communicator(rank, n, uid), dev, shared


def _data(rank, nbytes, seed):
    """Rank `rank`'s send bytes of a call: every rank computes every rank's."""
    import numpy as np

    x = np.random.default_rng(1000 * seed + rank).integers(0, 255, nbytes, dtype=np.uint8)
    x[x == GUARD] = 0x5A
    return x


class Runner:
    """Calls on fresh tensors (all kept alive, so no address comes back) and their judgement."""

    def __init__(self, torch, m, comm, rank, n):
        self.torch, self.m, self.comm, self.rank, self.n = torch, m, comm, rank, n
        self.keep = []

    def account(self):
        c = self.comm
        return c.a2a_ll_count(), c.pull_ll_count(), tuple(c.registration_exchanges()[:2])

    def guarded(self, nbytes):
        whole = self.torch.full((nbytes + 2 * PAD,), GUARD, dtype=self.torch.uint8, device="cuda")
        self.keep.append(whole)
        return whole, whole[PAD:PAD + nbytes]

    def fresh(self, x):
        t = self.torch.from_numpy(x.copy()).cuda()
        self.keep.append(t)
        return t

    def right(self, whole, want):
        import numpy as np

        self.torch.cuda.synchronize()
        got = whole.cpu().numpy()
        return bool((got[:PAD] == GUARD).all() and (got[PAD + len(want):] == GUARD).all() and
                    np.array_equal(got[PAD:PAD + len(want)], want))

    # -- equal split: `blk` bytes to every rank --------------------------------------------------
    def equal_want(self, blk, seed):
        import numpy as np

        return np.concatenate([_data(p, self.n * blk, seed)[self.rank * blk:(self.rank + 1) * blk] for p in range(self.n)])

    def equal(self, blk, seed):
        send = self.fresh(_data(self.rank, self.n * blk, seed))
        whole, recv = self.guarded(self.n * blk)
        self.comm.all_to_all(send, recv)
        return self.right(whole, self.equal_want(blk, seed))

    # -- AllToAllv: L[r][q] bytes from r to q, packed in peer order on both sides, `gap` guard bytes between
    # receive segments
    def v(self, L, seed, gap=3):
        import numpy as np

        n, me = self.n, self.rank
        sdis = [[sum(L[r][:q]) for q in range(n)] for r in range(n)]
        rdis, at = [], 0
        for p in range(n):
            rdis.append(at)
            at += L[p][me] + gap
        send = self.fresh(_data(me, max(1, sum(L[me])), seed))
        whole, recv = self.guarded(max(1, at))
        want = np.full(max(1, at), GUARD, np.uint8)
        for p in range(n):
            want[rdis[p]:rdis[p] + L[p][me]] = _data(p, max(1, sum(L[p])), seed)[sdis[p][me]:sdis[p][me] + L[p][me]]
        self.comm.all_to_all_v(send, L[me], sdis[me], recv, [L[p][me] for p in range(n)], rdis)
        return self.right(whole, want)

    def counted(self, fn, took_ll):
        """fn() is right, and the account moved as the path says: LL -- the count rose by one, nothing was
        registered, the reductions' count stayed; pull -- the count stayed and something was registered."""
        a0, p0, r0 = self.account()
        ok = fn()
        a1, p1, r1 = self.account()
        if took_ll:
            return ok and a1 == a0 + 1 and r1 == r0 and p1 == p0
        return ok and a1 == a0 and p1 == p0 and sum(r1) > sum(r0)


def v_matrix(n, most, zero_row=None):
    """Unequal lengths up to `most`, which rank n - 1 sends rank 0; optionally one rank sends nothing."""
    L = [[(37 * r + 11 * q) % 97 + 1 for q in range(n)] for r in range(n)]
    L[n - 1][0] = most
    if zero_row is not None:
        L[zero_row] = [0] * n
    return L


def _edges_worker(rank, n, uid, q):
    try:
        torch, m, comm, dev, shared = _setup(rank, n, uid, "4096")
        import time

        import numpy as np

        run = Runner(torch, m, comm, rank, n)
        res = {"device": dev, "shared": shared}
        res["rule"] = m.alltoall_takes_ll(n, 4096) and not m.alltoall_takes_ll(n, 4097)
        res["count_starts_at_zero"] = comm.a2a_ll_count() == 0
        # ---- at the edge, on tensors the communicator has never seen ---------------------------------
        res["alltoall_at_the_edge"] = run.counted(lambda: run.equal(4096, 1), True)
        res["alltoallv_at_the_edge"] = run.counted(lambda: run.v(v_matrix(n, 4096), 2), True)
        res["alltoall_one_byte"] = run.counted(lambda: run.equal(1, 3), True)
        # ---- one element above it: the pull kernel, which registers ----------------------------------
        res["alltoall_one_above"] = run.counted(lambda: run.equal(4097, 4), False)
        res["alltoallv_one_above"] = run.counted(lambda: run.v(v_matrix(n, 4097), 5), False)
        # ---- stream order: the send buffer is produced behind a sleep and overwritten right after ------
        blk = 520
        send = torch.empty(n * blk, dtype=torch.uint8, device="cuda")
        whole, recv = run.guarded(n * blk)
        ok, c0 = True, comm.a2a_ll_count()
        for it in range(3):
            fresh = run.fresh(_data(rank, n * blk, 10 + it))
            whole.fill_(GUARD)
            torch.cuda._sleep(20_000_000)
            send.copy_(fresh)
            comm.all_to_all(send, recv)
            send.fill_(0xEE)
            ok = ok and run.right(whole, run.equal_want(blk, 10 + it))
        res["stream_order"] = ok and comm.a2a_ll_count() == c0 + 3
        # ---- capture after one eager call of the same size, two replays on new data -------------------
        blk = 1000
        send = run.fresh(_data(rank, n * blk, 20))
        whole, recv = run.guarded(n * blk)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            comm.all_to_all(send, recv, stream=s)
        s.synchronize()
        ok = run.right(whole, run.equal_want(blk, 20))
        comm.barrier()
        c0 = comm.a2a_ll_count()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            comm.all_to_all(send, recv, stream=torch.cuda.current_stream())
        ok = ok and comm.a2a_ll_count() == c0 + 1  # the captured call is an LL call
        for it in (21, 22):
            send.copy_(torch.from_numpy(_data(rank, n * blk, it)).cuda())
            whole.fill_(GUARD)
            torch.cuda.synchronize()
            comm.barrier()  # every rank's new data is in place before any replay reads it
            g.replay()
            ok = ok and run.right(whole, run.equal_want(blk, it))
            comm.barrier()
        res["capture_and_two_replays"] = ok
        del g
        # ---- a seeded mixed sequence with a rotating late rank -------------------------------------
        ok, step = True, 0
        a0, p0, _ = run.account()

        def late():
            nonlocal step
            if step % n == rank:
                time.sleep(0.01)
            step += 1

        for rnd in range(2):
            seed = 30 + 10 * rnd
            late()
            ok = ok and run.equal(777, seed)  # LL AllToAll
            late()
            ok = ok and run.v(v_matrix(n, 2000, zero_row=(rnd + 1) % n), seed + 1)  # LL AllToAllv with a zero row
            xs = [np.random.default_rng(seed + 2 + 100 * r).integers(-999, 999, 301).astype(np.float32) for r in range(n)]
            x = run.fresh(xs[rank])
            late()
            y = comm.all_reduce(x, torch.empty_like(x), op="sum", algo="allpair")  # LL8 SUM AllReduce
            late()
            z = comm.all_reduce(x, torch.empty_like(x), op="max")  # LL MAX AllReduce
            late()
            ok = ok and run.equal(5000, seed + 3)  # a pull-sized AllToAll
            torch.cuda.synchronize()
            total = xs[0].copy()
            for r in range(1, n):
                total = total + xs[r]  # integers below 2^24: exact in any order
            ok = ok and np.array_equal(y.cpu().numpy(), total) and np.array_equal(z.cpu().numpy(), np.max(xs, axis=0))
        a1, p1, _ = run.account()
        res["mixed_sequence"] = ok and a1 == a0 + 4 and p1 == p0 + 2
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def _paths_worker(rank, n, uid, q, ll_max):
    """The same two small calls with the variable at 0 (every call takes the pull kernel) or unset (the
    account agrees with the rule at 64 bytes)."""
    try:
        torch, m, comm, dev, shared = _setup(rank, n, uid, ll_max)
        run = Runner(torch, m, comm, rank, n)
        takes = m.alltoall_takes_ll(n, 64)
        res = {"takes_ll": takes}
        res["alltoall_64"] = run.counted(lambda: run.equal(64, 50), takes)
        res["alltoallv_64"] = run.counted(lambda: run.v(v_matrix(n, 64), 51), takes)
        res["count"] = comm.a2a_ll_count()
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("n", [2, 3, 8])
def test_edges_stream_order_capture_and_mixed_sequence(built, n):
    got = _spawn(_edges_worker, n)
    ndev = mp_util.export_device_count()
    devices = {got[r]["device"] for r in range(n)}
    assert len(devices) == min(n, max(1, ndev)), devices  # distinct GPUs where the machine has them
    for rank in range(n):
        res = dict(got[rank])
        res.pop("device"), res.pop("shared")
        assert res.pop("err") == 0, (rank, got[rank])
        assert len(res) == 10
        assert not [k for k, ok in res.items() if not ok], (rank, res)


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("ll_max", ["0", None], ids=["variable_0", "unset"])
def test_both_paths_cross_processes(built, n, ll_max):
    import mscclpp_amd as m

    got = _spawn(_paths_worker, n, ll_max)
    for rank in range(n):
        res = got[rank]
        assert res["err"] == 0 and res["alltoall_64"] and res["alltoallv_64"], (rank, res)
        if ll_max == "0":
            assert not res["takes_ll"] and res["count"] == 0, (rank, res)
        else:
            assert res["takes_ll"] == m.alltoall_takes_ll(n, 64) and res["count"] == (2 if res["takes_ll"] else 0), (rank, res)
