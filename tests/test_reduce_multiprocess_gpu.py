"""ncclReduce through the NCCL ABI, one rank per process (placed by mp_util): every rank's send buffer
is IPC-registered per allocation, the root pulls and reduces in ring order from itself; everything is
bit-exact against oracle_lib.reduce_seq, the root's receive buffer carries a 0xA5 guard, and every
worker runs under the collect() watchdog from its first call."""
import multiprocessing as mp
import os
import traceback

import mp_util
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
INTERNAL_ERROR = 3


def _spawn(target, n, timeout=240, *extra):
    import mscclpp_amd as m

    uid = m.Communicator.unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, n, uid, q) + extra) for r in range(n)]
    for p in procs:
        p.start()
    return mp_util.collect(procs, q, n, timeout)


def _setup(rank, n, uid):
    os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "10000")
    os.environ.pop("MSCCLPP_AMD_NCCL_LIB_PATH", None)  # no vendor library: what is not carried is ncclInternalError
    os.environ.pop("MSCCLPP_NCCL_LIB_PATH", None)
    import torch

    import mscclpp_amd as m

    mp_util.place_rank(rank, n)
    return torch, m, m.Communicator(rank, n, uid)


def _expect(O, np, code, n, count, seq, root):
    """The root's result bytes: reduce_seq over the ranks' lcg inputs in ring order from the root."""
    nbytes = count * O.itemsize(code)
    pad = []
    for k in range(n):
        w = np.zeros((nbytes + 3) // 4, np.uint32)
        w.view(np.uint8)[:nbytes] = O.lcg(code, count, (root + k) % n, seq).view(np.uint8)
        pad.append(w)
    return O.reduce_seq(code, O.SUM, pad).view(np.uint8)[:nbytes]


def _worker(rank, n, uid, q):
    try:
        torch, m, comm = _setup(rank, n, uid)
        import numpy as np

        import oracle_lib as O

        res = {}
        tdt = {O.F16: torch.float16, O.F32: torch.float32, O.I32: torch.int32}

        def fill(send, code, count, seq):
            send.view(torch.uint8).copy_(torch.from_numpy(O.lcg(code, count, rank, seq).view(np.uint8).copy()))

        seq = 0
        for code, count in ((O.F16, 4097), (O.F32, 100003), (O.I32, 12)):
            es = O.itemsize(code)
            send = torch.empty(count, dtype=tdt[code], device="cuda")
            whole = torch.empty(count * es + GUARD, dtype=torch.uint8, device="cuda")
            recv = whole[:count * es].view(tdt[code])
            ok = True
            for root in (0, n - 1, n // 2, 0):  # the root changes from call to call
                seq += 1
                fill(send, code, count, seq)
                whole.fill_(FILL)
                # non-roots pass no receive buffer on every other call, a real one otherwise
                out = recv if rank == root or seq % 2 else None
                comm.reduce(send, out, root=root)
                torch.cuda.synchronize()
                got = whole.cpu().numpy()
                if rank == root:
                    ok = ok and np.array_equal(got[:count * es], _expect(O, np, code, n, count, seq, root))
                    ok = ok and bool((got[count * es:] == FILL).all())
                else:
                    ok = ok and bool((got == FILL).all())
                ok = ok and np.array_equal(send.view(torch.uint8).cpu().numpy(), O.lcg(code, count, rank, seq).view(np.uint8))
            res["out_of_place_%d" % code] = ok
            # the same buffers again: the registration of the send buffer is cached
            before = comm.registration_exchanges()[:2]
            seq += 1
            fill(send, code, count, seq)
            comm.reduce(send, recv if rank == 1 else None, root=1)
            torch.cuda.synchronize()
            res["cached_%d" % code] = comm.registration_exchanges()[:2] == before
            if rank == 1:
                res["again_%d" % code] = np.array_equal(whole[:count * es].cpu().numpy(), _expect(O, np, code, n, count, seq, 1))
            # in place on the root (recv=None everywhere)
            ok = True
            for root in (n - 1, 0):
                seq += 1
                fill(send, code, count, seq)
                comm.reduce(send, None, root=root)
                torch.cuda.synchronize()
                want = _expect(O, np, code, n, count, seq, root) if rank == root else O.lcg(code, count, rank, seq).view(np.uint8)
                ok = ok and np.array_equal(send.view(torch.uint8).cpu().numpy(), want)
            res["in_place_%d" % code] = ok
        # an all_reduce and a broadcast between two reduces: the token channels are shared
        count = 50001
        send = torch.empty(count, dtype=torch.float32, device="cuda")
        recv = torch.empty(count, dtype=torch.float32, device="cuda")
        x = torch.full((1 << 18,), float(rank + 1), dtype=torch.float16, device="cuda")
        y = torch.empty_like(x)
        b = torch.arange(12345, dtype=torch.float32, device="cuda") + 1000 * rank
        bc = torch.empty_like(b)
        ok = True
        for it in range(2):
            seq += 1
            fill(send, O.F32, count, seq)
            comm.reduce(send, recv, root=it % n)
            comm.all_reduce(x, y, algo="fullmesh")
            comm.broadcast(b, bc, root=n - 1)
            seq += 1
            first = recv.clone()
            fill(send, O.F32, count, seq)
            comm.reduce(send, recv, root=(it + 1) % n)
            torch.cuda.synchronize()
            if rank == it % n:
                ok = ok and np.array_equal(first.view(torch.uint8).cpu().numpy(), _expect(O, np, O.F32, n, count, seq - 1, it % n))
            if rank == (it + 1) % n:
                ok = ok and np.array_equal(recv.view(torch.uint8).cpu().numpy(), _expect(O, np, O.F32, n, count, seq, (it + 1) % n))
            ok = ok and bool((y == n * (n + 1) / 2).all())
            ok = ok and bool(torch.equal(bc, torch.arange(12345, dtype=torch.float32, device="cuda") + 1000 * (n - 1)))
        res["mixed"] = ok
        # float64 is not carried and there is no vendor library: ncclInternalError on every rank, no launch;
        # the next fp32 reduce still completes exactly
        d = torch.zeros(64, dtype=torch.float64, device="cuda")
        try:
            comm.reduce(d, d.clone(), root=0)
            res["f64"] = 0
        except m.MscclppError as e:
            res["f64"] = e.code
        seq += 1
        fill(send, O.F32, count, seq)
        comm.reduce(send, recv, root=n - 1)
        torch.cuda.synchronize()
        res["after_f64"] = rank != n - 1 or np.array_equal(recv.view(torch.uint8).cpu().numpy(),
                                                           _expect(O, np, O.F32, n, count, seq, n - 1))
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("n", [2, 4, 8])
def test_reduce_through_the_nccl_abi(built, n):
    got = _spawn(_worker, n)
    for rank in range(n):
        res = dict(got[rank])
        assert res.pop("err") == 0, (rank, got[rank])
        assert res.pop("f64") == INTERNAL_ERROR, (rank, got[rank])
        assert not [k for k, ok in res.items() if not ok], (rank, res)
