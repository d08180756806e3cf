"""ncclMax / ncclAvg through the NCCL ABI, one rank per process (placed by mp_util), no vendor library:
ncclAllReduce, ncclReduceScatter and ncclReduce take the pull-reduce kernel (kernels/pull_reduce.hip),
send (and an AllReduce's receive) buffers are IPC-registered per allocation.  Results are compared
with the numpy reference of pull_reduce_cases, which every rank computes from all ranks' inputs
(bit for bit; any NaN where the AVG reference is NaN at a planted position); every worker runs under
the collect() watchdog from its first call."""
import multiprocessing as mp
import os
import traceback

import mp_util
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
INVALID_ARGUMENT, INTERNAL_ERROR = 4, 3


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
    os.environ.pop("MSCCLPP_AMD_NCCL_LIB_PATH", None)  # no vendor library
    os.environ.pop("MSCCLPP_NCCL_LIB_PATH", None)
    import torch

    import mscclpp_amd as m

    dev, shared = mp_util.place_rank(rank, n)
    return torch, m, m.Communicator(rank, n, uid), dev, shared


def _worker(rank, n, uid, q):
    try:
        torch, m, comm, dev, shared = _setup(rank, n, uid)
        import numpy as np

        import oracle_lib as O
        import pull_reduce_cases as C

        res = {"device": dev, "shared": shared}
        tdt = {O.F16: torch.float16, O.BF16: torch.bfloat16, O.F32: torch.float32, O.I32: torch.int32}
        opname = {C.MAX: "max", C.AVG: "avg"}
        seed = [2000]

        def check(code, op, got_bytes, want, offset=0, planted=True):
            got = got_bytes.cpu().numpy().view(C.bits_dtype(code))
            return C.mismatches(code, op, got, want, planted, offset).size == 0

        def run(coll, code, op, count, send, whole, inplace=False, root=0):
            """One call on the given buffers with new data; True when this rank's result, guard and send buffer are right."""
            es = O.itemsize(code)
            total = count * (n if coll == C.REDUCE_SCATTER else 1)
            seed[0] += 1
            xs = C.inputs(code, op, n, total, seed[0])
            ref = C.reference(code, op, xs)
            mine = torch.from_numpy(xs[rank].view(np.uint8).copy())
            send.view(torch.uint8)[:total * es].copy_(mine)
            sv = send[:total]
            planted = total >= C.MIN_PLANT
            if inplace:
                if coll == C.ALLREDUCE:
                    comm.all_reduce(sv, sv, op=opname[op])
                    torch.cuda.synchronize()
                    return check(code, op, sv.view(torch.uint8), ref, 0, planted), sv.view(torch.uint8).cpu().numpy().tobytes()
                if coll == C.REDUCE_SCATTER:
                    comm.reduce_scatter(sv, sv[rank * count:(rank + 1) * count], op=opname[op])
                    torch.cuda.synchronize()
                    want = xs[rank].copy()
                    want[rank * count:(rank + 1) * count] = ref[rank * count:(rank + 1) * count]
                    return check(code, op, sv.view(torch.uint8), want, 0, planted and rank == 0), None
                comm.reduce(sv, None, root=root, op=opname[op])
                torch.cuda.synchronize()
                return check(code, op, sv.view(torch.uint8), ref if rank == root else xs[rank], 0, planted and rank == root), None
            whole.fill_(FILL)
            recv = whole[:count * es].view(tdt[code])
            if coll == C.ALLREDUCE:
                comm.all_reduce(sv, recv, op=opname[op])
            elif coll == C.REDUCE_SCATTER:
                comm.reduce_scatter(sv, recv, op=opname[op])
            else:
                comm.reduce(sv, recv if rank == root or seed[0] % 2 else None, root=root, op=opname[op])
            torch.cuda.synchronize()
            got = whole.cpu().numpy()
            ok = bool((got[count * es:] == FILL).all())
            if coll == C.REDUCE and rank != root:
                ok = ok and bool((got == FILL).all())
            elif coll == C.REDUCE_SCATTER:
                ok = ok and check(code, op, whole[:count * es], ref[rank * count:(rank + 1) * count], rank * count, planted)
            else:
                ok = ok and check(code, op, whole[:count * es], ref, 0, planted)
            ok = ok and np.array_equal(sv.view(torch.uint8).cpu().numpy(), xs[rank].view(np.uint8))
            return ok, got[:count * es].tobytes()

        big = 100003
        for code in (O.F16, O.BF16, O.F32, O.I32):
            es = O.itemsize(code)
            send = torch.empty(big * n, dtype=tdt[code], device="cuda")
            whole = torch.empty(big * es + GUARD, dtype=torch.uint8, device="cuda")
            for op in (C.MAX, C.AVG):
                ok, same = True, True
                for count in (1, 4097, big):
                    for coll in C.COLLS:
                        good, image = run(coll, code, op, count, send, whole, root=(count + coll) % n)
                        ok = ok and good
                        if coll == C.ALLREDUCE:  # byte-identical on all ranks
                            all_images = comm_gather(comm, m, image, n)
                            same = same and all(x == all_images[0] for x in all_images)
                res["%s_%s" % (C.NAMES[code], opname[op])] = ok
                res["identical_%s_%s" % (C.NAMES[code], opname[op])] = same
            # the same buffers again: both registrations are cached, no host exchange
            before = comm.registration_exchanges()[:2]
            ok = True
            for coll in C.COLLS:
                ok = run(coll, code, C.AVG, 4097, send, whole, root=1)[0] and ok
            res["again_%s" % C.NAMES[code]] = ok
            res["cached_%s" % C.NAMES[code]] = comm.registration_exchanges()[:2] == before
            ok = True
            for coll in C.COLLS:
                for op in (C.MAX, C.AVG):
                    ok = run(coll, code, op, 4097, send, None, inplace=True, root=n - 1)[0] and ok
            res["in_place_%s" % C.NAMES[code]] = ok
        # an existing SUM AllReduce and a Broadcast between two new calls: the token channels are shared
        send = torch.empty(50001, dtype=torch.float32, device="cuda")
        whole = torch.empty(50001 * 4 + GUARD, dtype=torch.uint8, device="cuda")
        x = torch.full((1 << 18,), float(rank + 1), dtype=torch.float16, device="cuda")
        y = torch.empty_like(x)
        b = torch.arange(12345, dtype=torch.float32, device="cuda") + 1000 * rank
        bc = torch.empty_like(b)
        ok = True
        for it in range(2):
            ok = run(C.ALLREDUCE, O.F32, C.AVG, 50001, send, whole)[0] and ok
            comm.all_reduce(x, y, algo="fullmesh")
            comm.broadcast(b, bc, root=n - 1)
            ok = run(C.COLLS[it], O.F32, C.MAX, 50001 // n, send, whole, root=it)[0] and ok
            ok = ok and bool((y == n * (n + 1) / 2).all())
            ok = ok and bool(torch.equal(bc, torch.arange(12345, dtype=torch.float32, device="cuda") + 1000 * (n - 1)))
        res["mixed"] = ok
        if n == 2:  # one capture and replay of an AllReduce AVG
            count = 4097
            sv = send[:count]
            whole.fill_(FILL)
            recv = whole[:count * 4].view(torch.float32)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                comm.all_reduce(sv, recv, op="avg", stream=s)  # eager once: the buffers are registered
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                comm.all_reduce(sv, recv, op="avg", stream=torch.cuda.current_stream())
            ok = True
            for it in range(2):
                xs = C.inputs(O.F32, C.AVG, n, count, 3000 + it)
                sv.view(torch.uint8).copy_(torch.from_numpy(xs[rank].view(np.uint8).copy()))
                torch.cuda.synchronize()
                comm.barrier()
                g.replay()
                torch.cuda.synchronize()
                comm.barrier()
                ok = ok and check(O.F32, C.AVG, whole[:count * 4], C.ref_avg(O.F32, xs))
            res["graph"] = ok
        # what the path does not carry answers as before: prod is ncclInvalidArgument from AllReduce,
        # max on float64 ncclInvalidArgument from AllReduce and ncclInternalError from Reduce
        codes = []
        h = torch.ones(64, dtype=torch.float16, device="cuda")
        d = torch.zeros(64, dtype=torch.float64, device="cuda")
        for call in (lambda: m.check(m.lib().ncclAllReduce(h.data_ptr(), h.data_ptr(), 64, m.NCCL_DTYPES[h.dtype], 1,
                                                           comm.comm, m.stream_ptr()), "prod"),
                     lambda: m.check(m.lib().ncclAllReduce(d.data_ptr(), d.data_ptr(), 64, 8, 2, comm.comm, m.stream_ptr()),
                                     "f64 max"),
                     lambda: comm.reduce(d, d.clone(), root=0, op="max")):
            try:
                call()
                codes.append(0)
            except m.MscclppError as e:
                codes.append(e.code)
        res["refused"] = codes
        res["after_refused"] = run(C.ALLREDUCE, O.F32, C.MAX, 4097, send, whole)[0]
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def comm_gather(comm, m, image, n):
    """Every rank's bytes, through the bootstrap all-gather."""
    import ctypes

    send = ctypes.create_string_buffer(image, len(image))
    recv = ctypes.create_string_buffer(len(image) * n)
    m.check(m.lib().mscclppAmdCommAllGatherHost(comm.comm, send, recv, len(image)), "all-gather")
    return [recv.raw[r * len(image):(r + 1) * len(image)] for r in range(n)]


@pytest.mark.parametrize("n", [2, 4, 8])
def test_max_and_avg_through_the_nccl_abi(built, n):
    got = _spawn(_worker, n)
    ndev = mp_util.export_device_count()
    devices = {got[r]["device"] for r in range(n)}
    assert len(devices) == min(n, max(1, ndev)), devices  # distinct GPUs where the machine has them
    print(f"\n{n} ranks on {len(devices)} device(s)" + (" (shared)" if got[0]["shared"] else " (one rank per GPU)"))
    for rank in range(n):
        res = dict(got[rank])
        res.pop("device"), res.pop("shared")
        assert res.pop("err") == 0, (rank, got[rank])
        assert res.pop("refused") == [INVALID_ARGUMENT, INVALID_ARGUMENT, INTERNAL_ERROR], (rank, got[rank])
        assert not [k for k, ok in res.items() if not ok], (rank, res)
