"""ncclMax / ncclAvg through the NCCL ABI, one rank per process (placed by mp_util), no vendor library,
on both kernels the dispatch chooses between.  Every row of the file is in abi_path_cases.MAXAVG with
the path it means to take, and every ncclAllReduce / ncclReduceScatter / ncclReduce call is checked
against the communicator's own account (abi_path_cases.Account: pull_ll_count() and
registration_exchanges() before and after).  Each rank count runs twice:

  "pull"  MSCCLPP_AMD_PULL_LL_MAX_BYTES=0: every call takes the pull-reduce kernel (kernels/pull_reduce.hip);
          send (and an AllReduce's receive) buffers are IPC-registered per allocation -- the first use
          exchanges, the repeat on the same buffers does not; in place is peerOutput = peerInput across
          real mappings; the capture pins registrations; "mixed" puts a pull AllReduce between a
          fullmesh SUM AllReduce and a Broadcast on the shared token counters.  Also at 3 ranks (the
          slice split of an odd rank count).
  "ll"    the default environment: the same rows; AllReduce and ReduceScatter take the LL kernel
          (kernels/pull_reduce_ll.hip) wherever the cutover says so -- everywhere at 2 and 4 ranks, all
          but the 100003-element calls at 8 -- and Reduce the pull kernel.  Then two pairs of rows at
          exactly the built-in cutover (LL) and one element above it (pull, on fresh buffers).

Results are compared with the numpy reference of pull_reduce_cases, which every rank computes from
all ranks' inputs (bit for bit; any NaN where the AVG reference is NaN at a planted position); every
worker runs under the collect() watchdog from its first call."""
import multiprocessing as mp
import os
import traceback

import abi_path_cases as T
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


def _setup(rank, n, uid, mode):
    os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "10000")
    os.environ.pop("MSCCLPP_AMD_NCCL_LIB_PATH", None)  # no vendor library
    os.environ.pop("MSCCLPP_NCCL_LIB_PATH", None)
    import abi_path_cases as T

    T.set_mode(mode)  # before the library is imported: it reads the variable once
    import torch

    import mscclpp_amd as m

    dev, shared = mp_util.place_rank(rank, n)
    return torch, m, m.Communicator(rank, n, uid), dev, shared


def _worker(rank, n, uid, q, mode):
    try:
        torch, m, comm, dev, shared = _setup(rank, n, uid, mode)
        import numpy as np

        import abi_path_cases as T
        import oracle_lib as O
        import pull_reduce_cases as C

        res = {"device": dev, "shared": shared}
        acct = T.Account(comm, n, mode)
        tdt = {O.F16: torch.float16, O.BF16: torch.bfloat16, O.F32: torch.float32, O.I32: torch.int32}
        opname = {C.MAX: "max", C.AVG: "avg"}
        seed = [2000]

        def check(code, op, got_bytes, want, offset=0, planted=True):
            got = got_bytes.cpu().numpy().view(C.bits_dtype(code))
            return C.mismatches(code, op, got, want, planted, offset).size == 0

        def run(row, send, whole, root=0):
            """One call of a table row on the given buffers with new data, under the account; True when
            this rank's result, guard and send buffer are right."""
            coll, code, op, inplace, count = row.coll, row.code, row.op, row.inplace, T.count_of(row, n)
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
                    acct.call(row, lambda: comm.all_reduce(sv, sv, op=opname[op]), sv.data_ptr(), sv.data_ptr())
                    torch.cuda.synchronize()
                    return check(code, op, sv.view(torch.uint8), ref, 0, planted), sv.view(torch.uint8).cpu().numpy().tobytes()
                if coll == C.REDUCE_SCATTER:
                    acct.call(row, lambda: comm.reduce_scatter(sv, sv[rank * count:(rank + 1) * count], op=opname[op]), sv.data_ptr())
                    torch.cuda.synchronize()
                    want = xs[rank].copy()
                    want[rank * count:(rank + 1) * count] = ref[rank * count:(rank + 1) * count]
                    return check(code, op, sv.view(torch.uint8), want, 0, planted and rank == 0), None
                acct.call(row, lambda: comm.reduce(sv, None, root=root, op=opname[op]), sv.data_ptr())
                torch.cuda.synchronize()
                return check(code, op, sv.view(torch.uint8), ref if rank == root else xs[rank], 0, planted and rank == root), None
            whole.fill_(FILL)
            recv = whole[:count * es].view(tdt[code])
            if coll == C.ALLREDUCE:
                acct.call(row, lambda: comm.all_reduce(sv, recv, op=opname[op]), sv.data_ptr(), recv.data_ptr())
            elif coll == C.REDUCE_SCATTER:
                acct.call(row, lambda: comm.reduce_scatter(sv, recv, op=opname[op]), sv.data_ptr())
            else:
                acct.call(row, lambda: comm.reduce(sv, recv if rank == root or seed[0] % 2 else None, root=root, op=opname[op]),
                          sv.data_ptr())
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

        big = max(T.MAXAVG_COUNTS)
        for code in T.MAXAVG_TYPES:
            es = O.itemsize(code)
            send = torch.empty(big * n, dtype=tdt[code], device="cuda")
            whole = torch.empty(big * es + GUARD, dtype=torch.uint8, device="cuda")
            acct.keep += [send, whole]  # kept alive: a later buffer at a registered address would exchange nothing
            first = comm.registration_exchanges()[:2]
            same = {}
            for row in T.part(T.MAXAVG, "main", code=code):
                good, image = run(row, send, whole, root=(row.count + row.coll) % n)
                res[row.key] = res.get(row.key, True) and good
                if row.coll == C.ALLREDUCE:  # byte-identical on all ranks
                    all_images = comm_gather(comm, m, image, n)
                    same[row.key] = same.get(row.key, True) and all(x == all_images[0] for x in all_images)
            for key, ok in same.items():
                res["identical_" + key] = ok
            # the same buffers again: both registrations are cached, no host exchange -- and under "pull"
            # there were exchanges to cache: the send and the receive buffer, a new pointer each
            before = comm.registration_exchanges()[:2]
            if mode == T.PULL:
                res["registered_%s" % C.NAMES[code]] = sum(before) >= sum(first) + 2
            ok = True
            for row in T.part(T.MAXAVG, "again", code=code):
                ok = run(row, send, whole, root=1)[0] and ok
            res["again_%s" % C.NAMES[code]] = ok
            res["cached_%s" % C.NAMES[code]] = comm.registration_exchanges()[:2] == before
            ok = True
            for row in T.part(T.MAXAVG, "in_place", code=code):
                ok = run(row, send, None, root=n - 1)[0] and ok
            res["in_place_%s" % C.NAMES[code]] = ok
        # an existing SUM AllReduce and a Broadcast between two new calls: the token channels are shared
        send = torch.empty(50001, dtype=torch.float32, device="cuda")
        whole = torch.empty(50001 * 4 + GUARD, dtype=torch.uint8, device="cuda")
        acct.keep += [send, whole]
        x = torch.full((1 << 18,), float(rank + 1), dtype=torch.float16, device="cuda")
        y = torch.empty_like(x)
        b = torch.arange(12345, dtype=torch.float32, device="cuda") + 1000 * rank
        bc = torch.empty_like(b)
        ok = True
        mixed = T.part(T.MAXAVG, "mixed")
        for it in range(2):
            ok = run(mixed[2 * it], send, whole)[0] and ok
            comm.all_reduce(x, y, algo="fullmesh")
            comm.broadcast(b, bc, root=n - 1)
            ok = run(mixed[2 * it + 1], send, whole, root=it)[0] and ok
            ok = ok and bool((y == n * (n + 1) / 2).all())
            ok = ok and bool(torch.equal(bc, torch.arange(12345, dtype=torch.float32, device="cuda") + 1000 * (n - 1)))
        res["mixed"] = ok
        if n == 2:  # one capture and replay of an AllReduce AVG
            row, = T.part(T.MAXAVG, "graph")
            count = row.count
            sv = send[:count]
            whole.fill_(FILL)
            recv = whole[:count * 4].view(torch.float32)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):  # eager once: under "pull" the buffers are registered
                acct.call(row, lambda: comm.all_reduce(sv, recv, op="avg", stream=s), sv.data_ptr(), recv.data_ptr())
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                acct.call(row, lambda: comm.all_reduce(sv, recv, op="avg", stream=torch.cuda.current_stream()),
                          sv.data_ptr(), recv.data_ptr())
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
        res["after_refused"] = run(T.part(T.MAXAVG, "after_refused")[0], send, whole)[0]
        # Buffers the ranks group into allocations differently, as a caching allocator fed rank-dependent
        # sizes does: even ranks hold A and C in one allocation and B in another, odd ranks A alone and B
        # and C together.  A and B make both allocations known; a peer pointer of C built from the base
        # cached with A (or B) and the peer's offset of C would then lie in the peer's other allocation.
        import ctypes

        slot = 1 << 15
        sizes = (2 * slot, slot) if rank % 2 == 0 else (slot, 2 * slot)
        hip = [ctypes.c_void_p(), ctypes.c_void_p()]
        for p, size in zip(hip, sizes):
            m.check(m.lib().mscclppAmdMalloc(ctypes.byref(p), size), "malloc")
        views = [m.device_view(p.value, size).view(torch.float32) for p, size in zip(hip, sizes)]
        buf_a, buf_b = views[0][:slot // 4], views[1][:slot // 4]
        buf_c = views[rank % 2][slot // 4:]
        rows = T.part(T.MAXAVG, "regrouped")
        ok = True
        for row, buf, root in zip(rows, (buf_a, buf_b, buf_c, buf_c, buf_c), (0, 1, 0, 1, 0)):
            ok = run(row, buf, None if row.inplace else whole, root=root)[0] and ok
        res["regrouped"] = ok
        # the default dispatch as a user meets it: at exactly the cutover (LL), one element above it (pull)
        for row, case_seed in T.cutover_rows(T.MAXAVG, mode):
            res[row.key] = T.run_fresh(torch, comm, rank, acct, row, case_seed)
        res["paths"] = acct.wrong
        res["calls"] = dict(acct.calls)
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        del views, buf_a, buf_b, buf_c
        for p in hip:
            m.check(m.lib().mscclppAmdFree(p), "free")
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


RANKS = T.MAXAVG_RANKS  # "ll": 2, 4, 8; "pull": 2, 3, 4, 8


@pytest.mark.parametrize("path,n", [(path, n) for path in ("ll", "pull") for n in RANKS[path]])
def test_max_and_avg_through_the_nccl_abi(built, path, n):
    got = _spawn(_worker, n, 240, path)
    ndev = mp_util.export_device_count()
    devices = {got[r]["device"] for r in range(n)}
    assert len(devices) == min(n, max(1, ndev)), devices  # distinct GPUs where the machine has them
    print(f"\n{n} ranks on {len(devices)} device(s)" + (" (shared)" if got[0]["shared"] else " (one rank per GPU)"))
    for rank in range(n):
        res = dict(got[rank])
        res.pop("device"), res.pop("shared")
        assert res.pop("err") == 0, (rank, got[rank])
        assert res.pop("refused") == [INVALID_ARGUMENT, INVALID_ARGUMENT, INTERNAL_ERROR], (rank, got[rank])
        # (part, key, coll, declared path, rise of pull_ll_count, exchanges before, after) of every call that
        # did not take the path its row declares
        assert res.pop("paths") == [], (rank, path)
        calls = res.pop("calls")
        assert calls["pull"] > 0 and (calls["ll"] > 0) == (path == "ll"), (rank, calls)
        assert ("registered_f32" in res) == (path == "pull") and ("at_the_cutover_bf16_avg_coll2" in res) == (path == "ll")
        assert not [k for k, ok in res.items() if not ok], (rank, res)
