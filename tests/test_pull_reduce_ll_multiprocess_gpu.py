"""Small MAX / AVG / int64 / PreMulSum AllReduce and ReduceScatter calls through the NCCL ABI take the
LL path (kernels/pull_reduce_ll.hip): one rank per process (placed by mp_util), no vendor library.
What shows the path is the communicator's own account -- pull_ll_count() rises by one per call and
registration_exchanges() does not move, on tensors the communicator has never seen -- beside results
compared bit for bit with the numpy references (through pull_reduce_ll_cases), which every rank
computes from all ranks' inputs.  Every worker runs under the collect() watchdog from its first call."""
import multiprocessing as mp
import os
import traceback

import mp_util
import pytest

pytestmark = pytest.mark.gpu


def _spawn(target, n, timeout=240, *extra):
    import mscclpp_amd as m

    uid = m.Communicator.unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, n, uid, q) + extra) for r in range(n)]
    for p in procs:
        p.start()
    return mp_util.collect(procs, q, n, timeout)


def _setup(rank, n, uid, ll_max=None):
    os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "10000")
    os.environ.pop("MSCCLPP_AMD_NCCL_LIB_PATH", None)  # no vendor library
    os.environ.pop("MSCCLPP_NCCL_LIB_PATH", None)
    os.environ.pop("MSCCLPP_AMD_PULL_LL_MAX_BYTES", None)
    if ll_max is not None:
        os.environ["MSCCLPP_AMD_PULL_LL_MAX_BYTES"] = ll_max
    import torch

    import mscclpp_amd as m

    dev, shared = mp_util.place_rank(rank, n)
    return torch, m, m.Communicator(rank, n, uid), dev, shared


class Runner:
    """Calls on fresh tensors (all kept alive, so no address comes back) and their judgement."""

    def __init__(self, torch, m, comm, rank, n):
        import int_reduce_cases as I
        import oracle_lib as O

        self.torch, self.m, self.comm, self.rank, self.n = torch, m, comm, rank, n
        self.keep = []
        self.tdt = {O.F16: torch.float16, O.BF16: torch.bfloat16, O.F32: torch.float32, O.I32: torch.int32,
                    I.I64: torch.int64, I.I8: torch.int8}

    def buffers(self, row, coll, count, seed, case=None):
        """(xs, ss, this rank's want, send, recv): new data in tensors never used before."""
        import numpy as np

        import pull_reduce_ll_cases as C

        torch, n, rank = self.torch, self.n, self.rank
        total = count * (n if coll == C.REDUCE_SCATTER else 1)
        xs, ss = case or C.make_case(row, n, total, seed)
        ref = C.reference(row, xs, ss)
        want = ref[rank * count:(rank + 1) * count] if coll == C.REDUCE_SCATTER else ref
        send = torch.from_numpy(xs[rank].view(np.uint8).copy()).cuda().view(self.tdt[row[1]])
        recv = torch.zeros(count, dtype=self.tdt[row[1]], device="cuda")
        self.keep += [send, recv]
        return xs, ss, want, send, recv

    def right(self, row, recv, want):
        import pull_reduce_ll_cases as C

        self.torch.cuda.synchronize()
        got = recv.view(self.torch.uint8).cpu().numpy().view(C.bits_dtype(row))
        return C.mismatches(row, got, want).size == 0

    def call(self, row, coll, send, recv, op=None, root=0):
        import pull_reduce_ll_cases as C

        op = {C.SUM: "sum", C.MIN: "min", C.MAX: "max", C.AVG: "avg"}[row[2]] if op is None else op
        if coll == C.ALLREDUCE:
            self.comm.all_reduce(send, recv, op=op)
        elif coll == C.REDUCE_SCATTER:
            self.comm.reduce_scatter(send, recv, op=op)
        else:
            self.comm.reduce(send, recv if self.rank == root else None, root=root, op=op)

    def run(self, row, coll, count, seed, took_ll=True):
        """True when the result is right, the count rose by one (or stayed) and nothing was registered
        (or something was)."""
        comm = self.comm
        count0, reg0 = comm.pull_ll_count(), comm.registration_exchanges()[:2]
        xs, ss, want, send, recv = self.buffers(row, coll, count, seed)
        self.call(row, coll, send, recv)
        ok = self.right(row, recv, want)
        if took_ll:
            return ok and comm.pull_ll_count() == count0 + 1 and comm.registration_exchanges()[:2] == reg0
        return ok and comm.pull_ll_count() == count0 and sum(comm.registration_exchanges()[:2]) > sum(reg0)


def _worker(rank, n, uid, q):
    try:
        torch, m, comm, dev, shared = _setup(rank, n, uid)
        import time

        import numpy as np

        import int_reduce_cases as I
        import oracle_lib as O
        import premul_sum_cases as S
        import pull_reduce_ll_cases as C

        res = {"device": dev, "shared": shared}
        run = Runner(torch, m, comm, rank, n)
        res["count_starts_at_zero"] = comm.pull_ll_count() == 0
        # ---- fresh tensors ---------------------------------------------------------------------
        res["int64_sum_one_element"] = run.run(("int", I.I64, C.SUM), C.ALLREDUCE, 1, 11)
        res["f32_max"] = run.run(("pull", O.F32, C.MAX), C.ALLREDUCE, 257, 12)
        res["bf16_avg"] = run.run(("pull", O.BF16, C.AVG), C.ALLREDUCE, 131, 13)
        res["reduce_scatter_3_element_blocks"] = run.run(("pull", O.F16, C.AVG), C.REDUCE_SCATTER, 3, 14) and \
            run.run(("int", I.I64, C.MAX), C.REDUCE_SCATTER, 3, 15)
        res["int8_min_in_place"] = True
        xs, ss, want, send, _ = run.buffers(("int", I.I8, C.MIN), C.ALLREDUCE, 67, 16)
        c0 = comm.pull_ll_count()
        comm.all_reduce(send, send, op="min")
        res["int8_min_in_place"] = run.right(("int", I.I8, C.MIN), send, want) and comm.pull_ll_count() == c0 + 1
        # the planted lanes: operands in rank order on every rank
        if n >= 3:
            row = ("pull", O.F32, C.AVG)
            xs, ss, want, send, recv = run.buffers(row, C.ALLREDUCE, C.ORDER_COUNT, 0, case=C.order_case(row, n))
            run.call(row, C.ALLREDUCE, send, recv)
            res["rank_order"] = run.right(row, recv, want) and bool(want[0] != 0)
        # ---- the largest size the rule sends to LL, and one element more --------------------------
        for coll in C.LL_COLLS:
            most = C.BUILTIN_MAX[(coll, C.measured_ranks(n))]
            row = ("pull", O.F32, C.MAX)
            res["at_the_cutover_%d" % coll] = run.run(row, coll, most // 4, 20 + coll)
            res["one_element_above_%d" % coll] = run.run(row, coll, most // 4 + 1, 22 + coll, took_ll=False)
        # ---- other paths -------------------------------------------------------------------------
        row = ("pull", O.F32, C.MAX)
        c0 = comm.pull_ll_count()
        xs, ss, want, send, recv = run.buffers(row, C.REDUCE, 257, 30)
        run.call(row, C.REDUCE, send, recv, root=n - 1)
        res["reduce_keeps_the_pull_path"] = (rank != n - 1 or run.right(row, recv, want)) and comm.pull_ll_count() == c0
        x = torch.full((257,), float(rank + 1), dtype=torch.float32, device="cuda")
        y = comm.all_reduce(x, torch.empty_like(x), op="sum")
        torch.cuda.synchronize()
        res["sum_is_not_counted"] = bool((y == n * (n + 1) / 2).all()) and comm.pull_ll_count() == c0
        # ---- PreMulSum: create / call / destroy at once ------------------------------------------
        for k, (code, coll) in enumerate(((O.BF16, C.ALLREDUCE), (O.F32, C.REDUCE_SCATTER))):
            row = ("premul", code, C.PREMUL_SUM)
            ss = S.scalars(code, n, 40 + k, "generic")
            total = 131 * (n if coll == C.REDUCE_SCATTER else 1)
            xs, ss, want, send, recv = run.buffers(row, coll, 131, 0, case=(S.inputs(code, n, total, 40 + k, ss), ss))
            c0, reg0 = comm.pull_ll_count(), comm.registration_exchanges()[:2]
            h = comm.create_premul_sum(float(ss[rank]), run.tdt[code])
            run.call(row, coll, send, recv, op=h)
            comm.destroy_op(h)  # at once: the stream has not run yet
            res["premul_immediate_%d" % k] = run.right(row, recv, want) and comm.pull_ll_count() == c0 + 1 and \
                comm.registration_exchanges()[:2] == reg0
            ss = S.scalars(code, n, 50 + k, "special")
            xs, ss, want, send, recv = run.buffers(row, coll, 131, 0, case=(S.inputs(code, n, total, 50 + k, ss), ss))
            factor = torch.from_numpy(S.scalar_bits(code, [ss[rank]]).view(np.uint8).copy()).cuda().view(run.tdt[code])
            h = comm.create_premul_sum(factor, run.tdt[code])
            run.call(row, coll, send, recv, op=h)
            comm.destroy_op(h)
            res["premul_device_%d" % k] = run.right(row, recv, want) and comm.pull_ll_count() == c0 + 2
        # ---- a late rank -------------------------------------------------------------------------
        row = ("pull", O.BF16, C.AVG)
        xs, ss, want, send, recv = run.buffers(row, C.ALLREDUCE, 131, 60)
        torch.cuda.synchronize()
        comm.barrier()
        if rank == n - 1:
            time.sleep(0.05)
        run.call(row, C.ALLREDUCE, send, recv)
        res["late_rank"] = run.right(row, recv, want)
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def _worker_disabled(rank, n, uid, q):
    """MSCCLPP_AMD_PULL_LL_MAX_BYTES=0: the same small AllReduce takes the pull path, and registers."""
    try:
        torch, m, comm, dev, shared = _setup(rank, n, uid, ll_max="0")
        import oracle_lib as O
        import pull_reduce_ll_cases as C

        run = Runner(torch, m, comm, rank, n)
        res = {"takes_ll": m.pull_reduce_takes_ll(m.PULL_ALLREDUCE, n, 4)}
        res["f32_max"] = run.run(("pull", O.F32, C.MAX), C.ALLREDUCE, 257, 12, took_ll=False)
        res["count"] = comm.pull_ll_count()
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def _worker_cold_capture(rank, n, uid, q):
    """A fresh communicator: a small AVG AllReduce is captured with no eager call before it."""
    try:
        torch, m, comm, dev, shared = _setup(rank, n, uid)
        import numpy as np

        import oracle_lib as O
        import pull_reduce_ll_cases as C

        run = Runner(torch, m, comm, rank, n)
        row, count = ("pull", O.BF16, C.AVG), 131
        xs, ss, want, send, recv = run.buffers(row, C.ALLREDUCE, count, 70)
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rc = m.lib().ncclAllReduce(send.data_ptr(), recv.data_ptr(), count, m.nccl_dtype(send.dtype), m.nccl_op("avg"),
                                       comm.comm, m.stream_ptr(torch.cuda.current_stream()))
        res = {"captured": rc == 0}
        ok = True
        for it in range(2):
            xs, ss = C.make_case(row, n, count, 71 + it)
            send.copy_(torch.from_numpy(xs[rank].view(np.uint8).copy()).cuda().view(send.dtype))
            torch.cuda.synchronize()
            comm.barrier()
            g.replay()
            ok = ok and run.right(row, recv, C.reference(row, xs, ss))
            comm.barrier()
        res["replays"] = ok
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("n", [2, 3, 8])
def test_small_calls_take_the_ll_path(built, n):
    got = _spawn(_worker, n)
    ndev = mp_util.export_device_count()
    devices = {got[r]["device"] for r in range(n)}
    assert len(devices) == min(n, max(1, ndev)), devices  # distinct GPUs where the machine has them
    for rank in range(n):
        res = dict(got[rank])
        res.pop("device"), res.pop("shared")
        assert res.pop("err") == 0, (rank, got[rank])
        assert (n >= 3) == ("rank_order" in res)
        assert len(res) >= 17
        assert not [k for k, ok in res.items() if not ok], (rank, res)


def test_variable_zero_sends_the_same_call_to_the_pull_path(built):
    n = 2
    got = _spawn(_worker_disabled, n)
    for rank in range(n):
        res = got[rank]
        assert res["err"] == 0 and res["count"] == 0 and not res["takes_ll"] and res["f32_max"], (rank, res)


def test_cold_capture(built):
    n = 2
    got = _spawn(_worker_cold_capture, n)
    for rank in range(n):
        res = got[rank]
        assert res["err"] == 0 and res["captured"] and res["replays"], (rank, res)
