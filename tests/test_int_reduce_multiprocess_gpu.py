"""int64 / uint64 / int8 reductions through the NCCL ABI, one rank per process (placed by mp_util), no
vendor library: ncclInt64 / ncclUint64 / ncclInt8 with sum, min, max and avg, on both kernels the
dispatch chooses between.  Every row is in abi_path_cases.INT with the path it means to take, and every
ncclAllReduce / ncclReduceScatter / ncclReduce call is checked against the communicator's own account
(abi_path_cases.Account).  Each rank count runs twice: "pull" (MSCCLPP_AMD_PULL_LL_MAX_BYTES=0) sends
every call to the pull-reduce kernel (kernels/pull_reduce.hip), the torch.int64 convenience calls and the
one-element AllReduce included; "ll" (the default environment) sends every AllReduce and ReduceScatter of
these sizes to the LL kernel (kernels/pull_reduce_ll.hip) and Reduce to the pull kernel, and then runs an
int64 SUM AllReduce in place and an int8 MIN ReduceScatter at exactly the built-in cutover (LL) and one
element above it (pull, on fresh buffers).  The C entry points are called through ctypes with the
ncclDataType_t / ncclRedOp_t values themselves (uint64 has no torch dtype to carry it), and once through
the Communicator methods with torch.int64 tensors.  Results are compared bit for bit with the numpy
reference of int_reduce_cases, which every rank computes from all ranks' inputs; every worker runs under
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
NCCL_INT8, NCCL_INT64, NCCL_UINT64 = 0, 4, 5
NCCL_SUM, NCCL_PROD, NCCL_MAX, NCCL_MIN, NCCL_AVG = 0, 1, 2, 3, 4


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
        import int_reduce_cases as C

        res = {"device": dev, "shared": shared}
        acct = T.Account(comm, n, mode)
        nccl_type = {C.I64: NCCL_INT64, C.U64: NCCL_UINT64, C.I8: NCCL_INT8}
        nccl_op = {C.SUM: NCCL_SUM, C.MIN: NCCL_MIN, C.MAX: NCCL_MAX, C.AVG: NCCL_AVG}
        L = m.lib()
        seed = [4000]
        count = 1031
        # views inside one allocation per direction: a send range of n blocks and a receive range, both
        # 24 bytes past the allocation's start
        send_all = torch.empty(24 + count * n * 8 + GUARD, dtype=torch.uint8, device="cuda")
        recv_all = torch.empty(24 + count * 8 + GUARD, dtype=torch.uint8, device="cuda")

        def call(coll, sp, rp, cnt, dt, op, root):
            """The C entry point itself; returns its ncclResult_t."""
            if coll == C.ALLREDUCE:
                return L.ncclAllReduce(sp, rp, cnt, dt, op, comm.comm, m.stream_ptr())
            if coll == C.REDUCE_SCATTER:
                return L.ncclReduceScatter(sp, rp, cnt, dt, op, comm.comm, m.stream_ptr())
            return L.ncclReduce(sp, rp, cnt, dt, op, root, comm.comm, m.stream_ptr())

        def run(row, root=0):
            """One call of a table row with new data, under the account; True when this rank's result,
            guard and send buffer are right."""
            coll, code, op, cnt, inplace = row.coll, row.code, row.op, T.count_of(row, n), row.inplace
            es = C.itemsize(code)
            total = cnt * (n if coll == C.REDUCE_SCATTER else 1)
            seed[0] += 1
            xs = C.inputs(code, op, n, total, seed[0])
            ref = C.reference(code, op, xs)
            send_all.fill_(FILL)
            recv_all.fill_(FILL)
            send = send_all[24:24 + total * es]
            send.copy_(torch.from_numpy(xs[rank].view(np.uint8).copy()))
            mine = slice(rank * cnt, (rank + 1) * cnt) if coll == C.REDUCE_SCATTER else slice(None)
            receives = coll != C.REDUCE or rank == root
            if inplace:
                recv = send[rank * cnt * es:(rank + 1) * cnt * es] if coll == C.REDUCE_SCATTER else send
            else:
                recv = recv_all[24:24 + cnt * es]
            # a Reduce's non-root ranks pass no receive buffer, or (every other call) one that must stay untouched
            rp = recv.data_ptr() if receives or (not inplace and seed[0] % 2) else None
            code_ = acct.call(row, lambda: call(coll, send.data_ptr(), rp, cnt, nccl_type[code], nccl_op[op], root),
                              send.data_ptr(), recv.data_ptr())
            torch.cuda.synchronize()
            if code_ != 0:
                return False
            want_send = xs[rank].copy()
            if inplace and receives:
                want_send[mine] = ref[mine]
            got_send = send_all.cpu().numpy()
            ok = np.array_equal(got_send[24:24 + total * es].view(C.bits_dtype(code)), want_send)
            ok = ok and bool((got_send[:24] == FILL).all()) and bool((got_send[24 + total * es:] == FILL).all())
            got = recv_all.cpu().numpy()
            if inplace or not receives:
                return ok and bool((got == FILL).all())
            ok = ok and np.array_equal(got[24:24 + cnt * es].view(C.bits_dtype(code)), ref[mine])
            return ok and bool((got[:24] == FILL).all()) and bool((got[24 + cnt * es:] == FILL).all())

        for row in T.part(T.INT, "main"):  # per (type, op): every collective, out of place and in place
            k = C.COLLS.index(row.coll)
            ok = run(row, root=(k + row.op + row.inplace) % n)
            res[row.key] = res.get(row.key, True) and ok
        assert len(res) == 2 + len(T.INT_CASES)
        res["one_element_max"] = run(T.part(T.INT, "one_element")[0])
        # the Communicator methods with torch.int64 tensors (PyTorch's default integer type)
        xs = C.inputs(C.I64, C.SUM, n, count * n, 4900)
        x = torch.from_numpy(xs[rank].view(np.int64).copy()).cuda()
        ref = C.ref_sum(C.I64, xs).view(np.int64)
        ar, rs, rd = T.part(T.INT, "communicator")
        y, block = torch.empty_like(x), torch.empty(count, dtype=torch.int64, device="cuda")
        acct.call(ar, lambda: comm.all_reduce(x, y, op="sum"), x.data_ptr(), y.data_ptr())
        acct.call(rs, lambda: comm.reduce_scatter(x, block, op="sum"), x.data_ptr())
        at_root = acct.call(rd, lambda: comm.reduce(x, torch.empty_like(x) if rank == 1 else None, root=1, op="sum"), x.data_ptr())
        torch.cuda.synchronize()
        ok = np.array_equal(y.cpu().numpy(), ref)
        ok = ok and np.array_equal(block.cpu().numpy(), ref[rank * count:(rank + 1) * count])
        ok = ok and (rank != 1 or np.array_equal(at_root.cpu().numpy(), ref))
        flag = torch.tensor([rank == n - 1], device="cuda").to(torch.int64)  # an early-stop flag
        total = torch.tensor([10 ** 12 + rank], device="cuda")                # a token counter
        acct.call(T.part(T.INT, "flag")[0], lambda: comm.all_reduce(flag, op="max"), flag.data_ptr(), flag.data_ptr())
        acct.call(T.part(T.INT, "counter")[0], lambda: comm.all_reduce(total, op="sum"), total.data_ptr(), total.data_ptr())
        torch.cuda.synchronize()
        res["communicator_int64"] = ok and int(flag.item()) == 1 and int(total.item()) == n * 10 ** 12 + n * (n - 1) // 2
        # ncclProd stays what an uncarried operation is: ncclInvalidArgument from AllReduce and
        # ReduceScatter, ncclInternalError from Reduce -- and nothing is launched
        send = send_all[24:24 + count * n * 8]
        recv = recv_all[24:24 + count * 8]
        send_all.fill_(FILL)
        recv_all.fill_(FILL)
        res["refused"] = [call(coll, send.data_ptr(), recv.data_ptr(), count, NCCL_INT64, NCCL_PROD, 0) for coll in C.COLLS]
        torch.cuda.synchronize()
        res["refused_wrote_nothing"] = bool((recv_all == FILL).all()) and bool((send_all == FILL).all())
        res["after_refused"] = run(T.part(T.INT, "after_refused")[0])
        # the default dispatch as a user meets it: at exactly the cutover (LL), one element above it (pull)
        for row, case_seed in T.cutover_rows(T.INT, mode):
            res[row.key] = T.run_fresh(torch, comm, rank, acct, row, case_seed)
        res["paths"] = acct.wrong
        res["calls"] = dict(acct.calls)
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("path", ["ll", "pull"])
def test_int_reductions_through_the_nccl_abi(built, path, n):
    got = _spawn(_worker, n, 240, path)
    ndev = mp_util.export_device_count()
    devices = {got[r]["device"] for r in range(n)}
    assert len(devices) == min(n, max(1, ndev)), devices  # distinct GPUs where the machine has them
    for rank in range(n):
        res = dict(got[rank])
        res.pop("device"), res.pop("shared")
        assert res.pop("err") == 0, (rank, got[rank])
        assert res.pop("refused") == [INTERNAL_ERROR, INVALID_ARGUMENT, INVALID_ARGUMENT], (rank, got[rank])
        # (part, key, coll, declared path, rise of pull_ll_count, exchanges before, after) of every call that
        # did not take the path its row declares
        assert res.pop("paths") == [], (rank, path)
        calls = res.pop("calls")
        assert calls["pull"] > 0 and (calls["ll"] > 0) == (path == "ll"), (rank, calls)
        assert ("one_element_above_i64_sum_coll2" in res) == ("one_element_above_i8_min_coll1" in res) == (path == "ll")
        assert not [k for k, ok in res.items() if not ok], (rank, res)
