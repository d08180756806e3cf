"""int64 / uint64 / int8 reductions through the NCCL ABI, one rank per process (placed by mp_util), no
vendor library: ncclAllReduce, ncclReduceScatter and ncclReduce take the pull-reduce kernel
(kernels/pull_reduce.hip) for ncclInt64 / ncclUint64 / ncclInt8 with sum, min, max and avg.  The C
entry points are called through ctypes with the ncclDataType_t / ncclRedOp_t values themselves
(uint64 has no torch dtype to carry it), and once through the Communicator methods with torch.int64
tensors.  Results are compared bit for bit with the numpy reference of int_reduce_cases, which every
rank computes from all ranks' inputs; every worker runs under the collect() watchdog from its first
call."""
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

        import int_reduce_cases as C

        res = {"device": dev, "shared": shared}
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

        def run(coll, code, op, cnt, inplace=False, root=0):
            """One call with new data; True when this rank's result, guard and send buffer are right."""
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
            code_ = call(coll, send.data_ptr(), rp, cnt, nccl_type[code], nccl_op[op], root)
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

        cases = [(C.I64, op) for op in C.OPS] + [(C.U64, C.MAX), (C.U64, C.AVG), (C.I8, C.SUM), (C.I8, C.AVG)]
        for code, op in cases:
            ok = True
            for k, coll in enumerate(C.COLLS):
                ok = run(coll, code, op, count, root=(k + op) % n) and ok
                ok = run(coll, code, op, count, inplace=True, root=(k + op + 1) % n) and ok
            res["%s_%s" % (C.NAMES[code], C.OP_NAMES[op])] = ok
        res["one_element_max"] = run(C.ALLREDUCE, C.I64, C.MAX, 1)
        # the Communicator methods with torch.int64 tensors (PyTorch's default integer type)
        xs = C.inputs(C.I64, C.SUM, n, count * n, 4900)
        x = torch.from_numpy(xs[rank].view(np.int64).copy()).cuda()
        ref = C.ref_sum(C.I64, xs).view(np.int64)
        y = comm.all_reduce(x, torch.empty_like(x), op="sum")
        block = comm.reduce_scatter(x, torch.empty(count, dtype=torch.int64, device="cuda"), op="sum")
        at_root = comm.reduce(x, torch.empty_like(x) if rank == 1 else None, root=1, op="sum")
        torch.cuda.synchronize()
        ok = np.array_equal(y.cpu().numpy(), ref)
        ok = ok and np.array_equal(block.cpu().numpy(), ref[rank * count:(rank + 1) * count])
        ok = ok and (rank != 1 or np.array_equal(at_root.cpu().numpy(), ref))
        flag = comm.all_reduce(torch.tensor([rank == n - 1], device="cuda").to(torch.int64), op="max")  # an early-stop flag
        total = comm.all_reduce(torch.tensor([10 ** 12 + rank], device="cuda"), op="sum")             # a token counter
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
        res["after_refused"] = run(C.ALLREDUCE, C.I64, C.SUM, count)
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("n", [2, 8])
def test_int_reductions_through_the_nccl_abi(built, n):
    got = _spawn(_worker, n)
    ndev = mp_util.export_device_count()
    devices = {got[r]["device"] for r in range(n)}
    assert len(devices) == min(n, max(1, ndev)), devices  # distinct GPUs where the machine has them
    for rank in range(n):
        res = dict(got[rank])
        res.pop("device"), res.pop("shared")
        assert res.pop("err") == 0, (rank, got[rank])
        assert res.pop("refused") == [INTERNAL_ERROR, INVALID_ARGUMENT, INVALID_ARGUMENT], (rank, got[rank])
        assert not [k for k, ok in res.items() if not ok], (rank, res)
