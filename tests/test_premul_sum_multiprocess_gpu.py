"""ncclRedOpCreatePreMulSum / ncclRedOpDestroy and the collectives that take their handles, through the NCCL
ABI, one rank per process (placed by mp_util), no vendor library, on both kernels the dispatch chooses
between.  Every row is in abi_path_cases.PREMUL with the path it means to take, and every ncclAllReduce /
ncclReduceScatter / ncclReduce call is checked against the communicator's own account
(abi_path_cases.Account).  Each rank count runs twice: "pull" (MSCCLPP_AMD_PULL_LL_MAX_BYTES=0) sends
every call to the pull-reduce kernel (kernels/pull_reduce.hip), where the scalars travel through the
token diagonal (written, read by the peers, zeroed again) -- host immediates, the device-resident scalar,
create / call / destroy at once and the graph replay with changed scalars; "ll" (the default environment)
sends the same AllReduce and ReduceScatter rows to the LL kernel (kernels/pull_reduce_ll.hip), where the
scalar rides in the packets, and then runs a bf16 AllReduce with a device-resident scalar and an fp32
ReduceScatter in place at exactly the built-in cutover (LL) and one element above it (pull, on fresh
buffers).  The sequence is PyTorch's (ProcessGroupNCCL): create the operation with a host-immediate scalar
of the element type, call the collective, destroy the operation at once -- before the stream has run --
and only then synchronise. Results are compared bit for bit with the numpy reference of premul_sum_cases
(any NaN where it is NaN), which every rank computes from all ranks' inputs and scalars; every worker
runs under the collect() watchdog from its first call."""
import multiprocessing as mp
import os
import traceback

import mp_util
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
INTERNAL_ERROR, INVALID_ARGUMENT = 3, 4
NCCL_INT32, NCCL_FLOAT16, NCCL_FLOAT32, NCCL_FLOAT64, NCCL_BFLOAT16 = 2, 6, 7, 8, 9
NCCL_SUM, NCCL_NUM_OPS = 0, 5
DEVICE, HOST_IMMEDIATE = 0, 1


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
        import ctypes

        import numpy as np

        import abi_path_cases as T
        import oracle_lib as O
        import premul_sum_cases as C

        res = {"device": dev, "shared": shared}
        acct = T.Account(comm, n, mode)
        nccl_type = {O.F16: NCCL_FLOAT16, O.BF16: NCCL_BFLOAT16, O.F32: NCCL_FLOAT32}
        tdt = {O.F16: torch.float16, O.BF16: torch.bfloat16, O.F32: torch.float32}
        L = m.lib()
        seed = [5000]
        count = 1031
        send_all = torch.empty(24 + count * n * 4 + GUARD, dtype=torch.uint8, device="cuda")
        recv_all = torch.empty(24 + count * 4 + GUARD, dtype=torch.uint8, device="cuda")

        def create(scalar_ptr, dt, residence=HOST_IMMEDIATE):
            """ncclRedOpCreatePreMulSum itself: (its ncclResult_t, the handle)."""
            h = ctypes.c_int(-1)
            rc = L.ncclRedOpCreatePreMulSum(ctypes.byref(h), scalar_ptr, dt, residence, comm.comm)
            return rc, h.value

        def host_scalar(code, value):
            """The scalar as one element of the element type in host memory (kept alive by the caller)."""
            raw = C.scalar_bits(code, [value]).tobytes()
            return ctypes.create_string_buffer(raw, len(raw))

        def call(coll, sp, rp, cnt, dt, op, root):
            """The C entry point itself; returns its ncclResult_t."""
            if coll == C.ALLREDUCE:
                return L.ncclAllReduce(sp, rp, cnt, dt, op, comm.comm, m.stream_ptr())
            if coll == C.REDUCE_SCATTER:
                return L.ncclReduceScatter(sp, rp, cnt, dt, op, comm.comm, m.stream_ptr())
            return L.ncclReduce(sp, rp, cnt, dt, op, root, comm.comm, m.stream_ptr())

        def load(coll, code, cnt, ss, inplace):
            """New data into the send buffer; (send, recv, what this rank must hold afterwards in each)."""
            es = O.itemsize(code)
            total = cnt * (n if coll == C.REDUCE_SCATTER else 1)
            seed[0] += 1
            xs = C.inputs(code, n, total, seed[0], ss)
            ref = C.reference(code, xs, ss)
            send_all.fill_(FILL)
            recv_all.fill_(FILL)
            send = send_all[24:24 + total * es]
            send.copy_(torch.from_numpy(xs[rank].view(np.uint8).copy()))
            if inplace:
                recv = send[rank * cnt * es:(rank + 1) * cnt * es] if coll == C.REDUCE_SCATTER else send
            else:
                recv = recv_all[24:24 + cnt * es]
            return xs, ref, send, recv

        def judge(coll, code, cnt, xs, ref, inplace, root):
            es = O.itemsize(code)
            total = cnt * (n if coll == C.REDUCE_SCATTER else 1)
            mine = slice(rank * cnt, (rank + 1) * cnt) if coll == C.REDUCE_SCATTER else slice(None)
            receives = coll != C.REDUCE or rank == root
            want_send = xs[rank].copy()
            if inplace and receives:
                want_send[mine] = ref[mine]
            got_send = send_all.cpu().numpy()
            ok = C.mismatches(code, got_send[24:24 + total * es].view(C.bits_dtype(code)), want_send).size == 0
            ok = ok and bool((got_send[:24] == FILL).all()) and bool((got_send[24 + total * es:] == FILL).all())
            got = recv_all.cpu().numpy()
            if inplace or not receives:
                return ok and bool((got == FILL).all())
            ok = ok and C.mismatches(code, got[24:24 + cnt * es].view(C.bits_dtype(code)), ref[mine]).size == 0
            return ok and bool((got[:24] == FILL).all()) and bool((got[24 + cnt * es:] == FILL).all())

        def run(row, ss, root=0):
            """PyTorch's sequence of a table row with new data, under the account; True when this rank's
            result, guards and send buffer are right."""
            coll, code, cnt, inplace = row.coll, row.code, T.count_of(row, n), row.inplace
            xs, ref, send, recv = load(coll, code, cnt, ss, inplace)
            receives = coll != C.REDUCE or rank == root
            keep = host_scalar(code, ss[rank])
            rc, h = create(keep, nccl_type[code])
            if rc != 0 or h < NCCL_NUM_OPS:
                return False
            rp = recv.data_ptr() if receives or (not inplace and seed[0] % 2) else None
            rc = acct.call(row, lambda: call(coll, send.data_ptr(), rp, cnt, nccl_type[code], h, root), send.data_ptr(),
                           recv.data_ptr())
            gone = L.ncclRedOpDestroy(h, comm.comm)  # at once: the stream has not run yet
            torch.cuda.synchronize()
            return rc == 0 and gone == 0 and judge(coll, code, cnt, xs, ref, inplace, root)

        for row in T.part(T.PREMUL, "main"):
            code, k = row.code, C.COLLS.index(row.coll)
            if row.key.endswith("_fsdp"):
                res[row.key] = run(row, C.fsdp_scalars(code, n), root=k % n)
            else:
                kind = "generic" if row.inplace else "special"
                res[row.key] = run(row, C.scalars(code, n, seed[0], kind), root=(k + 1) % n)
        assert len(res) == 2 + 2 * 3 * 3
        once, one = T.part(T.PREMUL, "once")
        res[once.key] = run(once, C.scalars(O.F16, n, 77, "generic"))
        res[one.key] = run(one, C.scalars(O.F32, n, 78, "generic"))
        # the Communicator methods: a Python factor (rounded to the dtype, a host immediate) and a handle as op=
        ss = C.fsdp_scalars(O.BF16, n)
        xs, ref, send, recv = load(C.REDUCE_SCATTER, O.BF16, count, ss, False)
        h = comm.create_premul_sum(1.0 / (2 * n), torch.bfloat16)
        acct.call(T.part(T.PREMUL, "communicator")[0],
                  lambda: comm.reduce_scatter(send.view(torch.bfloat16), recv.view(torch.bfloat16), op=h), send.data_ptr())
        comm.destroy_op(h)
        torch.cuda.synchronize()
        res["communicator_methods"] = judge(C.REDUCE_SCATTER, O.BF16, count, xs, ref, False, 0)

        # a device-resident scalar (what a tensor factor becomes)
        code, coll = O.F32, C.ALLREDUCE
        ss = C.scalars(code, n, 80, "generic")
        dev_scalar = torch.from_numpy(C.scalar_bits(code, [ss[rank]]).view(np.uint8).copy()).cuda()
        rc, hdev = create(dev_scalar.data_ptr(), nccl_type[code], DEVICE)
        xs, ref, send, recv = load(coll, code, count, ss, False)
        ok = rc == 0 and acct.call(T.part(T.PREMUL, "device")[0],
                                   lambda: call(coll, send.data_ptr(), recv.data_ptr(), count, nccl_type[code], hdev, 0),
                                   send.data_ptr(), recv.data_ptr()) == 0
        torch.cuda.synchronize()
        res["device_scalar"] = ok and judge(coll, code, count, xs, ref, False, 0)
        if n == 2:  # ... captured, and replayed after the scalar and the data were changed
            s = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = acct.call(T.part(T.PREMUL, "graph")[0],
                               lambda: L.ncclAllReduce(send.data_ptr(), recv.data_ptr(), count, nccl_type[code], hdev, comm.comm,
                                                       m.stream_ptr(torch.cuda.current_stream())),
                               send.data_ptr(), recv.data_ptr())
            ok = rc == 0
            for it in range(2):
                ss = C.scalars(code, n, 81 + it, C.KINDS[it])
                xs, ref, send, recv = load(coll, code, count, ss, False)
                dev_scalar.copy_(torch.from_numpy(C.scalar_bits(code, [ss[rank]]).view(np.uint8).copy()))
                torch.cuda.synchronize()
                comm.barrier()
                g.replay()
                torch.cuda.synchronize()
                comm.barrier()
                ok = ok and judge(coll, code, count, xs, ref, False, 0)
            res["graph"] = ok
        res["device_destroy"] = L.ncclRedOpDestroy(hdev, comm.comm) == 0

        # ---- handle rules ----------------------------------------------------------------------
        k1, k2 = host_scalar(O.F32, 0.5), host_scalar(O.BF16, 0.25)
        (rc1, h1), (rc2, h2) = create(k1, NCCL_FLOAT32), create(k2, NCCL_BFLOAT16)
        res["handles_distinct"] = rc1 == 0 and rc2 == 0 and h1 >= NCCL_NUM_OPS and h2 >= NCCL_NUM_OPS and h1 != h2
        res["destroy"] = L.ncclRedOpDestroy(h1, comm.comm) == 0
        res["destroy_twice"] = L.ncclRedOpDestroy(h1, comm.comm)
        rc3, h3 = create(k1, NCCL_FLOAT32)
        res["slot_reused"] = rc3 == 0 and h3 == h1
        res["destroy_rest"] = L.ncclRedOpDestroy(h3, comm.comm) == 0
        send = send_all[24:24 + count * n * 4]
        recv = recv_all[24:24 + count * 4]
        send_all.fill_(FILL)
        recv_all.fill_(FILL)
        # use after destroy: what an uncarried operation answers
        res["after_destroy"] = [call(coll, send.data_ptr(), recv.data_ptr(), count, NCCL_FLOAT32, h3, 0) for coll in C.COLLS]
        # h2 was created for bf16
        res["type_mismatch"] = [call(coll, send.data_ptr(), recv.data_ptr(), count, NCCL_FLOAT32, h2, 0) for coll in C.COLLS]
        res["never_created"] = call(C.ALLREDUCE, send.data_ptr(), recv.data_ptr(), count, NCCL_FLOAT32, h2 + 40, 0)
        res["destroy_never_created"] = L.ncclRedOpDestroy(h2 + 40, comm.comm)
        res["destroy_builtin"] = L.ncclRedOpDestroy(NCCL_SUM, comm.comm)
        res["destroy_last"] = L.ncclRedOpDestroy(h2, comm.comm) == 0
        res["create_int32"] = create(k1, NCCL_INT32)[0]
        res["create_float64"] = create(ctypes.create_string_buffer(8), NCCL_FLOAT64)[0]
        res["create_bad_residence"] = create(k1, NCCL_FLOAT32, 2)[0]
        res["create_null_scalar"] = create(None, NCCL_FLOAT32)[0]
        res["create_null_op"] = L.ncclRedOpCreatePreMulSum(None, k1, NCCL_FLOAT32, HOST_IMMEDIATE, comm.comm)
        torch.cuda.synchronize()
        res["refusals_wrote_nothing"] = bool((recv_all == FILL).all()) and bool((send_all == FILL).all())

        # ---- afterwards ------------------------------------------------------------------------
        x = torch.full((4099,), float(rank + 1), dtype=torch.float32, device="cuda")
        y = comm.all_reduce(x, torch.empty_like(x), op="sum")
        torch.cuda.synchronize()
        res["plain_all_reduce"] = bool((y == n * (n + 1) / 2).all())
        # the default dispatch as a user meets it: at exactly the cutover (LL), one element above it (pull)
        for row, case_seed in T.cutover_rows(T.PREMUL, mode):
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
def test_premul_sum_through_the_nccl_abi(built, path, n):
    got = _spawn(_worker, n, 240, path)
    ndev = mp_util.export_device_count()
    devices = {got[r]["device"] for r in range(n)}
    assert len(devices) == min(n, max(1, ndev)), devices  # distinct GPUs where the machine has them
    for rank in range(n):
        res = dict(got[rank])
        res.pop("device"), res.pop("shared")
        assert res.pop("err") == 0, (rank, got[rank])
        assert res.pop("destroy_twice") == INVALID_ARGUMENT, (rank, got[rank])
        assert res.pop("after_destroy") == [INTERNAL_ERROR, INVALID_ARGUMENT, INVALID_ARGUMENT], (rank, got[rank])
        assert res.pop("type_mismatch") == [INVALID_ARGUMENT] * 3, (rank, got[rank])
        assert res.pop("never_created") == INVALID_ARGUMENT, (rank, got[rank])
        assert res.pop("destroy_never_created") == INVALID_ARGUMENT and res.pop("destroy_builtin") == INVALID_ARGUMENT
        assert res.pop("create_int32") == INTERNAL_ERROR and res.pop("create_float64") == INTERNAL_ERROR, (rank, got[rank])
        assert res.pop("create_bad_residence") == INVALID_ARGUMENT, (rank, got[rank])
        assert res.pop("create_null_scalar") == INVALID_ARGUMENT and res.pop("create_null_op") == INVALID_ARGUMENT
        assert (n == 2) == ("graph" in res)
        # (part, key, coll, declared path, rise of pull_ll_count, exchanges before, after) of every call that
        # did not take the path its row declares
        assert res.pop("paths") == [], (rank, path)
        calls = res.pop("calls")
        assert calls["pull"] > 0 and (calls["ll"] > 0) == (path == "ll"), (rank, calls)
        assert ("one_element_above_bf16_premulsum_coll2" in res) == ("one_element_above_f32_premulsum_coll1" in res) == (path == "ll")
        assert not [k for k, ok in res.items() if not ok], (rank, res)
