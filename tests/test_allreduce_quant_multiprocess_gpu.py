"""Communicator.all_reduce_quant, one rank per process (2 and 8 ranks): a tensor view inside an allocation judged as in
test_allreduce_quant_gpu.py, a capture replayed twice on new data, and ncclAllReduce under
MSCCLPP_AMD_ALLREDUCE_QUANT on either side of ..._MIN_BYTES and with fp32, told apart by quant_count()."""
import multiprocessing as mp
import os
import traceback

import mp_util
import numpy as np
import pytest

import allreduce_quant_model as Q

pytestmark = pytest.mark.gpu
DT, MIN_BYTES = "bf16", 4096


def worker(rank, n, uid, fmt, q):
    try:
        os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "10000")
        os.environ["MSCCLPP_AMD_ALLREDUCE_QUANT"] = fmt
        os.environ["MSCCLPP_AMD_ALLREDUCE_QUANT_MIN_BYTES"] = str(MIN_BYTES)
        for var in ("MSCCLPP_AMD_NCCL_LIB_PATH", "MSCCLPP_NCCL_LIB_PATH"):
            os.environ.pop(var, None)
        import mscclpp_amd as m
        import torch

        mp_util.place_rank(rank, n)
        comm = m.Communicator(rank, n, uid)
        count = 32 * (64 * n + 5)
        room = torch.zeros(count + 64, dtype=torch.bfloat16, device="cuda")
        x, out = room[8:8 + count], torch.zeros(count, dtype=torch.bfloat16, device="cuda")  # a view 16 bytes in
        bits = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16)
        res = {}

        def step(seed, what, call):
            xs = Q.inputs(seed, n, count, DT, fmt)
            x.view(torch.int16).copy_(torch.from_numpy(xs[rank].view(np.int16)))
            torch.cuda.synchronize()
            comm.barrier()  # every rank's new data is in place before any replay reads it
            call()
            torch.cuda.synchronize()
            err, bound = Q.error_and_bound(xs, bits(out), DT, fmt)
            res[what] = (np.array_equal(bits(out), Q.model(xs, DT, fmt)), bool((err <= bound).all()))
            comm.barrier()

        step(10, "eager", lambda: comm.all_reduce_quant(x, out, fmt))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            comm.all_reduce_quant(x, out, fmt, stream=torch.cuda.current_stream())
        for seed in (11, 12):
            step(seed, f"replay {seed}", g.replay)
        del g
        c0 = comm.quant_count()
        step(13, "ncclAllReduce above the threshold", lambda: comm.all_reduce(x, out))
        c1 = comm.quant_count()
        few = MIN_BYTES // 4  # elements: half the threshold in bytes
        small = comm.all_reduce(torch.full((few,), float(rank + 1), dtype=torch.bfloat16, device="cuda"))
        f32 = comm.all_reduce(torch.full((count,), float(rank + 1), dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        exact = bool((small == n * (n + 1) // 2).all().item() and (f32 == n * (n + 1) // 2).all().item())
        counts = (c1 - c0, comm.quant_count() - c1)
        out_ = (res, counts, exact, comm.device_error())
        comm.barrier()
        comm.destroy()
        q.put((rank, out_, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("n,fmt", [(2, "mxint8"), (8, "mxfp4")])
def test_across_processes(built, n, fmt):
    import mscclpp_amd as m

    ctx, uid = mp.get_context("spawn"), m.Communicator.unique_id()
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, n, uid, fmt, q)) for r in range(n)]
    for p in procs:
        p.start()
    got = mp_util.collect(procs, q, n, 240)
    for rank in range(n):
        res, counts, exact, err = got[rank]
        assert err == 0 and counts == (1, 0) and exact, (rank, err, counts, exact)
        assert all(res[k] == (True, True) for k in res) and len(res) == 4, (rank, res)
