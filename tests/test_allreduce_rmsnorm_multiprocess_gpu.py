"""Communicator.all_reduce_rms_norm with one rank per process: the judges of test_allreduce_rmsnorm_gpu.py on
(3, 252) and (2, 8192), a captured call replayed on new data, the refusals alike on every rank with a good
call behind them, no device error; at 3 processes one call on `order_inputs` (fp32 adds that round, so "the own term
at position rank" is visible per process).  Not tested: a captured call whose scratch would have to grow (64 MiB are
held from init and the largest call carried needs 32 MiB, so no call reaches that refusal through the ABI)."""
import multiprocessing as mp
import os
import traceback

import mp_util
import numpy as np
import pytest

import allreduce_rmsnorm_model as M

pytestmark = pytest.mark.gpu


def call(torch, comm, rank, n, dt, rows, cols, mode, seed, graph=None, make=M.inputs):
    """A call on fresh inputs, or a replay of graph = (graph, x, residual, y, res_out, gamma): (failed checks, y)."""
    xs, res, gamma = make(seed, n, rows, cols, dt, mode != "none")
    if graph:
        g, x, r_in, y, r_out, gam = graph
        for buf, bits in ((x, xs[rank]), (r_in, res), (gam, gamma)):
            buf.t.view(torch.int16).copy_(torch.from_numpy(bits.view(np.int16)).view(buf.t.shape))
        torch.cuda.synchronize()
        comm.barrier()  # every rank's new data is in place before any replay reads it
        g.replay()
    else:
        gam = M.Guarded(torch, 1, cols, dt, gamma.reshape(1, cols))
        x = M.Guarded(torch, rows, cols, dt, xs[rank])
        y = x if mode == "in_place" else M.Guarded(torch, rows, cols, dt)
        r_in = M.Guarded(torch, rows, cols, dt, res) if mode != "none" else None
        r_out = r_in if mode != "out_of_place" else M.Guarded(torch, rows, cols, dt)
        comm.all_reduce_rms_norm(x.t, gam.t[0], y.t, r_in and r_in.t, r_out and r_out.t, eps=float(M.EPS))
    torch.cuda.synchronize()
    (got_y, ok_y), (got_r, ok_r) = y.read(), r_out.read() if r_out else (None, True)
    return M.judge(xs, res, gamma, dt, got_y, got_r) + ([] if ok_y and ok_r else ["guard bytes overwritten"]), got_y


def refusals(torch, comm):
    # cols % 4, over the lane limit, fp32, res_out without a residual, y overlapping x, a misaligned gamma; above 1 MiB
    import mscclpp_amd as m

    t = lambda *s, d=torch.bfloat16: torch.zeros(*s, dtype=d, device="cuda")
    x, y, r, g, big = t(4, 64), t(4, 64), t(4, 64), t(64), t(5, 64)
    codes = []
    for args, kw in (((t(4, 62), t(62)), {}), ((t(1, 16388), t(16388)), {}),
                     ((t(4, 64, d=torch.float32), t(64, d=torch.float32)), {}), ((x, g, y), dict(res_out=r)),
                     ((big[:4], g, big[1:]), {}), ((x, t(68).view(torch.int16)[1:65].view(torch.bfloat16), y), {}),
                     ((t(65, 8192), t(8192)), {})):
        try:
            comm.all_reduce_rms_norm(*args, **kw)
            codes.append(0)
        except m.MscclppError as e:
            codes.append(e.code)
    return codes


def worker(rank, n, uid, q):
    try:
        os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "10000")
        for var in ("MSCCLPP_AMD_NCCL_LIB_PATH", "MSCCLPP_NCCL_LIB_PATH", "MSCCLPP_AMD_ARNORM_MAX_BYTES"):
            os.environ.pop(var, None)
        import mscclpp_amd as m
        import torch

        mp_util.place_rank(rank, n)
        comm = m.Communicator(rank, n, uid)
        res, seed = {}, 100
        for dt in M.DTYPES:
            for rows, cols in ((3, 252), (2, 8192)):
                for mode in ("none", "out_of_place", "in_place"):
                    seed += 1
                    res[f"{dt} {rows}x{cols} {mode}"] = call(torch, comm, rank, n, dt, rows, cols, mode, seed)
        if n == 3:  # adds that round: a process that summed its own term first would show here
            res["order_inputs"] = call(torch, comm, rank, n, "bf16", 6, 2056, "out_of_place", 160, make=M.order_inputs)
        rows, cols, dt = 3, 252, "bf16"  # a capture behind an eager call of the same shape, replayed on new data
        res["eager before the capture"] = call(torch, comm, rank, n, dt, rows, cols, "out_of_place", 200)
        bufs = [M.Guarded(torch, rows, cols, dt) for _ in range(4)] + [M.Guarded(torch, 1, cols, dt)]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            comm.all_reduce_rms_norm(bufs[0].t, bufs[4].t[0], bufs[2].t, bufs[1].t, bufs[3].t, eps=float(M.EPS),
                                     stream=torch.cuda.current_stream())
        for it in (201, 202, 203):
            res[f"replay {it}"] = call(torch, comm, rank, n, dt, rows, cols, "out_of_place", it, (g, *bufs))
            comm.barrier()
        del g
        codes = refusals(torch, comm)
        res["after the refusals"] = call(torch, comm, rank, n, "fp16", 3, 252, "in_place", 300)
        out = ({k: (bad, y.tobytes()) for k, (bad, y) in res.items()}, codes, comm.device_error())
        comm.barrier()
        comm.destroy()
        q.put((rank, out, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("n", [2, 3])
def test_across_processes(built, n):
    import mscclpp_amd as m

    ctx, uid = mp.get_context("spawn"), m.Communicator.unique_id()
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, n, uid, q)) for r in range(n)]
    for p in procs:
        p.start()
    got = mp_util.collect(procs, q, n, 240)
    for rank in range(n):
        res, codes, err = got[rank]
        assert err == 0 and codes == [4, 4, 4, 4, 4, 4, 5], (rank, err, codes)
        for k, (bad, y) in res.items():
            assert not bad, (rank, k, bad)
            assert y == got[0][0][k][1], f"{k}: y of rank {rank} differs from rank 0's"
