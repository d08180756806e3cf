"""Communicator.all_reduce_rms_norm_quant_pull, one rank per process: test_allreduce_rmsnorm_quant_pull_gpu.py's judges
on (7, 2064) and 65 x 8192, an eager call then captured and replayed three times on new data, refusals alike on every
rank with a good call behind them, no device error, q and scale equal across the ranks."""
import multiprocessing as mp
import os
import traceback

import mp_util
import numpy as np
import pytest

import allreduce_rmsnorm_model as M
import test_allreduce_rmsnorm_quant_pull_gpu as Q

pytestmark = pytest.mark.gpu
DT = "bf16"


def buffers(torch, rows, cols, mode):  # x, gamma, q, scale, residual, res_out: the method's arguments
    t = lambda *s, d=torch.bfloat16: torch.zeros(*s, dtype=d, device="cuda")
    r_in = t(rows, cols) if mode != "none" else None
    return (t(rows, cols), t(cols), t(rows, cols, d=torch.uint8), t(rows, d=torch.float32), r_in,
            r_in if mode != "out_of_place" else t(rows, cols))


def call(torch, comm, rank, n, rows, cols, mode, seed, bufs=None, graph=None):
    """A call on fresh inputs (in `bufs`, or in new buffers), or a replay of `graph` over bufs: (failed checks, q + scale)."""
    xs, res, gamma = M.inputs(seed, n, rows, cols, DT, mode != "none")
    bufs = bufs or buffers(torch, rows, cols, mode)
    for buf, bits in ((bufs[0], xs[rank]), (bufs[4], res), (bufs[1], gamma)):
        if buf is not None:
            buf.view(torch.int16).copy_(torch.from_numpy(bits.view(np.int16)))
    torch.cuda.synchronize()
    if graph:
        comm.barrier()  # every rank's new data is in place before any replay reads it
        graph.replay()
    else:
        comm.all_reduce_rms_norm_quant_pull(*bufs, eps=float(M.EPS))
    torch.cuda.synchronize()
    q, s, ro = bufs[2].cpu().numpy(), bufs[3].cpu().numpy(), bufs[5]
    ro = None if ro is None else ro.view(torch.int16).cpu().numpy().view(np.uint16)
    bad = Q.judge(torch, M.model(xs, res, gamma, DT), DT, q, s, ro)[0]
    return bad, q.tobytes() + s.tobytes()


def refusals(torch, comm):  # cols % 16, a bf16 q, a scale of the wrong length, a q inside x
    import mscclpp_amd as m

    t = lambda *s, d=torch.bfloat16: torch.zeros(*s, dtype=d, device="cuda")
    x, g, q, sc, codes = t(4, 64), t(64), t(4, 64, d=torch.uint8), t(4, d=torch.float32), []
    for args in ((t(4, 24), t(24), t(4, 24, d=torch.uint8), sc), (x, g, t(4, 64), sc), (x, g, q, t(5, d=torch.float32)),
                 (x, g, x.view(torch.uint8).view(8, 64)[:4], sc)):
        try:
            comm.all_reduce_rms_norm_quant_pull(*args)
            codes.append(0)
        except m.MscclppError as e:
            codes.append(e.code)
    return codes


def worker(rank, n, uid, q):
    try:
        os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "10000")
        for var in ("MSCCLPP_AMD_NCCL_LIB_PATH", "MSCCLPP_NCCL_LIB_PATH"):
            os.environ.pop(var, None)
        import mscclpp_amd as m
        import torch

        mp_util.place_rank(rank, n)
        comm = m.Communicator(rank, n, uid)
        res = {}
        for rows, cols in ((7, 2064), (65, 8192)):
            for mode in ("none", "out_of_place", "in_place"):
                res[f"{rows}x{cols} {mode}"] = call(torch, comm, rank, n, rows, cols, mode, [rows, len(mode)])
        bufs = buffers(torch, 7, 2064, "out_of_place")  # an eager call, then the same buffers captured and replayed
        res["eager before the capture"] = call(torch, comm, rank, n, 7, 2064, "out_of_place", 200, bufs)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            comm.all_reduce_rms_norm_quant_pull(*bufs, eps=float(M.EPS), stream=torch.cuda.current_stream())
        for it in (201, 202, 203):
            res[f"replay {it}"] = call(torch, comm, rank, n, 7, 2064, "out_of_place", it, bufs, g)
            comm.barrier()
        del g
        codes = refusals(torch, comm)
        res["after the refusals"] = call(torch, comm, rank, n, 7, 2064, "in_place", 300)
        out = (res, codes, comm.device_error())
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
        assert err == 0 and codes == [4] * 4, (rank, err, codes)
        for k, (bad, bits) in res.items():
            assert not bad, (rank, k, bad)
            assert bits == got[0][0][k][1], f"{k}: q or scale of rank {rank} differs from rank 0's"
