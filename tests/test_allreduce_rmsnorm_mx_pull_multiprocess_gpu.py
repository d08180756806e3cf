"""Communicator.all_reduce_rms_norm_mx_pull, one rank per process: test_allreduce_rmsnorm_mx_pull_gpu.py's judges on
(7, 2080) and 65 x 8192 in both formats, an eager call then captured and replayed twice on new data, refusals alike on
every rank with a good call behind them, no device error, q and scale equal across the ranks."""
import multiprocessing as mp
import os
import traceback

import mp_util
import numpy as np
import pytest

import allreduce_rmsnorm_model as M
import test_allreduce_rmsnorm_mx_pull_gpu as X

pytestmark = pytest.mark.gpu
DT = "bf16"


def buffers(torch, rows, cols, fmt, mode):  # x, gamma, fmt, q, scale, residual, res_out: the method's arguments
    t = lambda *s, d=torch.bfloat16: torch.zeros(*s, dtype=d, device="cuda")
    r_in = t(rows, cols) if mode != "none" else None
    return [t(rows, cols), t(cols), fmt, t(rows, cols if fmt == "mxfp8" else cols // 2, d=torch.uint8),
            t(rows, cols // 32, d=torch.uint8), r_in, r_in if mode != "out_of_place" else t(rows, cols)]


def call(torch, comm, rank, n, rows, cols, fmt, mode, seed, bufs=None, graph=None):
    """A call on fresh inputs (in `bufs`, or in new buffers), or a replay of `graph` over bufs: (failed checks, q + scale)."""
    xs, res, _ = M.inputs(seed, n, rows, cols, DT, mode != "none")
    gamma = X.block_gamma(seed, cols, DT)
    bufs = bufs or buffers(torch, rows, cols, fmt, mode)
    put = lambda buf, bits: buf.view(torch.int16).copy_(torch.from_numpy(bits.view(np.int16)))
    y = torch.zeros(rows, cols, dtype=torch.bfloat16, device="cuda")  # the pull method's y of the same inputs
    r_in = None if res is None else put(torch.zeros_like(y), res).view(torch.bfloat16)
    for buf, bits in ((bufs[0], xs[rank]), (bufs[5], res), (bufs[1], gamma)):
        if buf is not None:
            put(buf, bits)
    torch.cuda.synchronize()
    comm.barrier()  # every rank's new data is in place before any replay reads it
    if graph:
        graph.replay()
    else:
        comm.all_reduce_rms_norm_mx_pull(*bufs, eps=float(M.EPS))
    comm.all_reduce_rms_norm_pull(bufs[0], bufs[1], y, r_in, r_in, eps=float(M.EPS))
    torch.cuda.synchronize()
    q, e, ro = bufs[3].cpu().numpy(), bufs[4].cpu().numpy(), bufs[6]
    bits = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16)
    bad = X.judge(M.model(xs, res, gamma, DT), bits(y), DT, fmt, q, e, None if ro is None else bits(ro))[0]
    return bad, q.tobytes() + e.tobytes()


def refusals(torch, comm):  # cols % 32, an unknown format, a bf16 q, a scale of the wrong shape, a q inside x
    import mscclpp_amd as m

    t = lambda *s, d=torch.bfloat16: torch.zeros(*s, dtype=d, device="cuda")
    x, g, q, sc, codes = t(4, 64), t(64), t(4, 64, d=torch.uint8), t(4, 2, d=torch.uint8), []
    for args in ((t(4, 48), t(48), "mxfp8", t(4, 48, d=torch.uint8), t(4, 1, d=torch.uint8)), (x, g, "mxfp6", q, sc),
                 (x, g, "mxfp8", t(4, 64), sc), (x, g, "mxfp4", q[:, :32].contiguous(), t(4, 4, d=torch.uint8)),
                 (x, g, "mxfp4", x.view(torch.uint8).view(-1)[:128].view(4, 32), sc)):
        try:
            comm.all_reduce_rms_norm_mx_pull(*args)
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
        for fmt in X.FORMATS:
            for rows, cols, mode in ((7, 2080, "none"), (7, 2080, "in_place"), (65, 8192, "out_of_place")):
                res[f"{fmt} {rows}x{cols} {mode}"] = call(torch, comm, rank, n, rows, cols, fmt, mode, [rows, len(mode)])
            bufs = buffers(torch, 7, 2080, fmt, "out_of_place")  # an eager call, then the same buffers captured and replayed
            res[f"{fmt} eager before the capture"] = call(torch, comm, rank, n, 7, 2080, fmt, "out_of_place", 200, bufs)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=torch.cuda.Stream()):
                comm.all_reduce_rms_norm_mx_pull(*bufs, eps=float(M.EPS), stream=torch.cuda.current_stream())
            for it in (201, 202):
                res[f"{fmt} replay {it}"] = call(torch, comm, rank, n, 7, 2080, fmt, "out_of_place", it, bufs, g)
                comm.barrier()
            del g
        codes = refusals(torch, comm)
        res["after the refusals"] = call(torch, comm, rank, n, 7, 2080, "mxfp4", "in_place", 300)
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
        assert err == 0 and codes == [4] * 5, (rank, err, codes)
        for k, (bad, bits) in res.items():
            assert not bad, (rank, k, bad)
            assert bits == got[0][0][k][1], f"{k}: q or scale of rank {rank} differs from rank 0's"
