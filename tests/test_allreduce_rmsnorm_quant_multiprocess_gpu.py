"""Communicator.all_reduce_rms_norm_quant, one rank per process: test_allreduce_rmsnorm_quant_gpu.py's judges on (7, 2080)
in the three formats, an eager call then captured and replayed twice on new data, refusals alike on every rank with a
good call behind them, no device error, q and scale equal across the ranks, and nothing registered by any of it."""
import multiprocessing as mp
import os
import traceback

import mp_util
import numpy as np
import pytest

import allreduce_rmsnorm_model as M
import test_allreduce_rmsnorm_quant_gpu as Q

pytestmark = pytest.mark.gpu
DT, ROWS, COLS = "bf16", 7, 2080


def buffers(torch, fmt, mode):  # x, gamma, fmt, q, scale, residual, res_out: the method's arguments
    t = lambda *s, d=torch.bfloat16: torch.zeros(*s, dtype=d, device="cuda")
    r_in = t(ROWS, COLS) if mode != "none" else None
    scale = t(ROWS, d=torch.float32) if fmt == "fp8_row" else t(ROWS, COLS // 32, d=torch.uint8)
    return [t(ROWS, COLS), t(COLS), fmt, t(ROWS, COLS // 2 if fmt == "mxfp4" else COLS, d=torch.uint8), scale, r_in,
            r_in if mode != "out_of_place" else t(ROWS, COLS)]


def call(torch, comm, rank, n, fmt, mode, seed, bufs=None, graph=None):
    """A call on fresh inputs (in `bufs`, or in new buffers), or a replay of `graph` over bufs: (failed checks, q + scale)."""
    xs, res, gamma = M.inputs(seed, n, ROWS, COLS, DT, mode != "none")
    gamma = Q.gamma_of(fmt, seed, COLS, DT, gamma)
    bufs = bufs or buffers(torch, fmt, mode)
    put = lambda buf, bits: buf.view(torch.int16).copy_(torch.from_numpy(bits.view(np.int16)))
    y = torch.zeros(ROWS, COLS, dtype=torch.bfloat16, device="cuda")  # all_reduce_rms_norm's y of the same inputs
    r_in = None if res is None else put(torch.zeros_like(y), res).view(torch.bfloat16)
    for buf, bits in ((bufs[0], xs[rank]), (bufs[5], res), (bufs[1], gamma)):
        if buf is not None:
            put(buf, bits)
    torch.cuda.synchronize()
    comm.barrier()  # every rank's new data is in place before any replay reads it
    if graph:
        graph.replay()
    else:
        comm.all_reduce_rms_norm_quant(*bufs, eps=float(M.EPS))
    comm.all_reduce_rms_norm(bufs[0], bufs[1], y, r_in, r_in, eps=float(M.EPS))
    torch.cuda.synchronize()
    q, s, ro = bufs[3].cpu().numpy(), bufs[4].cpu().numpy(), bufs[6]
    bits = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16)
    ref, ro = M.model(xs, res, gamma, DT), None if ro is None else bits(ro)
    if fmt == "fp8_row":
        bad = Q.ROW.judge(torch, ref, DT, q, s, ro)[0]
        want_q, want_s = Q.ROW.steps_5_to_7(torch, bits(y), DT)
        bad += [] if np.array_equal(q, want_q) and np.array_equal(s.view(np.uint32), want_s.view(np.uint32)) else ["steps 5-7 differ"]
    else:
        bad = Q.MX.judge(ref, bits(y), DT, fmt, q, s, ro)[0]
    return bad, q.tobytes() + s.tobytes()


def refusals(torch, comm):  # cols % 32 in an MX format, an unknown format, a bf16 q, an MX scale for fp8_row, a q inside x
    import mscclpp_amd as m

    t = lambda *s, d=torch.bfloat16: torch.zeros(*s, dtype=d, device="cuda")
    x, g, q, sc, codes = t(4, 64), t(64), t(4, 64, d=torch.uint8), t(4, 2, d=torch.uint8), []
    for args in ((t(4, 48), t(48), "mxfp8", t(4, 48, d=torch.uint8), t(4, 1, d=torch.uint8)), (x, g, "fp8", q, sc),
                 (x, g, "mxfp8", t(4, 64), sc), (x, g, "fp8_row", q, sc),
                 (x, g, "mxfp4", x.view(torch.uint8).view(-1)[:128].view(4, 32), sc)):
        try:
            comm.all_reduce_rms_norm_quant(*args)
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
        res, reg0 = {}, tuple(comm.registration_exchanges()[:2])
        for fmt in Q.FORMATS:
            for mode in ("none", "in_place"):
                res[f"{fmt} {mode}"] = call(torch, comm, rank, n, fmt, mode, [len(fmt), len(mode)])
            bufs = buffers(torch, fmt, "out_of_place")  # an eager call, then the same buffers captured and replayed
            res[f"{fmt} eager before the capture"] = call(torch, comm, rank, n, fmt, "out_of_place", 200, bufs)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=torch.cuda.Stream()):
                comm.all_reduce_rms_norm_quant(*bufs, eps=float(M.EPS), stream=torch.cuda.current_stream())
            for it in (201, 202):
                res[f"{fmt} replay {it}"] = call(torch, comm, rank, n, fmt, "out_of_place", it, bufs, g)
                comm.barrier()
            del g
        codes = refusals(torch, comm)
        res["after the refusals"] = call(torch, comm, rank, n, "mxfp4", "in_place", 300)
        out = (res, codes, comm.device_error(), tuple(comm.registration_exchanges()[:2]) == reg0)
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
        res, codes, err, unregistered = got[rank]
        assert err == 0 and codes == [4] * 5 and unregistered, (rank, err, codes, unregistered)
        for k, (bad, bits) in res.items():
            assert not bad, (rank, k, bad)
            assert bits == got[0][0][k][1], f"{k}: q or scale of rank {rank} differs from rank 0's"
