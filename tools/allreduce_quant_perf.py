"""Timing of the quantised-wire AllReduce (kernels/allreduce_quant.hip) beside ncclAllReduce through the
selector, one rank per process (rank r on device r % device_count: with a GPU per rank every byte between ranks
crosses xGMI; on fewer GPUs the ranks share devices and no link is priced -- the header says which).  Per rank count
and size, fp16, in place, in the same run and alternating, each captured in a HIP graph of K calls, median of ROUNDS
rounds with min / max, after the outputs are checked (quantised: inside the block bound of §17n against the
selector's sum):

  mxint8, mxfp4  Communicator.all_reduce_quant
  selector       Communicator.all_reduce (ncclAllReduce; MSCCLPP_AMD_ALLREDUCE_QUANT is removed from the environment)

us per call and the algorithmic GB/s of the UNQUANTISED payload (bytes / time), so the columns compare.

    python tools/allreduce_quant_perf.py   (NRANKS=2,4,8 SIZES_MIB=1,2,...,256; writes profiles/allreduce_quant_mp.json, or $OUT)
"""
import json
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NRANKS = [int(v) for v in os.environ.get("NRANKS", "2,4,8").split(",")]
SIZES = [int(float(v) * (1 << 20)) for v in os.environ.get("SIZES_MIB", "1,2,4,8,16,32,64,128,256").split(",")]
ROUNDS = int(os.environ.get("ROUNDS", 5))
K = {"mxint8": 2.0 ** -6, "mxfp4": 0.5}


def graph_us(torch, comm, fn, calls, replays):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn(s)  # eager once on this stream: first-launch set-up stays out of the capture
    s.synchronize()
    comm.barrier()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(calls):
            fn(torch.cuda.current_stream())
    g.replay()
    torch.cuda.synchronize()
    comm.barrier()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (calls * replays)


def worker(rank, n, uid, q):
    os.environ.pop("MSCCLPP_AMD_ALLREDUCE_QUANT", None)
    import mp_util
    import numpy as np

    import mscclpp_amd as m

    _, shared = mp_util.place_rank(rank, n)
    import torch

    comm, rows = m.Communicator(rank, n, uid), []
    for nbytes in SIZES:
        count = nbytes // 2
        torch.manual_seed(rank)
        x = torch.empty(count, dtype=torch.float16, device="cuda").uniform_(-1, 1)
        bufs = {k: torch.empty_like(x) for k in ("mxint8", "mxfp4", "selector")}
        cands = {"mxint8": lambda s: comm.all_reduce_quant(x, bufs["mxint8"], "mxint8", stream=s),
                 "mxfp4": lambda s: comm.all_reduce_quant(x, bufs["mxfp4"], "mxfp4", stream=s),
                 "selector": lambda s: comm.all_reduce(x, bufs["selector"], stream=s)}
        for fn in cands.values():
            fn(torch.cuda.current_stream())
        torch.cuda.synchronize()
        # |x| < 1 on every rank: a block's amax_r < 1 and amax_s < n, so the block bound is below 2 k n (+ roundings)
        row = {"bytes": nbytes, "device_error": comm.device_error()}
        for k in K:
            worst = float((bufs[k].float() - bufs["selector"].float()).abs().max())
            row[k + "_max_abs_diff"] = round(worst, 5)
            assert worst <= 2 * K[k] * n + n * 2.0 ** -10, (k, nbytes, worst)
        calls, replays = (4, 3) if nbytes >= (32 << 20) else (10, 3)
        t = {k: [] for k in cands}
        for _ in range(ROUNDS):
            for name, fn in cands.items():
                t[name].append(graph_us(torch, comm, fn, calls, replays))
        for k, v in t.items():
            us = float(np.median(v))
            row.update({k + "_us": round(us, 2), k + "_us_min_max": [round(min(v), 2), round(max(v), 2)],
                        k + "_algo_GBps": round(nbytes / us / 1e3, 1)})
        rows.append(row)
        if rank == 0:
            print(n, row, flush=True)
    comm.barrier()
    comm.destroy()
    q.put((rank, {"nranks": n, "ranks_share_devices": shared, "rows": rows}, None))


if __name__ == "__main__":
    import mp_util

    import mscclpp_amd as m

    mp_util.export_device_count()
    ctx, results = mp.get_context("spawn"), []
    for n in NRANKS:
        uid, q = m.Communicator.unique_id(), ctx.Queue()
        procs = [ctx.Process(target=worker, args=(r, n, uid, q)) for r in range(n)]
        for p in procs:
            p.start()
        got = {}
        while len(got) < n:
            rank, res, _ = q.get(timeout=900)
            got[rank] = res
        for p in procs:
            p.join(timeout=30)
        results.append(got[0])
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "allreduce_quant_mp.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    head = {"tool": "tools/allreduce_quant_perf.py", "dtype": "fp16", "rounds": ROUNDS,
            "note": "one rank per process; graph-captured, alternating, median of rounds; GB/s of the unquantised payload"}
    with open(out, "w") as f:
        json.dump(dict(head, results=results), f, indent=1)
