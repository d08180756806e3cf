"""Fabric-free timing of the native Reduce (kernels/reduce.hip): 8 ranks in ONE launch on one GPU
(blockIdx.y = rank, every peer buffer local HBM), so no link is priced -- what is measured is the
root's memory pipeline (n S bytes read, S written, by the root's workgroups alone) and the two
handshakes.  Per size S (bytes per rank, fp16), each timing from a HIP graph of K calls:

  sweep      the Reduce at nblocks in {8, 16, 32, 64, 128} x nthreads in {512, 256}; a grid the device
             cannot hold at once is refused by the launcher (code 5) and recorded as such
  reduce     the default launch shape
  broadcast  the in-process Broadcast from the same root at its default shape (S read by each of the
             n - 1 readers)
  rsag_zc    the zero-copy AllReduce at its default shape (64 x 512): every rank reduces a slice

the last three alternating in the same run; plus, for the largest size, the Reduce's phase stamps on
the root and on a non-root rank.

    python tools/reduce_perf.py        (writes profiles/reduce_perf_inprocess_n8.json, or $OUT)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mscclpp_amd as m  # noqa: E402

N = int(os.environ.get("NRANKS", 8))
SIZES = [int(s) for s in os.environ.get("SIZES", f"{48 << 20},{1 << 20},{64 << 10}").split(",")]
ROUNDS = int(os.environ.get("ROUNDS", 5))
ROOT_RANK = int(os.environ.get("ROOT_RANK", 3)) % N
SWEEP_BLOCKS = (8, 16, 32, 64, 128)
SWEEP_THREADS = (512, 256)
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def graph_us(fn, calls, replays):
    """us per call of fn, from `replays` replays of a graph of `calls` calls (events around them)."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()  # eager once on this stream: first-launch set-up stays out of the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (calls * replays)


def med(v):
    return round(float(np.median(v)), 2)


rows = []
for S in SIZES:
    count = S // 2
    sends = [torch.rand(count, dtype=torch.float32, device=dev).to(torch.float16) for _ in range(N)]
    recv = torch.zeros(count, dtype=torch.float16, device=dev)
    outs = [recv if r == ROOT_RANK else None for r in range(N)]
    bcast = [torch.empty(count, dtype=torch.float16, device=dev) for _ in range(N)]
    summed = [torch.empty(count, dtype=torch.float16, device=dev) for _ in range(N)]
    ranks = m.InProcessRanks(N, 1 << 16)

    def reduce(nblocks=0, nthreads=0):
        ranks.reduce(sends, outs, ROOT_RANK, nblocks=nblocks, nthreads=nthreads, budget_ticks=300_000_000,
                     stream=torch.cuda.current_stream())

    def broadcast():
        ranks.broadcast(sends, bcast, ROOT_RANK, budget_ticks=300_000_000, stream=torch.cuda.current_stream())

    def rsag_zc():
        ranks.all_reduce(sends, summed, m.ALGO_RSAG_ZC, budget_ticks=300_000_000, stream=torch.cuda.current_stream())

    reduce()
    torch.cuda.synchronize()
    want = sends[ROOT_RANK].clone()
    for k in range(1, N):  # fp16 adds in ring order from the root (values in [0, 1): nothing saturates)
        want = want + sends[(ROOT_RANK + k) % N]
    ok = ranks.errors() == [0] * N and bool(torch.equal(recv, want))
    calls, replays = (10, 5) if S >= (8 << 20) else (50, 10)
    sweep = []
    for nthreads in SWEEP_THREADS:
        for nblocks in SWEEP_BLOCKS:
            try:
                reduce(nblocks, nthreads)
            except m.MscclppError as e:
                sweep.append({"nblocks": nblocks, "nthreads": nthreads, "refused": e.code})
                continue
            torch.cuda.synchronize()
            t = [graph_us(lambda: reduce(nblocks, nthreads), calls, replays) for _ in range(ROUNDS)]
            sweep.append({"nblocks": nblocks, "nthreads": nthreads, "us": med(t), "us_min_max": [round(min(t), 2), round(max(t), 2)]})
    t = {"reduce": [], "broadcast": [], "rsag_zc": []}
    for _ in range(ROUNDS):
        for name, fn in (("reduce", reduce), ("broadcast", broadcast), ("rsag_zc", rsag_zc)):
            t[name].append(graph_us(fn, calls, replays))
    us = {k: med(v) for k, v in t.items()}
    row = {"bytes_per_rank": S, "dtype": "float16", "root": ROOT_RANK, "correct": bool(ok), "errors": ranks.errors(),
           "graph_calls": calls, "replays": replays, "rounds": ROUNDS, "sweep": sweep,
           "reduce_us": us["reduce"], "broadcast_us": us["broadcast"], "rsag_zc_us": us["rsag_zc"],
           "reduce_us_min_max": [round(min(t["reduce"]), 2), round(max(t["reduce"]), 2)],
           "broadcast_us_min_max": [round(min(t["broadcast"]), 2), round(max(t["broadcast"]), 2)],
           "rsag_zc_us_min_max": [round(min(t["rsag_zc"]), 2), round(max(t["rsag_zc"]), 2)],
           # bytes the kernels must move through HBM: Reduce n S read + S written; Broadcast (n - 1) (S read
           # + S written); rsag_zc n S read + n S written
           "reduce_hbm_TBs": round((N + 1) * S / us["reduce"] / 1e6, 3),
           "broadcast_hbm_TBs": round(2 * (N - 1) * S / us["broadcast"] / 1e6, 3),
           "rsag_zc_hbm_TBs": round(2 * N * S / us["rsag_zc"] / 1e6, 3)}
    if S == max(SIZES):
        with m.PhaseTrace() as tr:
            reduce()
            torch.cuda.synchronize()
        row["phases_root"] = tr.phases("reduce", view=ROOT_RANK)
        row["phases_non_root"] = tr.phases("reduce", view=(ROOT_RANK + 1) % N)
    rows.append(row)
    print(row, flush=True)
    del sends, recv, outs, bcast, summed, ranks

res = {"tool": "tools/reduce_perf.py", "fabric_free": True, "gpus": 1, "nranks": N,
       "note": "in-process ranks on one GPU: no xGMI byte is priced; graph-captured, median of rounds", "rows": rows}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out = os.environ.get("OUT", os.path.join(ROOT, "profiles", f"reduce_perf_inprocess_n{N}.json"))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
