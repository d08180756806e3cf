"""Fabric-free timing of the native AllToAll (kernels/alltoall.hip): 8 ranks in ONE launch on one
GPU (blockIdx.y = rank, every peer buffer local HBM), so no link is priced -- what is measured is
the kernel's own memory pipeline and its two handshakes.  Per size (total bytes per rank), in the
same run and alternating, each captured in a HIP graph of K calls:

  alltoall   the default launch shape; 2 S bytes of HBM traffic per rank (S read, S written)
  copy_jobs  mscclppAmdCopyJobsPolicy moving the same bytes with the same cache policies (system
             loads, plain stores) and as many lanes, one job per rank, no handshake: the
             streaming-copy yardstick of this run
  allgather  the in-process bulk AllGather with the same per-rank output size S

plus, for the largest size, the AllToAll's phase stamps (entry handshake, pull, exit handshake).
With nviews > 1 the AllToAll's segment table travels through a one-workgroup fill kernel in front
of each launch (the one-rank-per-process launch passes it by value), which the time includes.

    python tools/alltoall_perf.py        (writes profiles/alltoall_perf_inprocess_n8.json, or $OUT)

MODE=ll: the small-message sweep behind the LL cutover.  Per segment size 8 B ... 1 MiB
(equal split, NRANKS in-process ranks), the pull kernel and the LL kernel of kernels/alltoall_ll.hip at
their default shapes, alternating in one run, each captured in a HIP graph of K calls, median of ROUNDS
rounds; the bound is the largest swept size up to which the LL median is at or below the pull median.

    MODE=ll NRANKS=4 python tools/alltoall_perf.py   (writes profiles/alltoall_ll_perf_inprocess_n4.json)
"""
import ctypes
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
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
L = m.lib()
vp, sz = ctypes.c_void_p, ctypes.c_size_t


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


def blocks_for(S):
    want = (S + (256 << 10) - 1) // (256 << 10)
    return min(max(want, 8), 128)


def ll_sweep():
    sizes = [int(x) for x in os.environ["SIZES"].split(",")] if "SIZES" in os.environ else [8 << k for k in range(18)]
    need = m.alltoall_ll_scratch_required(N, max(sizes))
    ranks = m.InProcessRanks(N, need)
    out_rows, bound, beaten = [], 0, False
    for seg in sizes:
        S = seg * N
        sends = [torch.randint(0, 256, (S,), dtype=torch.uint8, device=dev) for _ in range(N)]
        outs = {k: [torch.full((S,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(N)] for k in ("pull", "ll")}

        def pull():
            ranks.all_to_all(sends, outs["pull"], budget_ticks=300_000_000, stream=torch.cuda.current_stream())

        def ll():
            ranks.all_to_all_ll(sends, outs["ll"], budget_ticks=300_000_000, stream=torch.cuda.current_stream())

        pull(), ll()
        torch.cuda.synchronize()
        ok = ranks.errors() == [0] * N and all(
            torch.equal(outs[k][r][p * seg:(p + 1) * seg], sends[p][r * seg:(r + 1) * seg])
            for k in outs for r in range(N) for p in range(N))
        calls, replays = (10, 5) if seg >= (256 << 10) else (50, 10)
        t = {"pull": [], "ll": []}
        for _ in range(ROUNDS):
            for name, fn in (("pull", pull), ("ll", ll)):
                t[name].append(graph_us(fn, calls, replays))
        us = {k: float(np.median(v)) for k, v in t.items()}
        wins = us["ll"] <= us["pull"]
        if wins and not beaten:
            bound = seg
        beaten = beaten or not wins
        row = {"segment_bytes": seg, "correct": bool(ok), "errors": ranks.errors(), "graph_calls": calls,
               "replays": replays, "rounds": ROUNDS, "pull_us": round(us["pull"], 2), "ll_us": round(us["ll"], 2),
               "pull_us_all": [round(x, 2) for x in t["pull"]], "ll_us_all": [round(x, 2) for x in t["ll"]],
               "ll_at_or_below_pull": bool(wins)}
        out_rows.append(row)
        print(row, flush=True)
        del sends, outs
    with m.PhaseTrace() as tr:
        x = [torch.randint(0, 256, (N * 4096,), dtype=torch.uint8, device=dev) for _ in range(N)]
        ranks.all_to_all_ll(x, [torch.empty_like(t) for t in x])
        torch.cuda.synchronize()
    res = {"tool": "tools/alltoall_perf.py MODE=ll", "fabric_free": True, "gpus": 1, "nranks": N,
           "note": "in-process ranks on one GPU: no xGMI byte is priced; graph-captured, median of rounds; the "
                   "in-process pull launch includes its one-workgroup table fill kernel, the LL launch carries its "
                   "table by value", "bound_bytes": bound, "phases_rank0_4096": tr.phases("alltoall_ll", view=0),
           "rows": out_rows}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.environ.get("OUT", os.path.join(root, "profiles", f"alltoall_ll_perf_inprocess_n{N}.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print({"nranks": N, "bound_bytes": bound}, flush=True)


if os.environ.get("MODE") == "ll":
    ll_sweep()
    sys.exit(0)

rows = []
for S in SIZES:
    blk = S // N
    assert blk % 16 == 0
    sends = [torch.randint(0, 256, (S,), dtype=torch.uint8, device=dev) for _ in range(N)]
    recvs = [torch.full((S,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(N)]
    copies = [torch.empty(S, dtype=torch.uint8, device=dev) for _ in range(N)]
    gathered = [torch.empty(S, dtype=torch.uint8, device=dev) for _ in range(N)]
    ranks = m.InProcessRanks(N, 1 << 16, bulk_scratch_bytes=S + (16 << 20))
    nb = blocks_for(S)

    def alltoall():
        ranks.all_to_all(sends, recvs, budget_ticks=300_000_000, stream=torch.cuda.current_stream())

    srcs = (vp * N)(*[t.data_ptr() for t in sends])
    dsts = (vp * N)(*[t.data_ptr() for t in copies])
    lens = (sz * N)(*[S] * N)

    def copy_jobs():  # 256-lane workgroups: twice the AllToAll's 512-lane grid
        m.check(L.mscclppAmdCopyJobsPolicy(srcs, dsts, lens, N, 2 * nb, 0, 1, m.stream_ptr(torch.cuda.current_stream())),
                "copy jobs")

    def allgather():
        ranks.collective(2, [t[:blk] for t in sends], gathered, nblocks=64, nthreads=512, budget_ticks=300_000_000,
                         stream=torch.cuda.current_stream())

    alltoall()
    torch.cuda.synchronize()
    ok = ranks.errors() == [0] * N and all(
        torch.equal(recvs[r][p * blk:(p + 1) * blk], sends[p][r * blk:(r + 1) * blk]) for r in range(N) for p in range(N))
    calls, replays = (10, 5) if S >= (8 << 20) else (50, 10)
    t = {"alltoall": [], "copy_jobs": [], "allgather": []}
    for _ in range(ROUNDS):
        for name, fn in (("alltoall", alltoall), ("copy_jobs", copy_jobs), ("allgather", allgather)):
            t[name].append(graph_us(fn, calls, replays))
    us = {k: float(np.median(v)) for k, v in t.items()}
    row = {"bytes_per_rank": S, "nblocks": nb, "nthreads": 512, "correct": bool(ok), "errors": ranks.errors(),
           "graph_calls": calls, "replays": replays, "rounds": ROUNDS,
           "alltoall_us": round(us["alltoall"], 2), "copy_jobs_us": round(us["copy_jobs"], 2),
           "allgather_us": round(us["allgather"], 2),
           "alltoall_us_min_max": [round(min(t["alltoall"]), 2), round(max(t["alltoall"]), 2)],
           "copy_jobs_us_min_max": [round(min(t["copy_jobs"]), 2), round(max(t["copy_jobs"]), 2)],
           "alltoall_hbm_TBs": round(2 * N * S / us["alltoall"] / 1e6, 3),
           "copy_jobs_hbm_TBs": round(2 * N * S / us["copy_jobs"] / 1e6, 3),
           "alltoall_over_copy_jobs": round(us["copy_jobs"] / us["alltoall"], 3),
           "alltoall_per_rank_GBs": round(S / us["alltoall"] / 1e3, 1)}
    if S == max(SIZES):
        with m.PhaseTrace() as tr:
            alltoall()
            torch.cuda.synchronize()
        row["phases_rank0"] = tr.phases("alltoall", view=0)
    rows.append(row)
    print(row, flush=True)
    del sends, recvs, copies, gathered, ranks

res = {"tool": "tools/alltoall_perf.py", "fabric_free": True, "gpus": 1, "nranks": N,
       "note": "8 in-process ranks on one GPU: no xGMI byte is priced; graph-captured, median of rounds", "rows": rows}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out = os.environ.get("OUT", os.path.join(ROOT, "profiles", f"alltoall_perf_inprocess_n{N}.json"))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
