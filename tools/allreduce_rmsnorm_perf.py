"""Fabric-free timing of the fused AllReduce + residual add + RMSNorm (kernels/allreduce_rmsnorm_ll.hip;
DESIGN.md §17i): 8 ranks in ONE launch on one GPU (blockIdx.y = rank, every peer scratch local HBM), so no
link is priced.  Per shape, bf16, in the same run and alternating, each captured in a HIP graph of K calls
(K = 50, or 10 from 512 KiB), median of ROUNDS rounds with min / max:

  fused      InProcessRanks.all_reduce_rms_norm, out of place, with a residual
  ll8        this library's LL8 AllReduce (allpair, SUM) of the same bytes alone, at its default shape -- from
             256 KiB, where eight in-process ranks of that shape are not co-resident on one GPU, 32
             workgroups of 512 lanes per rank (the row's ll8_nblocks)
  ll8_torch  ll8 followed by torch's residual add and torch.nn.functional.rms_norm on ONE rank's result --
             what one GPU of a node would run behind its collective (the eight in-process ranks share this
             GPU, so normalising all eight results would price eight GPUs' work on one)

plus the fused kernel's phase stamps of rank 0 at the largest shape (put, reduce, normalise; of each
workgroup's last row).

    python tools/allreduce_rmsnorm_perf.py   (writes profiles/allreduce_rmsnorm_inprocess_n8.json, or $OUT)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mscclpp_amd as m  # noqa: E402

N = int(os.environ.get("NRANKS", 8))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SHAPES", "1x4096,16x4096,16x8192,64x8192").split(",")]
ROUNDS = int(os.environ.get("ROUNDS", 5))
EPS = 1e-5
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


need = max(max(m.all_reduce_rms_norm_scratch_required(N, r, c, m.BF16) for r, c in SHAPES),
           max(m.scratch_required(m.ALGO_ALLPAIR, N, r * c * 2, m.BF16) for r, c in SHAPES))
ranks = m.InProcessRanks(N, need)
rows_out = []
for rows, cols in SHAPES:
    mk = lambda: [torch.empty(rows, cols, dtype=torch.bfloat16, device=dev).uniform_(-1, 1) for _ in range(N)]
    xs, res = mk(), mk()
    gam = [torch.empty(cols, dtype=torch.bfloat16, device=dev).uniform_(0.5, 2)] * N
    ys, ros, sums = mk(), mk(), mk()
    flat = lambda ts: [t.view(-1) for t in ts]
    ll8_shape = dict(nblocks=32, nthreads=512) if rows * cols * 2 >= (256 << 10) else {}

    def fused():
        ranks.all_reduce_rms_norm(xs, ys, gam, res, ros, eps=EPS, budget_ticks=300_000_000,
                                  stream=torch.cuda.current_stream())

    def ll8():
        ranks.all_reduce(flat(xs), flat(sums), m.ALGO_ALLPAIR, budget_ticks=300_000_000, stream=torch.cuda.current_stream(),
                         **ll8_shape)

    def ll8_torch():
        ll8()
        z = torch.add(sums[0], res[0])
        return z, torch.nn.functional.rms_norm(z, (cols,), gam[0], EPS)

    fused()
    z, y = ll8_torch()
    torch.cuda.synchronize()
    # (a sanity figure, not a check: the LL8 SUM accumulates in bf16 and rounds before the residual is added)
    diff = round(float((ys[0].float() - y.float()).abs().max()), 4)
    calls, replays = (10, 5) if rows * cols * 2 >= (512 << 10) else (50, 10)
    t = {"fused": [], "ll8": [], "ll8_torch": []}
    for _ in range(ROUNDS):
        for name, fn in (("fused", fused), ("ll8", ll8), ("ll8_torch", ll8_torch)):
            t[name].append(graph_us(fn, calls, replays))
    row = {"rows": rows, "cols": cols, "bytes": rows * cols * 2, "errors": ranks.errors(), "max_abs_diff_to_torch": diff,
           "graph_calls": calls, "replays": replays, "rounds": ROUNDS, "ll8_nblocks": ll8_shape.get("nblocks", 0)}
    for k, v in t.items():
        row[k + "_us"] = round(float(np.median(v)), 2)
        row[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    if (rows, cols) == SHAPES[-1]:
        with m.PhaseTrace() as tr:
            fused()
            torch.cuda.synchronize()
        row["phases_rank0"] = tr.phases("allreduce_rms_norm", view=0)
    rows_out.append(row)
    print(row, flush=True)

out = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                         f"allreduce_rmsnorm_inprocess_n{N}.json"))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
head = {"tool": "tools/allreduce_rmsnorm_perf.py", "fabric_free": True, "gpus": 1, "nranks": N, "dtype": "bf16",
        "note": "in-process ranks on one GPU: no xGMI byte is priced; graph-captured, median of rounds; ll8_torch "
                "normalises one rank's result"}
with open(out, "w") as f:  # one shape per line
    f.write(json.dumps(head)[:-1] + ', "rows": [\n ' + ",\n ".join(json.dumps(r) for r in rows_out) + "\n]}\n")
