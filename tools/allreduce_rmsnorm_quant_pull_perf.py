"""Fabric-free timing of the fused AllReduce + residual add + RMSNorm with an FP8 per-row quantised y
(kernels/allreduce_rmsnorm_quant_pull.hip): 8 ranks in ONE launch on one GPU (blockIdx.y = rank,
every peer buffer local HBM), so no link is priced -- and the halved gather of y, the part of the kernel a fabric
would price most, is the part this measurement prices least.  Per shape, bf16, out of place with a residual, in the
same run and alternating, each captured in a HIP graph of K calls (K = 10, or 4 from 32 MiB), median of ROUNDS
rounds with min / max:

  quant            InProcessRanks.all_reduce_rms_norm_quant_pull at its default grid
  pull             InProcessRanks.all_reduce_rms_norm_pull at its default grid: the bf16 y alone
  pull_then_torch  that, then torch's per-row quantisation of ONE rank's y (amax, scale, divide, clamp, convert)
                   -- what one GPU of a node runs behind the unquantised kernel

plus one traced quant call's phase stamps of rank 0 at 8 MiB, and how far quant's q and scale are from torch's.

    python tools/allreduce_rmsnorm_quant_pull_perf.py   (writes profiles/allreduce_rmsnorm_quant_pull_inprocess_n8.json, or $OUT)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mscclpp_amd as m  # noqa: E402

N = int(os.environ.get("NRANKS", 8))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SHAPES", "256x8192,512x8192,2048x8192").split(",")]
ROUNDS = int(os.environ.get("ROUNDS", 5))
TRACE_AT = 8 << 20
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


def torch_quant(y):
    amax = y.abs().amax(dim=1).float()
    scale = (amax / 448.0).clamp_min(2.0 ** -126)
    return (y.float() / scale[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn), scale


ranks = m.InProcessRanks(N, 1 << 16)
rows_out = []
for rows, cols in SHAPES:
    nbytes = rows * cols * 2
    mk = lambda: [torch.empty(rows, cols, dtype=torch.bfloat16, device=dev).uniform_(-1, 1) for _ in range(N)]
    xs, res = mk(), mk()
    for t in res[1:]:
        t.copy_(res[0])  # the residual is replicated: a row's owner adds its own copy
    gam = [torch.empty(cols, dtype=torch.bfloat16, device=dev).uniform_(0.5, 2)] * N
    ys, ros, qros = mk(), mk(), mk()
    qs = [torch.empty(rows, cols, dtype=torch.float8_e4m3fn, device=dev) for _ in range(N)]
    scs = [torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(N)]

    def quant():
        ranks.all_reduce_rms_norm_quant_pull(xs, qs, scs, gam, res, qros, eps=EPS, budget_ticks=300_000_000,
                                             stream=torch.cuda.current_stream())

    def pull():
        ranks.all_reduce_rms_norm_pull(xs, ys, gam, res, ros, eps=EPS, budget_ticks=300_000_000,
                                       stream=torch.cuda.current_stream())

    def pull_then_torch():
        pull()
        return torch_quant(ys[0])

    quant()
    tq, ts = pull_then_torch()
    torch.cuda.synchronize()
    cands = {"quant": quant, "pull": pull, "pull_then_torch": pull_then_torch}
    # (sanity figures, not checks: torch divides by the scale where the kernel multiplies by its reciprocal, and its
    # scale need not be the correctly rounded quotient)
    row = {"rows": rows, "cols": cols, "bytes": nbytes,
           "q_bytes_differing_from_torch": int((qs[0].view(torch.uint8) != tq.view(torch.uint8)).sum()),
           "scale_equal_to_torch": torch.equal(scs[0], ts), "res_out_equal_to_pull": torch.equal(qros[0], ros[0]),
           "q_and_scale_equal_on_all_ranks": all(torch.equal(qs[0].view(torch.uint8), t.view(torch.uint8)) for t in qs[1:])
           and all(torch.equal(scs[0], t) for t in scs[1:])}
    calls, replays = (4, 5) if nbytes >= (32 << 20) else (10, 5)
    t = {k: [] for k in cands}
    for _ in range(ROUNDS):
        for name, fn in cands.items():
            t[name].append(graph_us(fn, calls, replays))
    row.update(errors=ranks.errors(), graph_calls=calls, replays=replays, rounds=ROUNDS)
    for k, v in t.items():
        row[k + "_us"] = round(float(np.median(v)), 2)
        row[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    if nbytes == TRACE_AT:
        with m.PhaseTrace() as tr:
            quant()
            torch.cuda.synchronize()
        row["phases_rank0"] = tr.phases("allreduce_rms_norm_quant_pull", view=0)
    rows_out.append(row)
    print(row, flush=True)

out = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                         f"allreduce_rmsnorm_quant_pull_inprocess_n{N}.json"))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
head = {"tool": "tools/allreduce_rmsnorm_quant_pull_perf.py", "fabric_free": True, "gpus": 1, "nranks": N, "dtype": "bf16",
        "note": "in-process ranks on one GPU: no xGMI byte is priced; graph-captured, median of rounds; pull_then_torch "
                "quantises one rank's y"}
with open(out, "w") as f:  # one shape per line
    f.write(json.dumps(head)[:-1] + ', "rows": [\n ' + ",\n ".join(json.dumps(r) for r in rows_out) + "\n]}\n")
