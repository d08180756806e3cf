"""Fabric-free timing of the fused AllReduce + residual add + RMSNorm for prefill sizes
(kernels/allreduce_rmsnorm_pull.hip): 8 ranks in ONE launch on one GPU (blockIdx.y = rank, every
peer buffer local HBM), so no link is priced.  Per shape, bf16, out of place with a residual, in the same run and
alternating, each captured in a HIP graph of K calls (K = 10, or 4 from 32 MiB), median of ROUNDS rounds with
min / max:

  pull       InProcessRanks.all_reduce_rms_norm_pull at its default grid
  pull_nbG   the same on G workgroups per rank (G in GRIDS): what the default grid is read off
  ll         InProcessRanks.all_reduce_rms_norm, the one-hop LL kernel, where it is carried (<= 1 MiB)
  unfused    the library's default SUM all_reduce of that size (the selector's algorithm, at its default shape
             or, where eight in-process ranks of that shape are not co-resident on one GPU, on 32 workgroups
             of 512 lanes: the row's unfused_shape), then torch's residual add and rms_norm on ONE rank's
             result -- what one GPU of a node runs behind its collective

plus one traced pull call's phase stamps of rank 0 at 8 MiB.

    python tools/allreduce_rmsnorm_pull_perf.py   (writes profiles/allreduce_rmsnorm_pull_inprocess_n8.json, or $OUT)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mscclpp_amd as m  # noqa: E402

N = int(os.environ.get("NRANKS", 8))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in
          os.environ.get("SHAPES", "64x8192,512x4096,512x8192,2048x8192").split(",")]
GRIDS = [int(g) for g in os.environ.get("GRIDS", "16,32,64").split(",") if g]
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


top = max(r * c * 2 for r, c in SHAPES)
ll_need = max([m.all_reduce_rms_norm_scratch_required(N, r, c, m.BF16) for r, c in SHAPES] +
              [m.scratch_required(m.ALGO_PACKET, N, r * c * 2, m.BF16) for r, c in SHAPES if r * c * 2 <= (1 << 20)])
ranks = m.InProcessRanks(N, ll_need, bulk_scratch_bytes=top + (1 << 20))
rows_out = []
for rows, cols in SHAPES:
    nbytes = rows * cols * 2
    mk = lambda: [torch.empty(rows, cols, dtype=torch.bfloat16, device=dev).uniform_(-1, 1) for _ in range(N)]
    xs, res = mk(), mk()
    for t in res[1:]:
        t.copy_(res[0])  # the residual is replicated: a row's owner adds its own copy
    gam = [torch.empty(cols, dtype=torch.bfloat16, device=dev).uniform_(0.5, 2)] * N
    ys, ros, lys, lros, sums = mk(), mk(), mk(), mk(), mk()
    flat = lambda ts: [t.view(-1) for t in ts]
    algo = m.lib().mscclppAmdSelectAlgo(N, nbytes, m.BF16)
    shape = {}

    def pull(**grid):
        ranks.all_reduce_rms_norm_pull(xs, ys, gam, res, ros, eps=EPS, budget_ticks=300_000_000,
                                       stream=torch.cuda.current_stream(), **grid)

    def ll():
        ranks.all_reduce_rms_norm(xs, lys, gam, res, lros, eps=EPS, budget_ticks=300_000_000,
                                  stream=torch.cuda.current_stream())

    def unfused():
        ranks.all_reduce(flat(xs), flat(sums), algo, budget_ticks=300_000_000, stream=torch.cuda.current_stream(), **shape)
        z = torch.add(sums[0], res[0])
        return z, torch.nn.functional.rms_norm(z, (cols,), gam[0], EPS)

    pull()
    try:
        unfused()
    except m.MscclppError as e:  # the default shape of eight in-process ranks is not co-resident on one GPU
        if e.code != 5:
            raise
        shape = dict(nblocks=32, nthreads=512)
    z, y = unfused()
    torch.cuda.synchronize()
    cands = {"pull": pull, "unfused": unfused}
    cands.update({f"pull_nb{g}": (lambda g=g: pull(nblocks=g)) for g in GRIDS if g <= (rows + N - 1) // N})
    if nbytes <= (1 << 20):
        ll()
        torch.cuda.synchronize()
        cands["ll"] = ll
    # (sanity figures, not checks: the library's SUM accumulates in bf16 and rounds before the residual is added)
    row = {"rows": rows, "cols": cols, "bytes": nbytes, "unfused_algo": algo, "unfused_shape": shape,
           "max_abs_diff_to_torch": round(float((ys[0].float() - y.float()).abs().max()), 4),
           "y_equal_on_all_ranks": all(torch.equal(ys[0], t) for t in ys[1:]),
           "res_out_equal_to_ll": torch.equal(ros[0], lros[0]) if "ll" in cands else None}
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
            pull()
            torch.cuda.synchronize()
        row["phases_rank0"] = tr.phases("allreduce_rms_norm_pull", view=0)
    rows_out.append(row)
    print(row, flush=True)

out = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                         f"allreduce_rmsnorm_pull_inprocess_n{N}.json"))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
head = {"tool": "tools/allreduce_rmsnorm_pull_perf.py", "fabric_free": True, "gpus": 1, "nranks": N, "dtype": "bf16",
        "note": "in-process ranks on one GPU: no xGMI byte is priced; graph-captured, median of rounds; unfused "
                "normalises one rank's result"}
with open(out, "w") as f:  # one shape per line
    f.write(json.dumps(head)[:-1] + ', "rows": [\n ' + ",\n ".join(json.dumps(r) for r in rows_out) + "\n]}\n")
