"""Fabric-free timing of the fused AllReduce + residual add + RMSNorm for DECODE sizes with a quantised y
(kernels/allreduce_rmsnorm_quant_ll.hip): 8 ranks in ONE launch on one GPU (blockIdx.y = rank, every
peer buffer local HBM), so no link is priced.  Per shape, bf16, out of place with a replicated residual, in the same
run and alternating, each captured in a HIP graph of 10 calls, median of ROUNDS rounds with min / max:

  fp8_row, mxfp8, mxfp4   InProcessRanks.all_reduce_rms_norm_quant at its default grid
  ll                      (a) InProcessRanks.all_reduce_rms_norm at its default grid: the bf16 y alone
  ll_torch_fp8_row        (b) that, and behind it in the same graph the per-row FP8 quantisation a caller launches
                          today, in torch, over the 8 ranks' y at once (one tensor)
  ll_torch_mxfp8          (b) that with a torch MXFP8 block quantisation (torch has no fp4 cast: MXFP4 has no (b))

    python tools/allreduce_rmsnorm_quant_perf.py   (writes profiles/allreduce_rmsnorm_quant_inprocess_n8.json, or $OUT)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mscclpp_amd as m  # noqa: E402

N = int(os.environ.get("NRANKS", 8))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SHAPES", "1x8192,8x8192,64x8192").split(",")]
ROUNDS = int(os.environ.get("ROUNDS", 5))
CALLS, REPLAYS = 10, int(os.environ.get("REPLAYS", 200))
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


def torch_fp8_row(y, q, scale):
    """§17k's steps 5-7 as a caller writes them in torch: y [R, cols] -> q (float8_e4m3fn), scale [R]."""
    torch.clamp(y.abs().amax(dim=1).float() / 448.0, min=2.0 ** -126, out=scale)
    q.copy_((y.float() / scale[:, None]).clamp(-448.0, 448.0))


def torch_mxfp8(y, q, e):
    """§17l's steps 5-7 for MXFP8 in torch: y [R, cols] -> q (float8_e4m3fn), e [R, cols / 32] uint8."""
    b = y.float().view(y.shape[0], -1, 32)
    exp = ((b.abs().amax(dim=2).view(torch.int32) >> 23) - 8).clamp(min=0)
    e.copy_(exp)
    q.copy_((b * ((254 - exp) << 23).view(torch.float32)[:, :, None]).clamp(-448.0, 448.0).view(y.shape))


ranks = m.InProcessRanks(N, max(m.all_reduce_rms_norm_scratch_required(N, r, c, m.BF16) for r, c in SHAPES))
rows_out = []
for rows, cols in SHAPES:
    mk = lambda: [torch.empty(rows, cols, dtype=torch.bfloat16, device=dev).uniform_(-1, 1) for _ in range(N)]
    u8 = lambda c: [torch.empty(rows, c, dtype=torch.uint8, device=dev) for _ in range(N)]
    xs, res = mk(), mk()
    for t in res[1:]:
        t.copy_(res[0])  # the residual is replicated
    gam = [torch.empty(cols, dtype=torch.bfloat16, device=dev).uniform_(0.5, 2)] * N
    yall = torch.empty(N, rows, cols, dtype=torch.bfloat16, device=dev)  # the ranks' y, one tensor for the torch steps
    ys, ros, qros = list(yall), mk(), mk()
    qr, q8, q4, e8, e4 = u8(cols), u8(cols), u8(cols // 2), u8(cols // 32), u8(cols // 32)
    scs = [torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(N)]
    tq = torch.empty(N * rows, cols, dtype=torch.float8_e4m3fn, device=dev)
    tsc = torch.empty(N * rows, dtype=torch.float32, device=dev)
    te = torch.empty(N * rows, cols // 32, dtype=torch.uint8, device=dev)
    kw = dict(eps=EPS, budget_ticks=300_000_000)
    fused = lambda fmt, q, sc: lambda: ranks.all_reduce_rms_norm_quant(xs, q, sc, gam, fmt, res, qros,
                                                                        stream=torch.cuda.current_stream(), **kw)

    def ll():
        ranks.all_reduce_rms_norm(xs, ys, gam, res, ros, stream=torch.cuda.current_stream(), **kw)

    def ll_torch_fp8_row():
        ll()
        torch_fp8_row(yall.view(N * rows, cols), tq, tsc)

    def ll_torch_mxfp8():
        ll()
        torch_mxfp8(yall.view(N * rows, cols), tq, te)

    cands = {"fp8_row": fused("fp8_row", qr, scs), "mxfp8": fused("mxfp8", q8, e8), "mxfp4": fused("mxfp4", q4, e4),
             "ll": ll, "ll_torch_fp8_row": ll_torch_fp8_row, "ll_torch_mxfp8": ll_torch_mxfp8}
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    same = lambda ts: all(torch.equal(ts[0], t) for t in ts[1:])
    # (sanity figures, not checks: the bit-exact judges are the tests)
    row = {"rows": rows, "cols": cols, "bytes": rows * cols * 2, "res_out_equal_to_ll": torch.equal(qros[0], ros[0]),
           "q_and_scale_equal_on_all_ranks": all(same(ts) for ts in (qr, q8, q4, e8, e4, scs)),
           "mxfp8_equal_to_the_torch_steps": torch.equal(q8[0], tq[:rows].view(torch.uint8)) and torch.equal(e8[0], te[:rows])}
    t = {k: [] for k in cands}
    for _ in range(ROUNDS):
        for name, fn in cands.items():
            t[name].append(graph_us(fn, CALLS, REPLAYS))
    row.update(errors=ranks.errors(), graph_calls=CALLS, replays=REPLAYS, rounds=ROUNDS)
    for k, v in t.items():
        row[k + "_us"] = round(float(np.median(v)), 2)
        row[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    rows_out.append(row)
    print(row, flush=True)

out = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                         f"allreduce_rmsnorm_quant_inprocess_n{N}.json"))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
head = {"tool": "tools/allreduce_rmsnorm_quant_perf.py", "fabric_free": True, "gpus": 1, "nranks": N, "dtype": "bf16",
        "note": "in-process ranks on one GPU: no xGMI byte is priced; graph-captured, alternating, median of rounds",
        "not_measured": ["anything across GPUs or over xGMI", "fp16 timings", "grids other than the default",
                         "a call without a residual", "a torch MXFP4 quantisation behind the LL kernel (no fp4 cast)",
                         "a downstream scaled GEMM reading q and scale"]}
with open(out, "w") as f:  # one shape per line
    f.write(json.dumps(head)[:-1] + ', "rows": [\n ' + ",\n ".join(json.dumps(r) for r in rows_out) + "\n]}\n")
