"""Fabric-free timing of the ncclMax / ncclAvg kernel (kernels/pull_reduce.hip): 8 ranks in ONE launch
on one GPU (blockIdx.y = rank, every peer buffer local HBM), so no link is priced -- what is measured
is the memory pipeline and the handshakes (two; three for an AllReduce).  Per dtype (fp16, bf16) and
size S (bytes of a rank's send buffer; a ReduceScatter's block is S / n), each timing from a HIP
graph of K calls, median of ROUNDS with the spread:

  sweep      AVG AllReduce / ReduceScatter / Reduce at nblocks in {8, 16, 32, 64} x 512 lanes (fp16): the
             default-grid rule (pullReduceDefaultBlocks) is read off this
  lines      at the default shapes, alternating in the same run: AVG AllReduce / ReduceScatter / Reduce
             and the SUM paths at the same shapes -- rsag_zc AllReduce, the selector's ReduceScatter
             (tuned-config store; fullmesh 8 x 256 where it names none), reduceKernel
  latency    MAX AllReduce (fp32) of 4 bytes and 1 KiB beside the LL8 (allpair) SUM AllReduce

An AllReduce here moves the bytes of rsag_zc over the links, 2 (n - 1) / n * S per rank, all of them as
reads (rsag_zc: half reads, half remote stores); whether reads beat remote stores over real xGMI
links this tool cannot say.

    python tools/pull_reduce_perf.py   (writes profiles/pull_reduce_perf_inprocess_n8.json, or $OUT)

TYPES=int64 runs another, shorter programme instead: int64 SUM and AVG beside fp32 MAX
at the same byte counts, default grids, the three collectives, alternating in the same run; SIZES
defaults to 8 bytes, 1 MiB and 48 MiB (a ReduceScatter needs n elements), and the result goes to
profiles/int_reduce_perf_inprocess_n8.json.

TYPES=premul: PreMulSum beside AVG of the same type and collective, fp16 / bf16 / fp32,
SIZES 64 KiB, 1 MiB and 48 MiB by default; the result goes to profiles/premul_sum_perf_inprocess_n8.json.

TYPES=ll: the small-message LL path (kernels/pull_reduce_ll.hip) beside the pull launcher
at its default grid and the LL8 SUM AllReduce, alternating in the same run: AllReduce and ReduceScatter
of fp32 MAX, fp16 AVG and int64 SUM, 4 bytes .. 1 MiB in powers of two (the message, or a ReduceScatter's
per-rank block), NRANKS ranks.  The result, with the cutover read off it, goes to
profiles/pull_reduce_ll_perf_inprocess_n{NRANKS}.json.
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
SWEEP_BLOCKS = (8, 16, 32, 64)
COLLS = (("allreduce", m.PULL_ALLREDUCE), ("reducescatter", m.PULL_REDUCE_SCATTER), ("reduce", m.PULL_REDUCE))
BUDGET = 300_000_000
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


def stat(v):
    return {"us": round(float(np.median(v)), 2), "us_min_max": [round(min(v), 2), round(max(v), 2)]}


def cur():
    return torch.cuda.current_stream()


def int64_programme():
    sizes = [int(s) for s in os.environ.get("SIZES", f"8,{1 << 20},{48 << 20}").split(",")]
    rows = []
    for S in sizes:
        ranks = m.InProcessRanks(N, 1 << 16)
        bufs = {}
        for name, tdt, es in (("i64", torch.int64, 8), ("f32", torch.float32, 4)):
            count = S // es
            if tdt == torch.int64:  # all 64 bits: sums wrap, averages need the 67-bit sum
                sends = [(torch.randint(-2 ** 31, 2 ** 31, (count,), dtype=tdt, device=dev) << 32) |
                         torch.randint(0, 2 ** 32, (count,), dtype=tdt, device=dev) for _ in range(N)]
            else:
                sends = [torch.rand(count, dtype=tdt, device=dev) for _ in range(N)]
            full = [torch.zeros(count, dtype=tdt, device=dev) for _ in range(N)]
            blk = count // N
            part = [torch.zeros(max(blk, 1), dtype=tdt, device=dev) for _ in range(N)]
            bufs[name] = (sends, {m.PULL_ALLREDUCE: (sends, full), m.PULL_REDUCE_SCATTER: ([t[:blk * N] for t in sends], part),
                                  m.PULL_REDUCE: (sends, [full[r] if r == ROOT_RANK else None for r in range(N)])})
        colls = [(name, c) for name, c in COLLS if c != m.PULL_REDUCE_SCATTER or S // 8 >= N]

        def call(name, coll, op):
            ins, outs = bufs[name][1][coll]
            ranks.pull_reduce(coll, ins, outs, op, root=ROOT_RANK, budget_ticks=BUDGET, stream=cur())

        # correctness of what is timed: the wrapping sum everywhere, the exact average on a sample
        x = bufs["i64"][0]
        full = bufs["i64"][1][m.PULL_ALLREDUCE][1]
        call("i64", m.PULL_ALLREDUCE, m.SUM)
        torch.cuda.synchronize()
        ok = all(torch.equal(t, torch.stack(x).sum(dim=0)) for t in full)
        call("i64", m.PULL_ALLREDUCE, m.AVG)
        torch.cuda.synchronize()
        for i in range(0, S // 8, max(1, S // 8 // 61)):
            s = sum(int(t[i].item()) for t in x)
            ok = ok and int(full[0][i].item()) == abs(s) // N * (1 if s >= 0 else -1)
        ok = ok and ranks.errors() == [0] * N
        calls, replays = (10, 5) if S >= (8 << 20) else (50, 10)
        lines = [(f"{cname}_{label}", (lambda b=b, c=c, op=op: call(b, c, op)))
                 for cname, c in colls for label, b, op in (("i64_sum", "i64", m.SUM), ("i64_avg", "i64", m.AVG),
                                                            ("f32_max", "f32", m.MAX))]
        t = {name: [] for name, _ in lines}
        for _ in range(ROUNDS):
            for name, fn in lines:
                t[name].append(graph_us(fn, calls, replays))
        row = {"send_bytes_per_rank": S, "root": ROOT_RANK, "correct": bool(ok), "graph_calls": calls, "replays": replays,
               "rounds": ROUNDS,
               "default_nblocks": {name: m.lib().mscclppAmdPullReduceDefaultBlocks(c, S // N if c == m.PULL_REDUCE_SCATTER else S)
                                   for name, c in colls},
               "lines": {name: stat(v) for name, v in t.items()}, "errors": ranks.errors()}
        rows.append(row)
        print(row, flush=True)
        del bufs, ranks
    res = {"tool": "tools/pull_reduce_perf.py TYPES=int64", "fabric_free": True, "gpus": 1, "nranks": N,
           "note": "in-process ranks on one GPU: no xGMI byte is priced; graph-captured, median of rounds", "rows": rows}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.environ.get("OUT", os.path.join(root, "profiles", f"int_reduce_perf_inprocess_n{N}.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)


def premul_programme():
    """PreMulSum beside AVG of the same type and collective, alternating in the same
    run, default grids: AVG is the yardstick (the same loads, stores and handshakes; PreMulSum adds a
    multiply per operand and the scalar exchange: one 8-byte store and one 8-byte load of n slots per
    wave).  Per-rank scalars as immediates, and once more read through device pointers."""
    sizes = [int(s) for s in os.environ.get("SIZES", f"{64 << 10},{1 << 20},{48 << 20}").split(",")]
    scal = [1.0, -0.5, 0.25, 0.75, -0.125, 0.5, 0.375, -0.25][:N]  # exact in fp16 / bf16 / fp32
    rows = []
    for tdt in (torch.float16, torch.bfloat16, torch.float32):
        es = torch.empty(0, dtype=tdt).element_size()
        for S in sizes:
            count, blk = S // es, S // es // N
            ranks = m.InProcessRanks(N, 1 << 16)
            sends = [torch.rand(count, dtype=torch.float32, device=dev).to(tdt) for _ in range(N)]
            full = [torch.zeros(count, dtype=tdt, device=dev) for _ in range(N)]
            part = [torch.zeros(blk, dtype=tdt, device=dev) for _ in range(N)]
            outs = {m.PULL_ALLREDUCE: full, m.PULL_REDUCE_SCATTER: part,
                    m.PULL_REDUCE: [full[r] if r == ROOT_RANK else None for r in range(N)]}
            ins = {c: ([t[:blk * N] for t in sends] if c == m.PULL_REDUCE_SCATTER else sends) for _, c in COLLS}
            ptrs = [torch.tensor([s], dtype=tdt, device=dev) for s in scal]

            def avg(coll):
                ranks.pull_reduce(coll, ins[coll], outs[coll], m.AVG, root=ROOT_RANK, budget_ticks=BUDGET, stream=cur())

            def premul(coll, device=False):
                ranks.pull_reduce(coll, ins[coll], outs[coll], m.PREMUL_SUM, root=ROOT_RANK, budget_ticks=BUDGET,
                                  stream=cur(), scales=scal, scale_tensors=ptrs if device else None)

            # correctness of what is timed: fp32 products and sum in rank order, rounded once
            want = sends[0].float() * scal[0]
            for k in range(1, N):
                want = want + sends[k].float() * scal[k]
            want = want.to(tdt)
            for _, c in COLLS:
                premul(c, device=(c == m.PULL_REDUCE))
            torch.cuda.synchronize()
            ok = all(torch.equal(t, want) for t in full)
            ok = ok and all(torch.equal(part[r], want[r * blk:(r + 1) * blk]) for r in range(N))
            ok = ok and ranks.errors() == [0] * N
            calls, replays = (10, 5) if S >= (8 << 20) else (50, 10)
            lines = []
            for name, c in COLLS:
                lines += [("avg_" + name, (lambda c=c: avg(c))), ("premul_" + name, (lambda c=c: premul(c)))]
            lines.append(("premul_allreduce_device_scalars", lambda: premul(m.PULL_ALLREDUCE, device=True)))
            t = {name: [] for name, _ in lines}
            for _ in range(ROUNDS):
                for name, fn in lines:
                    t[name].append(graph_us(fn, calls, replays))
            row = {"dtype": str(tdt).replace("torch.", ""), "send_bytes_per_rank": S, "root": ROOT_RANK, "correct": bool(ok),
                   "graph_calls": calls, "replays": replays, "rounds": ROUNDS,
                   "default_nblocks": {name: m.lib().mscclppAmdPullReduceDefaultBlocks(c, blk * es if c == m.PULL_REDUCE_SCATTER else S)
                                       for name, c in COLLS},
                   "lines": {name: stat(v) for name, v in t.items()}}
            row["premul_over_avg"] = {name: round(row["lines"]["premul_" + name]["us"] / row["lines"]["avg_" + name]["us"], 3)
                                      for name, _ in COLLS}
            phases = {}
            for label, fn in (("avg", lambda: avg(m.PULL_ALLREDUCE)), ("premul", lambda: premul(m.PULL_ALLREDUCE))):
                with m.PhaseTrace() as tr:
                    fn()
                    torch.cuda.synchronize()
                phases[label] = tr.phases("pull_allreduce", view=ROOT_RANK)
            row["phases_allreduce"] = phases
            row["errors"] = ranks.errors()
            rows.append(row)
            print(row, flush=True)
            del sends, full, part, outs, ins, ranks
    res = {"tool": "tools/pull_reduce_perf.py TYPES=premul", "fabric_free": True, "gpus": 1, "nranks": N, "scalars": scal,
           "note": "in-process ranks on one GPU: no xGMI byte is priced, so neither is the scalar exchange over a link; "
                   "graph-captured, median of rounds; AVG of the same type and collective from the same run is the yardstick",
           "rows": rows}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.environ.get("OUT", os.path.join(root, "profiles", f"premul_sum_perf_inprocess_n{N}.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)


def ll_programme():
    """LL path against the pull launcher (default grids) and the LL8 SUM AllReduce.  S: the message of an
    AllReduce, the per-rank block of a ReduceScatter -- what the cutover rule is a function of."""
    sizes = [int(s) for s in os.environ.get("SIZES", ",".join(str(1 << k) for k in range(2, 21))).split(",")]
    kinds = (("f32_max", torch.float32, 4, m.MAX), ("f16_avg", torch.float16, 2, m.AVG), ("i64_sum", torch.int64, 8, m.SUM))
    colls = (("allreduce", m.PULL_ALLREDUCE), ("reducescatter", m.PULL_REDUCE_SCATTER))
    need = max(m.pull_reduce_ll_scratch_required(c, N, max(sizes), m.F32, m.MAX) for _, c in colls)
    need = max(need, m.scratch_required(m.ALGO_ALLPAIR, N, max(sizes), m.F32), 1 << 16)
    ranks = m.InProcessRanks(N, need)
    rows = []
    for S in sizes:
        for cname, coll in colls:
            mult = N if coll == m.PULL_REDUCE_SCATTER else 1
            bufs = {}
            for name, tdt, es, op in kinds:
                if S % es:
                    continue
                count = S // es
                if tdt == torch.int64:
                    x = [torch.randint(-2 ** 40, 2 ** 40, (count * mult,), dtype=tdt, device=dev) for _ in range(N)]
                else:
                    x = [torch.rand(count * mult, dtype=torch.float32, device=dev).to(tdt) for _ in range(N)]
                bufs[name] = (x, [torch.zeros(count, dtype=tdt, device=dev) for _ in range(N)],
                              [torch.zeros(count, dtype=tdt, device=dev) for _ in range(N)], op)

            def ll(name):
                x, y, _, op = bufs[name]
                ranks.pull_reduce_ll(coll, x, y, op, budget_ticks=BUDGET, stream=cur())

            def pull(name):
                x, _, z, op = bufs[name]
                ranks.pull_reduce(coll, x, z, op, budget_ticks=BUDGET, stream=cur())

            def ll8_sum():
                x, y, _, _ = bufs["f32_max"]
                ranks.all_reduce(x, y, m.ALGO_ALLPAIR, budget_ticks=BUDGET, stream=cur())

            ll8_runs = coll == m.PULL_ALLREDUCE
            if ll8_runs:  # (its default grid of 512-lane workgroups is not resident for 4 and 8 ranks on one GPU from 512 KiB)
                try:
                    ll8_sum()
                except m.MscclppError as e:
                    assert e.code == 5
                    ll8_runs = False

            ok = True
            for name in bufs:  # what is timed gives the same bytes on both paths
                ll(name)
                pull(name)
                torch.cuda.synchronize()
                ok = ok and all(torch.equal(a, b) for a, b in zip(bufs[name][1], bufs[name][2]))
            ok = ok and ranks.errors() == [0] * N
            lines = []
            for name in bufs:
                lines += [("ll_" + name, (lambda k=name: ll(k))), ("pull_" + name, (lambda k=name: pull(k)))]
            if ll8_runs:
                lines.append(("sum_allreduce_ll8_f32", ll8_sum))
            calls, replays = (20, 5) if S >= (256 << 10) else (50, 10)
            t = {name: [] for name, _ in lines}
            for _ in range(ROUNDS):
                for name, fn in lines:
                    t[name].append(graph_us(fn, calls, replays))
            row = {"coll": cname, "bytes": S, "correct": bool(ok), "graph_calls": calls, "replays": replays, "rounds": ROUNDS,
                   "lines": {name: stat(v) for name, v in t.items()}}
            row["ll_beats_pull"] = {name: row["lines"]["ll_" + name]["us"] < row["lines"]["pull_" + name]["us"] for name in bufs}
            if coll == m.PULL_ALLREDUCE and S <= 1024:
                base = row["lines"]["sum_allreduce_ll8_f32"]
                row["ll_f32_max_over_ll8_sum"] = round(row["lines"]["ll_f32_max"]["us"] / base["us"], 3)
                row["ll8_sum_spread_us"] = round(base["us_min_max"][1] - base["us_min_max"][0], 2)
                if S == 1024:
                    phases = {}
                    for label, fn, fam in (("ll_f32_max", lambda: ll("f32_max"), "pull_reduce_ll"), ("ll8_sum", ll8_sum, "allpair")):
                        with m.PhaseTrace() as tr:
                            fn()
                            torch.cuda.synchronize()
                        phases[label] = tr.phases(fam, view=0)
                    row["phases"] = phases
            row["errors"] = ranks.errors()
            rows.append(row)
            print(row, flush=True)
            del bufs
    # the rule: per collective the largest swept size such that at it and at every smaller swept size the LL
    # median beats the pull median for all three (dtype, op)
    cutover = {}
    for cname, _ in colls:
        best = 0
        for row in sorted((r for r in rows if r["coll"] == cname), key=lambda r: r["bytes"]):
            if not all(row["ll_beats_pull"].values()):
                break
            best = row["bytes"]
        cutover[cname] = best
    res = {"tool": "tools/pull_reduce_perf.py TYPES=ll", "fabric_free": True, "gpus": 1, "nranks": N,
           "note": "in-process ranks on one GPU: no xGMI byte is priced (the LL path writes 2 (n - 1) x the message "
                   "over the links, the pull path reads 2 (n - 1) / n x); graph-captured, median of rounds; bytes = the "
                   "message of an AllReduce, the per-rank block of a ReduceScatter",
           "cutover_bytes": cutover, "rows": rows}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.environ.get("OUT", os.path.join(root, "profiles", f"pull_reduce_ll_perf_inprocess_n{N}.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print("cutover", cutover, flush=True)


if os.environ.get("TYPES") == "ll":
    ll_programme()
    sys.exit(0)
if os.environ.get("TYPES") == "int64":
    int64_programme()
    sys.exit(0)
if os.environ.get("TYPES") == "premul":
    premul_programme()
    sys.exit(0)


rows = []
for tdt in (torch.float16, torch.bfloat16):
    for S in SIZES:
        count, blk = S // 2, S // 2 // N
        sends = [torch.rand(count, dtype=torch.float32, device=dev).to(tdt) for _ in range(N)]
        full = [torch.zeros(count, dtype=tdt, device=dev) for _ in range(N)]
        part = [torch.zeros(blk, dtype=tdt, device=dev) for _ in range(N)]
        outs = {m.PULL_ALLREDUCE: full, m.PULL_REDUCE_SCATTER: part,
                m.PULL_REDUCE: [full[r] if r == ROOT_RANK else None for r in range(N)]}
        ins = {c: ([t[:blk * N] for t in sends] if c == m.PULL_REDUCE_SCATTER else sends) for _, c in COLLS}
        rs_cfg = m.tuned_config("reducescatter", N, blk * N * 2)
        rs_algo = m.ALGO_NAMES.get((rs_cfg[0] if rs_cfg else "").replace("default_reducescatter_", ""), 0)
        if rs_algo not in (m.ALGO_FULLMESH, m.ALGO_RSAG):
            rs_algo, rs_cfg = m.ALGO_FULLMESH, None
        bulk = max(m.scratch_required(rs_algo, N, blk * N * 2, m.reduce_code(tdt)), 1 << 20)
        ranks = m.InProcessRanks(N, 1 << 16, bulk_scratch_bytes=bulk)

        def avg(coll, nblocks=0):
            ranks.pull_reduce(coll, ins[coll], outs[coll], m.AVG, root=ROOT_RANK, nblocks=nblocks, budget_ticks=BUDGET,
                              stream=cur())

        def sum_allreduce():
            ranks.all_reduce(sends, full, m.ALGO_RSAG_ZC, budget_ticks=BUDGET, stream=cur())

        def sum_reducescatter():
            shape = {"nblocks": rs_cfg[1], "nthreads": rs_cfg[2]} if rs_cfg and rs_cfg[1] > 0 else {}
            ranks.collective(1, ins[m.PULL_REDUCE_SCATTER], part, algo=rs_algo, budget_ticks=BUDGET, stream=cur(), **shape)

        def sum_reduce():
            ranks.reduce(sends, outs[m.PULL_REDUCE], ROOT_RANK, budget_ticks=BUDGET, stream=cur())

        # correctness of what is timed: the mean in fp32, rank order, rounded once (values in [0, 1))
        want = sends[0].float()
        for k in range(1, N):
            want = want + sends[k].float()
        want = (want * (np.float32(1.0) / np.float32(N))).to(tdt)
        ok = True
        for _, c in COLLS:
            avg(c)
        torch.cuda.synchronize()
        ok = ok and all(torch.equal(t, want) for t in full)
        ok = ok and all(torch.equal(part[r], want[r * blk:(r + 1) * blk]) for r in range(N))
        ok = ok and ranks.errors() == [0] * N
        calls, replays = (10, 5) if S >= (8 << 20) else (50, 10)
        row = {"dtype": str(tdt).replace("torch.", ""), "send_bytes_per_rank": S, "root": ROOT_RANK, "correct": bool(ok),
               "graph_calls": calls, "replays": replays, "rounds": ROUNDS,
               "default_nblocks": {name: m.lib().mscclppAmdPullReduceDefaultBlocks(c, blk * 2 if c == m.PULL_REDUCE_SCATTER else S)
                                   for name, c in COLLS},
               "sum_reducescatter_algo": rs_cfg[0] if rs_cfg else "fullmesh (8 x 256)"}
        if tdt == torch.float16:
            sweep = {}
            for name, c in COLLS:
                sweep[name] = []
                for nblocks in SWEEP_BLOCKS:
                    t = [graph_us(lambda: avg(c, nblocks), calls, replays) for _ in range(ROUNDS)]
                    sweep[name].append(dict(nblocks=nblocks, nthreads=512, **stat(t)))
            row["sweep"] = sweep
        lines = [("avg_" + name, (lambda c=c: avg(c))) for name, c in COLLS]
        lines += [("sum_allreduce_rsag_zc", sum_allreduce), ("sum_reducescatter", sum_reducescatter),
                  ("sum_reduce", sum_reduce)]
        t = {name: [] for name, _ in lines}
        for _ in range(ROUNDS):
            for name, fn in lines:
                t[name].append(graph_us(fn, calls, replays))
        row["lines"] = {name: stat(v) for name, v in t.items()}
        row["errors"] = ranks.errors()
        if S == max(SIZES) and tdt == torch.float16:
            with m.PhaseTrace() as tr:
                avg(m.PULL_ALLREDUCE)
                torch.cuda.synchronize()
            row["phases_allreduce"] = tr.phases("pull_allreduce", view=ROOT_RANK)
        rows.append(row)
        print(row, flush=True)
        del sends, full, part, outs, ins, ranks

# small-message latency: MAX AllReduce (three handshakes) beside LL8 (allpair, SUM)
latency = []
for nbytes in (4, 1024):
    count = nbytes // 4
    x = [torch.rand(count, dtype=torch.float32, device=dev) for _ in range(N)]
    y = [torch.zeros(count, dtype=torch.float32, device=dev) for _ in range(N)]
    ranks = m.InProcessRanks(N, max(m.scratch_required(m.ALGO_ALLPAIR, N, nbytes, m.F32), 1 << 16))
    fns = {"max_allreduce_default_grid": lambda: ranks.pull_reduce(m.PULL_ALLREDUCE, x, y, m.MAX, budget_ticks=BUDGET, stream=cur()),
           "max_allreduce_1_workgroup": lambda: ranks.pull_reduce(m.PULL_ALLREDUCE, x, y, m.MAX, nblocks=1, nthreads=64,
                                                                  budget_ticks=BUDGET, stream=cur()),
           "sum_allreduce_ll8": lambda: ranks.all_reduce(x, y, m.ALGO_ALLPAIR, budget_ticks=BUDGET, stream=cur())}
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(graph_us(fn, 50, 10))
    fns["max_allreduce_default_grid"]()
    torch.cuda.synchronize()
    ok = all(torch.equal(v, torch.stack(x).max(dim=0).values) for v in y) and ranks.errors() == [0] * N
    latency.append(dict(bytes=nbytes, dtype="float32", correct=bool(ok), **{k: stat(v) for k, v in t.items()}))
    print(latency[-1], flush=True)
    del ranks

res = {"tool": "tools/pull_reduce_perf.py", "fabric_free": True, "gpus": 1, "nranks": N,
       "note": "in-process ranks on one GPU: no xGMI byte is priced; graph-captured, median of rounds",
       "rows": rows, "latency": latency}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out = os.environ.get("OUT", os.path.join(ROOT, "profiles", f"pull_reduce_perf_inprocess_n{N}.json"))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
