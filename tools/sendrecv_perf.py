"""Fabric-free timing of the native Send / Recv (kernels/sendrecv.hip): 8 ranks in ONE launch on one
GPU (blockIdx.y = rank, every peer buffer local HBM), so no link is priced -- what is measured is
the kernel's own memory pipeline and its ready / done tokens.  Two tables per size S:

  ring    every rank sends S bytes to rank + 1 (8 transfers, 8 S bytes in all)
  single  rank 0 sends S bytes to rank 1 (the other six views launch and find nothing to do)

each at several explicit grids (workgroups per operation) and at the default one, and in the same
run, alternating, each captured in a HIP graph of K calls:

  memcpy    hipMemcpyAsync device-to-device of the same bytes (8 copies of S, or one)
  alltoall  the native AllToAll at its default shape moving the same total (8 S: S per rank;
            S: S / 8 per rank)

plus, for the largest size, the ring's phase stamps (readies posted, pull, dones seen) on rank 0.

    python tools/sendrecv_perf.py        (writes profiles/sendrecv_perf_inprocess_n8.json, or $OUT)
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
GRIDS = [int(s) for s in os.environ.get("GRIDS", "0,1,2,4,8,16,32,64").split(",")]  # 0: the default
ROUNDS = int(os.environ.get("ROUNDS", 3))
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
L = m.lib()


def hip_runtime():
    """The HIP runtime torch has loaded (for hipMemcpyAsync, which torch's own copies do not use)."""
    for ln in open("/proc/self/maps"):
        path = ln.split()[-1]
        if os.path.basename(path).startswith("libamdhip64.so"):
            return ctypes.CDLL(path)
    raise RuntimeError("libamdhip64.so is not loaded")


hip = hip_runtime()
hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
hip.hipMemcpyAsync.restype = ctypes.c_int
D2D = 3  # hipMemcpyDeviceToDevice


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


rows = []
for S in SIZES:
    sends = [torch.randint(0, 256, (S,), dtype=torch.uint8, device=dev) for _ in range(N)]
    recvs = [torch.full((S,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(N)]
    copies = [torch.empty(S, dtype=torch.uint8, device=dev) for _ in range(N)]
    a2a_out = [torch.empty(S, dtype=torch.uint8, device=dev) for _ in range(N)]
    ranks = m.InProcessRanks(N, 1 << 16)
    calls, replays = (10, 5) if S >= (8 << 20) else (50, 10)
    for pattern in ("ring", "single"):
        pairs = [(r, (r + 1) % N) for r in range(N)] if pattern == "ring" else [(0, 1)]
        table = [(s, d, sends[s], recvs[d]) for s, d in pairs]
        per_rank = S if pattern == "ring" else S // N  # the AllToAll moving the same total
        assert per_rank % (16 * N) == 0

        def memcpy():
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for s, d in pairs:
                assert hip.hipMemcpyAsync(copies[d].data_ptr(), sends[s].data_ptr(), S, D2D, st) == 0

        def alltoall():
            ranks.all_to_all([t[:per_rank] for t in sends], [t[:per_rank] for t in a2a_out], budget_ticks=300_000_000,
                             stream=torch.cuda.current_stream())

        for nb in GRIDS:
            def sendrecv():
                ranks.send_recv(table, nblocks=nb, budget_ticks=300_000_000, stream=torch.cuda.current_stream())

            for t in recvs:
                t.fill_(0xA5)
            sendrecv()
            torch.cuda.synchronize()
            ok = ranks.errors() == [0] * N and all(torch.equal(recvs[d], sends[s]) for s, d in pairs)
            t = {"sendrecv": [], "memcpy": [], "alltoall": []}
            for _ in range(ROUNDS):
                for name, fn in (("sendrecv", sendrecv), ("memcpy", memcpy), ("alltoall", alltoall)):
                    t[name].append(graph_us(fn, calls, replays))
            us = {k: float(np.median(v)) for k, v in t.items()}
            moved = S * len(pairs)
            row = {"pattern": pattern, "bytes_per_transfer": S, "transfers": len(pairs), "nblocks": nb,
                   "default_nblocks": L.mscclppAmdSendRecvDefaultBlocks(S), "nthreads": 512, "correct": bool(ok),
                   "errors": ranks.errors(), "graph_calls": calls, "replays": replays, "rounds": ROUNDS,
                   "sendrecv_us": round(us["sendrecv"], 2), "memcpy_us": round(us["memcpy"], 2),
                   "alltoall_us": round(us["alltoall"], 2),
                   "sendrecv_us_min_max": [round(min(t["sendrecv"]), 2), round(max(t["sendrecv"]), 2)],
                   "memcpy_us_min_max": [round(min(t["memcpy"]), 2), round(max(t["memcpy"]), 2)],
                   "alltoall_us_min_max": [round(min(t["alltoall"]), 2), round(max(t["alltoall"]), 2)],
                   "sendrecv_GBs_moved": round(moved / us["sendrecv"] / 1e3, 1),
                   "memcpy_GBs_moved": round(moved / us["memcpy"] / 1e3, 1)}
            if S == max(SIZES) and pattern == "ring" and nb == 0:
                with m.PhaseTrace() as tr:
                    sendrecv()
                    torch.cuda.synchronize()
                row["phases_rank0"] = tr.phases("sendrecv", view=0)
            rows.append(row)
            print(row, flush=True)
    del sends, recvs, copies, a2a_out, ranks

res = {"tool": "tools/sendrecv_perf.py", "fabric_free": True, "gpus": 1, "nranks": N,
       "note": "8 in-process ranks on one GPU: no xGMI byte is priced; graph-captured, median of rounds", "rows": rows}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out = os.environ.get("OUT", os.path.join(ROOT, "profiles", f"sendrecv_perf_inprocess_n{N}.json"))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
