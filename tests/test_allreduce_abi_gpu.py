"""ncclAllReduce across processes as frameworks call it: through the library's own selector
(selectAndExecute -> Algorithm::execute -> ncclComm::allReduceLaunch), in place, on views at an
offset inside an allocation, on every element type the ABI maps, SUM and MIN, at sizes on each side
of the selector's thresholds, at 2, 3 and 8 ranks (tables, layouts and expectations in
allreduce_abi_cases.py, proved non-vacuous on the CPU by test_allreduce_abi_cases.py).

One process per rank; the rows of a list run in order on one communicator, three calls per row back
to back on fresh inputs with no host synchronisation between them.  Every call's allocations are
filled with 0xA5 and compared whole afterwards: the receive view with the bytes of the oracle of the
algorithm that ran (for f32, a lane whose expected value is a NaN must hold a NaN), every other byte
-- guards, an out-of-place send view -- unchanged; I32 / U32 calls and the finite float calls are
judged by the plain numpy / fp64 reference as well.  The table of a rank count is dealt over several
process groups (allreduce_abi_cases.parts) so that one test item stays near the cost of the existing
8-process AllReduce test; no row is left out.  The refusals (group 5) run at the end of the first list.

With one GPU the ranks share it: the protocol is the same, the bytes move through local HBM."""
import multiprocessing as mp
import traceback

import pytest

import allreduce_abi_cases as A
import mp_util

pytestmark = pytest.mark.gpu

# process groups per rank count: each rank computes the oracle of all n ranks for every call
PARTS = {2: 2, 3: 3, 8: 24}


def _worker(rank, n, uid, q, part, nparts):
    try:
        import ctypes
        import os

        os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "5000")
        os.environ.pop("MSCCLPP_AMD_TUNED_CONFIG", None)  # the built-in table decides
        os.environ.pop("MSCCLPP_AMD_ALGO", None)
        import numpy as np
        import torch

        import mscclpp_amd as m
        import allreduce_abi_cases as A
        import collective_edge_cases as C
        import oracle_lib as O

        import mp_util

        mp_util.place_rank(rank, n)
        torch.set_num_threads(1)  # n processes share the host: no thread pool each for the references
        comm = m.Communicator(rank, n, uid)
        L, vp = m.lib(), ctypes.c_void_p
        res, detail = {}, {}

        def all_reduce(send, recv, count, code, op, algo=None):
            if algo is None:
                return L.ncclAllReduce(vp(send.data_ptr()), vp(recv.data_ptr()), count, A.NCCL_TYPE[code], A.NCCL_OP[op],
                                       comm.comm, m.stream_ptr())
            return L.mscclppAmdCommAllReduce(comm.comm, vp(send.data_ptr()), vp(recv.data_ptr()), count,
                                             A.NCCL_TYPE[code], A.NCCL_OP[op], m.ALGO_NAMES[algo], 0, 0, m.stream_ptr())

        def report(name, bad):
            res[name] = not bad
            if bad:
                detail[name] = bad

        # ---- groups 1 to 4 ------------------------------------------------------------------------
        for row in A.parts(n, nparts)[part]:
            (sa, so), (ra, ro), sizes = A.layout(row)
            count, nb = row.nbytes // O.itemsize(row.code), row.nbytes
            algo = row.algo or A.selected(L, n, nb, row.code)
            # every buffer of the three calls first (an upload from host memory waits for the stream) ...
            made = []
            for call in range(A.CALLS):
                ins = A.row_inputs(n, row, call)
                host = [np.full(s, C.GUARD, np.uint8) for s in sizes]
                host[sa][so:so + nb] = C.as_bytes(ins[rank])
                dev = [torch.from_numpy(a).cuda() for a in host]
                send, recv = dev[sa][so:so + nb], dev[ra][ro:ro + nb]
                assert send.data_ptr() % 16 == so % 16 and recv.data_ptr() % 16 == ro % 16
                made.append((ins, host, dev, send, recv))
            torch.cuda.synchronize()
            # ... then the three calls with nothing between them: registration, scratch and flags are
            # reused while the previous kernel may still wait for its peers
            calls = [(ins, host, dev, all_reduce(send, recv, count, row.code, row.op, row.algo))
                     for ins, host, dev, send, recv in made]
            torch.cuda.synchronize()
            del made
            bad = []
            for call, (ins, host, dev, rc) in enumerate(calls):
                if rc != 0:
                    bad.append(f"call {call}: returned {rc}")
                    continue
                got = [t.cpu().numpy() for t in dev]
                out = got[ra][ro:ro + nb].copy()
                exp = A.oracle_outputs(L, algo, row.code, row.op, ins, nb)
                wrong = A.judge(row, call, ins, out, None if exp is None else exp[rank])
                # everything but the receive view: the guards and an out-of-place send view
                got[ra][ro:ro + nb] = host[ra][ro:ro + nb]
                outside = sum(int(np.count_nonzero(g != h)) for g, h in zip(got, host))
                if wrong or outside:
                    bad.append(f"call {call} via {algo}: {wrong} wrong bytes / lanes in the result, {outside} bytes "
                               f"changed outside it")
            report(A.row_name(row), bad)
            del calls

        # ---- group 5: overlapping ranges are refused, nothing is launched ----------------------------
        if part == 0:
            cid = C.case_id("allreduce-abi-refusals", n)
            for k, ref in enumerate(A.REFUSALS):
                s_off, s_len, r_off, r_len, total = A.refusal_layout(ref, rank, n)
                image = np.full(total, C.GUARD, np.uint8)
                image[s_off:s_off + s_len] = C.as_bytes(C.bits(ref.code, s_len // O.itemsize(ref.code), cid, k, rank))
                whole = torch.from_numpy(image).cuda()
                send, recv = whole[s_off:s_off + s_len], whole[r_off:r_off + r_len]
                count = r_len // O.itemsize(ref.code)
                if ref.what == "allreduce":
                    rc = all_reduce(send, recv, count, ref.code, ref.op)
                else:
                    rc = L.ncclReduceScatter(vp(send.data_ptr()), vp(recv.data_ptr()), count, A.NCCL_TYPE[ref.code],
                                             A.NCCL_OP[ref.op], comm.comm, m.stream_ptr())
                torch.cuda.synchronize()
                changed = int(np.count_nonzero(whole.cpu().numpy() != image))
                report(A.refusal_name(ref), [] if rc == A.REFUSED and not changed else
                       [f"returned {rc} (expected {A.REFUSED}), {changed} bytes of the buffers changed"])
            # the token channels are still in step: the next valid calls are exact
            B = A.AFTER_BLOCK
            mine = slice(rank * B, (rank + 1) * B)
            ins = C.reduce_inputs(O.F32, O.SUM, n, n * B // 4, cid, len(A.REFUSALS), "finite")
            exp = C.rs_expected(O.F32, O.SUM, ins, B, 0)
            x = torch.from_numpy(C.as_bytes(ins[rank]).copy()).cuda()
            y = torch.full((n * B,), C.GUARD, dtype=torch.uint8, device="cuda")
            rc = all_reduce(x, y, n * B // 4, O.F32, O.SUM)  # the refused entry point itself, through the selector
            torch.cuda.synchronize()
            got = y.cpu().numpy()
            cnt = B // 4
            ar = A.oracle_outputs(L, A.selected(L, n, n * B, O.F32), O.F32, O.SUM, ins, n * B)[rank]
            wrong = int(C.mismatches(O.F32, got.copy(), ar.copy()).size) + \
                int(C.plain_failures(O.F32, O.SUM, ins, got.copy()).size)
            report(A.AFTER_CHECKS[0], [] if rc == 0 and not wrong else [f"returned {rc}, {wrong} wrong lanes"])
            y = torch.full((B,), C.GUARD, dtype=torch.uint8, device="cuda")
            comm.reduce_scatter(x.view(torch.float32), y.view(torch.float32))
            torch.cuda.synchronize()
            got = y.cpu().numpy()
            wrong = int(C.mismatches(O.F32, got.copy(), exp[mine].copy()).size) + \
                int(C.plain_failures(O.F32, O.SUM, [a[rank * cnt:(rank + 1) * cnt] for a in ins], got.copy()).size)
            report(A.AFTER_CHECKS[1], [] if not wrong else [f"{wrong} wrong lanes"])
            z = torch.full((n * B,), C.GUARD, dtype=torch.uint8, device="cuda")
            comm.all_gather(y.view(torch.float32), z.view(torch.float32))
            torch.cuda.synchronize()
            wrong = int(C.mismatches(O.F32, z.cpu().numpy(), exp.copy()).size)
            report(A.AFTER_CHECKS[2], [] if not wrong else [f"{wrong} wrong lanes"])

        res["device_error_words"] = comm.device_error_detail(clear=False)
        res["device_error"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, (res, detail), None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


CASES = [(n, part) for n in A.RANKS for part in range(PARTS[n])]


@pytest.mark.parametrize("n,part", CASES, ids=[f"n{n}-part{p}" for n, p in CASES])
def test_ncclallreduce_abi_matrix(built, n, part):
    import mscclpp_amd as m

    uid = m.Communicator.unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, n, uid, q, part, PARTS[n])) for r in range(n)]
    for p in procs:
        p.start()
    got = mp_util.collect(procs, q, n, 240)
    want = [A.row_name(row) for row in A.parts(n, PARTS[n])[part]]
    if part == 0:
        want += [A.refusal_name(ref) for ref in A.REFUSALS] + list(A.AFTER_CHECKS)
    lines = []
    for rank in range(n):
        res, detail = got[rank]
        if res["device_error"] != 0:
            lines.append(f"rank {rank}: device error words {res['device_error_words']}")
        lines += [f"rank {rank} {k}: {detail.get(k, 'not run')}" for k in want if res.get(k) is not True]
    assert not lines, "\n".join(lines)
