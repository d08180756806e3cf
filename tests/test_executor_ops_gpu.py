"""Every operation of the plan executor on the GPU against known answers.

The case tables of tests/executor_cases.py: plans that together reach every case of the device
switch (get, rre, res, pws / pwsf, flush, rppkt, repkt, recpkt, recspkt, cpkt besides what
tests/test_executor_gpu.py runs), reuse-scratch plans on both sides of the wrap threshold,
reduce_op min, int32 / uint32, buffer_alignment 4 and 8, eight ranks, the minimum message, slices
of nthreads-1 / nthreads / nthreads+1 units and an odd size, two message sizes in turn on the same
buffers and two plans in turn on one Executor.

One spawn per rank count runs all of that count's cases on one Communicator and one Executor.
Messages sit at a fixed offset inside two 1 MiB arenas (input, output) filled with 0xA5 before every
call; after every call the rank checks its guard bytes and, out of place, that its input is
unchanged, and returns the output.  The tests then compare every rank's output of every call bit
for bit with the CPU oracle's simulation and, for int32 / uint32, with the plain numpy answer
(wrapping sum, min, concatenation) computed without the oracle."""
import multiprocessing as mp
import os
import traceback

import numpy as np
import pytest

import executor_cases as X
import mp_util

pytestmark = pytest.mark.gpu


def _worker(rank, n, uid, cases, q):
    try:
        os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "5000")
        import torch

        import mscclpp_amd as m

        mp_util.place_rank(rank, n)
        comm = m.Communicator(rank, n, uid)
        ex = m.Executor(comm)
        mdt = {"i32": m.DataType.int32, "u32": m.DataType.uint32, "f16": m.DataType.float16,
               "bf16": m.DataType.bfloat16, "f32": m.DataType.float32, "e4m3": m.DataType.float8_e4m3fn,
               "e5m2": m.DataType.float8_e5m2, "u8": m.DataType.uint8, "b15": m.DataType.float8_e4m3b15}
        arena_in = torch.empty(X.ARENA_BYTES, dtype=torch.uint8, device="cuda")
        arena_out = torch.empty(X.ARENA_BYTES, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream()
        plans, results, call = {}, [], 0
        g = X.GUARD_BYTES
        for steps, dtype, pkt in cases:
            outs, problems = [], []
            for fname, msg in steps:
                call += 1
                if fname not in plans:
                    plans[fname] = m.ExecutionPlan(os.path.join(X.PLANS, fname), rank)
                plan, d = plans[fname], X.doc(fname)
                ib, ob = X.in_out_bytes(d, msg)
                mine = X.make_inputs(dtype, n, ib, seq=call)[rank]
                arena_in.fill_(X.GUARD)
                arena_out.fill_(X.GUARD)
                arena_in[g:g + ib].copy_(torch.from_numpy(mine))
                torch.cuda.synchronize()
                inplace = plan.is_in_place()
                recv = arena_in if inplace else arena_out
                ex.execute(rank, arena_in.data_ptr() + g, recv.data_ptr() + g, ib, ob, mdt[dtype], plan, stream,
                           m.PacketType.LL16 if pkt == "LL16" else m.PacketType.LL8)
                torch.cuda.synchronize()
                hin, hout = arena_in.cpu().numpy(), arena_out.cpu().numpy()
                if inplace:
                    out, tails = hin[g:g + ob].copy(), ((hin, ob), (hout, -g))
                else:
                    out, tails = hout[g:g + ob].copy(), ((hin, ib), (hout, ob))
                    if not np.array_equal(hin[g:g + ib], mine):
                        problems.append((call, "input changed"))
                for name, (h, size) in zip(("input", "output"), tails):  # size -g: the whole arena is guard
                    bad = np.nonzero(np.concatenate([h[:g], h[g + size:]]) != X.GUARD)[0]
                    if bad.size:
                        problems.append((call, f"{name} arena guard bytes written", int(bad.size), int(bad[0])))
                outs.append(out)
            results.append((outs, problems, ex.device_error()))
            comm.barrier()
        ex.destroy()
        comm.barrier()
        comm.destroy()
        q.put((rank, results, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def _run(n):
    import mscclpp_amd as m

    cases = [(c.steps, c.dtype, c.pkt) for c in X.CASES[n]]
    uid = m.Communicator.unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, n, uid, cases, q)) for r in range(n)]
    for p in procs:
        p.start()
    return mp_util.collect(procs, q, n, 600)


@pytest.fixture(scope="module")
def ran2(built):
    return _run(2)


@pytest.fixture(scope="module")
def ran4(built):
    return _run(4)


@pytest.fixture(scope="module")
def ran8(built):
    return _run(8)


def _first_flag(n, index):
    return 1 + sum(len(c.steps) for c in X.CASES[n][:index])


def _check(n, index, got):
    case = X.CASES[n][index]
    steps = X.run_oracle(case, _first_flag(n, index))
    for rank in range(n):
        outs, problems, err = got[rank][index]
        assert err == [0, 0, 0, 0], (case.id, rank, err)
        assert not problems, (case.id, rank, problems)
        for k, (ins, exp, plain) in enumerate(steps):
            bad = np.nonzero(outs[k] != exp[rank])[0]
            assert bad.size == 0, (case.id, "oracle", rank, k, case.steps[k], bad.size, bad[:8])
            if plain is not None:
                bad = np.nonzero(outs[k] != plain[rank])[0]
                assert bad.size == 0, (case.id, "numpy", rank, k, case.steps[k], bad.size, bad[:8])
            else:
                assert case.dtype not in X.NP_INT or X.is_min(X.doc(case.steps[k][0])), case.id


@pytest.mark.parametrize("index", range(len(X.CASES[2])), ids=[c.id for c in X.CASES[2]])
def test_two_ranks(ran2, index):
    _check(2, index, ran2)


@pytest.mark.parametrize("index", range(len(X.CASES[4])), ids=[c.id for c in X.CASES[4]])
def test_four_ranks(ran4, index):
    _check(4, index, ran4)


@pytest.mark.parametrize("index", range(len(X.CASES[8])), ids=[c.id for c in X.CASES[8]])
def test_eight_ranks(ran8, index):
    _check(8, index, ran8)
