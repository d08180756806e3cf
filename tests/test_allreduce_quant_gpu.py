"""InProcessRanks.all_reduce_quant against the numpy model (bit for bit, on every rank) and the fp64 sum (the block
bound of DESIGN.md §17n): one block, a short last slice and a count with a lane remainder and a ragged scale
dword; one workgroup and several at two thread counts; in and out of place; 0xA5 guards around out; a scratch that
forces three passes; back-to-back calls; a call between two fullmesh AllReduces; the refusals."""
import functools

import numpy as np
import pytest

import allreduce_quant_model as Q

pytestmark = pytest.mark.gpu
TORCH_DT = {"fp16": "float16", "bf16": "bfloat16"}
GUARD = 64  # bytes on either side of out


def counts(n):
    return (32, 32 * (n + 1), 32 * (64 * n + 5))


@functools.lru_cache(maxsize=None)
def case(seed, n, count, dt, fmt):  # (inputs, the model's out): computed once, never written
    xs = Q.inputs(seed, n, count, dt, fmt)
    return xs, Q.model(xs, dt, fmt)


def run(torch, ranks, xs, dt, fmt, in_place=False, **shape):
    """One call on fresh buffers: out's patterns per rank, after the guards and the error words are checked."""
    tdt, n, count = getattr(torch, TORCH_DT[dt]), len(xs), xs[0].size
    raw = [torch.full((2 * GUARD + 2 * count,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(n)]
    outs = [r[GUARD:GUARD + 2 * count].view(tdt) for r in raw]
    ins = outs if in_place else [torch.empty(count, dtype=tdt, device="cuda") for _ in range(n)]
    for t, x in zip(ins, xs):
        t.view(torch.int16).copy_(torch.from_numpy(x.view(np.int16)))
    ranks.all_reduce_quant(ins, outs, fmt, **shape)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n
    for r in raw:
        g = r.cpu().numpy()
        assert (g[:GUARD] == 0xA5).all() and (g[GUARD + 2 * count:] == 0xA5).all(), "a guard byte was written"
    return [o.view(torch.int16).cpu().numpy().view(np.uint16) for o in outs]


def judge(xs, ref, got, dt, fmt, what):
    for r, out in enumerate(got):
        assert np.array_equal(out, ref), (what, r, np.flatnonzero(out != ref)[:8])
    err, bound = Q.error_and_bound(xs, got[0], dt, fmt)
    assert (err <= bound).all(), what


@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("dt", Q.DTYPES)
@pytest.mark.parametrize("n", [2, 3, 8])
def test_counts_grids_and_placement(built, n, dt, fmt):
    import mscclpp_amd as m
    import torch

    need = m.all_reduce_quant_scratch_required(n, counts(n)[-1], m.DTYPE_CODES[getattr(torch, TORCH_DT[dt])], fmt)
    ranks = m.InProcessRanks(n, 4096, bulk_scratch_bytes=need)
    for count in counts(n):
        xs, ref = case(1, n, count, dt, fmt)
        for nblocks in (1, 3):
            for nthreads in (64, 256):
                for in_place in (False, True):
                    got = run(torch, ranks, xs, dt, fmt, in_place, nblocks=nblocks, nthreads=nthreads)
                    judge(xs, ref, got, dt, fmt, (count, nblocks, nthreads, in_place))


@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("dt", Q.DTYPES)
@pytest.mark.parametrize("n", [2, 3, 8])
def test_passes_and_neighbours(built, n, dt, fmt):
    import mscclpp_amd as m
    import torch

    count = counts(n)[-1]  # a slice of 65 .. 67 blocks: passes of 2 x 12 blocks are 24 + 24 + the rest
    small = m.InProcessRanks(n, 4096, bulk_scratch_bytes=Q.scratch_bytes(n, fmt, 2, 12))
    xs, ref = case(1, n, count, dt, fmt)
    judge(xs, ref, run(torch, small, xs, dt, fmt, nblocks=2, nthreads=64), dt, fmt, "three passes")
    judge(xs, ref, run(torch, small, xs, dt, fmt, True, nblocks=2, nthreads=64), dt, fmt, "three passes in place")

    code = m.DTYPE_CODES[getattr(torch, TORCH_DT[dt])]
    need = max(m.all_reduce_quant_scratch_required(n, count, code, fmt), m.scratch_required(m.ALGO_FULLMESH, n, 2 * count, code))
    ranks = m.InProcessRanks(n, 4096, bulk_scratch_bytes=need)
    for seed in (2, 3, 4):  # back to back on new data, the default grid
        xs, ref = case(seed, n, count, dt, fmt)
        judge(xs, ref, run(torch, ranks, xs, dt, fmt), dt, fmt, ("back to back", seed))
    # between two fullmesh AllReduces on the same ranks and scratch (integers: their sum is exact)
    ones = [torch.full((count,), r + 1, dtype=getattr(torch, TORCH_DT[dt]), device="cuda") for r in range(n)]
    for step in range(3):
        if step == 1:
            judge(xs, ref, run(torch, ranks, xs, dt, fmt, nblocks=3, nthreads=128), dt, fmt, "between fullmesh calls")
            continue
        sums = [torch.empty_like(o) for o in ones]
        ranks.all_reduce(ones, sums, m.ALGO_FULLMESH, nblocks=4, nthreads=128)
        torch.cuda.synchronize()
        assert ranks.errors() == [0] * n and all((s == n * (n + 1) // 2).all().item() for s in sums), step


def test_refusals(built):
    import mscclpp_amd as m
    import torch

    n = 2
    ranks, one = (m.InProcessRanks(k, 4096, bulk_scratch_bytes=1 << 16) for k in (n, 1))
    t = lambda count=64, d=torch.float16: [torch.zeros(count, dtype=d, device="cuda") for _ in range(n)]
    x, o, whole = t(), t(), t(96)
    bad = {"fp32": (ranks, t(d=torch.float32), t(d=torch.float32), "mxint8"), "count % 32": (ranks, t(48), t(48), "mxint8"),
           "empty": (ranks, t(0), t(0), "mxint8"), "format": (ranks, x, o, "mxfp8"),
           "alignment": (ranks, [w[4:68] for w in whole], o, "mxfp4"),
           "out alignment": (ranks, x, [w[4:68] for w in whole], "mxfp4"),
           "overlap": (ranks, [w[:64] for w in whole], [w[32:] for w in whole], "mxint8"),
           "one rank": (one, x[:1], o[:1], "mxint8")}
    for what, (rk, ins, outs, fmt) in bad.items():
        with pytest.raises(m.MscclppError) as e:
            rk.all_reduce_quant(ins, outs, fmt)
        assert e.value.code == 4, what
    torch.cuda.synchronize()
    assert all((b == 0).all().item() for b in o) and ranks.errors() == [0] * n  # nothing was launched
    xs, ref = case(1, n, 64, "fp16", "mxint8")  # ... and a good call still runs
    judge(xs, ref, run(torch, ranks, xs, "fp16", "mxint8"), "fp16", "mxint8", "after the refusals")
