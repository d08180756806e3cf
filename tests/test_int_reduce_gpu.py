"""SUM / MIN / MAX / AVG of int64, uint64 and int8 through Reduce, ReduceScatter and AllReduce by the
zero-copy pull-reduce kernel (kernels/pull_reduce.hip), in-process ranks (one launch, blockIdx.y =
rank).  Every result is compared bit for bit with the numpy reference of int_reduce_cases; there is
no tolerance.

Invariants of every call (run_once, the structure of test_pull_reduce_gpu): every receive buffer sits
in a 0xA5 arena whose bytes around the written range stay intact, buffers that receive nothing stay
0xA5, every send buffer is unchanged unless the call is in place (then only the result range
differs), and every error word is 0.  Every case makes three calls on one InProcessRanks with new
data and a rotating root."""
import numpy as np
import pytest
import torch

import int_reduce_cases as C

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
_RANKS = {}


def type_table():
    import mscclpp_amd as m

    return {C.I64: (torch.int64, None), C.U64: (torch.int64, m.U64), C.I8: (torch.int8, None)}


def ranks_of(n):
    """One InProcessRanks per rank count for the whole module: the token counters run on."""
    import mscclpp_amd as m

    if n not in _RANKS:
        _RANKS[n] = m.InProcessRanks(n, 1 << 16)
    return _RANKS[n]


def arena(nbytes, shift, fill=None):
    """A uint8 device buffer of nbytes starting `shift` bytes past a 16-byte boundary, inside an
    allocation with at least 16 bytes before and GUARD bytes after it."""
    whole = torch.empty(16 + shift + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    if fill is not None:
        whole.fill_(fill)
    return whole, whole[16 + shift:16 + shift + nbytes]


def expected(code, op, coll, xs, count, root):
    """Per rank: the bits it must receive, or None."""
    n = len(xs)
    ref = C.reference(code, op, xs)
    if coll == C.REDUCE:
        return [ref if r == root else None for r in range(n)]
    if coll == C.REDUCE_SCATTER:
        return [ref[r * count:(r + 1) * count] for r in range(n)]
    return [ref] * n


def run_once(ranks, n, code, op, coll, count, seed, root, inplace=False, send_shift=None, recv_shift=None, **shape):
    tdt, accum = type_table()[code]
    es = C.itemsize(code)
    total = count * (n if coll == C.REDUCE_SCATTER else 1)
    xs = C.inputs(code, op, n, total, seed)
    want = expected(code, op, coll, xs, count, root)
    sends, swholes = [], []
    for r in range(n):
        w, s = arena(total * es, send_shift[r] if send_shift else 0, FILL)
        s.copy_(torch.from_numpy(xs[r].view(np.uint8).copy()))
        swholes.append(w)
        sends.append(s)
    before = [w.cpu().numpy() for w in swholes]
    wholes, recvs, los = [], [], []
    for r in range(n):
        if inplace and want[r] is not None:
            wholes.append(None)
            los.append(None)
            recvs.append(sends[r][r * count * es:(r + 1) * count * es] if coll == C.REDUCE_SCATTER else sends[r])
            continue
        sh = recv_shift[r] if recv_shift else 0
        w, v = arena(count * es, sh, FILL)
        wholes.append(w)
        los.append(16 + sh)
        recvs.append(v)
    # a Reduce's non-roots pass no receive buffer on odd ranks, a real one (which must stay 0xA5) on even ones
    outs = [v.view(tdt) if want[r] is not None or r % 2 == 0 else None for r, v in enumerate(recvs)]
    ranks.pull_reduce(coll, [s.view(tdt) for s in sends], outs, op, root=root, accum=accum, **shape)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    for r in range(n):
        tag = f"{C.NAMES[code]} {C.OP_NAMES[op]} coll {coll} n {n} count {count} rank {r} root {root}"
        if want[r] is not None:
            got = recvs[r].cpu().numpy().view(C.bits_dtype(code))
            bad = C.mismatches(got, want[r])
            assert bad.size == 0, f"{tag}: {bad.size} of {count} elements differ, first at {bad[:8]}: " \
                                  f"got {got[bad[:4]]} want {want[r][bad[:4]]}"
        if wholes[r] is not None:
            w = wholes[r].cpu().numpy()
            if want[r] is None:
                assert (w == FILL).all(), f"{tag}: a buffer that receives nothing was written"
            else:
                assert (w[:los[r]] == FILL).all() and (w[los[r] + count * es:] == FILL).all(), f"{tag}: guard"
        after = swholes[r].cpu().numpy()
        if inplace and want[r] is not None:  # only the result range may differ from the input
            lo = 16 + (send_shift[r] if send_shift else 0) + (r * count * es if coll == C.REDUCE_SCATTER else 0)
            after[lo:lo + count * es] = before[r][lo:lo + count * es]
        assert np.array_equal(after, before[r]), f"{tag}: send buffer (or its guard) changed"


def three_calls(n, code, op, coll, count, seed, **kw):
    ranks = ranks_of(n)
    for c in range(3):
        run_once(ranks, n, code, op, coll, count, seed * 8 + c, (seed + c) % n, **kw)


# ---- every type x operation x collective x rank count ------------------------------------------------
@pytest.mark.parametrize("n", C.RANKS)
@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("op", C.OPS)
@pytest.mark.parametrize("code", C.TYPES)
def test_every_type_operation_and_collective(built, code, op, coll, n):
    ranks = ranks_of(n)
    # the first call: the committed table case the CPU test proves non-vacuous (ReduceScatter: its own length)
    run_once(ranks, n, code, op, coll, C.COUNT, C.table_seed(code, op, n), n - 1)
    for c in (1, 2):
        run_once(ranks, n, code, op, coll, C.COUNT, 50000 + 8 * C.table_seed(code, op, n) + c, (c + coll) % n)


# ---- sizes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("code", C.TYPES)
def test_small_messages(built, code, coll, n):
    """One element, and three: three 64-bit elements are one 16-byte unit and an 8-byte tail, and an
    8-rank AllReduce of them has six empty slices and one of 8 bytes."""
    for i, count in enumerate(C.SMALL_COUNTS):
        for op in C.OPS:
            three_calls(n, code, op, coll, count, 300 + i)


@pytest.mark.parametrize("coll,count", [(C.REDUCE, 257), (C.REDUCE_SCATTER, 257), (C.ALLREDUCE, 257), (C.ALLREDUCE, 515)])
def test_one_workgroup_whose_second_trip_holds_only_the_tail(built, coll, count):
    """64 lanes x U = 2 units cover 128 units per loop trip; 257 int64 elements are 128 units and an
    8-byte tail.  An AllReduce of 515 elements at 2 ranks: slices of 2064 and 2056 bytes, the second one
    that shape (of 257 elements: 1040 and 1016 bytes, a tail in the first trip)."""
    for op in C.OPS:
        three_calls(2, C.I64, op, coll, count, 400, nblocks=1, nthreads=64)


# ---- in place, alignment ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("code", C.TYPES)
def test_in_place(built, code, coll, n):
    """Reduce: send == recv on the root; ReduceScatter: recv == send + rank * bytes; AllReduce: send == recv."""
    for op in C.OPS:
        three_calls(n, code, op, coll, 1031, 500, inplace=True)


@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("code", C.TYPES)
def test_buffers_shifted_differently_per_rank(built, code, coll):
    """64-bit: +0 / +8 past a 16-byte boundary; int8: +1, +7, +15; send and receive differ, and so do the ranks."""
    n = 8
    shifts = (1, 7, 15) if code == C.I8 else (0, 8)
    for k in range(2):
        send_shift = [shifts[(r + k) % len(shifts)] for r in range(n)]
        recv_shift = [shifts[(r // 2 + k) % len(shifts)] for r in range(n)]
        assert any(s != t for s, t in zip(send_shift, recv_shift)) and len(set(send_shift)) > 1 < len(set(recv_shift))
        three_calls(n, code, C.AVG if k else C.SUM, coll, 2051, 600 + k, send_shift=send_shift, recv_shift=recv_shift)
        three_calls(n, code, C.MIN if k else C.MAX, coll, 2051, 610 + k, send_shift=send_shift, inplace=True)


# ---- grid shapes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("coll", C.COLLS)
def test_grid_shapes(built, coll):
    n = 8
    for nblocks in (1, 8, 64):  # 64 workgroups over 4097 elements: most int8 ones are empty
        three_calls(n, C.I64, C.AVG, coll, C.COUNT, 800 + nblocks, nblocks=nblocks)
        three_calls(n, C.I8, C.SUM, coll, C.COUNT, 810 + nblocks, nblocks=nblocks)
        three_calls(n, C.U64, C.MIN, coll, C.COUNT, 820 + nblocks, nblocks=nblocks)


# ---- beside the existing collectives -----------------------------------------------------------------
def test_fp32_sum_all_reduce_between_two_int64_calls(built):
    """The token counters are shared with the bulk kernels."""
    import mscclpp_amd as m

    n = 8
    ranks = ranks_of(n)
    x = [torch.full((1 << 14,), float(r + 1), dtype=torch.float32, device="cuda") for r in range(n)]
    y = [torch.zeros_like(t) for t in x]
    for k, coll in enumerate(C.COLLS):
        run_once(ranks, n, C.I64, C.SUM, coll, C.COUNT, 900 + k, k)
        ranks.all_reduce(x, y, m.ALGO_RSAG_ZC)
        run_once(ranks, n, C.I64, C.AVG, coll, C.COUNT, 910 + k, n - 1 - k)
        torch.cuda.synchronize()
        assert ranks.errors() == [0] * n
        for t in y:
            assert bool((t == n * (n + 1) / 2).all())
            t.zero_()


def test_graph_capture_replays(built):
    import mscclpp_amd as m

    n, code, count = 4, C.I64, 5001
    ranks = ranks_of(n)
    sends = [torch.zeros(count, dtype=torch.int64, device="cuda") for _ in range(n)]
    wholes, recvs = zip(*[arena(count * 8, 0, FILL) for _ in range(n)])
    outs = [v.view(torch.int64) for v in recvs]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ranks.pull_reduce(m.PULL_ALLREDUCE, sends, outs, m.SUM, stream=s)  # eager once
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ranks.pull_reduce(m.PULL_ALLREDUCE, sends, outs, m.SUM, stream=torch.cuda.current_stream())
    for it in range(3):
        xs = C.inputs(code, C.SUM, n, count, 950 + it)
        for r in range(n):
            sends[r].view(torch.uint8).copy_(torch.from_numpy(xs[r].view(np.uint8).copy()))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert ranks.errors() == [0] * n, ranks.error_details()
        want = C.ref_sum(code, xs)
        for r in range(n):
            w = wholes[r].cpu().numpy()
            bad = C.mismatches(w[16:16 + count * 8].view(np.uint64), want)
            assert bad.size == 0, (it, r, bad[:8])
            assert (w[:16] == FILL).all() and (w[16 + count * 8:] == FILL).all()


# ---- refusals launch nothing -------------------------------------------------------------------------
def test_refusals_launch_nothing(built):
    import mscclpp_amd as m

    n, count = 3, 1024
    ranks = ranks_of(n)
    sends = [torch.ones(count, dtype=torch.int64, device="cuda") for _ in range(n)]
    wholes, recvs = zip(*[arena(count * 8, 0, FILL) for _ in range(n)])
    outs = [v.view(torch.int64) for v in recvs]
    halves = [t.view(torch.float16) for t in sends]

    def refused(code, inputs=sends, outputs=outs, **kw):
        args = dict(coll=m.PULL_ALLREDUCE, op=m.SUM)
        args.update(kw)
        with pytest.raises(m.MscclppError) as e:
            ranks.pull_reduce(args.pop("coll"), inputs, outputs, args.pop("op"), **args)
        assert e.value.code == code, kw

    for coll in C.COLLS:
        refused(4, coll=coll, op=4)
        # a byte count that splits an element: int8 views of 1021 bytes taken as int64 / uint64
        bytes_in = [t.view(torch.int8)[:1021 * (n if coll == m.PULL_REDUCE_SCATTER else 1)] for t in sends]
        bytes_out = [v.view(torch.int8)[:1021] for v in recvs]
        refused(4, inputs=bytes_in, outputs=bytes_out, coll=coll, accum=m.I64)
        refused(4, inputs=bytes_in, outputs=bytes_out, coll=coll, accum=m.U64, op=m.MAX)
        for op in (m.SUM, m.MIN):  # fp16 keeps its own kernels for these
            refused(4, inputs=halves, outputs=[v.view(torch.float16) for v in recvs], coll=coll, op=op)
    torch.cuda.synchronize()
    for w in wholes:
        assert bool((w == FILL).all())
    assert ranks.errors() == [0] * n
    three_calls(n, C.I64, C.SUM, C.ALLREDUCE, count, 990)  # and the ranks still work
