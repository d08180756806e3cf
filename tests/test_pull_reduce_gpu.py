"""ncclMax / ncclAvg of Reduce, ReduceScatter and AllReduce by the zero-copy pull-reduce kernel
(kernels/pull_reduce.hip), in-process ranks (one launch, blockIdx.y = rank).  Every result is
compared bit for bit with the numpy reference of pull_reduce_cases (operands in rank order) -- the
one tolerance: where the AVG reference is NaN at a planted position, any NaN.

Invariants of every call (run_once): every receive buffer sits in a 0xA5 arena whose bytes around
the written range stay intact, buffers that receive nothing stay 0xA5, every send buffer is
unchanged unless the call is in place (then only the result range differs), and every error word is
0.  Every case makes three calls on one InProcessRanks with new data and a rotating root."""
import numpy as np
import pytest
import torch

import oracle_lib as O
import pull_reduce_cases as C

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
_RANKS = {}


def type_table():
    import mscclpp_amd as m

    return {O.F16: (torch.float16, None), O.BF16: (torch.bfloat16, None), O.F32: (torch.float32, None),
            O.I32: (torch.int32, None), O.U32: (torch.int32, m.U32), O.U8: (torch.uint8, None),
            O.E4M3: (torch.float8_e4m3fn, None), O.E5M2: (torch.float8_e5m2, None)}


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
    es = O.itemsize(code)
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
    planted = total >= C.MIN_PLANT
    for r in range(n):
        tag = f"{C.NAMES[code]} op {op} coll {coll} n {n} count {count} rank {r} root {root}"
        if want[r] is not None:
            got = recvs[r].cpu().numpy().view(C.bits_dtype(code))
            bad = C.mismatches(code, op, got, want[r], planted, r * count if coll == C.REDUCE_SCATTER else 0)
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
@pytest.mark.parametrize("op", [C.MAX, C.AVG])
@pytest.mark.parametrize("code", C.TYPES)
def test_every_type_operation_and_collective(built, code, op, coll, n):
    import mscclpp_amd as m

    ranks = ranks_of(n)
    # the first call: the committed table case the CPU test proves non-vacuous (ReduceScatter: its own length)
    run_once(ranks, n, code, op, coll, C.COUNT, C.table_seed(code, op, n), n - 1)
    for c in (1, 2):
        run_once(ranks, n, code, op, coll, C.COUNT, 50000 + 8 * C.table_seed(code, op, n) + c, (c + coll) % n)


# ---- sizes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("code", C.SIZE_TYPES)
def test_small_messages(built, code, coll, n):
    """One element, and 12, 16 and 20 bytes: an AllReduce of 20 bytes at 8 ranks has six empty slices,
    and the first slice of one of 20 bytes at 3 ranks ends in the middle of nothing."""
    es = O.itemsize(code)
    for i, nbytes in enumerate((es,) + C.SMALL_BYTES):
        for op in (C.MAX, C.AVG):
            three_calls(n, code, op, coll, nbytes // es, 300 + i)


@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("code", C.SIZE_TYPES)
def test_one_element_either_side_of_a_workgroup_sweep(built, code, coll):
    """One workgroup of 512 lanes covers 512 * U * 16 bytes per loop trip: a range one element
    shorter and one element longer (AllReduce at 2 ranks: the first slice)."""
    es = O.itemsize(code)
    n = 2
    for delta in (-es, es):
        nbytes = C.SWEEP * (n if coll == C.ALLREDUCE else 1) + delta
        for op in (C.MAX, C.AVG):
            three_calls(n, code, op, coll, nbytes // es, 400, nblocks=1, nthreads=512)


# ---- in place, alignment ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("op", [C.MAX, C.AVG])
def test_in_place(built, op, coll, n):
    """Reduce: send == recv on the root; ReduceScatter: recv == send + rank * bytes; AllReduce: send == recv."""
    for code in (O.F16, O.I32, O.E5M2):
        three_calls(n, code, op, coll, 1031, 500, inplace=True)


@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("code", [O.BF16, O.F32, O.U8])
def test_buffers_shifted_differently_per_rank(built, code, coll):
    es, n = O.itemsize(code), 8
    for k in range(2):
        send_shift = [((3 * r + 5 * k + 1) * es) % 16 for r in range(n)]
        recv_shift = [((5 * r + 7 * k + 2) * es) % 16 for r in range(n)]
        three_calls(n, code, C.AVG if k else C.MAX, coll, 2051, 600 + k, send_shift=send_shift, recv_shift=recv_shift)
        three_calls(n, code, C.MAX if k else C.AVG, coll, 2051, 610 + k, send_shift=send_shift, inplace=True)


@pytest.mark.parametrize("n", [3, 8])
def test_reduce_scatter_of_six_bytes_per_rank(built, n):
    """recvcount * size = 6: every block but the first starts off a 16-byte boundary."""
    for code, count in ((O.F16, 3), (O.U8, 6)):
        for op in (C.MAX, C.AVG):
            three_calls(n, code, op, C.REDUCE_SCATTER, count, 700)
            three_calls(n, code, op, C.REDUCE_SCATTER, count, 701, inplace=True)


# ---- grid shapes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("coll", C.COLLS)
def test_grid_shapes(built, coll):
    n = 8
    for nblocks in (1, 3):
        three_calls(n, O.F16, C.AVG, coll, C.COUNT, 800 + nblocks, nblocks=nblocks)
    three_calls(n, O.F32, C.MAX, coll, 12, 810, nblocks=64)  # 64 workgroups over 48 bytes: most are empty
    for nthreads in (64, 256, 512):
        three_calls(n, O.BF16, C.AVG, coll, C.COUNT, 820 + nthreads, nthreads=nthreads)


def test_default_grid_is_resident_at_eight_ranks(built):
    """8 in-process ranks x the default grids' upper ends in one launch: 64 workgroups of 512 lanes for
    a Reduce (every rank's workgroups hand-shake, the root's reduce), 32 for an AllReduce."""
    import mscclpp_amd as m

    count = (4 << 20) // 2 + 1
    assert m.lib().mscclppAmdPullReduceDefaultBlocks(m.PULL_REDUCE, count * 2) == 64
    assert m.lib().mscclppAmdPullReduceDefaultBlocks(m.PULL_ALLREDUCE, count * 2) == 32
    run_once(ranks_of(8), 8, O.F16, C.AVG, C.REDUCE, count, 830, 5)
    run_once(ranks_of(8), 8, O.F16, C.MAX, C.ALLREDUCE, count, 831, 0)


# ---- beside the existing collectives -----------------------------------------------------------------
def test_sum_all_reduce_between_two_pull_reduces(built):
    """The token counters are shared with the bulk kernels."""
    import mscclpp_amd as m

    n = 8
    ranks = ranks_of(n)
    x = [torch.full((1 << 16,), float(r + 1), dtype=torch.float16, device="cuda") for r in range(n)]
    y = [torch.zeros_like(t) for t in x]
    for k, coll in enumerate(C.COLLS):
        run_once(ranks, n, O.F16, C.AVG, coll, C.COUNT, 900 + k, k)
        ranks.all_reduce(x, y, m.ALGO_RSAG_ZC)
        run_once(ranks, n, O.BF16, C.MAX, coll, C.COUNT, 910 + k, n - 1 - k)
        torch.cuda.synchronize()
        assert ranks.errors() == [0] * n
        for t in y:
            assert bool((t == n * (n + 1) / 2).all())
            t.zero_()


def test_graph_capture_replays(built):
    import mscclpp_amd as m

    n, code, count = 4, O.F16, 50001
    tdt, _ = type_table()[code]
    ranks = ranks_of(n)
    sends = [torch.zeros(count, dtype=tdt, device="cuda") for _ in range(n)]
    wholes, recvs = zip(*[arena(count * 2, 0, FILL) for _ in range(n)])
    outs = [v.view(tdt) for v in recvs]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ranks.pull_reduce(m.PULL_ALLREDUCE, sends, outs, m.AVG, stream=s)  # eager once
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ranks.pull_reduce(m.PULL_ALLREDUCE, sends, outs, m.AVG, stream=torch.cuda.current_stream())
    for it in range(3):
        xs = C.inputs(code, C.AVG, n, count, 950 + it)
        for r in range(n):
            sends[r].view(torch.uint8).copy_(torch.from_numpy(xs[r].view(np.uint8).copy()))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert ranks.errors() == [0] * n, ranks.error_details()
        want = C.ref_avg(code, xs)
        for r in range(n):
            w = wholes[r].cpu().numpy()
            bad = C.mismatches(code, C.AVG, w[16:16 + count * 2].view(np.uint16), want, True)
            assert bad.size == 0, (it, r, bad[:8])
            assert (w[:16] == FILL).all() and (w[16 + count * 2:] == FILL).all()


# ---- refusals launch nothing -------------------------------------------------------------------------
def test_refusals_launch_nothing(built):
    import mscclpp_amd as m

    n, count = 3, 1024
    ranks = ranks_of(n)
    sends = [torch.ones(count, dtype=torch.float16, device="cuda") for _ in range(n)]
    wholes, recvs = zip(*[arena(count * 2, 0, FILL) for _ in range(n)])
    outs = [v.view(torch.float16) for v in recvs]

    def refused(code, **kw):
        args = dict(coll=m.PULL_ALLREDUCE, inputs=sends, outputs=outs, op=m.MAX)
        args.update(kw)
        with pytest.raises(m.MscclppError) as e:
            ranks.pull_reduce(args.pop("coll"), args.pop("inputs"), args.pop("outputs"), args.pop("op"), **args)
        assert e.value.code == code, kw

    for coll in C.COLLS:
        for op in (m.SUM, m.MIN):
            refused(4, coll=coll, op=op)
        for accum in (m.E4M3_ACC_F16, m.E5M2_ACC_F32, m.E4M3B15, m.E4M3B15_ACC_F32):
            refused(4, coll=coll, accum=accum)
        refused(4, coll=coll, nblocks=m.MAX_CHANNELS + 1)
        refused(4, coll=coll, nthreads=96)
        refused(5, coll=coll, nblocks=m.MAX_CHANNELS, nthreads=512)  # 3 x 256 workgroups of 512 lanes are not resident
    refused(4, coll=m.PULL_REDUCE, root=n)
    refused(4, coll=3)
    torch.cuda.synchronize()
    for w in wholes:
        assert bool((w == FILL).all())
    assert ranks.errors() == [0] * n
    three_calls(n, O.F16, C.MAX, C.ALLREDUCE, count, 990)  # and the ranks still work
