"""ncclReduce by a zero-copy pull-reduce at the root (kernels/reduce.hip), in-process ranks (one
launch, blockIdx.y = rank).  Every comparison is bit-exact against oracle_lib.reduce_seq over the
inputs in ring order from the root (root, root + 1, ..., mod n), on oracle_lib.lcg inputs.

Invariants of every call (reduce_once): the root's receive buffer is followed by 64 bytes of 0xA5 that
stay intact, the other ranks' receive buffers are all 0xA5 and stay so, every send buffer is
unchanged and every error word is 0.  Every parametrisation makes three calls on one InProcessRanks
with the root rotating, so the token counters advance and the roles change."""
import numpy as np
import pytest
import torch

import kernel_edge_cases as K
import oracle_lib as O

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
UNITS = 2  # kReduceUnits of kernels/reduce.hip: 16-byte units per lane and step


def type_table():
    """reduce-type code -> (torch dtype of the buffers, the `accum` argument that selects the code)."""
    import mscclpp_amd as m

    f8a, f8b = torch.float8_e4m3fn, torch.float8_e5m2
    return {
        O.F16: (torch.float16, None), O.BF16: (torch.bfloat16, None), O.F32: (torch.float32, None),
        O.I32: (torch.int32, None), O.U32: (torch.int32, m.U32),
        O.E4M3: (f8a, None), O.E5M2: (f8b, None),
        O.E4M3_ACC_F16: (f8a, torch.float16), O.E5M2_ACC_F16: (f8b, torch.float16),
        O.E4M3_ACC_F32: (f8a, torch.float32), O.E5M2_ACC_F32: (f8b, torch.float32),
        O.U8: (torch.uint8, None),
        O.B15: (torch.uint8, m.E4M3B15), O.B15_ACC_F16: (torch.uint8, m.E4M3B15_ACC_F16),
        O.B15_ACC_F32: (torch.uint8, m.E4M3B15_ACC_F32),
    }


ALL_TYPES = (O.F16, O.BF16, O.F32, O.I32, O.U32) + O.FP8_TYPES + (O.U8,) + O.B15_TYPES


def test_type_table_names_every_reduce_code(built):
    import mscclpp_amd as m

    tab = type_table()
    assert sorted(tab) == list(range(15)) == sorted(ALL_TYPES)
    for code, (tdt, accum) in tab.items():
        assert m.reduce_code(tdt, accum) == code


def ring_expect(code, op, ins, root):
    """reduce_seq over [in[root], in[root + 1], ...] (bytes), zero-padded to whole words for the oracle."""
    n, nbytes = len(ins), ins[0].view(np.uint8).size
    pad = []
    for k in range(n):
        w = np.zeros((nbytes + 3) // 4, np.uint32)
        w.view(np.uint8)[:nbytes] = ins[(root + k) % n].view(np.uint8)
        pad.append(w)
    exp = O.reduce_seq(code, op, pad).view(np.uint8)[:nbytes]
    if code in (O.I32, O.U32, O.U8):  # the oracle itself against plain wrapping numpy arithmetic
        wide = np.stack([a.view({O.I32: np.int32, O.U32: np.uint32, O.U8: np.uint8}[code]) for a in ins])
        with np.errstate(over="ignore"):
            plain = wide.sum(axis=0, dtype=wide.dtype) if op == O.SUM else wide.min(axis=0)
        assert np.array_equal(plain.view(np.uint8), exp)
    return exp


def arena(nbytes, shift, fill=None):
    """A uint8 device buffer of nbytes that starts `shift` bytes past a 16-byte boundary, and the whole
    allocation around it (GUARD bytes of it follow the buffer)."""
    whole = torch.empty(16 + shift + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    if fill is not None:
        whole.fill_(fill)
    return whole, whole[16 + shift:16 + shift + nbytes]


def reduce_once(ranks, n, code, op, ins, root, inplace=False, send_shift=None, recv_shift=0, **shape):
    """One call, all invariants checked.  ins: per-rank numpy inputs.  send_shift[r] / recv_shift: bytes
    past a 16-byte boundary of rank r's send buffer / the root's receive buffer."""
    tdt, accum = type_table()[code]
    nbytes = ins[0].view(np.uint8).size
    sends = []
    for r in range(n):
        _, s = arena(nbytes, send_shift[r] if send_shift else 0)
        s.copy_(torch.from_numpy(ins[r].view(np.uint8).copy()))
        sends.append(s)
    wholes, recvs = [], []
    for r in range(n):
        if inplace and r == root:
            wholes.append(None)
            recvs.append(sends[r])
            continue
        w, v = arena(nbytes, recv_shift if r == root else 0, FILL)
        wholes.append(w)
        recvs.append(v)
    outs = [v.view(tdt) if r == root else (None if r % 2 else v.view(tdt)) for r, v in enumerate(recvs)]
    ranks.reduce([s.view(tdt) for s in sends], outs, root, op=op, accum=accum, **shape)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    exp = ring_expect(code, op, ins, root)
    got = recvs[root].cpu().numpy()
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"root {root}: {bad.size} of {nbytes} bytes differ, first at {bad[:8]}"
    for r in range(n):
        if wholes[r] is not None:
            w = wholes[r].cpu().numpy()
            lo = 16 + (recv_shift if r == root else 0)
            if r == root:
                assert (w[:lo] == FILL).all() and (w[lo + nbytes:] == FILL).all(), f"guard of the root {r}"
            else:
                assert (w == FILL).all(), f"receive buffer of rank {r} written"
        if not (inplace and r == root):
            assert np.array_equal(sends[r].cpu().numpy(), ins[r].view(np.uint8)), f"send buffer of rank {r} changed"


def three_calls(n, code, op, count, roots, seq0=0, **kw):
    import mscclpp_amd as m

    ranks = m.InProcessRanks(n, 1 << 16)
    for call, root in enumerate(roots):
        ins = [O.lcg(code, count, r, seq0 + 16 * call) for r in range(n)]
        reduce_once(ranks, n, code, op, ins, root, **kw)


def roots_of(n):
    return (0, n // 2, n - 1)


# ---- types and ops -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("op", [O.SUM, O.MIN])
@pytest.mark.parametrize("code", ALL_TYPES)
def test_every_type_and_op(built, code, op, n):
    """4097 elements: more than one workgroup at the default grid, a ragged tail for every type."""
    three_calls(n, code, op, 4097, roots_of(n), seq0=code)


# ---- sizes -------------------------------------------------------------------------------------------
def size_counts(es):
    """Element counts giving: one element; 12, 16 and 20 bytes; one element either side of one workgroup
    sweep (512 lanes * UNITS * 16 bytes); 4097 elements."""
    sweep = 512 * UNITS * 16 // es
    return sorted({1, 12 // es, 16 // es, 20 // es, sweep - 1, sweep, sweep + 1, 4097})


SIZE_CASES = [(code, count) for code in (O.F16, O.F32, O.U8, O.E4M3_ACC_F32) for count in size_counts(O.itemsize(code))]


@pytest.mark.parametrize("code,count", SIZE_CASES)
def test_sizes(built, code, count):
    """One workgroup (nblocks = 1), so the sweep sizes sit at the end of one lane pass; n = 3."""
    three_calls(3, code, O.SUM, count, roots_of(3), seq0=count % 97, nblocks=1, nthreads=512)


@pytest.mark.parametrize("code,count", [(c, n) for c, n in SIZE_CASES if n < 100])
def test_small_sizes_default_grid(built, code, count):
    three_calls(8, code, O.SUM, count, roots_of(8), seq0=3)


def test_one_mib_plus_one_element(built):
    three_calls(8, O.F16, O.SUM, (1 << 19) + 1, (5, 0, 7), seq0=1)


# ---- in place, launch shapes, misaligned views ---------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("code,count", [(O.F16, 4097), (O.F32, 16384 + 3), (O.E5M2_ACC_F16, 20001)])
def test_in_place_on_the_root(built, n, code, count):
    three_calls(n, code, O.SUM, count, roots_of(n), seq0=7, inplace=True)


@pytest.mark.parametrize("count", [4097, (1 << 18) + 5])
@pytest.mark.parametrize("nblocks", [1, 3, 0])
@pytest.mark.parametrize("nthreads", [64, 512])
def test_launch_shapes(built, count, nblocks, nthreads):
    three_calls(3, O.BF16, O.SUM, count, roots_of(3), seq0=nblocks + nthreads, nblocks=nblocks, nthreads=nthreads)


def test_more_workgroups_than_units(built):
    """64 workgroups over 48 bytes: 61 own nothing, hand-shake all the same, and the call completes."""
    three_calls(3, O.F32, O.SUM, 12, roots_of(3), nblocks=64, nthreads=64)


@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("code,count", [(O.F16, 4097), (O.F16, 2048), (O.F32, 1001), (O.F32, 4096)])
def test_misaligned_views(built, n, code, count):
    """The root's receive buffer and rank 1's send buffer start one element past a 16-byte boundary,
    the others on one (so the root's own send buffer is misaligned exactly when the root is rank 1)."""
    es = O.itemsize(code)
    shifts = [es if r == 1 else 0 for r in range(n)]
    three_calls(n, code, O.SUM, count, (0, 1, n - 1), seq0=9, send_shift=shifts, recv_shift=es)


# ---- MIN over planted specials -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("code", [O.F16, O.BF16, O.F32])
def test_min_of_planted_specials(built, code, n):
    """NaN against numbers, +0 against -0, subnormals, +-inf (table C's planted lanes, kernel_edge_cases.inputs)."""
    import mscclpp_amd as m

    count = 1001
    ranks = m.InProcessRanks(n, 1 << 16)
    for call, root in enumerate(roots_of(n)):
        ins = K.inputs(code, n, count, seq=call, special=True, edges=True)
        st = np.stack(ins)
        nan, inf, zero, sub = K.float_classes(code, st)
        sign = (st.astype(np.uint32) >> (8 * K.ITEM[code] - 1)) & 1
        assert np.any(nan.any(0) & ~nan.all(0))  # NaN against a number
        assert np.any((zero & (sign == 0)).any(0) & (zero & (sign == 1)).any(0) & zero.all(0))  # +0 against -0
        assert np.any(sub.sum(0) >= 2) and np.any(inf.any(0) & ~inf.all(0)) and np.any(inf.all(0))
        reduce_once(ranks, n, code, O.MIN, ins, root)


@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("code", [O.F16, O.F32])
def test_sum_of_random_bit_patterns(built, code, n):
    """The lcg values are multiples of 1/4096 below 1, whose fp32 sums are exact in any order; random
    bit patterns on a quarter of the lanes (kernel_edge_cases.inputs) make the fp32 sum depend on the
    ring order from the root too."""
    import mscclpp_amd as m

    ranks = m.InProcessRanks(n, 1 << 16)
    for call, root in enumerate(roots_of(n)):
        reduce_once(ranks, n, code, O.SUM, K.inputs(code, n, 4097, seq=call, special=True), root)


# ---- past 4 GiB ------------------------------------------------------------------------------------------
def test_offsets_past_4gib(built):
    """4 GiB + 16 bytes of int32 per rank at the default grid: the last workgroups' ranges start past
    4 GiB; checked on the device against torch's integer addition."""
    import mscclpp_amd as m

    n, nbytes = 2, (4 << 30) + 16
    need = 3 * nbytes + GUARD + 2 * nbytes  # two sends, one receive, and the temporaries of the check
    if torch.cuda.mem_get_info()[0] < need + (1 << 30):
        pytest.skip("free device memory is short of %d GiB" % ((need >> 30) + 2))
    count = nbytes // 4
    ranks = m.InProcessRanks(n, 1 << 16)
    sends = [(torch.arange(count, dtype=torch.int32, device="cuda") * (2 * r + 3)) for r in range(n)]
    whole = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    root = 1
    ranks.reduce(sends, [None, whole[:nbytes].view(torch.int32)], root)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    assert bool((whole[nbytes:] == FILL).all())
    got = whole[:nbytes].view(torch.int32)
    step = 1 << 28
    for lo in range(0, count, step):  # in pieces: the temporaries stay small
        a = torch.arange(lo, min(lo + step, count), dtype=torch.int32, device="cuda")
        assert torch.equal(got[lo:lo + step], a * 3 + a * 5), lo
        assert torch.equal(sends[0][lo:lo + step], a * 3) and torch.equal(sends[1][lo:lo + step], a * 5), lo


# ---- graph capture ---------------------------------------------------------------------------------------
def test_graph_capture_replays(built):
    import mscclpp_amd as m

    n, code, count, root = 4, O.F32, 50001, 2
    tdt, _ = type_table()[code]
    ranks = m.InProcessRanks(n, 1 << 16)
    sends = [torch.zeros(count, dtype=tdt, device="cuda") for _ in range(n)]
    whole, recv = arena(count * 4, 0, FILL)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ranks.reduce(sends, [recv.view(tdt) if r == root else None for r in range(n)], root, stream=s)  # eager once
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ranks.reduce(sends, [recv.view(tdt) if r == root else None for r in range(n)], root,
                     stream=torch.cuda.current_stream())
    for it in range(3):
        ins = [O.lcg(code, count, r, 100 + 10 * it) for r in range(n)]
        for r in range(n):
            sends[r].copy_(torch.from_numpy(ins[r].view(np.int32).copy()).view(tdt))
        whole.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert ranks.errors() == [0] * n, ranks.error_details()
        w = whole.cpu().numpy()
        assert np.array_equal(w[16:16 + count * 4], ring_expect(code, O.SUM, ins, root)), it
        assert (w[:16] == FILL).all() and (w[16 + count * 4:] == FILL).all(), it


# ---- refusals ----------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(built):
    import mscclpp_amd as m

    n, count, root = 3, 1024, 1
    ranks = m.InProcessRanks(n, 1 << 16)
    sends = [torch.zeros(count, dtype=torch.float32, device="cuda") for _ in range(n)]
    recvs = [torch.full((count * 4,), FILL, dtype=torch.uint8, device="cuda") for _ in range(n)]
    outs = [v.view(torch.float32) for v in recvs]
    tokens = [m.device_view(t.ptr, t.nbytes).clone() for t in ranks.tokens]
    for shape in ({"nblocks": m.MAX_CHANNELS + 1}, {"nthreads": 32}, {"nthreads": 96}, {"nthreads": 576},
                  {"nthreads": 1024}):
        with pytest.raises(m.MscclppError) as e:
            ranks.reduce(sends, outs, root, **shape)
        assert e.value.code == 4, shape
    for bad_root in (-1, n):
        with pytest.raises(m.MscclppError) as e:
            ranks.reduce(sends, outs, bad_root)
        assert e.value.code == 4, bad_root
    with pytest.raises(m.MscclppError) as e:
        ranks.reduce(sends, [None] * n, root)  # no receive buffer on the root
    assert e.value.code == 4
    launch = m.lib().mscclppAmdReduceLaunch
    sp = m.stream_ptr()
    nbytes = count * 4
    arr = ranks.views(sends, outs)
    assert launch(None, n, n, nbytes, m.F32, m.SUM, root, 0, 0, 0, sp) == 4
    for nviews, nranks in ((0, n), (2, n), (1, 1), (1, 9)):
        assert launch(arr, nviews, nranks, nbytes, m.F32, m.SUM, 0, 0, 0, 0, sp) == 4, (nviews, nranks)
    assert launch(arr, n, n, 0, m.F32, m.SUM, root, 0, 0, 0, sp) == 4
    assert launch(arr, n, n, nbytes - 2, m.F32, m.SUM, root, 0, 0, 0, sp) == 4  # splits an element
    assert launch(arr, n, n, nbytes - 1, m.F16, m.SUM, root, 0, 0, 0, sp) == 4
    for dtype, op in ((15, m.SUM), (-1, m.SUM), (m.F32, 2), (m.F32, -1)):
        assert launch(arr, n, n, nbytes, dtype, op, root, 0, 0, 0, sp) == 4, (dtype, op)
    for field in ("input", "tokens", "expected", "err"):
        bad = ranks.views(sends, outs)
        setattr(bad[2], field, None)
        assert launch(bad, n, n, nbytes, m.F32, m.SUM, root, 0, 0, 0, sp) == 4, field
    bad = ranks.views(sends, outs)
    bad[root].peerInput[0] = None
    assert launch(bad, n, n, nbytes, m.F32, m.SUM, root, 0, 0, 0, sp) == 4
    torch.cuda.synchronize()
    for r in range(n):  # nothing ran: no byte written, no token moved
        assert bool((recvs[r] == FILL).all())
        assert bool((sends[r] == 0).all())
        assert torch.equal(m.device_view(ranks.tokens[r].ptr, ranks.tokens[r].nbytes), tokens[r])
    assert ranks.errors() == [0] * n
    # and the same ranks still reduce afterwards
    ins = [O.lcg(O.F32, count, r, 5) for r in range(n)]
    reduce_once(ranks, n, O.F32, O.SUM, ins, root)
