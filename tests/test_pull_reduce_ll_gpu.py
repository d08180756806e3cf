"""The small-message LL path of the pull-reduce operations (kernels/pull_reduce_ll.hip): AllReduce and
ReduceScatter of every (dtype, op) the pull path takes, in-process ranks (one launch, blockIdx.y = rank).
Every result is compared bit for bit with the numpy references of the three existing case modules
(through pull_reduce_ll_cases; where a float sum's reference is NaN, any NaN passes) AND byte for byte
with what the pull launcher gives on the same inputs; there is no tolerance.

Invariants of every call (Call.check): every receive buffer sits in a 0xA5 arena whose bytes around the
written range stay intact, every send buffer is unchanged unless the call is in place (then only the
result range differs), and every error word is 0.  The path never handshakes: the last test of the
module checks that no call of it changed a byte of a token array or of an expected-counter array
(the pull launcher's comparison runs use ranks of their own)."""
import numpy as np
import pytest
import torch

import int_reduce_cases as I
import oracle_lib as O
import pull_reduce_cases as P
import pull_reduce_ll_cases as C

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
SCRATCH = 1 << 16
_RANKS, _PULL_RANKS, _TOKENS = {}, {}, {}


def type_table():
    import mscclpp_amd as m

    return {O.F16: (torch.float16, None), O.BF16: (torch.bfloat16, None), O.F32: (torch.float32, None),
            O.I32: (torch.int32, None), O.U32: (torch.int32, m.U32), O.U8: (torch.uint8, None),
            O.E4M3: (torch.float8_e4m3fn, None), O.E5M2: (torch.float8_e5m2, None),
            I.I64: (torch.int64, None), I.U64: (torch.int64, m.U64), I.I8: (torch.int8, None)}


def token_bytes(ranks):
    import mscclpp_amd as m

    return [(m.device_view(ranks.tokens[r].ptr, ranks.tokens[r].nbytes).cpu().numpy().copy(),
             ranks.expected[r].cpu().numpy().copy()) for r in range(ranks.n)]


def ranks_of(n):
    """One InProcessRanks per rank count for the whole module's LL calls: the flags run on."""
    import mscclpp_amd as m

    if n not in _RANKS:
        _RANKS[n] = m.InProcessRanks(n, SCRATCH)
        _TOKENS[n] = token_bytes(_RANKS[n])
    return _RANKS[n]


def pull_ranks_of(n):
    """... and one for the pull launcher's runs, which handshake."""
    import mscclpp_amd as m

    if n not in _PULL_RANKS:
        _PULL_RANKS[n] = m.InProcessRanks(n, SCRATCH)
    return _PULL_RANKS[n]


def arena(nbytes, shift, fill=None):
    """A uint8 device buffer of nbytes starting `shift` bytes past a 16-byte boundary, inside an
    allocation with at least 16 bytes before and GUARD bytes after it."""
    whole = torch.empty(16 + shift + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    if fill is not None:
        whole.fill_(fill)
    return whole, whole[16 + shift:16 + shift + nbytes]


def device_scalar(code, value):
    bits = P.round_to(code, np.asarray([value], np.float32))
    return torch.from_numpy(bits.view(np.uint8).copy()).cuda().view(type_table()[code][0])


class Call:
    """One call's buffers and expectations: launch() enqueues it, check() judges it after a synchronise.
    nbytes: the message of an AllReduce, the per-rank block of a ReduceScatter."""

    def __init__(self, n, row, coll, nbytes, seed, inplace=False, send_shift=None, recv_shift=None, case=None):
        self.n, self.row, self.coll, self.nbytes, self.inplace, self.send_shift = n, row, coll, nbytes, inplace, send_shift
        self.es = es = C.itemsize(row)
        self.count = count = nbytes // es
        self.total = count * (n if coll == C.REDUCE_SCATTER else 1)
        self.sends, self.swholes, self.wholes, self.recvs, self.los = [], [], [], [], []
        for r in range(n):
            w, s = arena(self.total * es, send_shift[r] if send_shift else 0, FILL)
            self.swholes.append(w)
            self.sends.append(s)
        for r in range(n):
            if inplace:
                s = self.sends[r]
                self.wholes.append(None)
                self.los.append(None)
                self.recvs.append(s[r * nbytes:(r + 1) * nbytes] if coll == C.REDUCE_SCATTER else s)
                continue
            sh = recv_shift[r] if recv_shift else 0
            w, v = arena(nbytes, sh, FILL)
            self.wholes.append(w)
            self.los.append(16 + sh)
            self.recvs.append(v)
        self.pull_out = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(n)]
        self.load(*(case or C.make_case(row, n, self.total, seed)))

    def load(self, xs, ss):
        """New data (and scalars) into the same buffers."""
        self.xs, self.ss = xs, ss
        ref = C.reference(self.row, xs, ss)
        c = self.count
        self.want = [ref[r * c:(r + 1) * c] if self.coll == C.REDUCE_SCATTER else ref for r in range(self.n)]
        for r in range(self.n):
            self.sends[r].copy_(torch.from_numpy(xs[r].view(np.uint8).copy()))
            if self.wholes[r] is not None:
                self.wholes[r].fill_(FILL)
        self.before = [w.cpu().numpy() for w in self.swholes]

    def scalars(self, device_scalars=None):
        if self.ss is None:
            return {}
        imm = [float(s) for s in self.ss]
        if device_scalars is not None:  # an immediate that must lose against its rank's pointer
            imm = [123.0 if t is not None else s for s, t in zip(imm, device_scalars)]
        return dict(scales=imm, scale_tensors=device_scalars)

    def launch_pull(self, device_scalars=None):
        """The pull launcher on the same inputs, into buffers of its own (before an in-place LL call)."""
        tdt, accum = type_table()[self.row[1]]
        pull_ranks_of(self.n).pull_reduce(self.coll, [s.view(tdt) for s in self.sends], [v.view(tdt) for v in self.pull_out],
                                          self.row[2], accum=accum, **self.scalars(device_scalars))

    def launch(self, ranks, device_scalars=None, stream=None, **shape):
        tdt, accum = type_table()[self.row[1]]
        ranks.pull_reduce_ll(self.coll, [s.view(tdt) for s in self.sends], [v.view(tdt) for v in self.recvs], self.row[2],
                             accum=accum, stream=stream, **self.scalars(device_scalars), **shape)

    def check(self, ranks, pull=True):
        n, row, coll, nbytes = self.n, self.row, self.coll, self.nbytes
        assert ranks.errors() == [0] * n, ranks.error_details()
        for r in range(n):
            tag = f"{C.row_name(row)} coll {coll} n {n} bytes {nbytes} rank {r}"
            raw = self.recvs[r].cpu().numpy()
            got = raw.view(C.bits_dtype(row))
            bad = C.mismatches(row, got, self.want[r])
            assert bad.size == 0, f"{tag}: {bad.size} of {self.count} elements differ, first at {bad[:8]}: " \
                                  f"got {got[bad[:4]]} want {self.want[r][bad[:4]]}"
            if pull:
                assert np.array_equal(raw, self.pull_out[r].cpu().numpy()), f"{tag}: not the pull path's bytes"
            if self.wholes[r] is not None:
                w, lo = self.wholes[r].cpu().numpy(), self.los[r]
                assert (w[:lo] == FILL).all() and (w[lo + nbytes:] == FILL).all(), f"{tag}: guard"
            after = self.swholes[r].cpu().numpy()
            if self.inplace:  # only the result range may differ from the input
                lo = 16 + (self.send_shift[r] if self.send_shift else 0) + (r * nbytes if coll == C.REDUCE_SCATTER else 0)
                after[lo:lo + nbytes] = self.before[r][lo:lo + nbytes]
            assert np.array_equal(after, self.before[r]), f"{tag}: send buffer (or its guard) changed"


def run_once(n, row, coll, nbytes, seed, device=False, **kw):
    shape = {k: kw.pop(k) for k in ("nblocks", "nthreads") if k in kw}
    ranks = ranks_of(n)
    call = Call(n, row, coll, nbytes, seed, **kw)
    tensors = None
    if device and call.ss is not None:  # device-resident scalars on the odd ranks, immediates on the others
        tensors = [device_scalar(row[1], s) if r % 2 else None for r, s in enumerate(call.ss)]
    call.launch_pull(tensors)
    torch.cuda.synchronize()
    assert pull_ranks_of(n).errors() == [0] * n
    call.launch(ranks, tensors, **shape)
    torch.cuda.synchronize()
    call.check(ranks)


# ---- every (dtype, op) x collective x rank count x size --------------------------------------------
@pytest.mark.parametrize("n", C.RANKS)
@pytest.mark.parametrize("row", C.ROWS, ids=C.row_name)
def test_every_operation_collective_rank_count_and_size(built, row, n):
    for coll in C.LL_COLLS:
        for k, nbytes in enumerate(C.SIZES[C.itemsize(row)]):
            run_once(n, row, coll, nbytes, 100 * n + 10 * coll + k, device=bool(k % 2))


@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("row", C.ROWS, ids=C.row_name)
def test_grids_of_several_passes_and_wider_than_the_units(built, row, n):
    """A 1 x 64 grid covers 65 and 129 units in two and three passes (a lane's later units are loaded
    again for the reduction); a 5 x 64 grid on at most three units leaves workgroups without a unit,
    which still bump their flags."""
    es = C.itemsize(row)
    for coll in C.LL_COLLS:
        for k, nbytes in enumerate(C.SEVERAL_PASSES[es]):
            run_once(n, row, coll, nbytes, 300 + k, **C.ONE_BY_64)
        for k, nbytes in enumerate(b for b in C.SIZES[es] if b <= 24):
            run_once(n, row, coll, nbytes, 320 + k, **C.WIDE_GRID)


@pytest.mark.parametrize("n", C.ORDER_RANKS)
@pytest.mark.parametrize("row", C.ORDER_ROWS, ids=C.row_name)
def test_operands_are_taken_in_rank_order(built, row, n):
    """The planted lanes (pull_reduce_ll_cases.order_case): own-first on rank r would give 0 in lane r - 2."""
    xs, ss = C.order_case(row, n)
    nbytes = C.ORDER_COUNT * C.itemsize(row)
    ranks = ranks_of(n)
    tiled = [np.tile(x, n) for x in xs]  # ReduceScatter: every block is the order case
    for coll, case in ((C.ALLREDUCE, (xs, ss)), (C.REDUCE_SCATTER, (tiled, ss))):
        call = Call(n, row, coll, nbytes, 0, case=case)
        call.launch_pull()
        call.launch(ranks)
        torch.cuda.synchronize()
        call.check(ranks)
        for r in range(2, n):
            got = call.recvs[r].cpu().numpy().view(C.bits_dtype(row))
            assert got[r - 2] != 0 and C.own_first(row, xs, ss, r)[r - 2] == 0


# ---- in place, alignment -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("row", C.ROWS, ids=C.row_name)
def test_in_place(built, row, n):
    """AllReduce: send == recv; ReduceScatter: recv == send + rank * bytes -- also in several passes."""
    es = C.itemsize(row)
    for coll in C.LL_COLLS:
        for k, nbytes in enumerate((es, 12 if es < 8 else 24, C.SEVERAL_PASSES[es][1])):
            run_once(n, row, coll, nbytes, 400 + k, inplace=True)
        run_once(n, row, coll, C.SEVERAL_PASSES[es][1], 410, inplace=True, **C.ONE_BY_64)


@pytest.mark.parametrize("row", C.ROWS, ids=C.row_name)
def test_buffers_shifted_to_element_alignment_differently_per_rank(built, row):
    n, es = 8, C.itemsize(row)
    shifts = {1: (1, 7, 13), 2: (2, 6, 14), 4: (4, 12, 0), 8: (8, 0, 8)}[es]
    send_shift = [shifts[r % 3] for r in range(n)]
    recv_shift = [shifts[(r // 2 + 1) % 3] for r in range(n)]
    assert any(s != t for s, t in zip(send_shift, recv_shift))
    for coll in C.LL_COLLS:
        for k, nbytes in enumerate((C.SIZES[es][1], C.SEVERAL_PASSES[es][0], C.SEVERAL_PASSES[es][1])):
            run_once(n, row, coll, nbytes, 500 + k, send_shift=send_shift, recv_shift=recv_shift)
            run_once(n, row, coll, nbytes, 510 + k, send_shift=send_shift, inplace=True)


# ---- the packets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.RANKS)
def test_packet_image_of_the_half_a_call_used(built, n):
    """After one AllReduce and one ReduceScatter on zeroed scratch, the half the flag's parity names
    holds, in region p of rank q, exactly the packets of rank p's message (AllReduce) or of block q
    of rank p's send buffer (ReduceScatter); the own region and the other half stay zero."""
    import mscclpp_amd as m

    ranks = m.InProcessRanks(n, SCRATCH)
    for row, coll, nbytes in ((("pull", O.F16, C.AVG), C.ALLREDUCE, 12), (("premul", O.F32, C.PREMUL_SUM), C.ALLREDUCE, 20),
                              (("int", I.I64, C.SUM), C.REDUCE_SCATTER, 24), (("pull", O.U8, C.MAX), C.REDUCE_SCATTER, 6)):
        for r in range(n):
            ranks.scratch_tensor(r).zero_()
        flag = int(ranks.flags[0][0].item())
        assert all(bool((f == flag).all()) for f in ranks.flags)
        call = Call(n, row, coll, nbytes, 600 + nbytes)
        call.launch(ranks)
        torch.cuda.synchronize()
        call.check(ranks, pull=False)
        es, premul = C.itemsize(row), row[0] == "premul"
        g = C.geometry(n, nbytes, es, premul)
        base = SCRATCH // 2 if flag & 1 else 0
        for q in range(n):
            scr = ranks.scratch_tensor(q).cpu().numpy()
            want = np.zeros(SCRATCH, np.uint8)
            for p in range(n):
                if p == q:
                    continue
                payload = call.xs[p].view(np.uint8)
                if coll == C.REDUCE_SCATTER:
                    payload = payload[q * nbytes:(q + 1) * nbytes]
                scalar = int(np.float32(call.ss[p]).view(np.uint32)) if premul else None
                lo = base + p * g["region"]
                want[lo:lo + g["region"]] = C.region_image(payload, es, flag, scalar)
            assert np.array_equal(scr, want), (C.row_name(row), coll, q, np.flatnonzero(scr != want)[:8])
        assert all(bool((f == flag + 1).all()) for f in ranks.flags)


# ---- calls back to back, capture -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8])
def test_five_calls_back_to_back_share_flags_and_scratch_with_the_sum_kernel(built, n):
    """No synchronisation between the calls: sizes, grids and the two collectives alternate, an LL8 SUM
    AllReduce (ALGO_ALLPAIR) runs on the same flags and scratch in the middle, and a pull-path call
    (which touches neither) sits in between."""
    import mscclpp_amd as m

    ranks = ranks_of(n)
    calls = [(Call(n, ("pull", O.F32, C.MAX), C.ALLREDUCE, 1028, 700), {}),
             (Call(n, ("int", I.I64, C.SUM), C.REDUCE_SCATTER, 8, 701), dict(nblocks=3, nthreads=64)),
             (Call(n, ("premul", O.BF16, C.PREMUL_SUM), C.ALLREDUCE, 514, 702), dict(nblocks=1, nthreads=64)),
             (Call(n, ("pull", O.E4M3, C.AVG), C.REDUCE_SCATTER, 1030, 703), {}),
             (Call(n, ("pull", O.F16, C.AVG), C.ALLREDUCE, 2, 704), {})]
    for call, _ in calls:
        call.launch_pull()
    sx = [torch.full((259,), float(r + 1), dtype=torch.float16, device="cuda") for r in range(n)]
    sy = [torch.zeros(259, dtype=torch.float16, device="cuda") for _ in range(n)]
    px = [torch.full((300,), r - 1, dtype=torch.int32, device="cuda") for r in range(n)]
    py = [torch.zeros(300, dtype=torch.int32, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    for k, (call, shape) in enumerate(calls):
        call.launch(ranks, **shape)
        if k == 1:
            ranks.all_reduce(sx, sy, m.ALGO_ALLPAIR)
        if k == 2:
            pull_ranks_of(n).pull_reduce(m.PULL_ALLREDUCE, px, py, m.MAX)
    torch.cuda.synchronize()
    for call, _ in calls:
        call.check(ranks)
    assert all(bool((y == n * (n + 1) / 2).all()) for y in sy)
    assert all(bool((y == n - 2).all()) for y in py)


def test_one_capture_and_two_replays_on_new_data(built):
    n, row, coll, nbytes = 4, ("pull", O.BF16, C.AVG), C.REDUCE_SCATTER, 1030
    ranks = ranks_of(n)
    call = Call(n, row, coll, nbytes, 800)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call.launch(ranks, stream=s)  # eager once
    s.synchronize()
    call.check(ranks, pull=False)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call.launch(ranks, stream=torch.cuda.current_stream())
    for it in range(2):
        call.load(*C.make_case(row, n, call.total, 801 + it))
        call.launch_pull()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        call.check(ranks)


def test_premul_sum_immediates_and_device_scalars_changed_between_replays(built):
    import premul_sum_cases as S

    n, code, nbytes = 8, O.F16, 514
    row = ("premul", code, C.PREMUL_SUM)
    ranks = ranks_of(n)
    for coll in C.LL_COLLS:  # per-rank immediates, all different
        run_once(n, row, coll, nbytes, 900 + coll)
    first = S.scalars(code, n, 950, "generic")
    tensors = [device_scalar(code, v) for v in first]
    call = Call(n, row, C.ALLREDUCE, nbytes, 950)
    call.ss = first
    call.load(call.xs, first)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call.launch(ranks, tensors, stream=s)  # eager once
    s.synchronize()
    call.check(ranks, pull=False)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call.launch(ranks, tensors, stream=torch.cuda.current_stream())
    for it in range(2):
        ss = S.scalars(code, n, 951 + it, S.KINDS[it % 2])
        call.load(S.inputs(code, n, call.total, 960 + it, ss), ss)
        for r in range(n):
            tensors[r].copy_(device_scalar(code, ss[r]))
        call.launch_pull(tensors)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        call.check(ranks)


# ---- refusals launch nothing ---------------------------------------------------------------------------
def test_refusals_launch_nothing(built):
    import mscclpp_amd as m

    n, count = 3, 64
    ranks = ranks_of(n)
    torch.cuda.synchronize()
    flags = [f.clone() for f in ranks.flags]
    sends = [torch.ones(count * n, dtype=torch.float32, device="cuda") for _ in range(n)]
    wholes, recvs = zip(*[arena(count * 4 * n, 0, FILL) for _ in range(n)])
    outs = [v.view(torch.float32) for v in recvs]
    ss = [0.5] * n

    def refused(code, inputs=sends, outputs=outs, op=m.MAX, coll=m.PULL_ALLREDUCE, **kw):
        with pytest.raises(m.MscclppError) as e:
            ranks.pull_reduce_ll(coll, inputs, outputs, op, **kw)
        assert e.value.code == code, (op, coll, kw)

    refused(4, coll=m.PULL_REDUCE)  # a Reduce keeps the pull path
    for coll in C.LL_COLLS:
        for op in (m.SUM, m.MIN, 4):
            refused(4, coll=coll, op=op)
        refused(4, coll=coll, op=m.PREMUL_SUM)  # no scalars
        refused(4, coll=coll, op=m.MAX, scales=ss)  # scalars, but not PreMulSum
        ints = [t.view(torch.int32) for t in sends]
        refused(4, inputs=ints, outputs=[v.view(torch.int32) for v in recvs], coll=coll, op=m.PREMUL_SUM, scales=ss)
        bytes_in = [t.view(torch.uint8)[:63 * (n if coll == m.PULL_REDUCE_SCATTER else 1)] for t in sends]
        refused(4, inputs=bytes_in, outputs=[v[:63] for v in recvs], coll=coll, accum=m.F16)  # splits an element
        refused(4, coll=coll, nblocks=m.FLAG_SLOTS + 1)
        refused(4, coll=coll, nblocks=2, nthreads=96)
    # more than the scratch holds: 3 regions of 16 KiB of packets per half
    big = [torch.ones(2048 * n, dtype=torch.float32, device="cuda") for _ in range(n)]
    assert m.pull_reduce_ll_scratch_required(m.PULL_ALLREDUCE, n, 2048 * 4 * n, m.F32, m.MAX) > SCRATCH
    refused(5, inputs=big, outputs=[torch.empty_like(t) for t in big])
    torch.cuda.synchronize()
    for w in wholes:
        assert bool((w == FILL).all())
    assert ranks.errors() == [0] * n
    assert all(torch.equal(f, g) for f, g in zip(ranks.flags, flags)), "a refused call changed the flags"
    run_once(n, ("pull", O.F32, C.MAX), C.ALLREDUCE, 256, 990)  # and the ranks still work


def test_zz_no_token_or_expected_counter_changed(built):
    """Every token array and expected-counter array of the ranks the LL calls of this module ran on is
    byte-equal to what it was when the ranks were made."""
    if not _RANKS:  # selected alone: some calls of its own
        run_once(8, ("pull", O.F16, C.AVG), C.ALLREDUCE, 514, 1200)
    torch.cuda.synchronize()
    for n, ranks in _RANKS.items():
        assert ranks.errors() == [0] * n
        for (tok0, exp0), (tok1, exp1) in zip(_TOKENS[n], token_bytes(ranks)):
            assert np.array_equal(tok0, tok1) and np.array_equal(exp0, exp1), f"n {n}: a token or counter changed"
        assert int(ranks.flags[0][0].item()) > 1  # ... and calls did run on them
