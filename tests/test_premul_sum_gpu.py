"""PreMulSum (ncclRedOpCreatePreMulSum's operation: rank k's operand times rank k's scalar, summed in
rank order) of fp16 / bf16 / fp32 through Reduce, ReduceScatter and AllReduce by the zero-copy
pull-reduce kernel (kernels/pull_reduce.hip), in-process ranks (one launch, blockIdx.y = rank).  Every
result is compared bit for bit with the numpy reference of premul_sum_cases (where the reference is
NaN, any NaN passes); there is no tolerance.

Invariants of every call (run_once, the structure of test_int_reduce_gpu): every receive buffer sits
in a 0xA5 arena whose bytes around the written range stay intact, buffers that receive nothing stay
0xA5, every send buffer is unchanged unless the call is in place (then only the result range
differs), and every error word is 0.  The ranks exchange their scalars through the diagonal of their
token arrays; the last test of the module checks that after all its calls every token array equals
its expected counters again."""
import numpy as np
import pytest
import torch

import oracle_lib as O
import premul_sum_cases as C
import pull_reduce_cases as P

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
_RANKS = {}
TORCH = {O.F16: torch.float16, O.BF16: torch.bfloat16, O.F32: torch.float32}


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


def device_scalar(code, value):
    """One element of the element type in device memory holding `value` (which the type holds exactly)."""
    bits = C.scalar_bits(code, [value])
    return torch.from_numpy(bits.view(np.uint8).copy()).cuda().view(TORCH[code])


def expected(code, coll, xs, ss, count, root):
    """Per rank: the bits it must receive, or None."""
    n = len(xs)
    ref = C.reference(code, xs, ss)
    if coll == C.REDUCE:
        return [ref if r == root else None for r in range(n)]
    if coll == C.REDUCE_SCATTER:
        return [ref[r * count:(r + 1) * count] for r in range(n)]
    return [ref] * n


class Call:
    """One call's buffers and expectations: launch() enqueues it, check() judges it after a synchronise."""

    def __init__(self, n, code, coll, count, seed, root, ss, inplace=False, send_shift=None, recv_shift=None):
        self.n, self.code, self.coll, self.count, self.root, self.ss, self.inplace = n, code, coll, count, root, ss, inplace
        self.send_shift = send_shift
        es = O.itemsize(code)
        self.total = total = count * (n if coll == C.REDUCE_SCATTER else 1)
        xs = C.inputs(code, n, total, seed, ss)
        self.want = want = expected(code, coll, xs, ss, count, root)
        self.sends, self.swholes = [], []
        for r in range(n):
            w, s = arena(total * es, send_shift[r] if send_shift else 0, FILL)
            s.copy_(torch.from_numpy(xs[r].view(np.uint8).copy()))
            self.swholes.append(w)
            self.sends.append(s)
        self.before = [w.cpu().numpy() for w in self.swholes]
        self.wholes, self.recvs, self.los = [], [], []
        for r in range(n):
            if inplace and want[r] is not None:
                self.wholes.append(None)
                self.los.append(None)
                s = self.sends[r]
                self.recvs.append(s[r * count * es:(r + 1) * count * es] if coll == C.REDUCE_SCATTER else s)
                continue
            sh = recv_shift[r] if recv_shift else 0
            w, v = arena(count * es, sh, FILL)
            self.wholes.append(w)
            self.los.append(16 + sh)
            self.recvs.append(v)

    def launch(self, ranks, device_scalars=None, stream=None, **shape):
        """device_scalars: per rank a device tensor or None (that rank's scalar is then an immediate)."""
        import mscclpp_amd as m

        tdt = TORCH[self.code]
        # a Reduce's non-roots pass no receive buffer on odd ranks, a real one (which must stay 0xA5) on even ones
        outs = [v.view(tdt) if self.want[r] is not None or r % 2 == 0 else None for r, v in enumerate(self.recvs)]
        imm = [float(s) for s in self.ss]
        if device_scalars is not None:  # an immediate that must lose against its rank's pointer
            imm = [123.0 if t is not None else s for s, t in zip(imm, device_scalars)]
        ranks.pull_reduce(self.coll, [s.view(tdt) for s in self.sends], outs, m.PREMUL_SUM, root=self.root, scales=imm,
                          scale_tensors=device_scalars, stream=stream, **shape)

    def check(self, ranks):
        n, code, coll, count, root = self.n, self.code, self.coll, self.count, self.root
        es = O.itemsize(code)
        assert ranks.errors() == [0] * n, ranks.error_details()
        for r in range(n):
            tag = f"{C.NAMES[code]} coll {coll} n {n} count {count} rank {r} root {root} scalars {list(self.ss)}"
            if self.want[r] is not None:
                got = self.recvs[r].cpu().numpy().view(C.bits_dtype(code))
                bad = C.mismatches(code, got, self.want[r])
                assert bad.size == 0, f"{tag}: {bad.size} of {count} elements differ, first at {bad[:8]}: " \
                                      f"got {got[bad[:4]]} want {self.want[r][bad[:4]]}"
            if self.wholes[r] is not None:
                w = self.wholes[r].cpu().numpy()
                if self.want[r] is None:
                    assert (w == FILL).all(), f"{tag}: a buffer that receives nothing was written"
                else:
                    lo = self.los[r]
                    assert (w[:lo] == FILL).all() and (w[lo + count * es:] == FILL).all(), f"{tag}: guard"
            after = self.swholes[r].cpu().numpy()
            if self.inplace and self.want[r] is not None:  # only the result range may differ from the input
                lo = 16 + (self.send_shift[r] if self.send_shift else 0) + (r * count * es if coll == C.REDUCE_SCATTER else 0)
                after[lo:lo + count * es] = self.before[r][lo:lo + count * es]
            assert np.array_equal(after, self.before[r]), f"{tag}: send buffer (or its guard) changed"


def run_once(ranks, n, code, coll, count, seed, root, ss, device=False, inplace=False, send_shift=None, recv_shift=None,
             **shape):
    call = Call(n, code, coll, count, seed, root, ss, inplace, send_shift, recv_shift)
    # device-resident scalars on the odd ranks (all ranks when `device` is "all"), immediates on the others
    tensors = None
    if device:
        tensors = [device_scalar(code, s) if (r % 2 or device == "all") else None for r, s in enumerate(ss)]
    call.launch(ranks, tensors, **shape)
    torch.cuda.synchronize()
    call.check(ranks)


def three_calls(n, code, coll, count, seed, **kw):
    """Three calls with new data, a rotating root and other scalars: special, generic, equal 1 / (2 n)."""
    ranks = ranks_of(n)
    run_once(ranks, n, code, coll, count, seed * 8, seed % n, C.scalars(code, n, seed, "special"), **kw)
    run_once(ranks, n, code, coll, count, seed * 8 + 1, (seed + 1) % n, C.scalars(code, n, seed + 1, "generic"), **kw)
    run_once(ranks, n, code, coll, count, seed * 8 + 2, (seed + 2) % n, C.fsdp_scalars(code, n), **kw)


# ---- every type x collective x rank count ------------------------------------------------------------
@pytest.mark.parametrize("n", C.RANKS)
@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("code", C.TYPES)
def test_every_type_collective_and_rank_count(built, code, coll, n):
    """The committed table case the CPU test proves non-vacuous with both kinds of scalars (ReduceScatter:
    its own length, n blocks), then equal scalars 1 / (2 n), the FSDP case."""
    ranks = ranks_of(n)
    for k, kind in enumerate(C.KINDS):
        seed = C.table_seed(code, n) + (500 if kind == "generic" else 0)
        run_once(ranks, n, code, coll, C.COUNT, seed, (n - 1 + k) % n, C.scalars(code, n, seed, kind))
    run_once(ranks, n, code, coll, C.COUNT, 60000 + C.table_seed(code, n), coll % n, C.fsdp_scalars(code, n))


# ---- counts and grids ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("code", C.TYPES)
def test_small_counts(built, code, coll, n):
    """One element and three: an 8-rank AllReduce of them leaves most slices empty; every workgroup
    still publishes its rank's scalar and takes part in the handshakes."""
    for i, count in enumerate(C.SMALL_COUNTS):
        three_calls(n, code, coll, count, 300 + i)


@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("nblocks", [1, 256])
def test_grid_shapes(built, coll, nblocks):
    """One workgroup, and 256 (the most there are channels) of 64 lanes, where most have an empty share."""
    nthreads = 64 if nblocks == 256 else 512  # 8 ranks x 256 workgroups must be resident at once
    three_calls(8, O.BF16, coll, C.COUNT, 800 + nblocks, nblocks=nblocks, nthreads=nthreads)
    three_calls(3, O.F32, coll, C.COUNT, 810 + nblocks, nblocks=nblocks, nthreads=nthreads)


# ---- in place, alignment -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("code", C.TYPES)
def test_in_place(built, code, coll, n):
    """Reduce: send == recv on the root; ReduceScatter: recv == send + rank * bytes; AllReduce: send == recv."""
    three_calls(n, code, coll, 1031, 500, inplace=True)


@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("code", C.TYPES)
def test_buffers_shifted_differently_per_rank(built, code, coll):
    """Element-aligned views: +2, +6, +14 past a 16-byte boundary (fp32: +4, +12, +0); send and receive
    differ, and so do the ranks."""
    n = 8
    shifts = (4, 12, 0) if code == O.F32 else (2, 6, 14)
    send_shift = [shifts[r % 3] for r in range(n)]
    recv_shift = [shifts[(r // 2 + 1) % 3] for r in range(n)]
    assert any(s != t for s, t in zip(send_shift, recv_shift))
    three_calls(n, code, coll, 2051, 600, send_shift=send_shift, recv_shift=recv_shift)
    three_calls(n, code, coll, 2051, 610, send_shift=send_shift, inplace=True)


# ---- scalar sources ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("coll", C.COLLS)
@pytest.mark.parametrize("code", C.TYPES)
def test_device_resident_scalars(built, code, coll, n):
    """Odd ranks read their scalar through a device pointer (their immediate is a decoy), even ranks
    take the immediate; then every rank through a pointer."""
    ranks = ranks_of(n)
    run_once(ranks, n, code, coll, C.COUNT, 700, 0, C.scalars(code, n, 700, "generic"), device=True)
    run_once(ranks, n, code, coll, C.COUNT, 701, n - 1, C.scalars(code, n, 701, "special"), device="all")


@pytest.mark.parametrize("coll", C.COLLS)
def test_three_calls_queued_back_to_back_reuse_the_slots(built, coll):
    """No synchronisation between the calls: a call's scalars are published into the slots the call
    before it has just zeroed, and each call must see its own."""
    n, code = 8, O.F16
    ranks = ranks_of(n)
    calls = [Call(n, code, coll, C.COUNT, 900 + k, k, C.scalars(code, n, 900 + k, C.KINDS[k % 2])) for k in range(3)]
    torch.cuda.synchronize()
    for call in calls:
        call.launch(ranks)
    torch.cuda.synchronize()
    for call in calls:
        call.check(ranks)


def test_graph_replay_reads_the_scalars_of_its_own_time(built):
    """A captured ReduceScatter with device-resident scalars is replayed after the scalars (and the
    data) were changed: the results follow the new scalars."""
    n, code, count = 4, O.BF16, 5001
    ranks = ranks_of(n)
    first = C.scalars(code, n, 950, "generic")
    tensors = [device_scalar(code, s) for s in first]
    call = Call(n, code, C.REDUCE_SCATTER, count, 950, 0, first)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call.launch(ranks, tensors, stream=s)  # eager once
    s.synchronize()
    call.check(ranks)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call.launch(ranks, tensors, stream=torch.cuda.current_stream())
    for it in range(3):
        ss = C.scalars(code, n, 951 + it, C.KINDS[it % 2])
        xs = C.inputs(code, n, count * n, 960 + it, ss)
        for r in range(n):
            tensors[r].copy_(device_scalar(code, ss[r]))
            call.sends[r].copy_(torch.from_numpy(xs[r].view(np.uint8).copy()))
            call.wholes[r].fill_(FILL)
        call.before = [w.cpu().numpy() for w in call.swholes]
        call.ss, call.want = ss, expected(code, C.REDUCE_SCATTER, xs, ss, count, 0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        call.check(ranks)


# ---- refusals launch nothing ---------------------------------------------------------------------------
def test_refusals_launch_nothing(built):
    import mscclpp_amd as m

    n, count = 3, 1024
    ranks = ranks_of(n)
    sends = [torch.ones(count, dtype=torch.float32, device="cuda") for _ in range(n)]
    wholes, recvs = zip(*[arena(count * 4, 0, FILL) for _ in range(n)])
    outs = [v.view(torch.float32) for v in recvs]
    ss = [0.5] * n

    def refused(code, inputs=sends, outputs=outs, op=m.PREMUL_SUM, **kw):
        with pytest.raises(m.MscclppError) as e:
            ranks.pull_reduce(kw.pop("coll", m.PULL_ALLREDUCE), inputs, outputs, op, **kw)
        assert e.value.code == code, kw

    for coll in C.COLLS:
        refused(4, coll=coll)  # PreMulSum through the entry point without scalars
        for op in (m.SUM, m.MAX, m.AVG, 4):  # the scaled entry point takes nothing else
            refused(4, coll=coll, op=op, scales=ss)
        ints = [t.view(torch.int32) for t in sends]
        refused(4, inputs=ints, outputs=[v.view(torch.int32) for v in recvs], coll=coll, scales=ss)
        # a byte count that splits an element: 1021 bytes taken as fp16
        bytes_in = [t.view(torch.uint8)[:1021 * (n if coll == m.PULL_REDUCE_SCATTER else 1)] for t in sends]
        refused(4, inputs=bytes_in, outputs=[v[:1021] for v in recvs], coll=coll, scales=ss, accum=m.F16)
    torch.cuda.synchronize()
    for w in wholes:
        assert bool((w == FILL).all())
    assert ranks.errors() == [0] * n
    three_calls(n, O.F32, C.ALLREDUCE, count, 990)  # and the ranks still work


# ---- beside the other operations (these two run last) ---------------------------------------------------
def test_avg_on_the_same_ranks_is_still_bit_exact(built):
    """PreMulSum leaves nothing behind that another kernel of the same ranks could read: its slots are
    zero again, and AVG (the same kernel's older operation) gives the reference's bits."""
    import mscclpp_amd as m

    n, count = 8, C.COUNT
    ranks = ranks_of(n)
    for k, (code, coll) in enumerate([(O.F16, C.ALLREDUCE), (O.F32, C.REDUCE_SCATTER), (O.BF16, C.REDUCE)]):
        run_once(ranks, n, code, coll, count, 1000 + k, k, C.scalars(code, n, 1000 + k, "generic"))
        total = count * (n if coll == C.REDUCE_SCATTER else 1)
        xs = P.inputs(code, P.AVG, n, total, 1100 + k)
        ref = P.reference(code, P.AVG, xs)
        x = [torch.from_numpy(a.view(np.uint8).copy()).cuda().view(TORCH[code]) for a in xs]
        y = [torch.zeros(count, dtype=TORCH[code], device="cuda") for _ in range(n)]
        ranks.pull_reduce(coll, x, y, m.AVG, root=k)
        torch.cuda.synchronize()
        assert ranks.errors() == [0] * n, ranks.error_details()
        for r in range(n):
            if coll == C.REDUCE and r != k:
                continue
            want = ref[r * count:(r + 1) * count] if coll == C.REDUCE_SCATTER else ref
            got = y[r].view(torch.uint8).cpu().numpy().view(C.bits_dtype(code))
            off = r * count if coll == C.REDUCE_SCATTER else 0
            assert P.mismatches(code, P.AVG, got, want, True, offset=off).size == 0, (code, coll, r)


def test_zz_token_arrays_equal_their_expected_counters(built):
    """After all the calls of this module (the scalars travel through the token arrays' diagonals and
    every launch zeroes its slots again) every rank's whole token array equals its expected counters."""
    import mscclpp_amd as m

    if not _RANKS:  # selected alone: some calls of its own
        three_calls(8, O.F16, C.ALLREDUCE, C.COUNT, 1200)
    torch.cuda.synchronize()
    for n, ranks in _RANKS.items():
        assert ranks.errors() == [0] * n
        for r in range(n):
            tok = m.device_view(ranks.tokens[r].ptr, ranks.tokens[r].nbytes).view(torch.int64)
            assert torch.equal(tok, ranks.expected[r]), f"n {n} rank {r}: tokens differ from the expected counters"
            assert int(tok.sum()) > 0
            diag = tok.view(m.MAX_RANKS, m.MAX_CHANNELS)[r]
            assert int(diag.abs().sum()) == 0, f"n {n} rank {r}: a scalar slot was left behind"
