"""GPU parity of ReduceScatter (the bulk kernel's MODE 1), AllGather (MODE 2) and Broadcast along the
axes the earlier tests hold fixed (tables, inputs and CPU expectations in collective_edge_cases.py,
proved non-vacuous on the CPU by test_collective_edge_cases.py):

  A  launch shapes: 1 .. 256 workgroups of 64 / 512 lanes, blocks from one 16-byte unit to 64 KiB + 16;
  B  a scratch so small that a block takes 3 .. 5 passes, the last one partial, then in place;
  C  all 15 reduce types x SUM / MIN x fullmesh / rsag order in MODE 1;
  D  guard bands, untouched inputs, element-aligned and 1-byte-aligned views, the NCCL in-place forms;
  E  Broadcast from every root, sizes around one unit, whole sweeps plus a byte tail;
  F  refusals by return code that launch nothing and leave the token counters in step;
  and the in-place, offset-view, odd-offset, refused-block and graph-captured calls through the NCCL
  ABI in two process groups.

Every in-process call places each rank's buffers inside one 0xA5 arena and compares the whole arena
afterwards: the output bit for bit with the oracle (for f32, a lane whose expected value is a NaN must
hold a NaN), every other byte -- guards, inputs, the other slices of an in-place input -- unchanged.
Reducing calls over I32 / U32 and over the `finite` float inputs are judged by the plain numpy / fp64
reference as well, no lane left out.  After every call every error word is 0 and every token counter
(received and expected) holds the number of handshakes made so far on its channel."""
import multiprocessing as mp
import traceback

import numpy as np
import pytest
import torch

import collective_edge_cases as C
import kernel_edge_cases as K
import mp_util
import oracle_lib as O
from test_reduce_gpu import type_table

pytestmark = pytest.mark.gpu

RS, AG, BC = C.RS, C.AG, C.BC


class _Tokens:
    """The handshakes made so far per channel of one InProcessRanks, and the check of its state."""

    def __init__(self, m, ranks):
        self.m, self.ranks = m, ranks
        self.count = np.zeros(K.MAX_CHANNELS, np.int64)

    def ran(self, nblocks, per_workgroup):
        self.count[:nblocks] += per_workgroup

    def snapshot(self):
        ranks = self.ranks
        return [(self.m.device_view(t.ptr, t.nbytes).cpu().numpy().copy(), e.cpu().numpy().copy(), x.cpu().numpy().copy())
                for t, e, x in zip(ranks.tokens, ranks.expected, ranks.err)]

    def check(self):
        ranks, n = self.ranks, self.ranks.n
        assert ranks.errors() == [0] * n, ranks.error_details()
        for r, (tok, exp, _) in enumerate(self.snapshot()):
            want = np.zeros((self.m.MAX_RANKS, K.MAX_CHANNELS), np.int64)
            for p in range(n):
                if p != r:
                    want[p] = self.count
            assert np.array_equal(exp.reshape(want.shape), want), f"rank {r}: expected-token counters out of step"
            assert np.array_equal(tok.view(np.int64).reshape(want.shape), want), f"rank {r}: tokens received out of step"


def _run(m, ranks, tk, coll, algo, code, op, block, cid, call, family="bits", nb=0, nt=0, passes=1, shifts=(0, 0),
         in_place=False, root=0, ins=None):
    """One call with every rank's buffers inside a 0xA5 arena, all checks made.  block: bytes per rank
    (Broadcast: of the buffer).  in_place: ReduceScatter out = in + rank * block, AllGather in = out +
    rank * block, Broadcast send is recv on the root.  Returns the expected outputs (bytes per rank)."""
    n = ranks.n
    tdt, accum = type_table()[code]
    item = O.itemsize(code)
    in_b, out_b = {RS: (n * block, block), AG: (block, n * block), BC: (block, block)}[coll]
    if ins is None:
        ins = C.reduce_inputs(code, op, n, in_b // item, cid, call, family) if coll == RS else \
            [C.bits(code, in_b // item, cid, call, r) for r in range(n)]
    i_off, o_off, total = C.d_layout(in_b, out_b, *shifts)
    in_at, out_at = [i_off] * n, [o_off] * n
    if in_place and coll == RS:
        out_at = [i_off + r * block for r in range(n)]
    elif in_place and coll == AG:
        in_at = [o_off + r * block for r in range(n)]
    elif in_place:
        in_at[root] = o_off
    if coll == RS:
        red = C.rs_expected(code, op, ins, block, C.ORDER[algo])
        exp = [red[r * block:(r + 1) * block] for r in range(n)]
    elif coll == AG:
        exp = [np.concatenate([C.as_bytes(a) for a in ins])] * n
    else:
        exp = [C.as_bytes(ins[root])] * n
    host, image = [], []
    for r in range(n):
        a = np.full(total, C.GUARD, np.uint8)
        a[in_at[r]:in_at[r] + in_b] = C.as_bytes(ins[r])
        host.append(a)
        b = a.copy()
        b[out_at[r]:out_at[r] + out_b] = exp[r]
        image.append(b)
    arenas = [torch.from_numpy(a).cuda() for a in host]
    dins = [arenas[r][in_at[r]:in_at[r] + in_b].view(tdt) for r in range(n)]
    douts = [arenas[r][out_at[r]:out_at[r] + out_b].view(tdt) for r in range(n)]
    if not in_place:
        assert all(t.data_ptr() % 16 == shifts[0] for t in dins) and all(t.data_ptr() % 16 == shifts[1] for t in douts)
    if coll == BC:
        ranks.broadcast(dins, douts, root, nblocks=nb, nthreads=nt)
        tk.ran(C.bcast_grid(block, nb, nt)[0], C.handshakes(BC))
    else:
        ranks.collective(coll, dins, douts, algo=m.ALGO_NAMES[algo], op=op, nblocks=nb, nthreads=nt, accum=accum)
        tk.ran(C.bulk_grid(nb, nt)[0], C.handshakes(coll, passes))
    torch.cuda.synchronize()
    tk.check()
    what = f"{C.COLL_NAMES[coll]} call {call}"
    for r in range(n):
        got = arenas[r].cpu().numpy()
        o = slice(out_at[r], out_at[r] + out_b)
        out = got[o].copy()
        bad = C.mismatches(code if coll == RS else O.U8, out, image[r][o].copy())
        assert bad.size == 0, f"{what} rank {r}: {bad.size} mismatches against the oracle, first {bad[:8]}"
        got[o] = image[r][o]
        bad = np.nonzero(got != image[r])[0]
        assert bad.size == 0, f"{what} rank {r}: {bad.size} bytes outside the output changed, first {bad[:8]}"
        if coll == RS and code in C.PLAIN_TYPES and (code not in C.FLOATS or family == "finite"):
            cnt = block // item
            bad = C.plain_failures(code, op, [a[r * cnt:(r + 1) * cnt] for a in ins], out)
            assert bad.size == 0, f"{what} rank {r}: {bad.size} lanes off the plain reference, first {bad[:8]}"
    return exp


def _group(m, n, bulk=C.A_SCRATCH):
    ranks = m.InProcessRanks(n, 1 << 16, bulk_scratch_bytes=bulk)
    return ranks, _Tokens(m, ranks)


# ---- A: launch shapes ----------------------------------------------------------------------------
@pytest.mark.parametrize("coll,algo,n,nb,nt,picks", C.A_CASES,
                         ids=[f"{C.COLL_NAMES[c[0]]}-{c[1]}-n{c[2]}-{c[3]}x{c[4]}" for c in C.A_CASES])
def test_launch_shapes(built, coll, algo, n, nb, nt, picks):
    """Every block size on one grid, three calls each on one group of ranks (the counters carry over)."""
    import mscclpp_amd as m

    ranks, tk = _group(m, n)
    for block, code, op in picks:
        cid = C.case_id("A", coll, algo, n, nb, nt, block)
        for call, family in enumerate(C.families(code)):
            _run(m, ranks, tk, coll, algo, code, op, block, cid, call, family, nb, nt)


# ---- B: multi-pass ---------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", C.ALGOS)
@pytest.mark.parametrize("n,code,op,block,scratch,nb,nt", C.B_CASES, ids=lambda v: str(v))
def test_multipass_reduce_scatter_then_all_gather(built, algo, n, code, op, block, scratch, nb, nt):
    """3 .. 5 passes with a partial last one, the scratch reused pass after pass: ReduceScatter, then
    AllGather of its result; three calls out of place and one in the NCCL in-place forms."""
    import mscclpp_amd as m

    ranks, tk = _group(m, n, scratch)
    passes = K.bulk_passes(n, n * block, scratch, nb)[1]
    cid = C.case_id("B", algo, n, code, block)
    for call, family in enumerate(C.families(code) + ("bits",)):
        exp = _run(m, ranks, tk, RS, algo, code, op, block, cid, call, family, nb, nt, passes, in_place=call == 3)
        _run(m, ranks, tk, AG, algo, code, op, block, cid, call, None, nb, nt, passes, in_place=call == 3,
             ins=[e.view(C.uint_of(code)) for e in exp])


@pytest.mark.parametrize("coll", [RS, AG])
@pytest.mark.parametrize("algo", C.ALGOS)
def test_scratch_below_one_pass_is_refused(built, coll, algo):
    import mscclpp_amd as m

    n, code, block, scratch, nb, nt = C.B_REFUSED
    ranks, tk = _group(m, n, scratch)
    big = [torch.full((n * block,), C.GUARD, dtype=torch.uint8, device="cuda") for _ in range(n)]
    small = [torch.full((block,), C.GUARD, dtype=torch.uint8, device="cuda") for _ in range(n)]
    ins, outs = (big, small) if coll == RS else (small, big)
    with pytest.raises(m.MscclppError) as e:
        ranks.collective(coll, [t.view(torch.float16) for t in ins], [t.view(torch.float16) for t in outs],
                         algo=m.ALGO_NAMES[algo], nblocks=nb, nthreads=nt)
    assert e.value.code == 5
    torch.cuda.synchronize()
    tk.check()
    assert all(bool((t == C.GUARD).all()) for t in big + small)


# ---- C: every reduce type and op in MODE 1 -------------------------------------------------------------
@pytest.mark.parametrize("code,op,algo,n", C.C_CASES, ids=lambda v: str(v))
def test_every_type_and_op_reduce_scatter(built, code, op, algo, n):
    """The narrow and the wide-accumulator branches of MODE 1 in both sum orders; the float types'
    second call takes the finite inputs and the fp64 reference, a float MIN's bits calls the planted
    NaN / +-0 / +-inf / subnormal groups."""
    import mscclpp_amd as m

    ranks, tk = _group(m, n)
    cid = C.case_id("C", code, op, algo, n)
    for call, family in enumerate(C.families(code)):
        _run(m, ranks, tk, RS, algo, code, op, C.C_BLOCK, cid, call, family, *C.C_GRID)


# ---- D: guards, views and in-place ----------------------------------------------------------------------
@pytest.mark.parametrize("coll,algo,n,code,nbytes,in_shift,out_shift", C.D_CASES,
                         ids=[f"{C.COLL_NAMES[c[0]]}-{c[1]}-n{c[2]}-t{c[3]}-in{c[5]}-out{c[6]}" for c in C.D_CASES])
def test_guards_views_and_in_place(built, coll, algo, n, code, nbytes, in_shift, out_shift):
    """Buffers 16-byte aligned, element-aligned, and (uint8 AllGather / Broadcast) 1-byte aligned on the
    send side, the receive side or both; the fourth call runs in place (at the output's alignment)."""
    import mscclpp_amd as m

    ranks, tk = _group(m, n)
    cid = C.case_id("D", coll, algo, n, code, in_shift, out_shift)
    roots = (0, n // 2, n - 1, 1)
    for call in range(4):
        _run(m, ranks, tk, coll, algo, code, O.SUM, nbytes, cid, call, C.families(code)[call % 3],
             shifts=(in_shift, out_shift), in_place=call == 3, root=roots[call])


# ---- E: Broadcast shapes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nbytes,nb,nt", C.E_CASES, ids=lambda v: str(v))
def test_broadcast_shapes(built, n, nbytes, nb, nt):
    """Every root in turn on one group; receive buffers 0xA5 and guarded, the send buffers of the
    non-roots hold other data and stay as they are."""
    import mscclpp_amd as m

    ranks, tk = _group(m, n)
    cid = C.case_id("E", n, nbytes, nb, nt)
    for root in range(n):
        _run(m, ranks, tk, BC, None, O.U8, O.SUM, nbytes, cid, root, nb=nb, nt=nt, root=root)


# ---- F: refusals launch nothing -------------------------------------------------------------------------------
def test_refusals_launch_nothing(built):
    """After a valid call of each kind: every refused call returns its code and changes no output byte,
    no error word and no token counter; the next valid calls on the same ranks are exact."""
    import mscclpp_amd as m

    n = C.F_N
    ranks, tk = _group(m, n)
    cid = C.case_id("F")
    for call, coll in enumerate((RS, AG, BC)):
        _run(m, ranks, tk, coll, "rsag", O.F32 if coll == RS else O.U8, O.SUM, C.F_BLOCK, cid, call, root=1)
    before = tk.snapshot()
    for what, args, code in C.F_CASES:
        if what == "coll":
            coll, algo, block, nb, nt = args
            in_b, out_b = (n * block, block) if coll == RS else (block, n * block)
            ins = [torch.zeros(in_b, dtype=torch.uint8, device="cuda") for _ in range(n)]
            outs = [torch.full((out_b,), C.GUARD, dtype=torch.uint8, device="cuda") for _ in range(n)]
            with pytest.raises(m.MscclppError) as e:
                ranks.collective(coll, [t.view(torch.float32) for t in ins], [t.view(torch.float32) for t in outs],
                                 algo=m.ALGO_NAMES[algo], nblocks=nb, nthreads=nt)
            assert e.value.code == code, (what, args)
        else:
            root, nbytes = args
            ins = [torch.zeros(C.F_BLOCK, dtype=torch.uint8, device="cuda") for _ in range(n)]
            outs = [torch.full((C.F_BLOCK,), C.GUARD, dtype=torch.uint8, device="cuda") for _ in range(n)]
            arr = ranks.views(ins, outs)
            rc = m.lib().mscclppAmdBroadcastLaunch(arr, n, n, nbytes, root, 0, 0, 500_000_000, m.stream_ptr())
            assert rc == code, (what, args)
        torch.cuda.synchronize()
        assert all(bool((t == C.GUARD).all()) for t in outs) and all(not bool(t.any()) for t in ins), (what, args)
        for r, (a, b) in enumerate(zip(before, tk.snapshot())):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (what, args, r)
    tk.check()
    for call, coll in enumerate((RS, AG, BC)):
        _run(m, ranks, tk, coll, "fullmesh", O.F32 if coll == RS else O.U8, O.SUM, C.F_BLOCK, cid, 3 + call, root=2)


# ---- through the NCCL ABI ------------------------------------------------------------------------------------
def _abi_worker(rank, n, uid, q):
    try:
        import os

        os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "5000")
        import torch

        import mscclpp_amd as m
        import collective_edge_cases as C
        import oracle_lib as O

        import mp_util

        mp_util.place_rank(rank, n)
        comm = m.Communicator(rank, n, uid)
        cid = C.case_id("abi", n)
        B, res = C.ABI_BLOCK, {}
        f16, bf16, f32, u8 = torch.float16, torch.bfloat16, torch.float32, torch.uint8
        mine = slice(rank * B, (rank + 1) * B)

        def dev(a):
            return torch.from_numpy(C.as_bytes(a).copy()).cuda()

        def host(t):
            torch.cuda.synchronize()
            return t.cpu().numpy()

        def arena(nbytes, off):
            whole = torch.full((off + nbytes + 256,), C.GUARD, dtype=u8, device="cuda")
            return whole, whole[off:off + nbytes]

        def image(nbytes, off, content):
            a = np.full(off + nbytes + 256, C.GUARD, np.uint8)
            a[off:off + nbytes] = content
            return a

        def gathered(ins):
            return np.concatenate([C.as_bytes(a) for a in ins])

        # -- AllGather in place: send is recv + rank * bytes (the form FSDP-style callers use)
        ins = [C.bits(O.F16, B // 2, cid, 0, r) for r in range(n)]
        recv = torch.full((n * B,), C.GUARD, dtype=u8, device="cuda")
        recv[mine] = dev(ins[rank])
        comm.all_gather(recv[mine].view(f16), recv.view(f16))
        res["ag_in_place"] = bool(np.array_equal(host(recv), gathered(ins)))

        # -- ReduceScatter in place: recv is send + rank * bytes; the other slices of send stay
        def rs_in_place(code, tdt, op, call, family):
            ins = C.reduce_inputs(code, op, n, n * B // O.itemsize(code), cid, call, family)
            buf = dev(ins[rank])
            comm.reduce_scatter(buf.view(tdt), buf[mine].view(tdt), op="sum" if op == O.SUM else "min")
            want = C.as_bytes(ins[rank]).copy()
            want[mine] = C.rs_expected(code, op, ins, B, 0)[mine]
            got = host(buf)
            ok = C.mismatches(code, got[mine].copy(), want[mine].copy()).size == 0
            got[mine] = want[mine]
            ok = ok and bool(np.array_equal(got, want))
            if family == "finite" or code not in C.FLOATS:
                cnt = B // O.itemsize(code)
                ok = ok and C.plain_failures(code, op, [a[rank * cnt:(rank + 1) * cnt] for a in ins],
                                             host(buf)[mine].copy()).size == 0
            return ok

        res["rs_in_place_bf16_sum"] = rs_in_place(O.BF16, bf16, O.SUM, 1, "bits") and \
            rs_in_place(O.BF16, bf16, O.SUM, 2, "finite")
        res["rs_in_place_f32_min"] = rs_in_place(O.F32, f32, O.MIN, 3, "bits") and \
            rs_in_place(O.F32, f32, O.MIN, 4, "finite")

        # -- the same two out of place on views at a non-zero storage offset, receive buffers guarded
        off = C.ABI_OFFSET
        ins = [C.bits(O.F16, B // 2, cid, 5, r) for r in range(n)]
        sw, s = arena(B, off)
        rw, r_ = arena(n * B, off)
        s.copy_(dev(ins[rank]))
        comm.all_gather(s.view(f16), r_.view(f16))
        res["ag_views"] = bool(np.array_equal(host(rw), image(n * B, off, gathered(ins)))) and \
            bool(np.array_equal(host(sw), image(B, off, C.as_bytes(ins[rank]))))
        ins = C.reduce_inputs(O.BF16, O.SUM, n, n * B // 2, cid, 6, "bits")
        sw, s = arena(n * B, off)
        rw, r_ = arena(B, off)
        s.copy_(dev(ins[rank]))
        comm.reduce_scatter(s.view(bf16), r_.view(bf16))
        res["rs_views"] = bool(np.array_equal(host(rw), image(B, off, C.rs_expected(O.BF16, O.SUM, ins, B, 0)[mine]))) and \
            bool(np.array_equal(host(sw), image(n * B, off, C.as_bytes(ins[rank]))))

        # -- uint8 views at an odd byte offset: Broadcast (a byte tail too) and AllGather
        odd, nb, root = C.ABI_ODD, C.D_BCAST, n - 1
        ins = [C.bits(O.U8, nb, cid, 7, r) for r in range(n)]
        sw, s = arena(nb, odd)
        rw, r_ = arena(nb, odd)
        s.copy_(dev(ins[rank]))
        comm.broadcast(s, r_, root=root)
        res["bcast_odd"] = bool(np.array_equal(host(rw), image(nb, odd, ins[root]))) and \
            bool(np.array_equal(host(sw), image(nb, odd, ins[rank])))
        ins = [C.bits(O.U8, B, cid, 8, r) for r in range(n)]
        sw, s = arena(B, odd)
        rw, r_ = arena(n * B, odd)
        s.copy_(dev(ins[rank]))
        comm.all_gather(s, r_)
        res["ag_odd"] = bool(np.array_equal(host(rw), image(n * B, odd, gathered(ins)))) and \
            bool(np.array_equal(host(sw), image(B, odd, ins[rank])))

        # -- a per-rank block of 8 bytes: ncclInvalidUsage on every rank, nothing launched
        small = C.ABI_SMALL
        s = torch.zeros(small, dtype=u8, device="cuda")
        big = torch.full((n * small,), C.GUARD, dtype=u8, device="cuda")
        for key, call in (("small_ag_refused", lambda: comm.all_gather(s.view(f16), big.view(f16))),
                          ("small_rs_refused", lambda: comm.reduce_scatter(big.view(f16), s.view(f16)))):
            try:
                call()
                res[key] = False
            except m.MscclppError as e:
                res[key] = e.code == 5
            res[key] = res[key] and bool((host(big) == C.GUARD).all()) and not bool(host(s).any())
        # ... and the token channels are still in step: the next valid calls are exact
        ins = C.reduce_inputs(O.F32, O.SUM, n, n * B // 4, cid, 9, "finite")
        x, y = dev(ins[rank]), torch.full((B,), C.GUARD, dtype=u8, device="cuda")
        comm.reduce_scatter(x.view(f32), y.view(f32))
        exp = C.rs_expected(O.F32, O.SUM, ins, B, 0)
        cnt = B // 4
        res["rs_after_refusal"] = bool(np.array_equal(host(y), exp[mine])) and \
            C.plain_failures(O.F32, O.SUM, [a[rank * cnt:(rank + 1) * cnt] for a in ins], host(y)).size == 0
        z = torch.full((n * B,), C.GUARD, dtype=u8, device="cuda")
        comm.all_gather(y.view(f32), z.view(f32))
        res["ag_after_refusal"] = bool(np.array_equal(host(z), exp))
        z.fill_(C.GUARD)
        comm.all_reduce(x.view(f32), z.view(f32), algo="fullmesh")
        res["ar_after_refusal"] = bool(np.array_equal(host(z), exp))  # n * B bytes: the slices are the blocks

        # -- AllGather in place, captured and replayed on new data (registered by one eager call first)
        recv = torch.full((n * B,), C.GUARD, dtype=u8, device="cuda")
        comm.all_gather(recv[mine].view(f16), recv.view(f16))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            comm.all_gather(recv[mine].view(f16), recv.view(f16))
        torch.cuda.synchronize()
        ok = True
        for k in range(C.ABI_REPLAYS):
            ins = [C.bits(O.F16, B // 2, cid, 10 + k, r) for r in range(n)]
            recv.fill_(C.GUARD)
            recv[mine] = dev(ins[rank])
            torch.cuda.synchronize()
            comm.barrier()  # every rank's buffer is set before any peer's replay writes into it
            g.replay()
            ok = ok and bool(np.array_equal(host(recv), gathered(ins)))
            comm.barrier()
        res["graph_ag_in_place"] = ok
        del g
        res["device_error"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("n", C.ABI_RANKS)
def test_nccl_abi_in_place_views_and_refusals(built, n):
    import mscclpp_amd as m

    uid = m.Communicator.unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_abi_worker, args=(r, n, uid, q)) for r in range(n)]
    for p in procs:
        p.start()
    got = mp_util.collect(procs, q, n, 240)
    for rank in range(n):
        assert got[rank]["device_error"] == 0, (rank, got[rank])
        failed = [k for k in C.ABI_CHECKS if got[rank].get(k) is not True]
        assert not failed, (rank, failed)
