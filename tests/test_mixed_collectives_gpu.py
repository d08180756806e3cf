"""Every native collective against every other on one communicator.  The kernels of AllReduce,
ReduceScatter, AllGather, Broadcast, Reduce, AllToAll(v), Send / Recv and the pull-reduce of ncclMax /
ncclAvg, int64 / int8 and PreMulSum share the token counters of kernels/handshake.hpp, and the small
calls of the latter take the LL kernel (kernels/pull_reduce_ll.hip) on the shared flags and LL scratch;
each was mixed only with a fixed sequence of its own.  Here a seeded shuffle runs all of them back to
back.  The pull-reduce entries are the rows of abi_path_cases.MIXED / inprocess_rows, each with the
kernel it means to run: `*_ll` entries are below the built-in cutover, `*_pull` entries one element above
it, a Reduce always takes the pull kernel, and across processes every rank's pull_ll_count() must end
at the number of LL entries x ROUNDS:

  1  across processes (3 and 8 ranks, one per process): two rounds of every entry point, each entry on
     buffers of its own that are built before the first call, no synchronisation between calls, one
     rank (rotating) launching 20 ms late before every third call.  After the stream drains, byte moves
     are compared with what every rank can recompute, SUM reductions with the oracle of the algorithm
     that ran, MAX / AVG / int64 / int8 / PreMulSum with the references behind
     pull_reduce_ll_cases.reference; receive buffers carry 0xA5 guards.  A PreMulSum handle is created
     before the first call and destroyed right after its own call is issued.
  2  in process (InProcessRanks, 3 and 8 ranks): every launcher the class has, each on two grids, so
     the channel counts differ from launch to launch -- pull_reduce_ll (int64; PreMulSum with device
     scalars), the scaled pull_reduce of every collective (its scalars cross the token diagonal, which
     a later handshake kernel must find zeroed) and an int8 pull_reduce among them; one synchronisation
     at the end, then every result is exact, every error word 0 and every rank's received tokens equal
     its expected ones.

With one GPU the process ranks share it."""
import multiprocessing as mp
import random
import traceback

import numpy as np
import pytest
import torch

import abi_path_cases as T
import mp_util

pytestmark = pytest.mark.gpu

GUARD = 256
COUNT = 4099              # elements of the byte moves: odd, no multiple of a 16-byte unit
ROUNDS = 2
ENTRIES = ("ar_4k", "ar_256k", "ar_1m", "rs_sum", "ag", "bcast", "reduce_sum", "a2a", "a2av", "ring", "pair") + \
    tuple(row.key for row in T.MIXED)  # ... and ar_max_ll, rs_avg_ll, reduce_max, ar_max_pull, ..., reduce_i8_min
LL_ENTRIES = tuple(row.key for row in T.MIXED if row.ll_at)  # the rows whose written-out path is "ll": the *_ll entries
AR_BYTES = {"ar_4k": 4 << 10, "ar_256k": 256 << 10, "ar_1m": (1 << 20) + 16}


def _sequence():
    seq = [(name, rnd) for rnd in range(ROUNDS) for name in ENTRIES]
    random.Random(4321).shuffle(seq)
    return seq


def a2av_counts(n):
    """counts[s][d]: elements rank s sends to rank d -- uneven, and a zero from every rank to its successor."""
    return [[0 if d == (s + 1) % n else 1 + (7 * s + 13 * d) % 5 * 811 for d in range(n)] for s in range(n)]


def _worker(rank, n, uid, q):
    try:
        import os
        import time

        os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "8000")
        os.environ.pop("MSCCLPP_AMD_TUNED_CONFIG", None)
        os.environ.pop("MSCCLPP_AMD_ALGO", None)
        import torch

        import mscclpp_amd as m
        import abi_path_cases as T
        import allreduce_abi_cases as A
        import collective_edge_cases as C
        import int_reduce_cases as I
        import oracle_lib as O
        import premul_sum_cases as S
        import pull_reduce_cases as P
        import pull_reduce_ll_cases as LC

        import mp_util

        mp_util.place_rank(rank, n)
        comm = m.Communicator(rank, n, uid)
        L = m.lib()
        tdt = {O.F16: torch.float16, O.BF16: torch.bfloat16, O.F32: torch.float32, O.I32: torch.int32, O.U8: torch.uint8,
               I.I64: torch.int64, I.I8: torch.int8}
        B = C.ABI_BLOCK       # ReduceScatter / AllGather blocks are whole 16-byte units

        # (AllToAllv's buffers have rank-dependent sizes, so torch's caching allocator groups the entries'
        # buffers into allocations differently per rank: registration must not depend on the grouping)
        def dev(a, code):
            return torch.from_numpy(C.as_bytes(a).copy()).cuda().view(tdt[code])

        class Recv:
            """A receive buffer of `nbytes` inside a 0xA5 allocation."""

            def __init__(self, nbytes, code):
                self.nbytes = nbytes
                self.whole = torch.full((nbytes + 2 * GUARD,), C.GUARD, dtype=torch.uint8, device="cuda")
                self.buf = self.whole[GUARD:GUARD + nbytes].view(tdt[code])

            def wrong(self, want, judge=None):
                """Wrong bytes: the buffer against `want` (None: untouched) plus changed guard bytes."""
                got = self.whole.cpu().numpy()
                body = got[GUARD:GUARD + self.nbytes]
                if want is None:
                    want = np.full(self.nbytes, C.GUARD, np.uint8)
                bad = int(np.count_nonzero(body != C.as_bytes(want))) if judge is None else judge(body.copy())
                return bad + int(np.count_nonzero(got[:GUARD] != C.GUARD)) + int(np.count_nonzero(got[GUARD + self.nbytes:] != C.GUARD))

        def build(name, rnd, i):
            """(issue, check) of one entry: its buffers and inputs are made here, before the first call."""
            cid = C.case_id("mixed", n, name, rnd)
            root = i % n
            if name in AR_BYTES:
                nb = AR_BYTES[name]
                ins = C.reduce_inputs(O.F16, O.SUM, n, nb // 2, cid, 0, "bits")
                x, y = dev(ins[rank], O.F16), Recv(nb, O.F16)
                exp = A.oracle_outputs(L, A.selected(L, n, nb, O.F16), O.F16, O.SUM, ins, nb)[rank]
                return (lambda: comm.all_reduce(x, y.buf)), (lambda: y.wrong(exp))
            if name in T.MIXED_FIRST:
                code, op = (O.F16, P.AVG) if name == "rs_avg_ll" else (O.F32, P.MAX)
                total = COUNT * (n if name == "rs_avg_ll" else 1)
                xs = P.inputs(code, op, n, total, cid % 100000)
                ref = P.reference(code, op, xs)
                x, y = dev(xs[rank], code), Recv(COUNT * O.itemsize(code), code)
                off = rank * COUNT if name == "rs_avg_ll" else 0
                want = ref[off:off + COUNT]

                def judge(body):
                    return int(P.mismatches(code, op, body.view(P.bits_dtype(code)), want, True, off).size)

                if name == "ar_max_ll":
                    return (lambda: comm.all_reduce(x, y.buf, op="max")), (lambda: y.wrong(want, judge))
                if name == "rs_avg_ll":
                    return (lambda: comm.reduce_scatter(x, y.buf, op="avg")), (lambda: y.wrong(want, judge))
                return (lambda: comm.reduce(x, y.buf if rank == root else None, root=root, op="max")), \
                    (lambda: y.wrong(want, judge) if rank == root else y.wrong(None))
            if name in T.MIXED_BY_NAME:  # the newer pull-reduce entries: a row of abi_path_cases.MIXED
                row = T.MIXED_BY_NAME[name]
                lrow, code, count = T.ll_row(row), row.code, T.count_of(row, n)
                total = count * (n if row.coll == T.REDUCE_SCATTER else 1)
                xs, ss = T.make_case(row, n, total, cid % 100000)
                ref = LC.reference(lrow, xs, ss)
                x, y = dev(xs[rank], code), Recv(count * T.itemsize(row), code)
                off = rank * count if row.coll == T.REDUCE_SCATTER else 0
                want = ref[off:off + count]

                def judge(body):
                    return int(LC.mismatches(lrow, body.view(LC.bits_dtype(lrow)), want).size)

                op, factor = LC.OP_NAMES[row.op], None
                if row.family == "premul":  # the handle exists before the first call of the sequence
                    if row.scalar == "dev":
                        factor = dev(S.scalar_bits(code, [ss[rank]]), code)
                    op = comm.create_premul_sum(float(ss[rank]) if factor is None else factor, tdt[code])

                def issue(factor=factor):  # (a device scalar lives as long as its entry: the kernel reads it when it runs)
                    if row.coll == T.ALLREDUCE:
                        comm.all_reduce(x, y.buf, op=op)
                    elif row.coll == T.REDUCE_SCATTER:
                        comm.reduce_scatter(x, y.buf, op=op)
                    else:
                        comm.reduce(x, y.buf if rank == root else None, root=root, op=op)
                    if row.family == "premul":
                        comm.destroy_op(op)  # right after its own call is issued: the stream has not run it yet

                receives = row.coll != T.REDUCE or rank == root
                return issue, (lambda: y.wrong(want, judge) if receives else y.wrong(None))
            if name == "rs_sum":
                ins = C.reduce_inputs(O.F32, O.SUM, n, n * B // 4, cid, 0, "bits")
                x, y = dev(ins[rank], O.F32), Recv(B, O.F32)
                exp = C.rs_expected(O.F32, O.SUM, ins, B, 0)[rank * B:(rank + 1) * B]
                return (lambda: comm.reduce_scatter(x, y.buf)), \
                    (lambda: y.wrong(exp, lambda body: int(C.mismatches(O.F32, body, exp.copy()).size)))
            if name == "reduce_sum":
                ins = C.reduce_inputs(O.F32, O.SUM, n, COUNT, cid, 0, "bits")
                x, y = dev(ins[rank], O.F32), Recv(COUNT * 4, O.F32)
                exp = O.reduce_seq(O.F32, O.SUM, [ins[(root + k) % n] for k in range(n)]).view(np.uint8)
                return (lambda: comm.reduce(x, y.buf if rank == root else None, root=root)), \
                    (lambda: y.wrong(exp, lambda body: int(C.mismatches(O.F32, body, exp.copy()).size)) if rank == root
                     else y.wrong(None))
            if name == "ag":
                ins = [C.bits(O.U8, B, cid, 0, r) for r in range(n)]
                x, y = dev(ins[rank], O.U8), Recv(n * B, O.U8)
                return (lambda: comm.all_gather(x, y.buf)), (lambda: y.wrong(np.concatenate(ins)))
            if name == "bcast":
                ins = [C.bits(O.F16, COUNT, cid, 0, r) for r in range(n)]
                x, y = dev(ins[rank], O.F16), Recv(COUNT * 2, O.F16)
                return (lambda: comm.broadcast(x, y.buf, root=root)), (lambda: y.wrong(ins[root]))
            if name == "a2a":
                ins = [C.bits(O.I32, n * COUNT, cid, 0, r) for r in range(n)]
                x, y = dev(ins[rank], O.I32), Recv(n * COUNT * 4, O.I32)
                want = np.concatenate([ins[p][rank * COUNT:(rank + 1) * COUNT] for p in range(n)])
                return (lambda: comm.all_to_all(x, y.buf)), (lambda: y.wrong(want))
            if name == "a2av":
                cnt = a2av_counts(n)
                sdis = [[sum(cnt[s][:d]) for d in range(n)] for s in range(n)]
                rcnt = [cnt[p][rank] for p in range(n)]
                rdis = [sum(rcnt[:p]) for p in range(n)]
                ins = [C.bits(O.I32, sum(cnt[r]), cid, 0, r) for r in range(n)]
                x, y = dev(ins[rank], O.I32), Recv(sum(rcnt) * 4, O.I32)
                want = np.concatenate([ins[p][sdis[p][rank]:sdis[p][rank] + cnt[p][rank]] for p in range(n)])
                return (lambda: comm.all_to_all_v(x, cnt[rank], sdis[rank], y.buf, rcnt, rdis)), (lambda: y.wrong(want))
            ins = [C.bits(O.F16, COUNT, cid, 0, r) for r in range(n)]
            x, y = dev(ins[rank], O.F16), Recv(COUNT * 2, O.F16)
            if name == "ring":
                def ring():
                    with comm.group():
                        comm.send(x, (rank + 1) % n)
                        comm.recv(y.buf, (rank - 1) % n)

                return ring, (lambda: y.wrong(ins[(rank - 1) % n]))
            assert name == "pair"
            peer = {0: n - 1, n - 1: 0}.get(rank)

            def pair():  # ungrouped: send first on rank 0, receive first on rank n - 1
                if rank == 0:
                    comm.send(x, peer)
                    comm.recv(y.buf, peer)
                elif rank == n - 1:
                    comm.recv(y.buf, peer)
                    comm.send(x, peer)

            return pair, (lambda: y.wrong(None if peer is None else ins[peer]))

        seq = _sequence()
        built = [build(name, rnd, i) for i, (name, rnd) in enumerate(seq)]
        torch.cuda.synchronize()
        comm.barrier()
        for i, (issue, _) in enumerate(built):
            if i % 3 == 1 and rank == i % n:
                time.sleep(0.02)  # this rank launches late: its peers run ahead by a call
            issue()
        torch.cuda.synchronize()
        bad = [(i, seq[i][0], seq[i][1], wrong) for i, (_, check) in enumerate(built) for wrong in [check()] if wrong]
        err = comm.device_error()
        took_ll = comm.pull_ll_count()
        comm.barrier()
        comm.destroy()
        q.put((rank, (bad, err, took_ll), None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("n", [3, 8])
def test_every_collective_back_to_back_across_processes(built, n):
    import mscclpp_amd as m

    assert 0 in [c for row in a2av_counts(n) for c in row] and len({c for row in a2av_counts(n) for c in row}) > 2
    uid = m.Communicator.unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, n, uid, q)) for r in range(n)]
    for p in procs:
        p.start()
    got = mp_util.collect(procs, q, n, 240)
    assert LL_ENTRIES == tuple(row.key for row in T.MIXED if T.declared(row, n, T.LL) == T.LL)
    for rank in range(n):
        bad, err, took_ll = got[rank]
        assert err == 0, (rank, err, bad)
        assert bad == [], (rank, bad)  # (call index, entry, round, wrong bytes)
        # the communicator's own account: the entries the table marks as LL took the LL kernel, no other did
        assert took_ll == len(LL_ENTRIES) * ROUNDS, (rank, took_ll)


# ---- in process ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8])
def test_every_launcher_back_to_back_in_process(built, n):
    import mscclpp_amd as m
    import collective_edge_cases as C
    import int_reduce_cases as I
    import kernel_edge_cases as K
    import oracle_lib as O
    import premul_sum_cases as S
    import pull_reduce_cases as P
    import pull_reduce_ll_cases as LC

    f16, f32, u8 = torch.float16, torch.float32, torch.uint8
    count = 1001                                   # f16: ragged slices, a tail below one 16-byte unit
    block = C.D_BLOCK                              # ReduceScatter / AllGather: 65 units per rank
    ll = max(m.scratch_required(m.ALGO_NAMES[a], n, count * 2, O.F16) for a in K.LL_ALGOS)
    grids = ((3, 64), (5, 256))
    assert count == T.INPROCESS_COUNT and n in T.INPROCESS_RANKS
    pull_ll = max(m.pull_reduce_ll_scratch_required(row.coll, n, count * T.itemsize(row), row.code, row.op)
                  for gi in range(len(grids)) for row in T.inprocess_rows(gi) if row.part == "ll")
    assert pull_ll > 0
    ranks = m.InProcessRanks(n, max(ll, 1 << 16, pull_ll), bulk_scratch_bytes=4 << 20)
    types = {O.F16: f16, O.BF16: torch.bfloat16, O.F32: f32, I.I64: torch.int64, I.I8: torch.int8}

    # judges of one rank's result bytes against the expected ones: (rank, got, want) -> wrong indices
    def as_bytes(r, got, want):
        return C.mismatches(O.U8, got, want)

    def as_f32(r, got, want):  # a lane whose expected value is a NaN may hold any NaN
        return C.mismatches(O.F32, got, want)

    def as_pull(op, block_count):  # pull_reduce_cases' rule; block_count: elements per ReduceScatter block, else 0
        return lambda r, got, want: P.mismatches(O.F32, op, got.view(np.uint32), want.view(np.uint32), True, r * block_count)

    def dev(arrs, dtype):
        return [torch.from_numpy(C.as_bytes(a).copy()).cuda().view(dtype) for a in arrs]

    def outs(nbytes, dtype):
        return [torch.full((nbytes,), C.GUARD, dtype=u8, device="cuda").view(dtype) for _ in range(n)]

    def launches():
        for gi, (nb, nt) in enumerate(grids):
            for algo in K.ALGOS + ("rsag_pipeline",):
                cid = C.case_id("mixed-inprocess", n, algo, gi)
                ins = C.reduce_inputs(O.F16, O.SUM, n, count, cid, 0, "bits")
                if algo == "rsag_pipeline":
                    g = (2 * (gi + 1), nt)
                    exp = [K.pipeline_expected(O.F16, O.SUM, ins, count * 2, n, *g).view(np.uint8)[:count * 2]] * n
                else:
                    g = ((gi + 1) * (n - 1), nt) if algo == "packet" else (nb, nt)
                    exp = K.expected(algo, O.F16, O.SUM, ins, count)[0]
                x, y = dev(ins, f16), outs(count * 2, f16)
                yield (f"all_reduce {algo} {g}", lambda x=x, y=y, algo=algo, g=g: ranks.all_reduce(
                    x, y, m.ALGO_NAMES[algo], nblocks=g[0], nthreads=g[1]), y, exp, as_bytes)
            for coll, algo in ((C.RS, "fullmesh"), (C.RS, "rsag"), (C.AG, "fullmesh"), (C.AG, "rsag")):
                cid = C.case_id("mixed-inprocess", n, coll, algo, gi)
                if coll == C.RS:
                    ins = C.reduce_inputs(O.F32, O.SUM, n, n * block // 4, cid, 0, "bits")
                    red = C.rs_expected(O.F32, O.SUM, ins, block, C.ORDER[algo])
                    x, y, exp = dev(ins, f32), outs(block, f32), [red[r * block:(r + 1) * block] for r in range(n)]
                else:
                    ins = [C.bits(O.U8, block, cid, 0, r) for r in range(n)]
                    x, y, exp = dev(ins, u8), outs(n * block, u8), [np.concatenate(ins)] * n
                yield (f"{C.COLL_NAMES[coll]} {algo} {nb}x{nt}", lambda x=x, y=y, coll=coll, algo=algo, nb=nb, nt=nt: ranks.collective(
                    coll, x, y, algo=m.ALGO_NAMES[algo], nblocks=nb, nthreads=nt), y, exp, as_f32 if coll == C.RS else as_bytes)
            cid = C.case_id("mixed-inprocess", n, "moves", gi)
            root = (gi + 1) % n
            ins = [C.bits(O.U8, C.D_BCAST, cid, 0, r) for r in range(n)]
            x, y = dev(ins, u8), outs(C.D_BCAST, u8)
            yield (f"broadcast {nb}x{nt}", lambda x=x, y=y, root=root, nb=nb, nt=nt: ranks.broadcast(x, y, root, nblocks=nb, nthreads=nt),
                   y, [ins[root]] * n, as_bytes)
            blk = 1001
            ins = [C.bits(O.U8, n * blk, cid, 1, r) for r in range(n)]
            x, y = dev(ins, u8), outs(n * blk, u8)
            yield (f"all_to_all {nb}x{nt}", lambda x=x, y=y, nb=nb, nt=nt: ranks.all_to_all(x, y, nblocks=nb, nthreads=nt), y,
                   [np.concatenate([ins[p][r * blk:(r + 1) * blk] for p in range(n)]) for r in range(n)], as_bytes)
            ins = C.reduce_inputs(O.F32, O.SUM, n, count, cid, 2, "bits")
            x, y = dev(ins, f32), outs(count * 4, f32)
            exp = [None] * n
            exp[root] = O.reduce_seq(O.F32, O.SUM, [ins[(root + k) % n] for k in range(n)]).view(np.uint8)
            yield (f"reduce {nb}x{nt}", lambda x=x, y=y, root=root, nb=nb, nt=nt: ranks.reduce(x, y, root, nblocks=nb, nthreads=nt), y, exp, as_f32)
            for coll in P.COLLS:
                op = (P.MAX, P.AVG)[(coll + gi) % 2]
                total = count * (n if coll == P.REDUCE_SCATTER else 1)
                xs = P.inputs(O.F32, op, n, total, 500 + 10 * gi + coll)
                ref = C.as_bytes(P.reference(O.F32, op, xs))
                x, y = dev(xs, f32), outs(count * 4, f32)
                if coll == P.REDUCE:
                    exp = [ref if r == root else None for r in range(n)]
                elif coll == P.REDUCE_SCATTER:
                    exp = [ref[r * count * 4:(r + 1) * count * 4] for r in range(n)]
                else:
                    exp = [ref] * n
                yield (f"pull_reduce {coll} op {op} {nb}x{nt}", lambda x=x, y=y, coll=coll, op=op, root=root, nb=nb, nt=nt: ranks.pull_reduce(
                    coll, x, y, op, root=root, nblocks=nb, nthreads=nt), y, exp,
                    as_pull(op, count if coll == P.REDUCE_SCATTER else 0))
            # the LL launcher (int64; PreMulSum with device scalars), the scaled pull launch of every
            # collective and an int8 pull launch: the rows of abi_path_cases.inprocess_rows
            for k, row in enumerate(T.inprocess_rows(gi)):
                lrow, dt = T.ll_row(row), types[row.code]
                total = count * (n if row.coll == T.REDUCE_SCATTER else 1)
                xs, ss = T.make_case(row, n, total, 600 + 10 * gi + k)
                ref = C.as_bytes(LC.reference(lrow, xs, ss))
                size = count * T.itemsize(row)
                x, y = dev(xs, dt), outs(size, dt)
                if row.coll == T.REDUCE:
                    exp = [ref if r == root else None for r in range(n)]
                elif row.coll == T.REDUCE_SCATTER:
                    exp = [ref[r * size:(r + 1) * size] for r in range(n)]
                else:
                    exp = [ref] * n
                kw = {}
                if row.scalar == "imm":
                    kw = dict(scales=[float(v) for v in ss])
                elif row.scalar == "dev":  # an immediate that must lose against its rank's pointer
                    kw = dict(scales=[123.0] * n, scale_tensors=dev([S.scalar_bits(row.code, [v]) for v in ss], dt))
                if row.part == "ll":
                    def launch(x=x, y=y, row=row, kw=kw, nb=nb, nt=nt):
                        ranks.pull_reduce_ll(row.coll, x, y, row.op, nblocks=nb, nthreads=nt, **kw)
                else:
                    def launch(x=x, y=y, row=row, kw=kw, root=root, nb=nb, nt=nt):
                        ranks.pull_reduce(row.coll, x, y, row.op, root=root, nblocks=nb, nthreads=nt, **kw)
                bits = LC.bits_dtype(lrow)
                yield (f"{row.part} {row.key} coll {row.coll} {nb}x{nt}", launch, y, exp,
                       lambda r, got, want, lrow=lrow, bits=bits: LC.mismatches(lrow, got.view(bits), want.view(bits)))
            ins = [C.bits(O.U8, C.D_BCAST, cid, 3, r) for r in range(n)]
            x, y = dev(ins, u8), outs(C.D_BCAST, u8)
            yield (f"send_recv ring {nb}x{nt}", lambda x=x, y=y, nb=nb, nt=nt: ranks.send_recv(
                [(r, (r + 1) % n, x[r], y[(r + 1) % n]) for r in range(n)], nblocks=nb, nthreads=nt), y,
                [ins[(r - 1) % n] for r in range(n)], as_bytes)

    todo = list(launches())
    new = 2 + len(P.COLLS) + 1  # pull_reduce_ll x 2, the scaled pull_reduce of every collective, an int8 pull_reduce
    assert [len(T.inprocess_rows(gi)) for gi in range(len(grids))] == [new] * len(grids)
    assert len({label for label, *_ in todo}) == len(todo) == 2 * (len(K.ALGOS) + 1 + 4 + 3 + len(P.COLLS) + 1 + new)
    random.Random(97 + n).shuffle(todo)
    torch.cuda.synchronize()
    for label, launch, y, exp, judge in todo:
        launch()
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    for r in range(n):
        tok = m.device_view(ranks.tokens[r].ptr, ranks.tokens[r].nbytes).view(torch.int64)
        assert torch.equal(tok, ranks.expected[r]), f"rank {r}: tokens received differ from the expected counters"
        assert int(tok.sum()) > 0
    for label, _, y, exp, judge in todo:
        for r in range(n):
            got = y[r].view(u8).cpu().numpy()
            if exp[r] is None:  # a rank the collective gives no result: its buffer is untouched
                bad = np.nonzero(got != C.GUARD)[0]
            else:
                bad = judge(r, got, np.ascontiguousarray(exp[r]))
            assert bad.size == 0, f"{label} rank {r}: {bad.size} mismatches, first {bad[:8]}"
