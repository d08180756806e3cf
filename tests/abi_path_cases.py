"""Which kernel every MAX / AVG / int64 / uint64 / int8 / PreMulSum call of the multi-process ABI tests
means to run (a helper, not collected): the row tables of test_pull_reduce_multiprocess_gpu,
test_int_reduce_multiprocess_gpu, test_premul_sum_multiprocess_gpu and of both halves of
test_mixed_collectives_gpu, each row with its DECLARED path, and the check of a call against the
communicator's own account (pull_ll_count(), registration_exchanges()).

A path is "ll" (pullReduceLLKernel, kernels/pull_reduce_ll.hip) or "pull" (pullReduceKernel,
kernels/pull_reduce.hip).  Every file runs its rows in two modes: "ll" is the default environment, where
a row takes LL at the rank counts written in its ll_at; "pull" sets MSCCLPP_AMD_PULL_LL_MAX_BYTES=0 before
the library is imported, and every row takes the pull kernel.  ll_at is written out per row -- it is not
asked of pull_reduce_takes_ll when the tests run; test_abi_path_cases compares the two on the CPU, so a
change of the dispatch rule fails there and in the GPU tests' path assertions, not silently.

Rows "at" and "above" the cutover (default environment only) have a count that follows the rank count:
the largest element count pull_reduce_ll_cases.BUILTIN_MAX sends to LL, and one element more -- the
smallest size at which the default dispatch reaches the pull kernel."""
import os
from collections import namedtuple

import numpy as np

import int_reduce_cases as I
import oracle_lib as O
import premul_sum_cases as S
import pull_reduce_cases as P
import pull_reduce_ll_cases as C

LL, PULL = "ll", "pull"
MODES = (LL, PULL)
VARIABLE = "MSCCLPP_AMD_PULL_LL_MAX_BYTES"
REDUCE, REDUCE_SCATTER, ALLREDUCE = C.REDUCE, C.REDUCE_SCATTER, C.ALLREDUCE
GUARD, FILL = 64, 0xA5

# ll_at: the rank counts at which the default rule sends the row to LL
EVERY = (2, 3, 4, 8)
UP_TO_4 = (2, 3, 4)
NEVER = ()

# part: the section of its file a row belongs to; key: the result (or entry) the row is judged under;
# count: elements of the message (Reduce, AllReduce) or of the per-rank block (ReduceScatter) -- a number,
# ("share", k): k // n, ("times", k): k * n, ("cutover", d): d elements above the built-in cutover of
# (coll, n); scalar: "imm" / "dev" for PreMulSum, else None
Row = namedtuple("Row", "part key coll family code op count inplace scalar ll_at")


def ll_row(row):
    """The (family, dtype code, op) row of pull_reduce_ll_cases."""
    return (row.family, row.code, row.op)


def itemsize(row):
    return C.itemsize(ll_row(row))


def count_of(row, n):
    if isinstance(row.count, tuple):
        kind, k = row.count
        if kind == "share":
            return k // n
        if kind == "times":
            return k * n
        assert kind == "cutover"
        return C.BUILTIN_MAX[(row.coll, C.measured_ranks(n))] // itemsize(row) + k
    return row.count


def nbytes_of(row, n):
    """What the dispatch rule sees: bytes of the message, or of a ReduceScatter's per-rank block."""
    return count_of(row, n) * itemsize(row)


def declared(row, n, mode):
    """The path the row means to take with n ranks in that mode."""
    assert mode in MODES
    if mode == PULL or row.coll == REDUCE:
        return PULL
    return LL if n in row.ll_at else PULL


def set_mode(mode):
    """The environment of a mode; before the library is imported (it reads the variable once)."""
    os.environ.pop(VARIABLE, None)
    if mode == PULL:
        os.environ[VARIABLE] = "0"


def part(table, name, **where):
    return [row for row in table if row.part == name and all(getattr(row, k) == v for k, v in where.items())]


# ---- the communicator's account ----------------------------------------------------------------------
class Account:
    """Reads pull_ll_count() and registration_exchanges()[:2] around every call.  "ll": the count rises
    by one and no exchange happens.  "pull": the count stays, and every pointer the communicator has not
    been given on this path before (the send buffer; an AllReduce's receive buffer when it is another
    one) costs exactly one pointer exchange and at most one new allocation; pointers seen before cost
    nothing.  What disagrees is listed in `wrong`."""

    def __init__(self, comm, n, mode):
        self.comm, self.n, self.mode = comm, n, mode
        self.seen, self.wrong, self.keep, self.calls = set(), [], [], {LL: 0, PULL: 0}

    def call(self, row, fn, send_ptr, recv_ptr=None):
        path = declared(row, self.n, self.mode)
        ptrs = {send_ptr}
        if row.coll == ALLREDUCE and recv_ptr is not None:
            ptrs.add(recv_ptr)
        comm = self.comm
        count0, reg0 = comm.pull_ll_count(), comm.registration_exchanges()[:2]
        out = fn()
        count1, reg1 = comm.pull_ll_count(), comm.registration_exchanges()[:2]
        if path == LL:
            ok = count1 == count0 + 1 and reg1 == reg0
        else:  # one exchange per pointer not seen before, none for the others
            fresh = len(ptrs - self.seen)
            self.seen |= ptrs
            ok = count1 == count0 and reg1[1] == reg0[1] + fresh and reg0[0] <= reg1[0] <= reg0[0] + fresh
        self.calls[path] += 1
        if not ok:
            self.wrong.append((row.part, row.key, row.coll, path, count1 - count0, reg0, reg1))
        return out


def run_fresh(torch, comm, rank, account, row, seed):
    """One AllReduce / ReduceScatter of `row` through the Communicator methods on tensors of its own inside
    0xA5 allocations (kept alive: no address comes back), under the account; True when this rank's
    result, its send buffer and every guard byte are right."""
    n = account.n
    lrow = ll_row(row)
    tdt = {O.F16: torch.float16, O.BF16: torch.bfloat16, O.F32: torch.float32, O.I32: torch.int32,
           I.I64: torch.int64, I.I8: torch.int8}[row.code]
    es, count = itemsize(row), count_of(row, n)
    total = count * (n if row.coll == REDUCE_SCATTER else 1)
    xs, ss = make_case(row, n, total, seed)
    ref = C.reference(lrow, xs, ss)
    mine = slice(rank * count, (rank + 1) * count) if row.coll == REDUCE_SCATTER else slice(None)
    swhole = torch.full((total * es + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    send = swhole[GUARD:GUARD + total * es]
    send.copy_(torch.from_numpy(xs[rank].view(np.uint8).copy()))
    sv = send.view(tdt)
    rwhole = None
    if row.inplace:
        recv = sv[mine]
    else:
        rwhole = torch.full((count * es + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        recv = rwhole[GUARD:GUARD + count * es].view(tdt)
    op, factor = C.OP_NAMES[row.op], None
    if row.family == "premul":
        if row.scalar == "dev":
            factor = torch.from_numpy(S.scalar_bits(row.code, [ss[rank]]).view(np.uint8).copy()).cuda().view(tdt)
            op = comm.create_premul_sum(factor, tdt)
        else:
            op = comm.create_premul_sum(float(ss[rank]), tdt)
    account.keep += [swhole, rwhole, factor]
    if row.coll == ALLREDUCE:
        account.call(row, lambda: comm.all_reduce(sv, recv, op=op), sv.data_ptr(), recv.data_ptr())
    else:
        account.call(row, lambda: comm.reduce_scatter(sv, recv, op=op), sv.data_ptr())
    if row.family == "premul":
        comm.destroy_op(op)  # at once: the stream has not run yet
    torch.cuda.synchronize()
    want_send = xs[rank].copy()
    if row.inplace:
        want_send[mine] = ref[mine]
    got = swhole.cpu().numpy()
    body = got[GUARD:GUARD + total * es].view(C.bits_dtype(lrow))
    ok = C.mismatches(lrow, body, want_send).size == 0
    ok = ok and bool((got[:GUARD] == FILL).all()) and bool((got[GUARD + total * es:] == FILL).all())
    if rwhole is not None:
        got = rwhole.cpu().numpy()
        ok = ok and C.mismatches(lrow, got[GUARD:GUARD + count * es].view(C.bits_dtype(lrow)), ref[mine]).size == 0
        ok = ok and bool((got[:GUARD] == FILL).all()) and bool((got[GUARD + count * es:] == FILL).all())
    return ok


def make_case(row, n, total, seed):
    """(xs, ss) of a row: pull_reduce_ll_cases.make_case, PreMulSum with the "generic" scalars (every
    product rounds, and at n = 2 the result is neither rank's operand)."""
    if row.family == "premul":
        ss = S.scalars(row.code, n, seed, "generic")
        return S.inputs(row.code, n, total, seed, ss), ss
    return C.make_case(ll_row(row), n, total, seed)


def _cutover(family, code, op, coll, inplace=False, scalar=None):
    """The partners at exactly the cutover (LL) and one element above it (pull)."""
    name = "%s_coll%d" % (C.row_name((family, code, op)).replace("-", "_"), coll)
    return [Row("cutover", "at_the_cutover_" + name, coll, family, code, op, ("cutover", 0), inplace, scalar, EVERY),
            Row("cutover", "one_element_above_" + name, coll, family, code, op, ("cutover", 1), inplace, scalar, NEVER)]


# ---- tests/test_pull_reduce_multiprocess_gpu.py (MAX / AVG; n = 2, 4, 8, and "pull" at n = 3) -----------
MAXAVG_RANKS = {LL: (2, 4, 8), PULL: (2, 3, 4, 8)}
MAXAVG_TYPES = (O.F16, O.BF16, O.F32, O.I32)
MAXAVG_COUNTS = (1, 4097, 100003)
# 100003 elements: 200006 bytes of the two-byte types, 400012 of the four-byte ones.  AllReduce takes LL
# up to 1 MiB / 512 KiB / 256 KiB at 2 / 3-4 / 5-8 ranks, a ReduceScatter block up to 512 / 512 / 128 KiB.
_BIG_LL_AT = {(REDUCE_SCATTER, 2): UP_TO_4, (REDUCE_SCATTER, 4): UP_TO_4, (ALLREDUCE, 2): EVERY, (ALLREDUCE, 4): UP_TO_4}


def _maxavg():
    rows = []
    for code in MAXAVG_TYPES:
        name, es = P.NAMES[code], O.itemsize(code)
        for op in (P.MAX, P.AVG):
            for count in MAXAVG_COUNTS:
                for coll in P.COLLS:
                    at = NEVER if coll == REDUCE else _BIG_LL_AT[(coll, es)] if count == 100003 else EVERY
                    rows.append(Row("main", "%s_%s" % (name, C.OP_NAMES[op]), coll, "pull", code, op, count, False, None, at))
        for coll in P.COLLS:
            rows.append(Row("again", "again_" + name, coll, "pull", code, P.AVG, 4097, False, None,
                            NEVER if coll == REDUCE else EVERY))
        for coll in P.COLLS:
            for op in (P.MAX, P.AVG):
                rows.append(Row("in_place", "in_place_" + name, coll, "pull", code, op, 4097, True, None,
                                NEVER if coll == REDUCE else EVERY))
    for it in range(2):  # between a fullmesh SUM AllReduce and a Broadcast
        rows.append(Row("mixed", "mixed", ALLREDUCE, "pull", O.F32, P.AVG, 50001, False, None, EVERY))
        coll = P.COLLS[it]
        rows.append(Row("mixed", "mixed", coll, "pull", O.F32, P.MAX, ("share", 50001), False, None,
                        NEVER if coll == REDUCE else EVERY))
    rows.append(Row("graph", "graph", ALLREDUCE, "pull", O.F32, P.AVG, 4097, False, None, EVERY))  # eager, then captured
    rows.append(Row("after_refused", "after_refused", ALLREDUCE, "pull", O.F32, P.MAX, 4097, False, None, EVERY))
    # buffers A, B, C that the ranks group into allocations differently (even ranks: A and C share one,
    # odd ranks: B and C): a Reduce on A, on B, two on C (an even and an odd root), an AllReduce in place on C
    for k in range(4):
        rows.append(Row("regrouped", "regrouped", REDUCE, "pull", O.F32, P.MAX, 4097, False, None, NEVER))
    rows.append(Row("regrouped", "regrouped", ALLREDUCE, "pull", O.F32, P.AVG, 4097, True, None, EVERY))
    rows += _cutover("pull", O.BF16, P.AVG, ALLREDUCE, inplace=True) + _cutover("pull", O.F16, P.MAX, REDUCE_SCATTER)
    return rows


MAXAVG = _maxavg()

# ---- tests/test_int_reduce_multiprocess_gpu.py (n = 2, 8) ---------------------------------------------
INT_RANKS = {LL: (2, 8), PULL: (2, 8)}
INT_CASES = [(I.I64, op) for op in I.OPS] + [(I.U64, I.MAX), (I.U64, I.AVG), (I.I8, I.SUM), (I.I8, I.AVG)]


def _int():
    rows = []
    for code, op in INT_CASES:
        for coll in I.COLLS:
            for inplace in (False, True):  # 1031 elements: 8248 bytes at most
                rows.append(Row("main", "%s_%s" % (I.NAMES[code], I.OP_NAMES[op]), coll, "int", code, op, 1031, inplace, None,
                                NEVER if coll == REDUCE else EVERY))
    rows.append(Row("one_element", "one_element_max", ALLREDUCE, "int", I.I64, I.MAX, 1, False, None, EVERY))
    # the Communicator methods with torch.int64 tensors: 1031 n elements (65984 bytes at n = 8), blocks of 1031
    rows.append(Row("communicator", "communicator_int64", ALLREDUCE, "int", I.I64, I.SUM, ("times", 1031), False, None, EVERY))
    rows.append(Row("communicator", "communicator_int64", REDUCE_SCATTER, "int", I.I64, I.SUM, 1031, False, None, EVERY))
    rows.append(Row("communicator", "communicator_int64", REDUCE, "int", I.I64, I.SUM, ("times", 1031), False, None, NEVER))
    rows.append(Row("flag", "communicator_int64", ALLREDUCE, "int", I.I64, I.MAX, 1, True, None, EVERY))
    rows.append(Row("counter", "communicator_int64", ALLREDUCE, "int", I.I64, I.SUM, 1, True, None, EVERY))
    rows.append(Row("after_refused", "after_refused", ALLREDUCE, "int", I.I64, I.SUM, 1031, False, None, EVERY))
    rows += _cutover("int", I.I64, I.SUM, ALLREDUCE, inplace=True) + _cutover("int", I.I8, I.MIN, REDUCE_SCATTER)
    return rows


INT = _int()

# ---- tests/test_premul_sum_multiprocess_gpu.py (n = 2, 8) ---------------------------------------------
PREMUL_RANKS = {LL: (2, 8), PULL: (2, 8)}


def _premul():
    rows = []
    op = C.PREMUL_SUM
    for code in (O.BF16, O.F32):  # 1031 elements: 4124 bytes at most
        for coll in S.COLLS:
            at = NEVER if coll == REDUCE else EVERY
            name = "%s_coll%d" % (S.NAMES[code], coll)
            rows.append(Row("main", name + "_fsdp", coll, "premul", code, op, 1031, False, "imm", at))
            rows.append(Row("main", name + "_per_rank", coll, "premul", code, op, 1031, False, "imm", at))
            rows.append(Row("main", name + "_in_place", coll, "premul", code, op, 1031, True, "imm", at))
    rows.append(Row("once", "f16_once", REDUCE_SCATTER, "premul", O.F16, op, 1031, False, "imm", EVERY))
    rows.append(Row("once", "one_element", ALLREDUCE, "premul", O.F32, op, 1, False, "imm", EVERY))
    rows.append(Row("communicator", "communicator_methods", REDUCE_SCATTER, "premul", O.BF16, op, 1031, False, "imm", EVERY))
    rows.append(Row("device", "device_scalar", ALLREDUCE, "premul", O.F32, op, 1031, False, "dev", EVERY))
    rows.append(Row("graph", "graph", ALLREDUCE, "premul", O.F32, op, 1031, False, "dev", EVERY))  # the capture
    rows += _cutover("premul", O.BF16, op, ALLREDUCE, scalar="dev")
    rows += _cutover("premul", O.F32, op, REDUCE_SCATTER, inplace=True, scalar="imm")
    return rows


PREMUL = _premul()

# (family, table, rank counts per mode); the "cutover" part runs in the default environment only
FILES = {"pull": (MAXAVG, MAXAVG_RANKS), "int": (INT, INT_RANKS), "premul": (PREMUL, PREMUL_RANKS)}


def rows_of_mode(table, mode):
    return [row for row in table if mode == LL or row.part != "cutover"]


CUTOVER_SEEDS = {"pull": 2500, "int": 4950, "premul": 5903}


def cutover_rows(table, mode):
    """(row, seed of its case) of the rows at and above the cutover; none under "pull"."""
    return [(row, CUTOVER_SEEDS[row.family] + k) for k, row in enumerate(part(rows_of_mode(table, mode), "cutover"))]


# ---- tests/test_mixed_collectives_gpu.py, across processes (n = 3, 8; default environment) -------------
MIXED_RANKS = (3, 8)
MIXED_COUNT = 4099  # 16396 bytes of the four-byte types, 32792 of int64
MIXED = [
    Row("mixed", "ar_max_ll", ALLREDUCE, "pull", O.F32, P.MAX, MIXED_COUNT, False, None, EVERY),
    Row("mixed", "rs_avg_ll", REDUCE_SCATTER, "pull", O.F16, P.AVG, MIXED_COUNT, False, None, EVERY),
    Row("mixed", "reduce_max", REDUCE, "pull", O.F32, P.MAX, MIXED_COUNT, False, None, NEVER),
    Row("mixed", "ar_max_pull", ALLREDUCE, "pull", O.F32, P.MAX, ("cutover", 1), False, None, NEVER),
    Row("mixed", "rs_avg_pull", REDUCE_SCATTER, "pull", O.F16, P.AVG, ("cutover", 1), False, None, NEVER),
    Row("mixed", "ar_i64_sum_ll", ALLREDUCE, "int", I.I64, I.SUM, MIXED_COUNT, False, None, EVERY),
    Row("mixed", "ar_i64_sum_pull", ALLREDUCE, "int", I.I64, I.SUM, ("cutover", 1), False, None, NEVER),
    Row("mixed", "ar_premul_ll", ALLREDUCE, "premul", O.BF16, C.PREMUL_SUM, MIXED_COUNT, False, "imm", EVERY),
    Row("mixed", "rs_premul_pull", REDUCE_SCATTER, "premul", O.F32, C.PREMUL_SUM, ("cutover", 1), False, "dev", NEVER),
    Row("mixed", "reduce_i8_min", REDUCE, "int", I.I8, I.MIN, MIXED_COUNT, False, None, NEVER),
]
MIXED_FIRST = ("ar_max_ll", "rs_avg_ll", "reduce_max")  # the entries the test had before, judged as before
MIXED_BY_NAME = {row.key: row for row in MIXED}

# ---- ... and in process (n = 3, 8): the launcher is chosen by the row, per grid gi = 0, 1 -----------------
# part "ll": InProcessRanks.pull_reduce_ll; part "pull": InProcessRanks.pull_reduce.  ll_at says what the
# ABI would do with the same call: the "ll" rows are sizes the default rule sends to LL, the "pull" rows of
# ReduceScatter / AllReduce are what it runs with the variable at 0.
INPROCESS_COUNT = 1001
INPROCESS_RANKS = (3, 8)


def inprocess_rows(gi):
    op = C.PREMUL_SUM
    a, b = (REDUCE_SCATTER, ALLREDUCE) if gi == 0 else (ALLREDUCE, REDUCE_SCATTER)
    rows = [Row("ll", "ll int64", a, "int", I.I64, (I.SUM, I.MAX)[gi], INPROCESS_COUNT, False, None, EVERY),
            Row("ll", "ll premul", b, "premul", (O.BF16, O.F32)[gi], op, INPROCESS_COUNT, False, "dev", EVERY)]
    for coll in P.COLLS:
        rows.append(Row("pull", "premul", coll, "premul", (O.F32, O.BF16, O.F16)[(coll + gi) % 3], op, INPROCESS_COUNT, False,
                        ("imm", "dev")[(coll + gi) % 2], NEVER if coll == REDUCE else EVERY))
    rows.append(Row("pull", "int8", b, "int", I.I8, (I.MIN, I.AVG)[gi], INPROCESS_COUNT, False, None, EVERY))
    return rows
