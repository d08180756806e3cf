"""CPU checks of the int64 / uint64 / int8 reductions: the numpy references against Python's integers,
the kernel's 64-bit AVG accumulators on the host against 128-bit integers, the committed case tables
against vacuity, and the host layer (codes, and what mscclppAmdPullReduceLaunch
takes and refuses with fake views: nothing touches a device)."""
import os
import subprocess

import numpy as np
import pytest

import int_reduce_cases as C


# ---- the references against Python's integers --------------------------------------------------
@pytest.mark.parametrize("n", C.RANKS)
@pytest.mark.parametrize("op", C.OPS)
@pytest.mark.parametrize("code", C.TYPES)
def test_reference_against_big_integers(code, op, n):
    xs = C.inputs(code, op, n, 300, 7)
    got = C.reference(code, op, xs)
    assert got.dtype == C.bits_dtype(code)
    for i in range(300):
        vals = [int(x[i]) for x in xs]
        assert int(got[i]) == C.big_reference(code, op, vals), (i, vals)


def test_kernel_avg64_accumulators_against_int128_on_the_host(built):
    """tests/cpp/test_avg64_host.hip: the kernel's own 96-bit accumulators, compiled for the host,
    against __int128 on 1.4 million cases (n = 2 .. 8)."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "bin", "test_avg64_host")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "avg64 OK 1400000" in r.stdout, r.stdout[-2000:]


# ---- the committed tables are not vacuous -------------------------------------------------------
def table_inputs(code, op, n):
    return C.inputs(code, op, n, C.COUNT, C.table_seed(code, op, n))


@pytest.mark.parametrize("n", C.RANKS)
@pytest.mark.parametrize("op", [C.MIN, C.MAX])
@pytest.mark.parametrize("code", C.TYPES)
def test_min_max_table_has_every_winner_and_the_planted_cases(code, op, n):
    xs = table_inputs(code, op, n)
    want = C.reference(code, op, xs)
    for r in range(n):  # rank r's element wins somewhere, and is the only one with those bits there
        only = (want == xs[r]) & np.all(np.stack([xs[q] != xs[r] for q in range(n) if q != r]), axis=0)
        assert only.any(), r
    # -5 vs 3: the other signedness gives other bits
    other = {C.I64: np.uint64, C.U64: np.int64, C.I8: np.uint8}[code]
    assert C.ref_select(code, xs, op == C.MAX, view=other)[0] != want[0]
    signed = code != C.U64
    minus5 = int(C.bits_dtype(code)(-5 & ((1 << (8 * C.itemsize(code))) - 1)))
    if op == C.MAX:
        assert int(want[0]) == (3 if signed else minus5)
    else:
        assert int(want[0]) == (minus5 if signed else (3 if n == 2 else 1))
    if code == C.I8:
        return
    lo, hi = np.uint64(0xffffffff), np.uint64(32)
    half = np.int32 if signed else np.uint32

    def by_one_word(high):
        """The selection a compare of one 32-bit word alone would make (the high word carries the sign)."""
        acc = xs[0].copy()
        for x in xs[1:]:
            a, b = ((acc >> hi, x >> hi) if high else (acc & lo, x & lo))
            a, b = a.astype(np.uint32).view(half if high else np.uint32), b.astype(np.uint32).view(half if high else np.uint32)
            acc = np.where(b > a if op == C.MAX else b < a, x, acc)
        return acc

    pair_a, pair_b = (2 if op == C.MAX else 3), slice(4, 6)
    assert int(xs[0][pair_a]) >> 32 == int(xs[1][pair_a]) >> 32 and int(want[pair_a]) == int(xs[1][pair_a])
    assert by_one_word(high=True)[pair_a] != want[pair_a]       # pair A: the high words are equal, the low words decide
    assert (by_one_word(high=False)[pair_b] != want[pair_b]).all()  # pair B: the low words order the other way


@pytest.mark.parametrize("n", C.RANKS)
def test_sum_table_has_the_planted_cases(n):
    for code in (C.I64, C.U64):
        xs = table_inputs(code, C.SUM, n)
        want = C.ref_sum(code, xs)
        assert int(xs[0][0]) == 0xffffffff and int(want[0]) == 1 << 32          # a carry out of the low word
        assert int(xs[0][1]) == (1 << 64) - 1 and int(want[1]) == 0             # a wrap at 2^64
        assert int(want[2]) == 1 << 63
        words = np.stack([x.view(np.uint32) for x in xs]).sum(axis=0, dtype=np.uint32)  # two 32-bit adds
        assert words.view(np.uint64)[0] != want[0]
    xs = table_inputs(C.I8, C.SUM, n)
    want = C.ref_sum(C.I8, xs)
    assert list(want[:4]) == [0x80, 0x00, 0x80, 0x00]
    word = np.stack([x[:4].view(np.uint32) for x in xs]).sum(axis=0, dtype=np.uint32)  # one word-wide add
    assert list(word.view(np.uint8)) == [0x80, 0x00, 0x81, 0x00] and word.view(np.uint8)[2] != want[2]


@pytest.mark.parametrize("n", C.RANKS)
def test_avg_table_has_the_planted_cases_and_separates_the_wrapped_sum(n):
    w = C.ref_avg(C.I64, table_inputs(C.I64, C.AVG, n)).view(np.int64)
    assert int(w[0]) == (1 << 63) - 1 and int(w[1]) == -(1 << 63)              # n x INT64_MAX, n x INT64_MIN
    assert int(w[2]) == -(7 // n) and -(7 // n) != (-7) // n                    # trunc, not floor
    assert int(w[3]) == -(9 // n)                                               # (exact at n = 3)
    assert int(w[4]) == 0                                                       # (INT64_MIN + INT64_MAX) / n = -1 / n
    w = C.ref_avg(C.U64, table_inputs(C.U64, C.AVG, n))
    assert int(w[0]) == (1 << 64) - 1 and int(w[1]) == 1 << 63 and int(w[5]) == (1 << 64) // n
    w = C.ref_avg(C.I8, table_inputs(C.I8, C.AVG, n)).view(np.int8)
    assert int(w[0]) == 127 and int(w[1]) == -128 and int(w[2]) == -(7 // n) and int(w[3]) == -(9 // n)
    for code in C.TYPES:  # the table body: the wrapped sum divided by n is another number somewhere
        xs = table_inputs(code, C.AVG, n)
        body = slice(C.PLANTED, None)
        assert (C.wrapped_avg(code, xs)[body] != C.ref_avg(code, xs)[body]).any(), code


# ---- host layer -----------------------------------------------------------------------------
N, ROOT = 3, 1


def fake_views(n):
    import mscclpp_amd as m

    arr = (m.RankView * n)()
    for r in range(n):
        v = arr[r]
        v.input = v.output = v.tokens = v.expected = v.err = 1 << 20
        v.rank = r
        for q in range(n):
            v.peerInput[q] = v.peerOutput[q] = v.peerTokens[q] = 1 << 20
    return arr


def launch(arr, coll, nbytes, dtype, op, nblocks=0, nthreads=0):
    import mscclpp_amd as m

    return m.lib().mscclppAmdPullReduceLaunch(arr, N, N, coll, nbytes, dtype, op, ROOT, nblocks, nthreads, 1000, None)


def test_codes(built):
    import torch

    import mscclpp_amd as m

    assert (m.I64, m.U64, m.I8) == (16, 17, 18) == C.TYPES
    assert m.reduce_code(torch.int64) == m.I64 and m.reduce_code(torch.int8) == m.I8
    assert m.reduce_code(torch.int64, m.U64) == m.U64
    assert (m.SUM, m.MIN, m.MAX, m.AVG) == C.OPS
    assert m.nccl_dtype(torch.int64) == 4 and m.nccl_dtype(torch.int8) == 0  # ncclInt64, ncclInt8


@pytest.mark.parametrize("coll", C.COLLS)
def test_launch_takes_the_new_types_with_all_four_ops(built, coll):
    """ncclInvalidUsage (5: a workgroup's range exceeds one descriptor) is answered only once every
    argument is accepted, and before a device is touched: a fake 1 TiB per reducing rank."""
    arr = fake_views(N)
    nbytes = (1 << 40) * (N if coll == C.ALLREDUCE else 1)
    for code in C.TYPES:
        for op in C.OPS:
            assert launch(arr, coll, nbytes, code, op, nblocks=8, nthreads=64) == 5, (code, op)
        for op in (4, -1):
            assert launch(arr, coll, nbytes, code, op, nblocks=8, nthreads=64) == 4, (code, op)
            assert launch(arr, coll, 64, code, op) == 4, (code, op)


@pytest.mark.parametrize("coll", C.COLLS)
def test_launch_still_refuses(built, coll):
    import mscclpp_amd as m

    arr = fake_views(N)
    assert launch(arr, coll, 68, m.I64, C.SUM) == 4  # splits an element
    assert launch(arr, coll, 68, m.U64, C.MAX) == 4
    for op in (C.SUM, C.MIN):  # the eight other types keep their own kernels for these
        for code in (m.F32, m.F16, m.I32, m.U32, m.U8, m.E4M3):
            assert launch(arr, coll, 64, code, op) == 4, (code, op)
            assert launch(arr, coll, 1 << 40, code, op, nblocks=8, nthreads=64) == 4, (code, op)
    for code in (15, 19, 100):
        for op in C.OPS:
            assert launch(arr, coll, 64, code, op) == 4, (code, op)
