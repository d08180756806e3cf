"""CPU checks of the PreMulSum tests: the numpy reference against exact rational arithmetic with
explicit roundings, the committed case tables against vacuity, and the host layer (codes, and what
mscclppAmdPullReduceLaunchScaled takes and refuses with fake views: nothing touches a device)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as O
import premul_sum_cases as C
import pull_reduce_cases as P


# ---- the reference against exact arithmetic ---------------------------------------------------
# (mantissa bits without the hidden one, smallest normal exponent, largest finite value)
FORMATS = {O.F32: (23, -126, Fraction(2 ** 24 - 1) * Fraction(2) ** 104),
           O.F16: (10, -14, Fraction(65504)),
           O.BF16: (7, -126, Fraction(2 ** 8 - 1) * Fraction(2) ** 120)}


def rne(x, code):
    """The value of the format nearest to the rational x, ties to even; None for an overflow to infinity."""
    mbits, emin, top = FORMATS[code]
    if x == 0:
        return Fraction(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1  # 2^e <= a < 2^(e + 1)
    e = max(e, emin)
    quantum = Fraction(2) ** (e - mbits)  # the spacing at this exponent (subnormals: the smallest normal's)
    q = a / quantum
    k = q.numerator // q.denominator
    rest = q - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k % 2):
        k += 1
    r = k * quantum
    if r > top:
        return None
    return r if x > 0 else -r


def exact_reference(code, vals, ss):
    """vals, ss: Fractions.  The definition, with every rounding spelled out."""
    acc = rne(vals[0] * ss[0], O.F32)  # (no product overflows: |s| <= 1)
    for v, s in zip(vals[1:], ss[1:]):
        acc = rne(acc + rne(v * s, O.F32), O.F32)
        if acc is None:
            return None  # the fp32 sum overflowed: infinity from here on, the operands being finite
    return rne(acc, code)


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("n", C.RANKS)
@pytest.mark.parametrize("code", C.TYPES)
def test_reference_against_exact_rationals(code, n, kind):
    xs, ss = C.table_case(code, n, kind)
    want = C.reference(code, xs, ss)
    assert want.dtype == C.bits_dtype(code)
    fs = [Fraction(float(s)) for s in ss]
    checked = 0
    for i in list(range(C.PLANTED)) + list(range(C.PLANTED, C.COUNT, 4))[:1000]:
        vals = P.decode(code, np.array([x[i] for x in xs]))
        if not np.isfinite(vals).all():
            continue  # the planted NaN and infinity: test_planted_positions
        exact = exact_reference(code, [Fraction(float(v)) for v in vals], fs)
        got = float(P.decode(code, want[i:i + 1])[0])
        if exact is None:
            assert np.isinf(got), i
        else:
            assert Fraction(got) == exact, (i, got, float(exact))
        checked += 1
    assert checked >= 1000


@pytest.mark.parametrize("n", C.RANKS)
@pytest.mark.parametrize("code", C.TYPES)
def test_planted_positions(code, n):
    for kind in C.KINDS:
        xs, ss = C.table_case(code, n, kind)
        want = C.reference(code, xs, ss)
        nan = P.is_nan_bits(code, want)
        # the NaN cap: NaNs at planted positions only, at most NAN_CAP of COUNT elements
        assert not nan[C.PLANTED:].any() and nan.sum() <= C.NAN_CAP
        assert nan[0]                                       # a NaN operand
        if kind == "special":
            z = C.zero_rank(ss)
            assert z is not None and int(xs[z][1]) == P.INF[code] and nan[1]  # inf x 0
            assert (ss == 1.0).sum() == 1
        else:
            assert np.isinf(P.decode(code, want[1:2]))[0] and C.zero_rank(ss) is None
        # -0 x s_k: the products are zeros of both signs and their sum is +0; with every scalar positive it were -0
        assert int(want[2]) == 0
        assert int(C.reference(code, xs, np.abs(ss))[2]) == P.SIGN[code]
        # 1 x s_k: the fp32 sum of the scalars, rounded once
        assert int(want[3]) == int(P.round_to(code, C.fp32_sum([np.float32(s) for s in ss]).reshape(1))[0])


# ---- the committed tables are not vacuous -------------------------------------------------------
@pytest.mark.parametrize("n", C.RANKS)
@pytest.mark.parametrize("code", C.TYPES)
def test_table_separates_the_implementations_it_must(code, n):
    """Per table case some element differs under: every rank taking rank 0's scalar, and the sum scaled
    afterwards (under both kinds of scalars); the product rounded to the element type (fp16 / bf16)
    and the products kept exact, i.e. fused (fp32) -- these two under the generic scalars, where every
    rank's product rounds: of the special ones 1.0 and -0 give exact products in any format (at n = 2
    they are the whole set).  A fused product cannot differ for fp16 and bf16 at all: two significands
    of 11 (8) bits give a product of at most 22 (16) bits, and with scalars of these magnitudes no
    product falls below fp32's subnormal spacing, so every product is exact in fp32 -- which is
    asserted in its place."""
    body = slice(C.PLANTED, None)
    for kind in C.KINDS:
        xs, ss = C.table_case(code, n, kind)
        want = C.reference(code, xs, ss)

        def differs(variant):
            return C.mismatches(code, variant(code, xs, ss), want).size > 0

        assert differs(C.variant_same_scalar), kind
        assert differs(C.variant_scaled_afterwards), kind
        if code == O.F32:
            if kind == "generic":
                assert differs(C.variant_fused)
                assert (C.variant_fused(code, xs, ss)[body] != want[body]).any()  # not at the planted elements alone
        else:
            if kind == "generic":
                assert differs(C.variant_element_product)
            assert not differs(C.variant_fused), kind
            for x, s in zip(xs, ss):  # every product is exact in fp32
                exact = P.decode(code, x[body]).astype(np.float64) * np.float64(s)
                assert np.array_equal(exact, C.product(code, x[body], s).astype(np.float64))


def test_scalars_are_of_the_element_type_and_rotate():
    for code in C.TYPES:
        for n in C.RANKS:
            for kind in C.KINDS:
                a, b = C.scalars(code, n, 10, kind), C.scalars(code, n, 11, kind)
                assert np.array_equal(C.scalar_values(code, a), a)  # rounding them again changes nothing
                assert not np.array_equal(a, b) and sorted(a.tolist()) == sorted(b.tolist())
        f = C.fsdp_scalars(code, 8)
        assert (f == np.float32(1.0 / 16)).all()


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


def launch_scaled(arr, coll, nbytes, dtype, op, nblocks=0, nthreads=0, scales=True, ptrs=None):
    import mscclpp_amd as m

    imm = (ctypes.c_float * N)(0.5, 1.0, -0.25) if scales else None
    return m.lib().mscclppAmdPullReduceLaunchScaled(arr, N, N, coll, nbytes, dtype, op, ROOT, nblocks, nthreads, 1000, None,
                                                    imm, ptrs)


def launch_plain(arr, coll, nbytes, dtype, op, nblocks=0, nthreads=0):
    import mscclpp_amd as m

    return m.lib().mscclppAmdPullReduceLaunch(arr, N, N, coll, nbytes, dtype, op, ROOT, nblocks, nthreads, 1000, None)


def test_codes(built):
    import torch

    import mscclpp_amd as m

    assert m.PREMUL_SUM == 5 == C.PREMUL_SUM and (m.MAX, m.AVG) == (2, 3)
    assert (m.F16, m.BF16, m.F32) == C.TYPES
    assert [m.reduce_code(t) for t in (torch.float16, torch.bfloat16, torch.float32)] == list(C.TYPES)
    assert (m.SCALAR_DEVICE, m.SCALAR_HOST_IMMEDIATE) == (0, 1)
    assert m.nccl_op("sum") == 0 and m.nccl_op("avg") == 4 and m.nccl_op(5) == 5 and m.nccl_op(7) == 7
    assert len(m.lib().mscclppAmdPullReduceLaunchScaled.argtypes) == 14
    assert len(m.lib().mscclppAmdPullReduceLaunch.argtypes) == 12  # the old entry point keeps its signature
    assert callable(m.Communicator.create_premul_sum) and callable(m.Communicator.destroy_op)


@pytest.mark.parametrize("coll", C.COLLS)
def test_scaled_launch_takes_premul_sum_of_the_three_float_types(built, coll):
    """ncclInvalidUsage (5: a workgroup's range exceeds one descriptor) is answered only once every
    argument is accepted, and before a device is touched: a fake 1 TiB per reducing rank."""
    arr = fake_views(N)
    nbytes = (1 << 40) * (N if coll == C.ALLREDUCE else 1)
    for code in C.TYPES:
        assert launch_scaled(arr, coll, nbytes, code, C.PREMUL_SUM, nblocks=8, nthreads=64) == 5, code
        ptrs = (ctypes.c_void_p * N)(None, 1 << 20, None)
        assert launch_scaled(arr, coll, nbytes, code, C.PREMUL_SUM, nblocks=8, nthreads=64, ptrs=ptrs) == 5, code


@pytest.mark.parametrize("coll", C.COLLS)
def test_scaled_launch_refuses_everything_else(built, coll):
    import mscclpp_amd as m

    arr = fake_views(N)
    big = (1 << 40) * (N if coll == C.ALLREDUCE else 1)
    for nbytes, shape in ((64, {}), (big, dict(nblocks=8, nthreads=64))):
        for code in C.TYPES:
            for op in (m.SUM, m.MIN, m.MAX, m.AVG, 4, 6, -1):
                assert launch_scaled(arr, coll, nbytes, code, op, **shape) == 4, (code, op)
            assert launch_scaled(arr, coll, nbytes, code, C.PREMUL_SUM, scales=False, **shape) == 4, code  # null scales
        for code in (m.I32, m.U32, m.E4M3, m.E5M2, m.U8, m.I64, m.U64, m.I8, -1, 7, 8, 9, 10, 12, 13, 14, 15, 19, 100):
            for op in (C.PREMUL_SUM, m.MAX, m.AVG, m.SUM):
                assert launch_scaled(arr, coll, nbytes, code, op, **shape) == 4, (code, op)
    assert launch_scaled(arr, coll, 66, m.F32, C.PREMUL_SUM) == 4  # splits an element
    assert launch_scaled(arr, coll, 63, m.F16, C.PREMUL_SUM) == 4
    assert launch_scaled(arr, coll, 63, m.BF16, C.PREMUL_SUM) == 4
    assert launch_scaled(arr, coll, 0, m.F32, C.PREMUL_SUM) == 4
    assert launch_scaled(arr, coll, 64, m.F32, C.PREMUL_SUM, nthreads=96) == 4  # launch shape, as the old entry point
    assert launch_scaled(None, coll, 64, m.F32, C.PREMUL_SUM) == 4
    for field in ("input", "tokens", "expected", "err"):
        bad = fake_views(N)
        setattr(bad[2], field, None)
        assert launch_scaled(bad, coll, 64, m.F32, C.PREMUL_SUM) == 4, field
    bad = fake_views(N)
    bad[2].rank = 0  # a rank twice
    assert launch_scaled(bad, coll, 64, m.F32, C.PREMUL_SUM) == 4


@pytest.mark.parametrize("coll", C.COLLS)
def test_old_entry_point_refuses_premul_sum_and_keeps_its_answers(built, coll):
    import mscclpp_amd as m

    arr = fake_views(N)
    big = (1 << 40) * (N if coll == C.ALLREDUCE else 1)
    for code in C.TYPES + (m.I64, m.I32, m.U8):
        assert launch_plain(arr, coll, 64, code, C.PREMUL_SUM) == 4, code
        assert launch_plain(arr, coll, big, code, C.PREMUL_SUM, nblocks=8, nthreads=64) == 4, code
        assert launch_plain(arr, coll, big, code, 4, nblocks=8, nthreads=64) == 4, code
    # the dispatch index dtype * 4 + op of the older operations: 4 * dtype + 5 names no kernel of dtype + 1
    for code in (m.F16, m.BF16, m.F32, m.I32, m.U32, m.E4M3, m.E5M2, m.U8):
        for op in (m.MAX, m.AVG):
            assert launch_plain(arr, coll, big, code, op, nblocks=8, nthreads=64) == 5, (code, op)
        for op in (m.SUM, m.MIN):
            assert launch_plain(arr, coll, big, code, op, nblocks=8, nthreads=64) == 4, (code, op)
    for code in (-1, 7, 8, 9, 10, 12, 13, 14, 15, 19, 100):
        for op in (m.SUM, m.MIN, m.MAX, m.AVG, 4, 5):
            assert launch_plain(arr, coll, big, code, op, nblocks=8, nthreads=64) == 4, (code, op)
