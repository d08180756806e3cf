"""CPU checks of the ncclMax / ncclAvg work: the numpy reference against independent statements, the
committed case tables against vacuity, and the host layer (exports, Python methods, every refusal
of mscclppAmdPullReduceLaunch with fake views: nothing touches a device)."""
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pull_reduce_cases as C


# ---- the reference against independent statements ---------------------------------------------
@pytest.mark.parametrize("code", [O.I32, O.U32, O.U8])
@pytest.mark.parametrize("n", C.RANKS)
def test_integer_avg_reference_against_big_integers(code, n):
    xs = C.inputs(code, C.AVG, n, 300, 7)
    got = C.ref_avg(code, xs)
    for i in range(300):
        vals = [int(x[i]) for x in xs]
        if code == O.I32:
            vals = [v - (1 << 32) if v >= 1 << 31 else v for v in vals]
        s = sum(vals)
        q = abs(s) // n * (1 if s >= 0 else -1)  # toward zero
        assert int(got[i]) == q % (1 << (8 * got.itemsize)), (i, vals)


@pytest.mark.parametrize("code", C.TYPES)
def test_max_reference_against_np_maximum_on_nan_free_data(code):
    n = 5
    xs = C.random_bits(code, n, 2000, 11, finite=True)
    got = C.ref_max(code, xs)
    if code in C.FLOAT_TYPES:
        vals = np.stack([C.decode(code, x) for x in xs])
        assert np.array_equal(C.decode(code, got), np.maximum.reduce(vals))
    else:
        view = np.int32 if code == O.I32 else xs[0].dtype
        assert np.array_equal(got.view(view), np.maximum.reduce(np.stack([x.view(view) for x in xs])))
    # a selection: every result is the bits of one rank's element
    assert np.any(np.stack([got == x for x in xs]), axis=0).all()


@pytest.mark.parametrize("e5m2", [False, True])
def test_fp8_rounding_against_the_oracle_encoder(e5m2):
    f = (C.mix64(4000, 3) >> np.uint64(32)).astype(np.uint32).view(np.float32)
    f = np.concatenate([f, C.fp8_table(e5m2).astype(np.float32), np.float32([0.0, -0.0, 1e-9, -1e-9, 1e9, -1e9, 464.0, 61440.0])])
    f = f[~np.isnan(f) & ~np.isinf(f)]
    got = C.fp8_round(f, e5m2)
    want = np.array([O.fp8_encode_sat(v, e5m2) for v in f], np.uint8)
    assert np.array_equal(got, want)
    # midpoints between neighbouring codes go to the even one
    t = C.fp8_table(e5m2).astype(np.float64)
    mid = ((t[1:0x70] + t[2:0x71]) / 2).astype(np.float32)
    assert np.array_equal(C.fp8_round(mid, e5m2), np.array([O.fp8_encode_sat(v, e5m2) for v in mid], np.uint8))


def test_bf16_rounding_is_nearest_even():
    f = np.float32([1.0, 1.00390625, 1.01171875, -1.00390625, 3.3895314e38, 1e-40])
    assert list(C.bf16_round(f)) == [0x3f80, 0x3f80, 0x3f82, 0xbf80, 0x7f7f, 0x0001]
    assert C.bf16_round(np.float32([3.4e38]))[0] == 0x7f80  # no clipping: beyond the range is inf


# ---- the committed tables are not vacuous -------------------------------------------------------
def table_inputs(code, op, n):
    return C.inputs(code, op, n, C.COUNT, C.table_seed(code, op, n))


@pytest.mark.parametrize("code", C.FLOAT_TYPES)
@pytest.mark.parametrize("n", [3, 8])
def test_avg_table_separates_the_definitions(code, n):
    xs = table_inputs(code, C.AVG, n)
    s = C.float_sum(code, xs)
    want = C.ref_avg(code, xs)
    body = slice(C.PLANTED, None)
    if code == O.E4M3:
        # e4m3 spans 2^-9 .. 448 with 4 significant bits: a sum of 8 needs 21 bits, so every fp32
        # add is exact and no order can change it; the rank-order rule is tested on the other types
        assert np.array_equal(C.float_sum(code, xs[::-1])[body].view(np.uint32), s[body].view(np.uint32))
    else:
        assert (C.float_sum(code, xs[::-1])[body].view(np.uint32) != s[body].view(np.uint32)).any()
    inv_n = np.float32(1.0) / np.float32(n)
    if n == 3:
        with np.errstate(over="ignore", invalid="ignore"):
            assert ((s / np.float32(3)).astype(np.float32)[body].view(np.uint32) != (s * inv_n)[body].view(np.uint32)).any()
    if code != O.F32:
        with np.errstate(over="ignore", invalid="ignore"):
            twice = C.round_to(code, (C.decode(code, C.round_to(code, s)) * inv_n).astype(np.float32))
        # (bf16 at n = 8 scales by a power of two, which commutes with the rounding except in the
        # subnormals: that element is planted)
        assert (twice != want)[7 if (code, n) == (O.BF16, 8) else body].any()
    if code == O.F16:
        big = (np.abs(s) > 65504) & np.isfinite(C.decode(code, want))
        assert big[:C.PLANTED].any()  # planted: the average of n x 65504 is 65504
        assert int(want[4]) == 0x7bff
    # NaN appears at planted positions only, so the NaN tolerance of the comparison stays there
    assert not C.is_nan_bits(code, want[body]).any()
    assert C.is_nan_bits(code, want[:C.PLANTED]).any()


@pytest.mark.parametrize("code", C.FLOAT_TYPES)
@pytest.mark.parametrize("n", C.RANKS)
def test_avg_inputs_are_finite_outside_the_planted_positions(code, n):
    xs = table_inputs(code, C.AVG, n)
    for x in xs:
        assert np.isfinite(C.decode(code, x[C.PLANTED:])).all()
    assert not C.is_nan_bits(code, C.ref_avg(code, xs)[C.PLANTED:]).any()


@pytest.mark.parametrize("code", C.TYPES)
@pytest.mark.parametrize("n", C.RANKS)
def test_max_table_has_every_winner_and_the_planted_cases(code, n):
    xs = table_inputs(code, C.MAX, n)
    want = C.ref_max(code, xs)
    for r in range(n):  # rank r's element wins somewhere, and is the only one with those bits there
        only = (want == xs[r]) & np.all(np.stack([xs[q] != xs[r] for q in range(n) if q != r]), axis=0)
        assert only.any(), r
    if code in C.FLOAT_TYPES:
        sg, one = C.SIGN[code], C.ONE[code]
        assert C.is_nan_bits(code, xs[0][:1]).all() and int(want[0]) == one | sg   # NaN on some ranks
        assert all(C.is_nan_bits(code, x[1:2]).all() for x in xs) and int(want[1]) == int(xs[n - 1][1])  # on all
        assert int(want[2]) == 0 and int(want[3]) == sg                              # +0 / -0 in both orders
        assert int(want[4]) == C.INF.get(code, C.TOP[code])                          # +inf
        assert int(want[5]) == C.TOP[code] | sg                                      # -inf loses
        assert int(want[6]) == one
    elif code == O.I32:
        assert int(want[0]) == 3 and int(want[1]) == 0x7fffffff and int(want[2]) == 0
    elif code == O.U32:
        assert int(want[0]) == 0xfffffffb and int(want[1]) == 0x80000000 and int(want[2]) == 0xffffffff


@pytest.mark.parametrize("n", C.RANKS)
def test_integer_avg_table_has_the_planted_cases(n):
    w = C.ref_avg(O.I32, table_inputs(O.I32, C.AVG, n))
    assert int(w[0]) == 0x7fffffff                      # n x INT32_MAX: the sum needs 64 bits
    assert int(w[1].view(np.int32)) == -(7 // n) and -(7 // n) != (-7) // n  # trunc, not floor
    assert int(w[3].view(np.int32)) == -(9 // n)
    assert int(C.ref_avg(O.U32, table_inputs(O.U32, C.AVG, n))[2]) == 0xffffffff
    assert int(C.ref_avg(O.U8, table_inputs(O.U8, C.AVG, n))[0]) == 255  # n x 255


# ---- host layer -----------------------------------------------------------------------------
def test_pull_reduce_symbols_and_methods_exist(built):
    import mscclpp_amd as m

    out = subprocess.run(["nm", "-D", "--defined-only", m.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"mscclppAmdPullReduceLaunch", "mscclppAmdPullReduceDefaultBlocks"} <= have
    L = m.lib()
    assert len(L.mscclppAmdPullReduceLaunch.argtypes) == 12 and len(L.mscclppAmdPullReduceDefaultBlocks.argtypes) == 2
    assert callable(m.InProcessRanks.pull_reduce)
    assert (m.MAX, m.AVG) == (2, 3) == (C.MAX, C.AVG) and m.NCCL_OPS["max"] == 2 and m.NCCL_OPS["avg"] == 4
    assert (m.PULL_REDUCE, m.PULL_REDUCE_SCATTER, m.PULL_ALLREDUCE) == C.COLLS
    # the default grid: a function of (collective, bytes) alone, 8..64, never shrinking with the size
    for coll in C.COLLS:
        grids = [L.mscclppAmdPullReduceDefaultBlocks(coll, b) for b in (1, 4096, 1 << 16, 1 << 20, 48 << 20, 1 << 40)]
        assert grids == sorted(grids) and grids[0] == 8 and grids[-1] == (64 if coll == C.REDUCE else 32), (coll, grids)


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


def launch(arr, nviews=N, nranks=N, coll=C.ALLREDUCE, nbytes=64, dtype=2, op=C.MAX, root=ROOT, nblocks=0, nthreads=0):
    import mscclpp_amd as m

    return m.lib().mscclppAmdPullReduceLaunch(arr, nviews, nranks, coll, nbytes, dtype, op, root, nblocks, nthreads, 1000,
                                              None)


@pytest.mark.parametrize("coll", C.COLLS)
def test_pull_reduce_launch_rejects_bad_arguments_without_gpu(built, coll):
    import mscclpp_amd as m

    arr = fake_views(N)
    assert launch(None, coll=coll) == 4
    assert launch(arr, coll=coll, nviews=0) == 4
    assert launch(arr, coll=coll, nviews=2) == 4
    assert launch(arr, coll=coll, nviews=1, nranks=1, root=0) == 4
    assert launch(arr, coll=coll, nviews=1, nranks=m.MAX_RANKS + 1) == 4
    for bad_coll in (-1, 3):
        assert launch(arr, coll=bad_coll) == 4
    assert launch(arr, coll=coll, nbytes=0) == 4
    assert launch(arr, coll=coll, nbytes=66, dtype=m.F32) == 4  # splits an element
    assert launch(arr, coll=coll, nbytes=63, dtype=m.F16) == 4
    for op in (m.SUM, m.MIN, -1, 4):  # SUM / MIN have their own kernels
        assert launch(arr, coll=coll, op=op) == 4, op
    # the accumulation-type codes, e4m3b15 and anything out of range
    for dtype in (-1, 7, 8, 9, 10, 12, 13, 14, 15, 100):
        assert launch(arr, coll=coll, dtype=dtype) == 4, dtype
    for field in ("input", "tokens", "expected", "err"):
        for r in range(N):
            bad = fake_views(N)
            setattr(bad[r], field, None)
            assert launch(bad, coll=coll) == 4, (field, r)
    bad = fake_views(N)
    bad[0].peerTokens[2] = None
    assert launch(bad, coll=coll) == 4
    bad = fake_views(N)
    bad[2].rank = N
    assert launch(bad, coll=coll) == 4
    bad = fake_views(N)
    bad[2].rank = 0  # a rank twice
    assert launch(bad, coll=coll) == 4
    readers = [ROOT] if coll == C.REDUCE else range(N)
    for r in readers:
        bad = fake_views(N)
        bad[r].output = None
        assert launch(bad, coll=coll) == 4, r
        for q in range(N):
            bad = fake_views(N)
            bad[r].peerInput[q] = None
            assert launch(bad, coll=coll) == 4, (r, q)
            if coll == C.ALLREDUCE:
                bad = fake_views(N)
                bad[r].peerOutput[q] = None
                assert launch(bad, coll=coll) == 4, (r, q)
    if coll == C.REDUCE:
        for root in (-1, N):
            assert launch(arr, coll=coll, root=root) == 4, root
    assert launch(arr, coll=coll, nblocks=m.MAX_CHANNELS + 1) == 4
    for nthreads in (32, 96, 576, 1024):
        assert launch(arr, coll=coll, nblocks=4, nthreads=nthreads) == 4, nthreads


@pytest.mark.parametrize("coll", C.COLLS)
def test_pull_reduce_launch_over_the_descriptor_limit_is_invalid_usage(built, coll):
    """A workgroup's range must fit one buffer descriptor (4 GiB): ncclInvalidUsage, checked after the
    arguments (a bad argument at that size is still 4) and before the device."""
    arr = fake_views(N)
    nbytes = (1 << 40) * (N if coll == C.ALLREDUCE else 1)  # a fake 1 TiB per reducing rank
    assert launch(arr, coll=coll, nbytes=nbytes, nblocks=8, nthreads=64) == 5
    assert launch(arr, coll=coll, nbytes=nbytes) == 5  # the default grid stops at 64 workgroups
    assert launch(arr, coll=coll, nbytes=nbytes, nblocks=8, nthreads=64, dtype=15) == 4
    assert launch(arr, coll=coll, nbytes=nbytes, nblocks=8, nthreads=64, op=0) == 4
