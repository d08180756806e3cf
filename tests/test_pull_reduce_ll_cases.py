"""The tables of pull_reduce_ll_cases are not vacuous, its lanes tell rank order from own-first order
(and the test says what cannot be told apart, and why), its geometry is the library's, and the host
layer of the LL path refuses what it must (mscclppAmdPullReduceLLLaunch with fake views: nothing
touches a device)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import int_reduce_cases as I
import oracle_lib as O
import pull_reduce_cases as P
import pull_reduce_ll_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the tables ---------------------------------------------------------------------------------
def test_every_operation_of_the_three_families_is_a_row():
    import mscclpp_amd as m

    assert len(C.ROWS) == len(set(C.ROWS)) == 16 + 12 + 3
    assert {(code, op) for fam, code, op in C.ROWS if fam == "pull"} == {(c, op) for c in P.TYPES for op in (P.MAX, P.AVG)}
    assert {(code, op) for fam, code, op in C.ROWS if fam == "int"} == {(c, op) for c in I.TYPES for op in I.OPS}
    assert {(code, op) for fam, code, op in C.ROWS if fam == "premul"} == {(c, 5) for c in (O.F16, O.BF16, O.F32)}
    assert C.RANKS == (2, 3, 8) and C.LL_COLLS == (m.PULL_REDUCE_SCATTER, m.PULL_ALLREDUCE)
    assert (C.SUM, C.MIN, C.MAX, C.AVG, C.PREMUL_SUM) == (m.SUM, m.MIN, m.MAX, m.AVG, m.PREMUL_SUM)
    assert {C.itemsize(row) for row in C.ROWS} == {1, 2, 4, 8} == set(C.SIZES)


def test_sizes_hold_every_shape_the_kernel_treats_differently():
    for es, sizes in C.SIZES.items():
        assert all(b % es == 0 for b in sizes)
        assert es in sizes  # one element
        geo = {b: C.geometry(8, b, es) for b in sizes}
        units = {g["units"] for g in geo.values()}
        assert {65, 129} <= units  # two and three passes of a 1 x 64 grid
        for b in C.SEVERAL_PASSES[es]:
            assert geo[b]["units"] > C.ONE_BY_64["nblocks"] * C.ONE_BY_64["nthreads"]
        if es == 8:
            assert {8, 16, 24} <= set(sizes)  # 1, 2 and 3 elements
            assert all(g["W"] % 2 == 0 for g in geo.values())  # one unit = one element: no lone packet
        else:
            assert 12 in sizes and geo[12]["W"] == 3  # an odd W: the lone trailing packet
            assert any(g["W"] % 2 and g["units"] > 64 for g in geo.values())  # ... and in a later pass
        if es == 1:
            assert set(range(1, 10)) <= set(sizes)
        if es in (1, 2):
            assert 6 in sizes  # ReduceScatter blocks whose starts are not word-aligned
        small = [b for b in sizes if b <= 24]
        wide = C.WIDE_GRID["nblocks"] * C.WIDE_GRID["nthreads"]
        assert small and all(geo[b]["units"] * 64 < wide for b in small)  # workgroups that own no unit
    # the words: every byte is covered, by at most one word more than needed
    for es in (1, 2, 4, 8):
        for b in range(es, 200, es):
            w = C.ll_words(b, es)
            assert 4 * w >= b and 4 * (w - 1) < b + es


@pytest.mark.parametrize("n", C.RANKS)
def test_cases_are_not_trivial(n):
    """Every row's inputs differ between the ranks and its reference is none of the operands."""
    for row in C.ROWS:
        count = C.SEVERAL_PASSES[C.itemsize(row)][1] // C.itemsize(row)
        xs, ss = C.make_case(row, n, count, 40 + n)
        assert (ss is None) == (row[0] != "premul")
        assert all(len(x) == count and x.dtype == C.bits_dtype(row) for x in xs)
        assert all(not np.array_equal(xs[0], x) for x in xs[1:])
        ref = C.reference(row, xs, ss)
        assert ref.dtype == xs[0].dtype and C.mismatches(row, ref, ref).size == 0
        if row[0] == "premul" and n == 2:
            continue  # scalars {1.0, -0} (premul_sum_cases): the result is one rank's operand
        if row[2] in (C.SUM, C.AVG, C.PREMUL_SUM):
            assert all(C.mismatches(row, x, ref).size > count // 2 for x in xs), row


def test_region_image():
    # 12 bytes of fp16: W = 3, two units, the second a lone 8-byte packet
    img = C.region_image(np.arange(1, 13, dtype=np.uint8), 2, 7).view(np.uint32)
    assert img.tolist() == [0x04030201, 7, 0x08070605, 7, 0x0c0b0a09, 7, 0, 0]
    # 5 bytes of int8: W = 2, the tail zero-filled
    img = C.region_image(np.arange(1, 6, dtype=np.uint8), 1, 9).view(np.uint32)
    assert img.tolist() == [0x04030201, 9, 0x00000005, 9]
    # PreMulSum: one more unit with the scalar's fp32 bits
    img = C.region_image(np.arange(1, 5, dtype=np.uint8), 4, 3, scalar=0x3f000000).view(np.uint32)
    assert img.tolist() == [0x04030201, 3, 0, 0, 0x3f000000, 3, 0, 3]


# ---- rank order against own-first order ------------------------------------------------------------
@pytest.mark.parametrize("n", C.ORDER_RANKS)
@pytest.mark.parametrize("row", C.ORDER_ROWS, ids=C.row_name)
def test_planted_lanes_tell_rank_order_from_own_first(row, n):
    """Lane r - 2: rank order gives eps / n (PreMulSum: eps / 2), own-first on rank r gives 0."""
    fam, code, op = row
    xs, ss = C.order_case(row, n)
    big, eps = C.ORDER_B_EPS[code]
    assert np.float32(big) + np.float32(eps) == np.float32(big)  # eps is lost beside B in fp32
    ref = C.reference(row, xs, ss)
    want = np.float32(eps) * (np.float32(0.5) if fam == "premul" else np.float32(1.0) / np.float32(n))
    want_bits = P.round_to(code, np.array([want], np.float32))[0]
    assert P.decode(code, np.array([want_bits]))[0] != 0  # a non-zero value of the element type
    for r in range(2, n):
        assert ref[r - 2] == want_bits, (row, n, r)
        assert C.own_first(row, xs, ss, r)[r - 2] == 0, (row, n, r)
    assert (ref[n - 2:] == 0).all()


def committed_inputs(row, n, count):
    """The existing case modules' inputs at the counts 67 and 130 (the specials planted)."""
    return C.make_case(row, n, count, 9 + count)


@pytest.mark.parametrize("n", C.RANKS)
def test_committed_inputs_and_the_two_orders(n):
    """What the committed inputs tell apart already, and what no input can."""
    for row in C.ROWS:
        fam, code, op = row
        differs = {}
        for count in (67, 130):
            xs, ss = committed_inputs(row, n, count)
            ref = C.reference(row, xs, ss)
            for r in range(n):
                differs[r] = differs.get(r, False) or C.mismatches(row, C.own_first(row, xs, ss, r), ref).size > 0
        # rank 0's own-first order IS rank order; rank 1's swaps the first two operands, and a + b = b + a
        # (for MAX the swap matters: of equal values and of NaNs the first operand's bits stay)
        assert not differs[0], row
        if op != C.MAX:
            assert not differs[1], row
        if fam == "int" or code not in P.FLOAT_TYPES:
            assert not any(differs.values()), row  # integers: every operation is exact
        elif code == O.E4M3 and op == C.AVG:
            assert not any(differs.values()), row  # sums of 8 e4m3 values are exact in fp32
        elif op == C.MAX:
            assert any(differs.values()), row  # selections: +0 / -0 and NaN payloads follow the order


# ---- the host layer --------------------------------------------------------------------------------
def test_symbols_and_methods_exist(built):
    import mscclpp_amd as m

    out = subprocess.run(["nm", "-D", "--defined-only", m.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"mscclppAmdPullReduceLLLaunch", "mscclppAmdPullReduceLLScratchRequired", "mscclppAmdPullReduceTakesLL",
            "mscclppAmdCommPullLLCount"} <= have
    assert len(m.lib().mscclppAmdPullReduceLLLaunch.argtypes) == 13
    assert callable(m.InProcessRanks.pull_reduce_ll) and callable(m.Communicator.pull_ll_count)
    assert callable(m.pull_reduce_takes_ll) and callable(m.pull_reduce_ll_scratch_required)


def test_scratch_requirement_is_the_restated_geometry(built):
    import mscclpp_amd as m

    for row in C.ROWS:
        fam, code, op = row
        es = C.itemsize(row)
        for n in range(2, 9):
            for coll in C.LL_COLLS:
                for b in C.SIZES[es] + (es << 10, (1 << 20) // es * es):
                    g = C.geometry(n, b, es, fam == "premul")
                    assert m.pull_reduce_ll_scratch_required(coll, n, b, code, op) == g["scratch"], (row, n, coll, b)
    f32 = O.F32
    assert m.pull_reduce_ll_scratch_required(m.PULL_REDUCE, 4, 64, f32, m.MAX) == 0  # Reduce is not carried
    assert m.pull_reduce_ll_scratch_required(m.PULL_ALLREDUCE, 4, 64, f32, m.SUM) == 0  # SUM has its own kernels
    assert m.pull_reduce_ll_scratch_required(m.PULL_ALLREDUCE, 4, 0, f32, m.MAX) == 0
    assert m.pull_reduce_ll_scratch_required(m.PULL_ALLREDUCE, 4, 66, f32, m.MAX) == 0  # splits an element
    assert m.pull_reduce_ll_scratch_required(m.PULL_ALLREDUCE, 1, 64, f32, m.MAX) == 0
    assert m.pull_reduce_ll_scratch_required(m.PULL_ALLREDUCE, 9, 64, f32, m.MAX) == 0
    assert m.pull_reduce_ll_scratch_required(m.PULL_ALLREDUCE, 4, 64, O.I32, m.PREMUL_SUM) == 0


N = 3
SCRATCH = 1 << 16


def fake_views(n, scratch_bytes=SCRATCH):
    import mscclpp_amd as m

    arr = (m.RankView * n)()
    for r in range(n):
        v = arr[r]
        v.input = v.output = v.scratch = v.flags = v.err = 1 << 20
        v.scratchBytes = scratch_bytes
        v.rank = r
        for q in range(n):
            v.peerScratch[q] = 1 << 20
    return arr


def launch(arr, nviews=N, nranks=N, coll=C.ALLREDUCE, nbytes=64, dtype=O.F32, op=C.MAX, nblocks=0, nthreads=0,
           scales=None, ptrs=None):
    import ctypes

    import mscclpp_amd as m

    imm = None if scales is None else (ctypes.c_float * len(scales))(*scales)
    return m.lib().mscclppAmdPullReduceLLLaunch(arr, nviews, nranks, coll, nbytes, dtype, op, nblocks, nthreads, 1000,
                                                None, imm, ptrs)


@pytest.mark.parametrize("coll", C.LL_COLLS)
def test_launch_rejects_bad_arguments_without_gpu(built, coll):
    import ctypes

    import mscclpp_amd as m

    arr = fake_views(N)
    assert launch(None, coll=coll) == 4
    assert launch(arr, coll=coll, nviews=0) == 4
    assert launch(arr, coll=coll, nviews=2) == 4
    assert launch(arr, coll=coll, nviews=1, nranks=1) == 4
    assert launch(arr, coll=coll, nviews=1, nranks=m.MAX_RANKS + 1) == 4
    for bad_coll in (m.PULL_REDUCE, -1, 3):  # a Reduce keeps the pull path
        assert launch(arr, coll=bad_coll) == 4
    assert launch(arr, coll=coll, nbytes=0) == 4
    assert launch(arr, coll=coll, nbytes=66, dtype=m.F32) == 4  # splits an element
    assert launch(arr, coll=coll, nbytes=63, dtype=m.F16) == 4
    assert launch(arr, coll=coll, nbytes=60, dtype=m.I64, op=m.SUM) == 4
    for op in (m.SUM, m.MIN, -1, 4):  # SUM / MIN of the eight types have their own kernels
        assert launch(arr, coll=coll, op=op) == 4, op
    for dtype in (-1, 7, 8, 9, 10, 12, 13, 14, 15, 100):
        assert launch(arr, coll=coll, dtype=dtype) == 4, dtype
    # PreMulSum: with scalars only, of the three float types only; scalars with nothing else
    ss = [0.5] * N
    assert launch(arr, coll=coll, op=m.PREMUL_SUM) == 4
    assert launch(arr, coll=coll, op=m.PREMUL_SUM, dtype=m.I32, scales=ss) == 4
    assert launch(arr, coll=coll, op=m.MAX, scales=ss) == 4
    assert launch(arr, coll=coll, op=m.MAX, ptrs=(ctypes.c_void_p * N)()) == 4
    for field in ("input", "output", "scratch", "flags", "err"):
        for r in range(N):
            bad = fake_views(N)
            setattr(bad[r], field, None)
            assert launch(bad, coll=coll) == 4, (field, r)
    bad = fake_views(N)
    bad[0].peerScratch[2] = None
    assert launch(bad, coll=coll) == 4
    bad = fake_views(N)
    bad[1].flags = (1 << 20) + 4  # the flag refresh stores 16 bytes at a time
    assert launch(bad, coll=coll) == 4
    bad = fake_views(N)
    bad[2].rank = N
    assert launch(bad, coll=coll) == 4
    bad = fake_views(N)
    bad[2].rank = 0  # a rank twice
    assert launch(bad, coll=coll) == 4
    assert launch(arr, coll=coll, nblocks=m.FLAG_SLOTS + 1) == 4
    for nthreads in (32, 96, 576, 1024):
        assert launch(arr, coll=coll, nblocks=4, nthreads=nthreads) == 4, nthreads


@pytest.mark.parametrize("coll", C.LL_COLLS)
def test_launch_with_too_little_scratch_is_invalid_usage(built, coll):
    """Checked after the arguments (a bad argument is still 4) and before the device."""
    import mscclpp_amd as m

    need = m.pull_reduce_ll_scratch_required(coll, N, 4096, O.F32, m.MAX)
    assert need == C.geometry(N, 4096, 4)["scratch"] > 0
    assert launch(fake_views(N, need - 256), coll=coll, nbytes=4096) == 5
    assert launch(fake_views(N, 0), coll=coll, nbytes=4096) == 5
    uneven = fake_views(N, need)
    uneven[1].scratchBytes = need + 256
    assert launch(uneven, coll=coll, nbytes=4096) == 5
    assert launch(fake_views(N, need - 256), coll=coll, nbytes=4096, op=m.SUM) == 4
    assert launch(fake_views(N, need - 256), coll=coll, nbytes=4098) == 4
    # PreMulSum needs one more unit per region
    ss = [0.5] * N
    need = m.pull_reduce_ll_scratch_required(coll, N, 4096 - 16, O.F32, m.PREMUL_SUM)
    assert need == m.pull_reduce_ll_scratch_required(coll, N, 4096, O.F32, m.MAX)
    assert launch(fake_views(N, need - 256), coll=coll, nbytes=4096 - 16, op=m.PREMUL_SUM, scales=ss) == 5
    assert launch(fake_views(N, 1 << 30), coll=coll, nbytes=1 << 32) == 5  # a size the path does not carry


# ---- the cutover -----------------------------------------------------------------------------------
def takes_in_a_process(value, queries):
    """mscclppAmdPullReduceTakesLL in a process of its own with the variable set to `value`, or unset
    for None (the library reads it once)."""
    code = ("import mscclpp_amd as m; "
            f"print([int(m.pull_reduce_takes_ll(c, n, b)) for c, n, b in {queries!r}])")
    env = {k: v for k, v in os.environ.items() if k != "MSCCLPP_AMD_PULL_LL_MAX_BYTES"}
    if value is not None:
        env["MSCCLPP_AMD_PULL_LL_MAX_BYTES"] = value
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True, check=True)
    return [int(x) for x in out.stdout.strip().splitlines()[-1].strip("[]").split(",")]


def test_builtin_cutover(built):
    """Up to the bound of (coll, nranks) a call takes the LL path, one byte and one element above it
    does not; a Reduce never does."""
    q, want = [], []
    for coll in C.LL_COLLS:
        for n in range(2, 9):
            most = C.BUILTIN_MAX[(coll, C.measured_ranks(n))]
            assert 8 <= most <= 1 << 20
            q += [(coll, n, 1), (coll, n, most), (coll, n, most + 1), (coll, n, most + 8), (coll, n, 0)]
            want += [1, 1, 0, 0, 0]
        q += [(coll, 1, 8), (coll, 9, 8)]
        want += [0, 0]
    q.append((C.REDUCE, 4, 8))
    want.append(0)
    assert takes_in_a_process(None, q) == want


def test_variable_zero_disables_the_path(built):
    q = [(c, n, b) for c in C.LL_COLLS for n in (2, 8) for b in (1, 8, 4096)]
    assert takes_in_a_process("0", q) == [0] * len(q)


def test_variable_overrides_both_collectives_and_is_clamped_to_1mib(built):
    q = [(c, n, b) for c in C.LL_COLLS for n in (2, 8) for b in (1 << 20, (1 << 20) + 1)] + [(C.REDUCE, 4, 8)]
    assert takes_in_a_process(str(1 << 30), q) == [1, 0] * 4 + [0]
    q = [(c, 4, b) for c in C.LL_COLLS for b in (4, 12, 13)]
    assert takes_in_a_process("12", q) == [1, 1, 0] * 2
