"""CPU check of the case tables in collective_edge_cases.py, which tests/test_collective_edges_gpu.py
runs on the GPU: every row is one the launchers accept (or is in the refusal list), the multi-pass rows
take three passes or more with the stated partial pass, the inputs make a wrong sum order, a wrong
slice and a MIN / SUM swap visible, the `finite` family is what it says, and the fp64 bound admits the
oracle's own result on every lane.  The oracle and numpy decide; no GPU."""
import numpy as np
import pytest

import collective_edge_cases as C
import kernel_edge_cases as K
import oracle_lib as O

RS, AG, BC = C.RS, C.AG, C.BC


def _launchable(block, nb, nt, n, scratch=C.A_SCRATCH):
    """The preconditions of launchCollectiveBulk for modes 1 and 2."""
    nb, nt = C.bulk_grid(nb, nt)
    assert 2 <= n <= 8 and 1 <= nb <= K.MAX_CHANNELS and nt % 64 == 0 and 64 <= nt <= 512
    assert block > 0 and block % 16 == 0
    assert K.slice_bytes(n, n * block) == block
    assert K.bulk_passes(n, n * block, scratch, nb)[0] > 0
    return nb, nt


def test_launch_shape_table():
    seen = set()
    for coll, algo, n, nb, nt, picks in C.A_CASES:
        gnb, gnt = _launchable(16, nb, nt, n)
        assert gnt == 64 or gnb * n <= C.A_MAX_WIDE_WORKGROUPS  # co-resident on one device
        assert [p[0] for p in picks] == list(C.A_BLOCKS)
        for block, code, op in picks:
            _launchable(block, nb, nt, n)
            assert K.bulk_passes(n, n * block, C.A_SCRATCH, gnb) == (block, 1)
            seen.add((coll, algo, n, code, op))
        seen.add((coll, algo, n, nb, nt))
    for coll in (RS, AG):
        for algo in C.ALGOS:
            for n in (2, 3, 8):
                assert {(coll, algo, n) + t for t in C.A_TYPES} <= seen
                for nb in (1, 3, 0, K.MAX_CHANNELS):
                    assert (coll, algo, n, nb, 64) in seen
                for nb in (1, 3) + ((0,) if n * 64 <= C.A_MAX_WIDE_WORKGROUPS else ()):
                    assert (coll, algo, n, nb, 512) in seen
            assert (coll, algo, 2, K.MAX_CHANNELS, 512) in seen and (coll, algo, 8, 0, 512) in seen
    assert C.A_MAX_WIDE_WORKGROUPS == 8 * C.bulk_grid(0, 0)[0]
    # one unit: one workgroup works, the others only handshake; 64 KiB + 16 on one workgroup of 64 lanes:
    # several strides per lane and one trailing unit
    assert C.A_BLOCKS[0] == 16 and (C.A_BLOCKS[3] // 16) // 64 >= 2 and (C.A_BLOCKS[3] // 16) % 64 == 1


def test_multipass_table():
    for n, code, op, block, scratch, nb, nt in C.B_CASES:
        _launchable(block, nb, nt, n, scratch)
        ps, passes = K.bulk_passes(n, n * block, scratch, nb)
        assert ps % (16 * nb) == 0 and passes >= 3
        assert block % ps != 0                      # a partial last pass
    n, code, op, block, scratch, nb, nt = C.B_CASES[0]
    assert K.bulk_passes(n, n * block, scratch, nb) == (8192, 3) and block % 8192 == 4096 + 16
    n, code, op, block, scratch, nb, nt = C.B_CASES[1]
    assert K.bulk_passes(n, n * block, scratch, nb) == (9984, 3) and scratch // n == 10000 and block % 9984 == 4992
    assert {(code, op) for _, code, op, *_ in C.B_CASES} >= {(O.F16, O.SUM), (O.F32, O.SUM), (O.I32, O.MIN)}
    n, code, block, scratch, nb, nt = C.B_REFUSED
    assert block % 16 == 0 and K.bulk_passes(n, n * block, scratch, nb)[0] == 0


def test_type_table_is_covered(built):
    """Every reduce code of the library's type table appears in group C, in both ops, orders and rank counts."""
    import mscclpp_amd as m
    from test_reduce_gpu import type_table

    tab = type_table()
    assert sorted(tab) == sorted(C.C_TYPES) == list(range(15))
    for code, (tdt, accum) in tab.items():
        assert m.reduce_code(tdt, accum) == code
        for op in (O.SUM, O.MIN):
            assert {(code, op, a, n) for a in C.ALGOS for n in (3, 8)} <= set(C.C_CASES)
    _launchable(C.C_BLOCK, *C.C_GRID, 8)
    assert C.C_BLOCK // 16 >= 2 * C.C_GRID[0]          # every slice has full units on every workgroup
    for code in C.C_TYPES:                              # the planted groups fit
        assert 3 * C.C_BLOCK // O.itemsize(code) >= K.EDGE_GROUPS * K.EDGE_LANES


def _calls(code, op, algo, n):
    cid = C.case_id("C", code, op, algo, n)
    for call, family in enumerate(C.families(code)):
        yield family, C.reduce_inputs(code, op, n, n * C.C_BLOCK // O.itemsize(code), cid, call, family)


@pytest.mark.parametrize("code,op,algo,n", C.C_CASES, ids=lambda v: str(v))
def test_reduce_rows_are_not_vacuous(code, op, algo, n):
    block = C.C_BLOCK
    seen = set()
    differs_from_fp64 = False
    for family, ins in _calls(code, op, algo, n):
        for a in ins:                                  # no two buffers of a case share content
            key = C.as_bytes(a).tobytes()
            assert key not in seen
            seen.add(key)
        exp = C.rs_expected(code, op, ins, block, C.ORDER[algo])
        slices = [exp[r * block:(r + 1) * block].tobytes() for r in range(n)]
        assert len(set(slices)) == n                   # a wrong slice offset is visible
        assert all(np.mean(exp[:block] != C.as_bytes(a)[:block]) > 0.25 for a in ins)  # no input passes for the result
        other = C.rs_expected(code, O.SUM if op == O.MIN else O.MIN, ins, block, C.ORDER[algo])
        assert np.mean(other != exp) > 0.25            # MIN and SUM expectations differ
        if code in C.FLOATS and op == O.SUM:
            flipped = C.rs_expected(code, op, ins, block, 1 - C.ORDER[algo])
            assert C.mismatches(code, flipped, exp).size > 0   # a wrong sum order is visible
        if code in C.PLAIN_TYPES and (family == "finite" or code not in C.FLOATS):
            cnt = block // O.itemsize(code)
            for r in range(n):                         # the plain reference admits the oracle, no lane excluded
                sl = [a[r * cnt:(r + 1) * cnt] for a in ins]
                assert C.plain_failures(code, op, sl, exp[r * block:(r + 1) * block].copy()).size == 0
            if code in C.FLOATS and op == O.SUM:
                ref, _ = C.sum_reference(code, ins)
                differs_from_fp64 |= bool(np.any(C.encode(code, ref) != exp.view(C.uint_of(code))))
        if family == "bits" and op == O.MIN and code in C.FLOATS:   # the planted pairings are there
            st = np.stack(ins)
            nan, inf, zero, sub = K.float_classes(code, st)
            sign = (st.astype(np.uint32) >> (8 * O.itemsize(code) - 1)) & 1
            assert np.any(nan.any(0) & ~nan.all(0))
            assert np.any((zero & (sign == 0)).any(0) & (zero & (sign == 1)).any(0) & zero.all(0))
            assert np.any(sub.sum(0) >= 2) and np.any(inf.all(0)) and np.any((inf & (sign == 1)).any(0))
            bases = K.edge_bases(st.shape[1])
            assert len({b * n // st.shape[1] for b in bases}) >= 3   # in the first, a middle and the last slice
    if code in C.FLOATS and op == O.SUM:
        assert differs_from_fp64                       # rounding per step shows: the order matters to the result


@pytest.mark.parametrize("code", C.FLOATS)
def test_finite_family(code):
    a = np.concatenate([C.finite(code, 4096, 77, 0, r) for r in range(8)])
    v = C.decode(code, a)
    assert np.all(np.isfinite(v)) and np.all(v != 0)
    assert np.all(np.abs(v) >= 2.0 ** C.FINITE_EXP[0]) and np.all(np.abs(v) <= 2.0 ** (C.FINITE_EXP[1] + 1))
    assert np.any(v < 0) and np.any(v > 0) and np.unique(a).size > 256
    assert np.array_equal(C.encode(code, v), a)         # encode and decode agree
    # the bound is the derived one and the sum cannot overflow
    ins = [C.finite(code, 512, 78, 0, r) for r in range(8)]
    ref, bound = C.sum_reference(code, ins)
    u = C.UNIT_ROUNDOFF[code]
    assert np.allclose(bound, 7 * u / (1 - 7 * u) * sum(np.abs(C.decode(code, x)) for x in ins) + C.SMALLEST_SUBNORMAL[code],
                       rtol=1e-12, atol=0)
    assert np.all(np.abs(ref) <= 8 * 128)
    # the rounded fp64 sum passes; the neighbouring lane's sum (a wrong offset) does not
    exp = C.encode(code, ref)
    assert C.plain_failures(code, O.SUM, ins, C.as_bytes(exp)).size == 0
    assert C.plain_failures(code, O.SUM, ins, C.as_bytes(np.roll(exp, 1))).size > exp.size // 2


def test_plain_integer_reference():
    a = [np.array([0x7FFFFFFF, 0xFFFFFFFF, 5], np.uint32), np.array([1, 2, 0x80000000], np.uint32)]
    assert C.plain_int(O.I32, O.SUM, a).view(np.uint32).tolist() == [0x80000000, 1, 0x80000005]
    assert C.plain_int(O.I32, O.MIN, a).view(np.uint32).tolist() == [1, 0xFFFFFFFF, 0x80000000]
    assert C.plain_int(O.U32, O.MIN, a).view(np.uint32).tolist() == [1, 2, 5]


def test_guard_and_broadcast_tables():
    for coll, algo, n, code, nbytes, si, so in C.D_CASES:
        item = O.itemsize(code)
        assert n in (3, 8) and si % item == 0 and so % item == 0 and nbytes % item == 0
        if coll != BC:
            _launchable(nbytes, 0, 0, n)
        in_b, out_b = {RS: (n * nbytes, nbytes), AG: (nbytes, n * nbytes), BC: (nbytes, nbytes)}[coll]
        i, o, total = C.d_layout(in_b, out_b, si, so)
        assert i % 256 == si and o % 256 == so and i >= 256 and o >= i + in_b + 252 and total >= o + out_b + 252
    rows = {(c[0], c[3], c[5], c[6]) for c in C.D_CASES}
    for coll in (AG, BC):   # 1-byte offsets of the send side, the receive side and both
        assert {(coll, O.U8, 1, 0), (coll, O.U8, 0, 1), (coll, O.U8, 1, 1)} <= rows
    assert {(RS, O.F16, 0, 0), (RS, O.BF16, 2, 2), (RS, O.F32, 4, 4), (AG, O.F16, 0, 0), (AG, O.F16, 2, 2)} <= rows
    assert {(c[0], c[1], c[2]) for c in C.D_CASES if c[0] != BC} == {(c, a, n) for c in (RS, AG) for a in C.ALGOS
                                                                      for n in (3, 8)}
    assert C.D_BCAST % 16 == 3
    seen = set()
    for n, nbytes, nb, nt in C.E_CASES:
        gnb, gnt = C.bcast_grid(nbytes, nb, nt)
        assert n in (2, 3, 8) and nbytes > 0 and 1 <= gnb <= K.MAX_CHANNELS and gnt in (64, 512)
        seen.add((n, nbytes, nb, nt))
    assert {(n, b, nb, nt) for n in (2, 3, 8) for b in (1, 15, 16, 17, 4097) for nb in (1, 3, 0) for nt in (64, 512)} <= seen
    for k in (1, 3):        # whole sweeps of T * U units, a partial sweep of one unit, a 3-byte tail
        assert all((n, C.E_SWEEP * k + 19, 1, 64) in seen for n in (2, 3, 8))
    assert C.E_SWEEP == 64 * 4 * 16


def test_refusal_and_abi_tables():
    n = C.F_N
    kinds = set()
    for what, args, code in C.F_CASES:
        if what == "coll":
            coll, algo, block, nb, nt = args
            gnb, gnt = C.bulk_grid(nb, nt)
            shape_bad = gnb > K.MAX_CHANNELS or gnt % 64 != 0 or gnt > 512 or gnt < 64
            if shape_bad or algo == "rsag_zc":
                assert code == 4 and block % 16 == 0   # nothing else is wrong with the call
                kinds.add((coll, "shape" if shape_bad else "zc"))
            elif gnt == 512 and gnb * n > C.A_MAX_WIDE_WORKGROUPS:
                assert code == 5 and block % 16 == 0   # more workgroups than the device holds at once
                kinds.add((coll, "resident"))
            else:
                assert code == 5 and (n * block) % (16 * n) != 0
                kinds.add((coll, "block"))
        else:
            root, nbytes = args
            assert code == 4 and (root < 0 or root >= n or nbytes == 0)
            kinds.add((BC, "root" if nbytes else "bytes"))
    assert kinds == {(c, k) for c in (RS, AG) for k in ("shape", "zc", "block", "resident")} | \
        {(BC, "root"), (BC, "bytes")}
    nts = {args[4] for what, args, _ in C.F_CASES if what == "coll" and args[3] == 4}
    assert nts == {32, 96, 576} and any(a[3] == K.MAX_CHANNELS + 1 for w, a, _ in C.F_CASES if w == "coll")
    _launchable(C.F_BLOCK, 0, 0, n)
    assert C.ABI_BLOCK % 16 == 0 and C.ABI_OFFSET % 16 == 0 and C.ABI_OFFSET > 0 and C.ABI_ODD % 2 == 1
    assert C.ABI_SMALL % 16 != 0 and C.ABI_SMALL % 2 == 0
    assert C.handshakes(RS, 3) == 6 and C.handshakes(AG, 3) == 4 and C.handshakes(BC) == 2
