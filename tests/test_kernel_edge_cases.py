"""CPU check of the case tables in kernel_edge_cases.py, which tests/test_kernel_edges_gpu.py runs on the
GPU: every launch shape is one the launchers accept (or is in the refusal list), the multi-pass rows
take three passes or more, the MIN / uint32 inputs hold the lanes that tell a wrong kernel apart, and
the self-reduce rows reach the forms their comments name.  The oracle and the library's host-side
queries (no GPU) decide; a bad table entry fails here instead of on the GPU box."""
import numpy as np
import pytest

import kernel_edge_cases as K
import oracle_lib as O


def test_launch_shape_tables():
    seen = set()
    for n, dt, count, nb, nt in K.LL16_SHAPE_CASES:
        assert 2 <= n <= 8 and nt % 64 == 0 and 0 <= nt <= 512 and (nb == 0 or n - 1 <= nb <= K.FLAG_SLOTS)
        seen.add((n, nb // (n - 1) if nb else 0, nb % (n - 1) != 0, nt))
    for n in (2, 3, 5, 8):
        for nt in (64, 192, 512):
            assert {(n, 1, False, nt), (n, 3, False, nt), (n, 0, False, nt)} <= seen
            if n > 2:  # a grid the launcher rounds down to a multiple of the peer count
                assert (n, 2, True, nt) in seen and K.accepted_ll16_grid(n, 2 * (n - 1) + 1) == 2 * (n - 1)
        assert (n, 0, False, 0) in seen
    assert {dt for _, dt, *_ in K.LL16_SHAPE_CASES} == {O.F16, O.BF16, O.F32}
    # below a wave, and several passes of 64 lanes on one workgroup per peer
    assert any(O.geometry(O.F16, c, n)[3] < 64 for n, _, c, _, _ in K.LL16_SHAPE_CASES)
    assert all(O.geometry(O.F16, 3000 * n + 3, n)[3] > 4 * 64 and (3000 * n + 3) % 4 for n in (2, 3, 5, 8))
    for n, count, units, nb, nt in K.LL16_THRESHOLD_CASES:
        assert O.geometry(O.F16, count, n)[3] == units and nb % (n - 1) == 0 and nt in (64, 512)
    assert {u for _, _, u, _, _ in K.LL16_THRESHOLD_CASES} == {8191, 8192, 8193}
    assert {(n, b) for n, b in K.LL16_DEFAULT_CASES} >= {(n, b) for n in range(2, 9)
                                                         for b in (1024, 32766, 32768, 262142, 262144)}
    for n, count, nb, nt in K.LL8_SHAPE_CASES:
        assert n in (3, 8) and count * 2 <= 16 * K.KIB and nb <= K.FLAG_SLOTS and nt % 64 == 0 and nt <= 512
    w = {c: O.ll_words(O.F16, c) for c in K.LL8_COUNTS}
    assert w[1002] % 2 == 1 and (1002 * 2) % 4 == 0      # a lone trailing packet of a whole word
    assert w[1003] % 2 == 0 and (1003 * 2) % 4 == 2      # a tail below one word
    assert 8192 * 2 == 16 * K.KIB
    for n, dt, count, nb, nt in K.BULK_SHAPE_CASES:
        assert n in (3, 8) and nb <= K.MAX_CHANNELS and nt in (64, 512)
    # most of the default 64 workgroups have no unit: a slice of 256 bytes is 16 units of 16 bytes
    assert K.slice_bytes(8, 1001 * 2) // 16 == 16
    # ragged: a tail below one 16-byte unit, inside the last rank's slice
    assert all(c * 2 % 16 != 0 and K.slice_bytes(n, c * 2) * (n - 1) < c * 2
               for n, dt, c, _, _ in K.BULK_SHAPE_CASES if dt == O.BF16)
    for algo, nb, nt in K.REFUSED_SHAPES:
        limit = K.FLAG_SLOTS if algo in K.LL_ALGOS else K.MAX_CHANNELS
        assert nt % 64 != 0 or nt > 512 or nb > limit


def test_multipass_tables(built):
    import mscclpp_amd as m

    for n, dt, count, scratch, nb, nt in K.MULTIPASS_CASES:
        nbytes = count * K.ITEM[dt]
        for algo in (m.ALGO_FULLMESH, m.ALGO_RSAG):
            assert 3 * scratch <= m.scratch_required(algo, n, nbytes, dt), (n, count)
        ps, passes = K.bulk_passes(n, nbytes, scratch, nb)
        assert ps > 0 and ps % (16 * nb) == 0 and passes >= 3
    n, dt, count, scratch, nb, nt = K.MULTIPASS_CASES[0]
    assert K.bulk_passes(n, count * 2, scratch, nb) == (8192, 9) and K.slice_bytes(n, count * 2) % 8192 == 16
    assert K.MULTIPASS_RS_AG_COUNT * 2 % (16 * n) == 0
    assert 3 * scratch <= m.scratch_required(m.ALGO_FULLMESH, n, K.MULTIPASS_RS_AG_COUNT * 2, dt)
    n, dt, count, scratch, nb, nt = K.MULTIPASS_CASES[1]
    ps, passes = K.bulk_passes(n, count * 4, scratch, nb)
    assert ps == 9984 and K.slice_bytes(n, count * 4) % ps != 0  # a partial last pass
    n, dt, count, scratch, nb, nt = K.MULTIPASS_REFUSED
    assert K.bulk_passes(n, count * K.ITEM[dt], scratch, nb)[0] == 0


@pytest.mark.parametrize("algo,dt,op,n", K.MIN_U32_CASES)
def test_min_and_u32_cases_are_not_vacuous(algo, dt, op, n):
    count = K.min_u32_count(algo, dt)
    assert algo != "allpair" or count * K.ITEM[dt] <= 16 * K.KIB
    for seq in range(3):
        ins = K.inputs(dt, n, count, seq=seq, special=True, edges=K.is_float(dt))
        exp, _ = K.expected(algo, dt, op, ins, count)
        e = exp[0].view(ins[0].dtype)
        assert np.mean(e != ins[0]) >= 0.5  # the result is not rank 0's input
        if dt == O.U32:
            # a kernel that took the int32 path would be wrong in these lanes
            signed, _ = K.expected(algo, O.I32, op, ins, count)
            differ = np.mean(signed[0].view(np.uint32) != e)
            assert differ >= 0.01 if op == O.MIN else differ == 0  # (the sum is the same in both)
            assert np.mean(np.stack(ins) >= 2**31) >= 0.05
        if K.is_float(dt):
            st = np.stack(ins)
            nan, inf, zero, sub = K.float_classes(dt, st)
            sign = (st.astype(np.uint32) >> (8 * K.ITEM[dt] - 1)) & 1
            assert np.any(nan.any(0) & ~nan.all(0))                               # NaN against a number
            assert np.any((zero & (sign == 0)).any(0) & (zero & (sign == 1)).any(0) & zero.all(0))  # +0 against -0
            assert np.any(sub.sum(0) >= 2) and np.any(K.float_classes(dt, e)[3])  # subnormals, one of them the result
            assert np.any((inf & (sign == 0)).any(0) & ~inf.all(0))               # +inf against numbers
            assert np.any((inf & (sign == 1)).any(0)) and np.any(inf.all(0))      # -inf; +inf in every rank
            # the planted lanes lie in the first, a middle and the last rank's part, and in the last 8 lanes
            bases = K.edge_bases(count)
            assert bases[0] == 0 and bases[-1] == count - K.EDGE_LANES and len(set(b * n // count for b in bases)) >= 3


def test_guard_tables():
    assert {a for a, *_ in K.GUARD_CASES} == set(K.ALGOS)
    assert any(c * K.ITEM[dt] % 16 == 0 for dt, c in K.GUARD_SIZES)
    assert {dt for dt, c in K.GUARD_SIZES if c * K.ITEM[dt] % 16} == {O.F16, O.BF16, O.F32, O.I32}
    for dt, count in K.GUARD_SIZES:
        nbytes, item = count * K.ITEM[dt], K.ITEM[dt]
        for view in (False, True):
            i, o, total = K.arena_layout(nbytes, item, view)
            assert i >= 256 and o >= i + nbytes + 256 and total >= o + nbytes + 256
            assert i % item == 0 and o % item == 0
            assert (i % 16 != 0 and o % 16 != 0) if view else (i % 256 == 0 and o % 256 == 0)


def test_self_reduce_tables(built):
    import mscclpp_amd as m

    for nbytes, nb, waves, grid, rounds, skew in K.SELF_REDUCE_CASES:
        assert nbytes % 16 == 0 and 0 < nb <= 1024
        assert K.self_reduce_shape_rule(nbytes, nb) == (waves, grid, rounds, skew)
        assert m.self_reduce_shape(nbytes, nb) == (waves, 1, grid, skew)  # the launcher's own answer (host only)
    forms = {(r == 1, s) for *_, r, s in K.SELF_REDUCE_CASES}
    assert forms == {(True, 0), (False, 1), (False, 2)}
    # the default shape for the band the (2 MiB, 512) row bypasses
    assert K.self_reduce_shape_rule(2048 * K.KIB, 0) == (8, 256, 1, 0)
    assert m.self_reduce_shape(2048 * K.KIB) == (8, 1, 256, 0)
    # one round is always the plain form: no grid reaches (skew 0, more than one round)
    for nbytes in (16, 4096, 64 * K.KIB, 4096 * K.KIB + 16):
        for nb in (1, 2, 6, 512, 1024):
            _, _, rounds, skew = K.self_reduce_shape_rule(nbytes, nb)
            assert (skew == 0) == (rounds == 1)
    with pytest.raises(m.MscclppError) as e:
        m.self_reduce_shape(4096, 1025)
    assert e.value.code == 4
