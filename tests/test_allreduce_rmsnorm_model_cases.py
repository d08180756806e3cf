"""What the input blocks of allreduce_rmsnorm_model.py can see, on the numpy model alone (no GPU, no library):
`order_inputs` tell every other summation order from rank order in at least a quarter of res_out (the ordinary
`inputs` in no element), `eps_inputs` tell a dropped, doubled or misplaced eps from the definition by more than
2 ulp in every row that is not zero, `judge` reports each of these mutants, the special rows have the classes
the definition gives them, and no block comes near FLT_MAX.  Prints the share of res_out each order changes."""
import numpy as np
import pytest

import allreduce_rmsnorm_model as M

ROWS, COLS = 8, 256
CASES = [(dt, n, residual) for dt in M.DTYPES for n in (2, 3, 8) for residual in (False, True)]
case = pytest.mark.parametrize("dt,n,residual", CASES, ids=lambda v: str(v))

# eps dropped, doubled, added outside the square root
EPS_MUTANTS = {"dropped": lambda ms, eps: 1.0 / np.sqrt(ms), "doubled": lambda ms, eps: 1.0 / np.sqrt(ms + 2 * eps),
               "outside": lambda ms, eps: 1.0 / (np.sqrt(ms) + eps)}


def as_patterns(y64, dt):
    return M.encode(y64.astype(np.float32), dt)


@case
def test_every_other_order_changes_a_quarter_of_res_out(dt, n, residual):
    xs, res, gamma = M.order_inputs([1, n], n, ROWS, COLS, dt, residual)
    zq, y64 = M.model(xs, res, gamma, dt)
    assert M.judge(xs, res, gamma, dt, as_patterns(y64, dt), zq if residual else None) == []
    for order in M.alternative_orders(n, residual):
        other, other_y = M.model(xs, res, gamma, dt, order=order)
        share = float((other != zq).mean())
        print(f"{dt} n={n} residual={residual} {order}: {share:.3f} of res_out differs")
        assert share >= 0.25, (order, share)
        # without a residual res_out is not stored: there the order shows through y, beyond the 2 ulp allowed
        bad = M.judge(xs, res, gamma, dt, as_patterns(other_y, dt), other if residual else None)
        assert any("ulp" in b for b in bad) and (not residual or any("res_out" in b for b in bad)), (order, bad)


@case
def test_the_ordinary_inputs_cannot_see_the_order(dt, n, residual):
    """Every fp32 add of `inputs` is exact: why order_inputs exist."""
    xs, res, _ = M.inputs([2, n], n, 64, 2048, dt, residual)
    assert int((M.zq_under(xs, res, dt, "reversed") != M.zq_under(xs, res, dt)).sum()) == 0


@case
def test_eps_shows_in_every_row(dt, n, residual):
    xs, res, gamma = M.eps_inputs([3, n], n, ROWS, COLS, dt, residual)
    zero = ROWS // 2
    live = np.arange(ROWS) != zero
    for eps in M.EPS_VALUES:
        zq, y64 = M.model(xs, res, gamma, dt, eps)
        assert np.isfinite(y64).all() and not y64[zero].any() and not zq[zero].any()
        assert M.judge(xs, res, gamma, dt, as_patterns(y64, dt), zq if residual else None, eps) == []
        for name, rstd in EPS_MUTANTS.items():
            if name == "outside" and eps == 1.0:  # sqrt(ms) + 1 and sqrt(ms + 1) differ by sqrt(ms) < 2^-10: not visible
                continue
            with np.errstate(all="ignore"):
                _, mutant = M.model(xs, res, gamma, dt, eps, rstd=rstd)
            err = M.ulps(as_patterns(mutant, dt)[live], y64[live], dt)
            assert (np.nan_to_num(err, nan=np.inf).max(axis=1) > 2.0).all(), (name, float(eps))
            if name == "dropped":
                assert not np.isfinite(mutant[zero]).any()
            assert M.judge(xs, res, gamma, dt, as_patterns(mutant, dt), zq if residual else None, eps), (name, float(eps))


@case
def test_special_rows_have_their_classes_and_judge_holds_them(dt, n, residual):
    row, c = 1, COLS // 3
    for kind in M.SPECIALS[dt]:
        xs, res, gamma = M.special_inputs([4, n], n, 3, COLS, dt, residual, kind, row)
        plain = M.model(*M.inputs([4, n], n, 3, COLS, dt, residual), dt)
        zq, y64 = M.model(xs, res, gamma, dt)
        got = as_patterns(y64, dt)
        assert M.judge(xs, res, gamma, dt, got, zq if residual else None) == [], kind
        others = np.arange(COLS) != c
        if kind != "gamma":  # the neighbours are the ordinary rows, untouched
            assert np.array_equal(zq[[0, 2]], plain[0][[0, 2]]) and np.array_equal(y64[[0, 2]], plain[1][[0, 2]])
        if kind in ("nan", "inf_minus_inf"):
            assert M.is_nan(zq[row, c], dt) and np.isnan(y64[row]).all()
        elif kind in ("inf", "overflow"):
            assert zq[row, c] == M.INF[dt] and np.isnan(y64[row, c]) and not y64[row, others].any()
        elif kind == "big":
            assert np.isfinite(M.decode(zq[row], dt)).all() and not y64[row].any()
        elif kind == "subnormal":
            assert (np.abs(M.decode(zq[row], dt)) < (n + 1) * 2.0 ** M.EMIN[dt]).all() and y64[row].any()
        elif kind == "neg_zero":
            assert (zq[row] == 0x8000).all() and not y64[row].any()
        else:
            assert not y64[:, 0::3].any() and (np.sign(y64[:, 1::3]) == -np.sign(M.decode(zq, dt)[:, 1::3])).all()
        if kind in ("nan", "inf", "inf_minus_inf", "overflow"):
            # a y that is a number where NaN is due, and a NaN row's neighbour that has been perturbed
            finite = got.copy()
            finite[row, c] = 0
            assert any("NaN" in b for b in M.judge(xs, res, gamma, dt, finite, None)), kind
            spilt = got.copy()
            spilt[row + 1, 5] = M.QNAN[dt]
            assert M.judge(xs, res, gamma, dt, spilt, None), kind
            nudged = got.copy()
            nudged[row - 1, 7] += 3  # three spacings of the element type
            assert M.judge(xs, res, gamma, dt, nudged, None), kind
            if residual:  # res_out: any NaN pattern where the model has one, nothing else
                other_nan = zq.copy()
                other_nan[M.is_nan(zq, dt)] |= 1
                assert M.judge(xs, res, gamma, dt, got, other_nan) == []
                other_nan[row + 1, 5] ^= 1
                assert M.judge(xs, res, gamma, dt, got, other_nan), kind


@case
def test_every_block_keeps_away_from_flt_max(dt, n, residual):
    assert M.in_band(*M.inputs([5, n], n, ROWS, 2056, dt, residual)[:2], dt)
    assert M.in_band(*M.order_inputs([5, n], n, ROWS, 2056, dt, residual)[:2], dt)
    assert M.in_band(*M.eps_inputs([5, n], n, ROWS, 2056, dt, residual)[:2], dt)
    for kind in M.SPECIALS[dt]:
        assert M.in_band(*M.special_inputs([5, n], n, 3, 2056, dt, residual, kind, 1)[:2], dt)
    # and the condition does refuse: one element of 2^63.5 puts the row sum at FLT_MAX / 2
    if dt == "bf16":
        xs = [np.zeros((3, 8), np.uint16) for _ in range(n)]
        xs[0][1, 2] = M.encode(np.float32([2.0 ** 63.5]), dt)[0]
        assert not M.in_band(xs, None, dt)
