"""Both fused AllReduce + RMSNorm kernels (allreduce_rmsnorm_ll.hip, allreduce_rmsnorm_pull.hip) on the blocks of
allreduce_rmsnorm_model.py that make the definition's steps visible (test_allreduce_rmsnorm_model_cases.py shows
that they do): adds that round (summation order), ms far below eps, and non-finite, overflowing, subnormal and
signed-zero rows between ordinary rows of one workgroup.  In-process ranks, the judges of `run_on`."""
import pytest

import allreduce_rmsnorm_model as M

pytestmark = pytest.mark.gpu

COLS = (256, 2056)  # one unit per lane with lanes to spare; a second (LL: third) unit for a few lanes
ROWS = {2: 6, 3: 9, 8: 12}  # the pull kernel's slices: 3 rows per rank; at 8 ranks 2 rows for six of them, none for two
_ranks = {}


def ranks_of(n):
    """One set of ranks per rank count, the LL scratch sized for this file's largest shape."""
    import mscclpp_amd as m

    if n not in _ranks:
        _ranks[n] = m.InProcessRanks(n, m.all_reduce_rms_norm_scratch_required(n, ROWS[n], max(COLS), m.F16))
    return _ranks[n]


def run(n, ll, block, dt, mode, eps=M.EPS):
    """block = (xs, res, gamma).  One workgroup per rank: the pull kernel's owns its rank's whole slice, the LL
    kernel's every row, so every row shares its LDS words and registers with the rows around it."""
    ranks = ranks_of(n)
    fn = ranks.all_reduce_rms_norm if ll else ranks.all_reduce_rms_norm_pull
    return M.run_on(ranks, fn, *block, dt, mode, eps, nblocks=1)


kernels = pytest.mark.parametrize("ll", [True, False], ids=["ll", "pull"])
dtypes = pytest.mark.parametrize("dt", M.DTYPES)


@pytest.mark.parametrize("mode", ["none", "out_of_place", "in_place"])
@pytest.mark.parametrize("n", [2, 3, 8])
@dtypes
@kernels
def test_the_sum_is_taken_in_rank_order(built, ll, dt, n, mode):
    """res_out bit for bit where it is stored; without a residual the order shows through y (the CPU test: the
    reversed order's y is beyond 2 ulp on these blocks)."""
    for cols in COLS:
        run(n, ll, M.order_inputs([n, cols, len(mode)], n, ROWS[n], cols, dt, mode != "none"), dt, mode)


@pytest.mark.parametrize("eps", M.EPS_VALUES, ids=lambda e: "eps%g" % e)
@dtypes
@kernels
def test_eps_is_added_under_the_root(built, ll, dt, eps):
    for cols in COLS:
        for n, mode in ((2, "none"), (3, "out_of_place"), (8, "in_place")):
            rows = ROWS[n]
            y = run(n, ll, M.eps_inputs([n, cols], n, rows, cols, dt, mode != "none"), dt, mode, eps)
            assert not (y[rows // 2] & 0x7FFF).any(), "the all-zero row's y is not zero"


@pytest.mark.parametrize("dt,kind", [(dt, kind) for dt in M.DTYPES for kind in M.SPECIALS[dt]])
@kernels
def test_a_special_row_between_ordinary_ones(built, ll, dt, kind):
    """3 ranks, 9 rows, the special row in the middle of rank 1's slice (rows 3 - 5), with and without a residual;
    then two ordinary calls, one per LL scratch half, which a NaN left behind in LDS or scratch would spoil."""
    n, rows, row = 3, ROWS[3], 4
    for cols in COLS:
        for mode in ("out_of_place", "none", "in_place"):
            seed = [cols, len(mode)]
            xs, res, gamma = M.special_inputs(seed, n, rows, cols, dt, mode != "none", kind, row)
            y = run(n, ll, (xs, res, gamma), dt, mode)
            # the class of the row, stated here apart from the model
            if kind in ("nan", "inf_minus_inf"):
                assert M.is_nan(y[row], dt).all()
            elif kind in ("inf", "overflow"):
                assert M.is_nan(y[row, cols // 3], dt) and int((y[row] & 0x7FFF != 0).sum()) == 1
            elif kind in ("big", "neg_zero"):
                assert not (y[row] & 0x7FFF).any()
            elif kind == "gamma":
                assert not (y[:, 0::3] & 0x7FFF).any()
            for call in (1, 2):
                run(n, ll, M.inputs(seed + [call], n, rows, cols, dt, mode != "none"), dt, mode)
