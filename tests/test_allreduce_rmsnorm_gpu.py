"""kernels/allreduce_rmsnorm_ll.hip with in-process ranks on one GPU against the numpy model: res_out bit for
bit, y within 2 ulp of the fp64 reference and the same on every rank, guards intact.  The shapes: one unit; fewer
units than lanes, no multiple of a wave; one unit per lane; one lane with a second unit; more rows than the
default grid; eight units per lane.  Then the per-lane counts that round up to a template value (3 -> 4; 5, 6, 7 ->
8, the slots past the row's end dead in every lane), three and more rows per workgroup at 8 units per lane, and
explicit lane counts."""
import numpy as np
import pytest

import allreduce_rmsnorm_model as M

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4), (3, 252), (1, 1024), (5, 1028), (65, 64), (2, 8192)]
# (rows, cols, lanes or 0): units per lane 3 -> 4, 5 -> 8, 7 -> 8, 6 -> 8 at 512 lanes, and 7 -> 8 with one lane in slot 6
ROUNDED = [(2, 3072, 0), (2, 5120, 0), (2, 7168, 0), (2, 12288, 512), (2, 6148, 0)]
MULTI_ROW = [(7, 4104), (7, 8192)]  # with 2 workgroups: 4 and 3 rows each, 5 -> 8 and 8 units per lane
LANES = [(4, 512, 64), (4, 512, 128), (4, 512, 512), (4, 2048, 64)]  # the last: 8 units per lane on one wave
_ranks = {}


def ranks_of(n):
    """One set of ranks per rank count: scratch and flags carry on from case to case, as a communicator's do."""
    import mscclpp_amd as m

    if n not in _ranks:
        _ranks[n] = m.InProcessRanks(n, max(m.all_reduce_rms_norm_scratch_required(n, r, c, m.F16) for r, c, *_ in SHAPES + ROUNDED + MULTI_ROW + LANES))
    return _ranks[n]


def run(n, dt, rows, cols, mode, seed, **shape):
    """One call on fresh inputs; returns rank 0's y patterns after every check (M.run_on)."""
    ranks = ranks_of(n)
    xs, res, gamma = M.inputs(seed, n, rows, cols, dt, mode != "none")
    return M.run_on(ranks, ranks.all_reduce_rms_norm, xs, res, gamma, dt, mode, **shape)


@pytest.mark.parametrize("mode", ["none", "out_of_place", "in_place"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dt", M.DTYPES)
@pytest.mark.parametrize("n", [2, 3, 8])
def test_three_calls_match_the_model(built, n, dt, shape, mode):
    for call in range(3):
        run(n, dt, shape[0], shape[1], mode, seed=[n, M.DTYPES.index(dt), shape[0], shape[1], call])


@pytest.mark.parametrize("dt", M.DTYPES)
def test_the_grid_changes_no_bit_of_y(built, dt):
    got = [run(8, dt, 5, 1028, "out_of_place", seed=7, nblocks=nb) for nb in (0, 1, 7)]
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    got = [run(8, dt, 7, 4104, "out_of_place", seed=8, nblocks=nb) for nb in (0, 1, 2)]
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


modes = pytest.mark.parametrize("mode", ["none", "out_of_place", "in_place"])
dtypes = pytest.mark.parametrize("dt", M.DTYPES)
two_and_eight = pytest.mark.parametrize("n", [2, 8])


@modes
@pytest.mark.parametrize("shape", ROUNDED, ids=lambda s: "%dx%d-%d" % s)
@dtypes
@two_and_eight
def test_units_per_lane_that_round_up(built, n, dt, shape, mode):
    run(n, dt, shape[0], shape[1], mode, seed=[n, shape[1], len(mode)], nthreads=shape[2])


@modes
@pytest.mark.parametrize("shape", MULTI_ROW, ids=lambda s: "%dx%d" % s)
@dtypes
@two_and_eight
def test_a_workgroup_with_three_and_four_rows(built, n, dt, shape, mode):
    run(n, dt, shape[0], shape[1], mode, seed=[n, shape[1], len(mode)], nblocks=2)


@modes
@pytest.mark.parametrize("shape", LANES, ids=lambda s: "%dx%d-%d" % s)
@dtypes
@two_and_eight
def test_explicit_lanes(built, n, dt, shape, mode):
    """The order of the row sum is a function of (cols, nthreads): the same lanes give the same bits twice; other
    lanes need not."""
    got = [run(n, dt, shape[0], shape[1], mode, seed=[n, shape[2], len(mode)], nthreads=shape[2]) for _ in range(2)]
    assert np.array_equal(got[0], got[1])
