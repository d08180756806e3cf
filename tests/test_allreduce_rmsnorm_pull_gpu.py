"""kernels/allreduce_rmsnorm_pull.hip with in-process ranks on one GPU against the numpy model: res_out bit for
bit, y within 2 ulp of the fp64 reference and the same on every rank, guards intact.  The shapes: one unit, all
but one rank own nothing; 31 units, rows < 8; one unit per lane, R does not divide the rows; one lane with a
second unit; slices of 3, ..., 3, 1, 0 rows at 8 ranks; four units per lane at 512 lanes.  Then three units per
lane, which run as four with the last slot dead in every lane, workgroups with two to four rows at 2 and 4 units
per lane (the prefetch of row i + 1, its re-issue at k0 > 0, the parity buffers), and explicit lane counts."""
import numpy as np
import pytest

import allreduce_rmsnorm_model as M

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8), (3, 248), (9, 2048), (5, 2056), (19, 64), (2, 16384)]
# (rows, cols, lanes or 0): 3 units per lane -> 4; at 6144 slot 2 is full in every lane; 12288 at the default 512 lanes
ROUNDED = [(3, 5120, 256), (3, 6144, 256), (2, 12288, 0)]
MULTI_ROW = [(2056, 0), (5120, 0), (16384, 512)]  # (cols, lanes), rows = 3 n + 1: 2, 4 (rounded) and 4 (full) units per lane
LANES = [(4, 512, 64), (4, 512, 128), (4, 512, 512), (4, 2048, 64)]  # the last: 4 units per lane on one wave
_ranks = {}


def ranks_of(n):
    """One set of ranks per rank count: tokens, counters and flags carry on from case to case."""
    import mscclpp_amd as m

    if n not in _ranks:
        _ranks[n] = m.InProcessRanks(n, m.all_reduce_rms_norm_scratch_required(n, 3, 248, m.F16))
    return _ranks[n]


def run(n, dt, rows, cols, mode, seed, ll=False, **shape):
    """One call on fresh inputs (ll: of the LL kernel); returns rank 0's y patterns after every check (M.run_on)."""
    ranks = ranks_of(n)
    xs, res, gamma = M.inputs(seed, n, rows, cols, dt, mode != "none")
    fn = ranks.all_reduce_rms_norm if ll else ranks.all_reduce_rms_norm_pull
    return M.run_on(ranks, fn, xs, res, gamma, dt, mode, **shape)


@pytest.mark.parametrize("mode", ["none", "out_of_place", "in_place"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dt", M.DTYPES)
@pytest.mark.parametrize("n", [2, 3, 8])
def test_three_calls_match_the_model(built, n, dt, shape, mode):
    for call in range(3):
        run(n, dt, shape[0], shape[1], mode, seed=[n, M.DTYPES.index(dt), shape[0], shape[1], call])


@pytest.mark.parametrize("dt", M.DTYPES)
def test_the_grid_changes_no_bit_of_y(built, dt):
    # 8 ranks: slices of 3, ..., 3, 1, 0 rows; with two workgroups one owns two rows of a slice and one owns one
    got = [run(8, dt, 19, 64, "out_of_place", seed=7, nblocks=nb) for nb in (0, 1, 2)]
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    got = [run(8, dt, 25, 5120, "out_of_place", seed=8, nblocks=nb) for nb in (0, 1, 2)]  # slices of 4 x 6, 1, 0 rows
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


modes = pytest.mark.parametrize("mode", ["none", "out_of_place", "in_place"])
dtypes = pytest.mark.parametrize("dt", M.DTYPES)
two_and_eight = pytest.mark.parametrize("n", [2, 8])


@modes
@pytest.mark.parametrize("shape", ROUNDED, ids=lambda s: "%dx%d-%d" % s)
@dtypes
@two_and_eight
def test_three_units_per_lane_run_as_four(built, n, dt, shape, mode):
    run(n, dt, shape[0], shape[1], mode, seed=[n, shape[1], len(mode)], nthreads=shape[2])


@modes
@pytest.mark.parametrize("nblocks", [1, 2])
@pytest.mark.parametrize("shape", MULTI_ROW, ids=lambda s: "%d-%d" % s)
@dtypes
@two_and_eight
def test_a_workgroup_with_several_rows(built, n, dt, shape, nblocks, mode):
    """rows = 3 n + 1: slices of 4 and 3 rows at 2 ranks, of 4 (six times), 1 and 0 at 8; one workgroup takes a whole
    slice, two take two rows each."""
    run(n, dt, 3 * n + 1, shape[0], mode, seed=[n, shape[0], nblocks, len(mode)], nblocks=nblocks, nthreads=shape[1])


@modes
@pytest.mark.parametrize("shape", LANES, ids=lambda s: "%dx%d-%d" % s)
@dtypes
@two_and_eight
def test_explicit_lanes(built, n, dt, shape, mode):
    """The order of the row sum is a function of (cols, nthreads): the same lanes give the same bits twice; other
    lanes need not."""
    got = [run(n, dt, shape[0], shape[1], mode, seed=[n, shape[2], len(mode)], nthreads=shape[2]) for _ in range(2)]
    assert np.array_equal(got[0], got[1])


def test_calls_alternate_with_the_ll_kernel_and_pull_reduce(built):
    """The token counters are shared with pull_reduce and the ranks' error words with the LL kernel."""
    import mscclpp_amd as m
    import torch

    n, ranks = 3, ranks_of(3)
    run(n, "bf16", 3, 248, "out_of_place", 11, ll=True)
    run(n, "bf16", 3, 248, "out_of_place", 12)
    ins = [torch.full((1000,), float(r + 1), device="cuda") for r in range(n)]
    outs = [torch.empty_like(t) for t in ins]
    ranks.pull_reduce(m.PULL_ALLREDUCE, ins, outs, m.AVG)
    torch.cuda.synchronize()
    assert all(bool((o == 2.0).all()) for o in outs)  # the mean of 1, 2, 3
    run(n, "fp16", 19, 64, "in_place", 13)
    assert ranks.errors() == [0] * n
