"""kernels/allreduce_rmsnorm_pull.hip with in-process ranks on one GPU against the numpy model: res_out bit for
bit, y within 2 ulp of the fp64 reference and the same on every rank, guards intact.  The shapes: one unit, all
but one rank own nothing; 31 units, rows < 8; one unit per lane, R does not divide the rows; one lane with a
second unit; slices of 3, ..., 3, 1, 0 rows at 8 ranks; four units per lane at 512 lanes."""
import numpy as np
import pytest

import allreduce_rmsnorm_model as M

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8), (3, 248), (9, 2048), (5, 2056), (19, 64), (2, 16384)]
_ranks = {}


def ranks_of(n):
    """One set of ranks per rank count: tokens, counters and flags carry on from case to case."""
    import mscclpp_amd as m

    if n not in _ranks:
        _ranks[n] = m.InProcessRanks(n, m.all_reduce_rms_norm_scratch_required(n, 3, 248, m.F16))
    return _ranks[n]


def run(n, dt, rows, cols, mode, seed, ll=False, **shape):
    """One call on fresh inputs (ll: of the LL kernel); returns rank 0's y patterns after every check."""
    import torch

    ranks = ranks_of(n)
    xs, res, gamma = M.inputs(seed, n, rows, cols, dt, mode != "none")
    g = M.Guarded(torch, 1, cols, dt, gamma.reshape(1, cols))
    x = [M.Guarded(torch, rows, cols, dt, xs[r]) for r in range(n)]
    y = x if mode == "in_place" else [M.Guarded(torch, rows, cols, dt) for _ in range(n)]
    r_in = r_out = None
    if mode != "none":
        r_in = [M.Guarded(torch, rows, cols, dt, res) for _ in range(n)]
        r_out = r_in if mode == "in_place" else [M.Guarded(torch, rows, cols, dt) for _ in range(n)]
    fn = ranks.all_reduce_rms_norm if ll else ranks.all_reduce_rms_norm_pull
    fn([b.t for b in x], [b.t for b in y], [g.t[0]] * n, r_in and [b.t for b in r_in], r_out and [b.t for b in r_out],
       eps=float(M.EPS), **shape)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    ys, rs = [b.read() for b in y], [b.read() for b in r_out] if r_out else [(None, True)] * n
    for r in range(n):
        assert ys[r][1] and rs[r][1], f"guard bytes of rank {r} overwritten"
        bad = M.judge(xs, res, gamma, dt, ys[r][0], rs[r][0])
        assert not bad, (r, bad)
        assert np.array_equal(ys[r][0], ys[0][0]), f"y of rank {r} differs from rank 0's"
    return ys[0][0]


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
