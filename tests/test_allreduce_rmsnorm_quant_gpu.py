"""kernels/allreduce_rmsnorm_quant_ll.hip with in-process ranks on one GPU, judged by §17k's and §17l's
own judges: res_out bit for bit against the numpy model; q and scale equal on all ranks and grids, bit for bit steps
5-7 in numpy on all_reduce_rms_norm's y at the same (cols, nthreads), and within the bounds of an fp64 reference;
guards intact.  The shapes are those at which the layout of 8-lane blocks can go wrong (SHAPES)."""
import functools

import numpy as np
import pytest

import allreduce_rmsnorm_model as M
import test_allreduce_rmsnorm_mx_pull_gpu as MX
import test_allreduce_rmsnorm_quant_pull_gpu as ROW

pytestmark = pytest.mark.gpu

FORMATS = ("fp8_row",) + MX.FORMATS
# one block on 8 live lanes; several rows of it; three blocks; 520 units -> 4 per lane, the last slot one 8-lane block;
# 8 units per lane; 8 per lane on one wave (no cross-wave word); 512 lanes; 4 and 3 rows per workgroup at 5 -> 8 units
SHAPES = [(1, 32, {}), (7, 32, {}), (3, 96, {}), (5, 2080, {}), (2, 8192, {}), (4, 2048, dict(nthreads=64)),
          (4, 512, dict(nthreads=512)), (7, 4128, dict(nblocks=2))]
ROW_ONLY = [(1, 4, {}), (5, 1028, {})]  # fp8_row: one unit; one lane alone in slot 1


@functools.lru_cache(None)
def ranks_of(n):
    import mscclpp_amd as m

    return m.InProcessRanks(n, max(m.all_reduce_rms_norm_scratch_required(n, r, c, m.F16) for r, c, _ in SHAPES + [(19, 96, 0)]))


def run(n, dt, fmt, xs, res, gamma, mode, skip=(), **shape):
    """One call, every rank judged, also on all_reduce_rms_norm's y of the same inputs.  -> rank 0's (q, scale, counts)."""
    import torch

    ranks, (rows, cols), row = ranks_of(n), xs[0].shape, fmt == "fp8_row"
    y = M.run_on(ranks, ranks.all_reduce_rms_norm, xs, res, gamma, dt, mode, **shape)
    mk = lambda r, c, bits=None: [M.Guarded(torch, r, c, dt, bits and bits[k]) for k in range(n)]  # bits: per rank
    x, g = mk(rows, cols, xs), mk(1, cols, [gamma.reshape(1, cols)] * n)
    qcols, nsc = cols // 2 if fmt == "mxfp4" else cols, rows * 4 if row else rows * cols // 32  # bytes: a row of q, a scale
    q, sc = mk(rows, qcols // 2), mk(1, nsc // 2 + 8)  # rank k's MX scale: nsc bytes from byte k on, guards around them
    off = [0 if row else k for k in range(n)]
    scale = lambda k, b: b.t.view(torch.uint8).view(-1)[off[k]:off[k] + nsc]
    r_in = mk(rows, cols, [res] * n) if mode != "none" else None
    r_out = r_in if mode != "out_of_place" else mk(rows, cols)
    ts = lambda bs: bs and [b.t for b in bs]
    ranks.all_reduce_rms_norm_quant(ts(x), [b.t.view(torch.uint8) for b in q],
                                    [scale(k, b).view(torch.float32) if row else scale(k, b).view(rows, cols // 32)
                                     for k, b in enumerate(sc)],
                                    [b.t[0] for b in g], fmt, ts(r_in), ts(r_out), eps=float(M.EPS), **shape)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    ref, worst, got, seen = M.model(xs, res, gamma, dt), 0.0, [], (1, 1, 1)
    keep = [r for r in range(rows) if r not in skip]
    for r in range(n):
        (qb, ok_q), (sb, ok_s), (rb, ok_r) = q[r].read(), sc[r].read(), r_out[r].read() if r_out else (None, True)
        sb = sb.view(np.uint8).reshape(-1)
        assert ok_q and ok_s and ok_r and (np.r_[sb[:off[r]], sb[off[r] + nsc:]] == 0xA5).all(), f"guard bytes of rank {r} overwritten"
        qb, sb = qb.view(np.uint8).reshape(rows, qcols), sb[off[r]:off[r] + nsc]
        if row:
            got.append((qb, sb.view(np.float32)))
            bad, ratio = ROW.judge(torch, ref, dt, *got[r], rb, skip)
            want_q, want_s = ROW.steps_5_to_7(torch, y, dt)
            bad += [] if np.array_equal(got[r][1][keep].view(np.uint32), want_s[keep].view(np.uint32)) else ["scale differs from steps 5-6"]
            bad += [] if np.array_equal(qb[keep], want_q[keep]) else ["q differs from step 7"]
        else:
            got.append((qb, sb.reshape(rows, cols // 32)))
            bad, ratio, seen = MX.judge(ref, y, dt, fmt, *got[r], rb, skip)
        worst = max(worst, ratio)
        assert not bad, (r, bad)
        assert np.array_equal(got[r][0], got[0][0]) and np.array_equal(got[r][1].view(np.uint8), got[0][1].view(np.uint8))
    print(f"n={n} {dt} {fmt} {rows}x{cols} {mode} {shape}: worst q error {worst:.3f} of its bound")
    return got[0] + (seen,)


def gamma_of(fmt, seed, cols, dt, plain):
    return plain if fmt == "fp8_row" else MX.block_gamma(seed, cols, dt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dt", M.DTYPES)
@pytest.mark.parametrize("n", [2, 3, 8])
def test_two_calls_match_the_references(built, n, dt, fmt):
    """Every shape twice on fresh inputs (out of place; (5, 2080) also without a residual and in place); then five rows
    of which row 1 is all zero and row 3 has a NaN term (q and scale unspecified there): no device error, the others judged."""
    seen = np.zeros(3, int)
    for shape in SHAPES + (ROW_ONLY if fmt == "fp8_row" else []):
        rows, cols, kw = shape
        for call in range(2):
            for mode in ("none", "out_of_place", "in_place") if (shape == SHAPES[3] and call) else ("out_of_place",):
                xs, res, gamma = M.inputs([n, M.DTYPES.index(dt), rows, cols, call], n, rows, cols, dt, mode != "none")
                seen += run(n, dt, fmt, xs, res, gamma_of(fmt, [cols, call], cols, dt, gamma), mode, **kw)[2]
    assert seen.min() > 0, f"ties, saturated elements, zero blocks met: {seen}"
    xs, res, gamma = M.inputs([9, n], n, 5, 2080, dt, True)
    for t in xs + [res]:
        t[1] = 0
    xs[1][3, 693] = M.QNAN[dt]
    run(n, dt, fmt, xs, res, gamma_of(fmt, 9, 2080, dt, gamma), "out_of_place", skip=(3,))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dt", M.DTYPES)
def test_the_grid_changes_no_bit(built, dt, fmt):
    xs, res, gamma = M.inputs(7, 8, 19, 96, dt, True)
    got = [run(8, dt, fmt, xs, res, gamma_of(fmt, 7, 96, dt, gamma), "out_of_place", nblocks=nb) for nb in (0, 1, 2)]
    for q, s, _ in got[1:]:
        assert np.array_equal(q, got[0][0]) and np.array_equal(s.view(np.uint8), got[0][1].view(np.uint8))
