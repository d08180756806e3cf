"""kernels/allreduce_rmsnorm_mx_pull.hip with in-process ranks on one GPU: res_out bit for bit against
the numpy model; q and scale equal on all ranks and grids, bit for bit steps 5-7 in numpy on all_reduce_rms_norm_pull's
y, and within the bound of an fp64 reference; guards intact.  gamma carries a magnitude 2^k per block of 32 columns,
one all-zero block and negative entries, so the blocks of a row need different scales."""
import functools

import numpy as np
import pytest

import allreduce_rmsnorm_model as M
from test_allreduce_rmsnorm_quant_pull_gpu import ulp

pytestmark = pytest.mark.gpu

FORMATS = ("mxfp8", "mxfp4")
# the finite magnitudes of the element format by code (the code's low bit is the mantissa's)
TABLE = {"mxfp8": np.array([(c & 7) * 2.0 ** -9 if c < 8 else (8 + (c & 7)) * 2.0 ** ((c >> 3) - 10) for c in range(127)]),
         "mxfp4": np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6.0])}
EXPS = {"mxfp8": (8, -6, 3), "mxfp4": (2, 0, 1)}  # (emax, the smallest normal exponent, mantissa bits)
SHAPES = [(1, 32, 0), (7, 32, 0), (3, 96, 0), (5, 2080, 0), (3, 5120, 0), (2, 16384, 0), (None, 2080, 1), (None, 2080, 2)]
ranks_of = functools.lru_cache(None)(lambda n: __import__("mscclpp_amd").InProcessRanks(n, 1 << 16))


def exponent_rule(amax, fmt):
    """Step 6 on fp64 magnitudes (of fp32's range): max(e32(amax) - emax, 0)."""
    with np.errstate(divide="ignore"):
        e32 = np.where(amax < 2.0 ** -126, 0, np.floor(np.log2(np.maximum(amax, 2.0 ** -126))) + 127)
    return np.maximum(e32 - EXPS[fmt][0], 0)


def quantise(y, fmt, truncate=False):
    """Steps 5-7 on finite y [rows, cols] -> (codes, sign on top; E [rows, cols / 32]; ties, saturated, zero blocks met)."""
    rows, cols = y.shape
    blocks = y.astype(np.float64).reshape(rows, cols // 32, 32)
    amax = np.abs(blocks).max(axis=2)
    E = exponent_rule(amax, fmt)
    table = TABLE[fmt]
    p = np.abs(blocks) * np.exp2(127 - E)[:, :, None]  # exact in fp64
    a = np.minimum(p, table[-1])
    lo = np.searchsorted(table, a, side="right") - 1
    hi = np.minimum(lo + 1, len(table) - 1)
    dlo, dhi = a - table[lo], table[hi] - a
    tie = (dlo == dhi) & (hi != lo)
    up = (not truncate) & (hi != lo) & ((dhi < dlo) | (tie & (hi % 2 == 0)))
    code = np.where(up, hi, lo) | np.where(np.signbit(blocks), len(table) + (1 if fmt == "mxfp8" else 0), 0)
    return code.reshape(rows, cols).astype(np.uint8), E.astype(np.uint8), (int(tie.sum()), int((p > table[-1]).sum()),
                                                                           int((amax == 0).sum()))


def block_gamma(seed, cols, dt):
    """gamma of magnitude 2^k per block, k in [-12, 4] (both ends present from three blocks on), a third of it
    negative, the block in the middle of the row zero (from two blocks on)."""
    rng, nb = np.random.default_rng(seed), cols // 32
    k = rng.permutation(np.r_[4, -12, np.arange(-11, 4), rng.integers(-12, 5, max(nb - 17, 0))][:nb])
    g = rng.uniform(0.5, 2.0, cols) * np.repeat(np.exp2(k), 32) * rng.choice([1, 1, -1], cols)
    if nb > 1:
        g[nb // 2 * 32:nb // 2 * 32 + 32] = 0
    return M.encode(g.astype(np.float32), dt)


def fp64_judge(y64, dt, fmt, codes, E):
    """(failed checks of the kernel's codes and E against the fp64 y, worst element error over its bound)."""
    amax, Ek = np.abs(y64).reshape(len(y64), -1, 32).max(axis=2), E.astype(np.float64)
    off = (Ek < exponent_rule(np.maximum(amax - 2 * ulp(amax, dt), 0), fmt)) | (Ek > exponent_rule(amax + 2 * ulp(amax, dt), fmt))
    bad = ["E is the rule of no value within 2 ulp of the reference amax"] if off.any() else []
    X = np.repeat(np.exp2(Ek - 127), 32, axis=1)
    sign_bit = 128 if fmt == "mxfp8" else 8
    d = TABLE[fmt][codes & (sign_bit - 1)] * np.where(codes & sign_bit, -1.0, 1.0) * X
    v = np.clip(y64, -TABLE[fmt][-1] * X, TABLE[fmt][-1] * X)
    _, emin, mant = EXPS[fmt]
    with np.errstate(divide="ignore"):
        spacing = np.exp2(np.maximum(np.floor(np.log2(np.maximum(np.abs(d), np.abs(v)) / X)), emin) - mant)
    ratio = float((np.abs(d - v) / (0.5 * spacing * X + 2 * ulp(y64, dt))).max())
    return bad + ([] if ratio <= 1 else ["q is %.3f of its bound from the fp64 reference" % ratio]), ratio


def judge(ref, y_bits, dt, fmt, q, E, got_res, skip=()):
    """One rank's results against ref = M.model(...) (res_out, fp64_judge) and, bit for bit, against steps 5-7 on the
    pull kernel's y; rows `skip`: no q / scale check.  -> (failed checks, worst ratio, quantise's counts)."""
    keep = [r for r in range(y_bits.shape[0]) if r not in skip]
    codes = (q if fmt == "mxfp8" else np.stack([q & 15, q >> 4], axis=2).reshape(len(q), -1))[keep]  # one per column
    bad, ratio = fp64_judge(ref[1][keep], dt, fmt, codes, E[keep])
    if got_res is not None and ((got_res != ref[0]) & ~(M.is_nan(got_res, dt) & M.is_nan(ref[0], dt))).any():
        bad.append("res_out differs from the model")
    want, want_e, seen = quantise(M.decode(y_bits[keep], dt), fmt)
    bad += [] if np.array_equal(E[keep], want_e) else ["scale differs from steps 5-6"]
    bad += [] if np.array_equal(codes, want) else ["q differs from step 7"]
    return bad, ratio, seen


def run(n, dt, fmt, xs, res, gamma, mode, skip=(), **shape):
    """One call, every rank judged, also on all_reduce_rms_norm_pull's y of the same inputs.  -> rank 0's (q, E, counts)."""
    import torch

    ranks, (rows, cols) = ranks_of(n), xs[0].shape
    y = M.run_on(ranks, ranks.all_reduce_rms_norm_pull, xs, res, gamma, dt, mode, **shape)
    mk = lambda r, c, bits=None: [M.Guarded(torch, r, c, dt, bits and bits[k]) for k in range(n)]  # bits: per rank
    x, g = mk(rows, cols, xs), mk(1, cols, [gamma.reshape(1, cols)] * n)
    qcols, nsc = cols if fmt == "mxfp8" else cols // 2, rows * cols // 32  # bytes of a row of q, and of a scale
    q, sc = mk(rows, qcols // 2), mk(1, nsc // 2 + 8)  # rank k's scale: nsc bytes from byte k on, guards around them
    r_in = mk(rows, cols, [res] * n) if mode != "none" else None
    r_out = r_in if mode != "out_of_place" else mk(rows, cols)
    ts = lambda bs: bs and [b.t for b in bs]
    ranks.all_reduce_rms_norm_mx_pull(ts(x), [b.t.view(torch.uint8) for b in q],
                                      [b.t.view(torch.uint8).view(-1)[k:k + nsc].view(rows, cols // 32) for k, b in enumerate(sc)],
                                      [b.t[0] for b in g], fmt, ts(r_in), ts(r_out), eps=float(M.EPS), **shape)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    ref, worst, got = M.model(xs, res, gamma, dt), 0.0, []
    for r in range(n):
        (qb, ok_q), (sb, ok_s), (rb, ok_r) = q[r].read(), sc[r].read(), r_out[r].read() if r_out else (None, True)
        sb = sb.view(np.uint8).reshape(-1)
        assert ok_q and ok_s and ok_r and (np.r_[sb[:r], sb[r + nsc:]] == 0xA5).all(), f"guard bytes of rank {r} overwritten"
        got.append((qb.view(np.uint8).reshape(rows, qcols), sb[r:r + nsc].reshape(rows, cols // 32)))
        bad, ratio, seen = judge(ref, y, dt, fmt, *got[r], rb, skip)
        worst = max(worst, ratio)
        assert not bad, (r, bad)
        assert np.array_equal(got[r][0], got[0][0]) and np.array_equal(got[r][1], got[0][1])
    print(f"n={n} {dt} {fmt} {rows}x{cols} {mode} {shape}: worst q error {worst:.3f} of its bound")
    return got[0] + (seen,)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dt", M.DTYPES)
@pytest.mark.parametrize("n", [2, 3, 8])
def test_two_calls_match_the_references(built, n, dt, fmt):
    """Every shape twice on fresh inputs (out of place; (5, 2080) also without a residual and in place); then row 2 of
    five with a NaN term (its y is NaN throughout, q and E unspecified): no device error, the other rows judged."""
    seen = np.zeros(3, int)
    for shape in SHAPES:
        rows, cols, kw = shape[0] or 3 * n + 1, shape[1], dict(nblocks=shape[2]) if shape[2] else {}
        for call in range(2):
            for mode in ("none", "out_of_place", "in_place") if (shape == SHAPES[3] and call) else ("out_of_place",):
                xs, res, _ = M.inputs([n, M.DTYPES.index(dt), rows, cols, call], n, rows, cols, dt, mode != "none")
                seen += run(n, dt, fmt, xs, res, block_gamma([cols, call], cols, dt), mode, **kw)[2]
    assert seen.min() > 0, f"ties, saturated elements, zero blocks met: {seen}"
    xs, res, _ = M.inputs([9, n], n, 5, 2080, dt, True)
    xs[1][2, 693] = M.QNAN[dt]
    run(n, dt, fmt, xs, res, block_gamma(9, 2080, dt), "out_of_place", skip=(2,))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dt", M.DTYPES)
def test_the_grid_changes_no_bit(built, dt, fmt):
    xs, res, _ = M.inputs(7, 8, 19, 96, dt, True)
    got = [run(8, dt, fmt, xs, res, block_gamma(7, 96, dt), "out_of_place", nblocks=nb) for nb in (0, 1, 2)]
    for q, e, _ in got[1:]:
        assert np.array_equal(q, got[0][0]) and np.array_equal(e, got[0][1])
