"""kernels/allreduce_rmsnorm_quant_pull.hip with in-process ranks on one GPU: res_out bit for bit
against the numpy model; q and scale equal on all ranks and grids, within the bound of an fp64 reference, and bit for
bit steps 5-7 in numpy fp32 on all_reduce_rms_norm_pull's y; guards intact.  Shapes: one unit pair with ranks that own
no row; a partial wave; 1, 2 (ragged), 3-as-4 and 4 units per lane; workgroups of several rows on 1 and 2 workgroups."""
import functools

import numpy as np
import pytest

import allreduce_rmsnorm_model as M

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 0), (3, 240, 0), (9, 2048, 0), (5, 2064, 0), (3, 5120, 0), (2, 16384, 0),
          (None, 2064, 1), (None, 2064, 2), (None, 5120, 1), (None, 5120, 2)]  # (rows or None for 3 n + 1, cols, workgroups)
TINY = np.float32(2.0 ** -126)
ranks_of = functools.lru_cache(None)(lambda n: __import__("mscclpp_amd").InProcessRanks(n, 1 << 16))
shape_of = lambda n, s: (s[0] or 3 * n + 1, s[1], dict(nblocks=s[2]) if s[2] else {})


def ulp(a, dt):
    with np.errstate(divide="ignore"):
        return np.exp2(np.maximum(np.floor(np.log2(np.abs(a))), M.EMIN[dt]) - M.MANT[dt])


def judge(torch, ref, dt, q, scale, got_res, skip=()):
    """(failed checks against ref = M.model(...), worst q error over its bound); rows `skip`: no q / scale check."""
    zq, y64 = ref
    bad = []
    if got_res is not None and ((got_res != zq) & ~(M.is_nan(got_res, dt) & M.is_nan(zq, dt))).any():
        bad.append("res_out differs from the model")
    rows = [r for r in range(y64.shape[0]) if r not in skip]
    y, s = y64[rows], scale[rows].astype(np.float64)[:, None]
    amax = np.abs(y).max(axis=1, keepdims=True)
    zero = amax[:, 0] == 0
    if (s[zero, 0] != TINY).any() or (q[rows][zero] & 0x7F).any():
        bad.append("an all-zero row without scale = 2^-126 and q = +-0")
    if (np.abs(s - amax / 448)[~zero] > ((2 * ulp(amax, dt) + 2.0 ** -22 * amax) / 448)[~zero]).any():
        bad.append("scale outside its bound")
    v, d = y / s, torch.from_numpy(q[rows]).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    with np.errstate(divide="ignore"):
        spacing = np.exp2(np.maximum(np.floor(np.log2(np.maximum(np.abs(v), np.abs(d)))), -6) - 3)
    ratio = float((np.abs(d - v) / (0.5 * spacing + 2 * ulp(y, dt) / s + 2.0 ** -20 * np.abs(v))).max())
    return bad + ([] if ratio <= 1 else ["q is %.3f of its bound from the fp64 reference" % ratio]), ratio


def steps_5_to_7(torch, y_bits, dt):
    """The definition's new steps in numpy fp32 on y's patterns: (q bytes, scale)."""
    y = M.decode(y_bits, dt)
    with np.errstate(invalid="ignore"):  # (a NaN row: left out by the caller)
        scale = np.maximum(np.abs(y).max(axis=1) / np.float32(448), TINY).astype(np.float32)
        p = np.clip(y * (np.float32(1) / scale)[:, None], np.float32(-448), np.float32(448)).astype(np.float32)
    return torch.from_numpy(p).to(torch.float8_e4m3fn).view(torch.uint8).numpy(), scale


def run(n, dt, xs, res, gamma, mode, skip=(), chain=False, **shape):
    """One judged call; chain: also bit-equal to steps 5-7 on all_reduce_rms_norm_pull's y.  -> rank 0's (q, scale)."""
    import torch

    ranks, (rows, cols) = ranks_of(n), xs[0].shape
    mk = lambda r, c, bits=None: [M.Guarded(torch, r, c, dt, bits and bits[k]) for k in range(n)]  # bits: per rank
    x, g = mk(rows, cols, xs), mk(1, cols, [gamma.reshape(1, cols)] * n)
    q, sc = mk(rows, cols // 2), mk(1, 2 * rows)  # rows x cols bytes; rows floats
    r_in = mk(rows, cols, [res] * n) if mode != "none" else None
    r_out = r_in if mode != "out_of_place" else mk(rows, cols)
    ts = lambda bs: bs and [b.t for b in bs]
    ranks.all_reduce_rms_norm_quant_pull(ts(x), [b.t.view(torch.uint8) for b in q], [b.t.view(torch.float32)[0] for b in sc],
                                         [b.t[0] for b in g], ts(r_in), ts(r_out), eps=float(M.EPS), **shape)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    ref, worst, got = M.model(xs, res, gamma, dt), 0.0, []
    for r in range(n):
        (qb, ok_q), (sb, ok_s), (rb, ok_r) = q[r].read(), sc[r].read(), r_out[r].read() if r_out else (None, True)
        assert ok_q and ok_s and ok_r, f"guard bytes of rank {r} overwritten"
        got.append((qb.view(np.uint8), sb.view(np.float32)[0]))
        bad, ratio = judge(torch, ref, dt, *got[r], rb, skip)
        worst = max(worst, ratio)
        assert not bad, (r, bad)
        assert np.array_equal(got[r][0], got[0][0]) and np.array_equal(got[r][1].view(np.uint32), got[0][1].view(np.uint32))
    print(f"n={n} {dt} {rows}x{cols} {mode} {shape}: worst q error {worst:.3f} of its bound")
    if chain:
        y = M.run_on(ranks, ranks.all_reduce_rms_norm_pull, xs, res, gamma, dt, mode, **shape)
        want_q, want_s = steps_5_to_7(torch, y, dt)
        keep = [r for r in range(rows) if r not in skip]
        assert np.array_equal(got[0][1][keep].view(np.uint32), want_s[keep].view(np.uint32)), "scale differs from steps 5-6"
        assert np.array_equal(got[0][0][keep], want_q[keep]), "q differs from step 7"
    return got[0]


@pytest.mark.parametrize("mode", ["none", "out_of_place", "in_place"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dt", M.DTYPES)
@pytest.mark.parametrize("n", [2, 3, 8])
def test_three_calls_match_the_references(built, n, dt, shape, mode):
    rows, cols, kw = shape_of(n, shape)
    for call in range(3):
        xs, res, gamma = M.inputs([n, M.DTYPES.index(dt), rows, cols, call], n, rows, cols, dt, mode != "none")
        run(n, dt, xs, res, gamma, mode, **kw)


@pytest.mark.parametrize("dt", M.DTYPES)
def test_the_grid_changes_no_bit(built, dt):
    xs, res, gamma = M.inputs(7, 8, 19, 64, dt, True)
    got = [run(8, dt, xs, res, gamma, "out_of_place", nblocks=nb) for nb in (0, 1, 2)]
    for q, s in got[1:]:
        assert np.array_equal(q, got[0][0]) and np.array_equal(s.view(np.uint32), got[0][1].view(np.uint32))


@pytest.mark.parametrize("shape", SHAPES[:7] + SHAPES[9:], ids=str)
@pytest.mark.parametrize("dt", M.DTYPES)
@pytest.mark.parametrize("n", [2, 8])
def test_bit_equal_to_the_definition_on_the_pull_kernels_y(built, n, dt, shape):
    rows, cols, kw = shape_of(n, shape)
    xs, res, gamma = M.inputs([n, rows, cols, 5], n, rows, cols, dt, True)
    run(n, dt, xs, res, gamma, "out_of_place", chain=True, **kw)


@pytest.mark.parametrize("kind", ["zero", "nan", "span"])
@pytest.mark.parametrize("dt", M.DTYPES)
def test_special_rows(built, dt, kind):
    """Row 2 of five: all zero; with a NaN term (unspecified there); of magnitudes down to 2^-20 of its largest."""
    n, rows, cols = 3, 5, 2064
    xs, res, gamma = M.inputs([9, M.DTYPES.index(dt)], n, rows, cols, dt, True)
    for t in xs + [res]:
        t[2] = 0
    if kind == "nan":
        xs[1][2, cols // 3] = M.QNAN[dt]
    elif kind == "span":
        rng = np.random.default_rng(10)
        xs[0][2] = M.encode(np.exp2(rng.uniform(-20, 0, cols)).astype(np.float32) * rng.choice(np.float32([-1, 1]), cols), dt)
    q, s = run(n, dt, xs, res, gamma, "out_of_place", skip=(2,) if kind == "nan" else (), chain=True)
    if kind == "span":
        assert ((q[2] & 0x78) == 0).sum() > 16 and ((q[2] & 0x7F) == 0).any() and (q[2] & 0x7F).max() == 0x7E
