"""The fused AllReduce + residual add + RMSNorm in numpy over 16-bit patterns: fp32 adds, fp64 y.

Besides the ordinary `inputs` (every fp32 add of which is exact, so they cannot tell one summation order from
another, and whose `ms` is of order n, so `eps` moves y by less than the rounding) there are three blocks that
make the definition's steps visible: `order_inputs` (adds that round), `eps_inputs` (`ms` far below `eps`) and
`special_inputs` (non-finite, subnormal, overflowing and signed-zero rows between ordinary ones)."""
import functools
import os

import numpy as np

DTYPES = ("fp16", "bf16")
MANT = {"fp16": 10, "bf16": 7}
EMIN = {"fp16": -14, "bf16": -126}
EPS = np.float32(1e-5)
EPS_VALUES = tuple(np.float32(e) for e in (1e-5, 1e-2, 1.0))
FLT_MAX = float(np.finfo(np.float32).max)
INF = {"fp16": 0x7C00, "bf16": 0x7F80}  # also the exponent mask
QNAN = {"fp16": 0x7E00, "bf16": 0x7FC0}
# order_inputs: log2 of the cancelling pair's magnitude and of every other term's
ORDER_RANGES = {"fp16": ((6, 13), (-14, -10)), "bf16": ((11, 18), (-12, -4))}
EPS_RANGES = {"fp16": (-14, -10), "bf16": (-20, -10)}  # eps_inputs: log2 of the terms' magnitudes, at most
SPECIALS = {"fp16": ("nan", "inf", "inf_minus_inf", "overflow", "subnormal", "neg_zero", "gamma"),
            "bf16": ("nan", "inf", "inf_minus_inf", "big", "subnormal", "neg_zero", "gamma")}


def decode(bits, dt):
    if dt == "fp16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def encode(a32, dt):
    """fp32 -> the element type, rounded to nearest even; overflow gives inf, a NaN stays one."""
    a32 = np.ascontiguousarray(a32, np.float32)
    if dt == "fp16":
        with np.errstate(over="ignore", invalid="ignore"):
            return a32.astype(np.float16).view(np.uint16)
    u = a32.view(np.uint32).astype(np.uint64)
    return np.where(np.isnan(a32), (u >> 16) | 0x40, (u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def is_nan(bits, dt):
    return (bits & 0x7FFF) > INF[dt]


def _values(rng, lo, hi, shape, dt):
    """Patterns of magnitude 2^[lo, hi] and random sign."""
    return encode(np.exp2(rng.uniform(lo, hi, shape)).astype(np.float32) * rng.choice(np.float32([-1, 1]), shape), dt)


def inputs(seed, n, rows, cols, dt, residual):
    """x of every rank and the residual: magnitudes in [2^-3, 2^2], random signs; gamma in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    val = lambda: encode(np.exp2(rng.uniform(-3, 2, (rows, cols))).astype(np.float32) *
                         rng.choice(np.float32([-1, 1]), (rows, cols)), dt)
    xs = [val() for _ in range(n)]
    res = val() if residual else None
    gamma = encode(rng.uniform(0.5, 2.0, cols).astype(np.float32), dt)
    return xs, res, gamma


def zq_under(xs, res, dt, order="rank"):
    """Steps 1 - 2 of the definition with the fp32 adds taken in `order`: "rank" (the definition), "reversed",
    ("first", r) (term r, then the others in rank order), "tree" (pairwise, n = 8), "residual_first" (the residual,
    then the terms in rank order) or "round_s" (rank order, s rounded to DT before the residual is added)."""
    d = [decode(x, dt) for x in xs]
    r = None if res is None else decode(res, dt)
    chain = lambda terms: functools.reduce(lambda a, b: a + b, terms)  # one fp32 add each
    with np.errstate(over="ignore", invalid="ignore"):
        if order == "residual_first":
            return encode(chain([r] + d), dt)
        if order == "tree":
            while len(d) > 1:
                d = [d[i] + d[i + 1] for i in range(0, len(d), 2)]
            s = d[0]
        elif order == "reversed":
            s = chain(d[::-1])
        elif isinstance(order, tuple):
            s = chain([d[order[1]]] + d[:order[1]] + d[order[1] + 1:])
        else:
            assert order in ("rank", "round_s"), order
            s = chain(d)
        if order == "round_s":
            s = decode(encode(s, dt), dt)
        return encode(s if r is None else s + r, dt)


def alternative_orders(n, residual):
    """The orders of zq_under that no commutation of a single add turns into rank order."""
    orders = (["reversed"] + [("first", r) for r in range(2, n)] if n >= 3 else []) + (["tree"] if n == 8 else [])
    return orders + (["residual_first", "round_s"] if residual else [])


def model(xs, res, gamma, dt, eps=EPS, order="rank", rstd=None):  # -> (res_out patterns, y in fp64)
    """ms follows fp32's range: a row whose sum of zq^2 exceeds FLT_MAX has ms = inf and rstd = 0, so its finite
    elements give y = 0 and its infinite ones NaN; a NaN in the row makes every y of it NaN.  rstd: another
    function of (ms, eps), for the mutants of the CPU test."""
    zq = zq_under(xs, res, dt, order)
    z = decode(zq, dt).astype(np.float64)
    with np.errstate(all="ignore"):
        ss = (z * z).sum(axis=1, keepdims=True)
        ms = np.where(ss > FLT_MAX, np.inf, ss) / z.shape[1]
        scale = 1.0 / np.sqrt(ms + np.float64(eps)) if rstd is None else rstd(ms, np.float64(eps))
        return zq, z * scale * decode(gamma, dt).astype(np.float64)


def in_band(xs, res, dt):
    """No finite row sum of zq^2 lies within a factor 2^4 of FLT_MAX, on either side: the fp64 sum and an fp32
    chain in any order then agree on whether the row overflows."""
    z = decode(zq_under(xs, res, dt), dt).astype(np.float64)
    with np.errstate(all="ignore"):
        ss = (z * z).sum(axis=1)
    ss = ss[np.isfinite(ss)]
    return bool(((ss < FLT_MAX / 16) | (ss > FLT_MAX * 16)).all())


def order_inputs(seed, n, rows, cols, dt, residual):
    """Terms whose fp32 adds round: per element two different positions among the n terms (and the residual)
    hold B and exactly -B, every other one a value many binades below B.  Whatever is added between the two is
    rounded at B's spacing, so res_out depends on the order of the adds.  Two thirds of the elements take a random
    pair of positions, one third ranks 0 and 1 (a random pair alone lets "term 2 first" of 8 change a sixth)."""
    rng = np.random.default_rng(seed)
    (blo, bhi), (slo, shi) = ORDER_RANGES[dt]
    m = n + (1 if residual else 0)
    terms = _values(rng, slo, shi, (m, rows, cols), dt)
    b = _values(rng, blo, bhi, (1, rows, cols), dt)
    pos = np.argsort(rng.random((m, rows, cols)), axis=0)[:2]  # a random pair of positions per element ...
    pos[:, rng.random((rows, cols)) < 1 / 3] = [[0], [1]]  # ... or ranks 0 and 1: any term moved ahead of them meets B
    np.put_along_axis(terms, pos[0:1], b, axis=0)
    np.put_along_axis(terms, pos[1:2], b ^ 0x8000, axis=0)
    xs, res = [terms[k].copy() for k in range(n)], terms[n].copy() if residual else None
    assert in_band(xs, res, dt)
    return xs, res, encode(rng.uniform(0.5, 2.0, cols).astype(np.float32), dt)


def eps_inputs(seed, n, rows, cols, dt, residual):
    """Rows whose ms is at most 1/16 of the smallest of EPS_VALUES, and one all-zero row (rows // 2).  The
    magnitudes start at the bottom of EPS_RANGES; the top is lowered by half a binade and by log2(terms) / 2, so
    that the sum of the terms keeps ms under that bound (asserted)."""
    rng = np.random.default_rng(seed)
    m = n + (1 if residual else 0)
    lo, hi = EPS_RANGES[dt]
    terms = _values(rng, lo, hi - 0.5 - 0.5 * np.log2(m), (m, rows, cols), dt)
    terms[:, rows // 2] = 0
    xs, res = [terms[k].copy() for k in range(n)], terms[n].copy() if residual else None
    z = decode(zq_under(xs, res, dt), dt).astype(np.float64)
    assert ((z * z).mean(axis=1) <= float(EPS_VALUES[0]) / 16).all() and in_band(xs, res, dt)
    return xs, res, encode(rng.uniform(0.5, 2.0, cols).astype(np.float32), dt)


def special_inputs(seed, n, rows, cols, dt, residual, kind, row):
    """Ordinary `inputs` with row `row` made special (one of SPECIALS[dt]); "gamma" changes gamma instead: every
    third entry zero (+0 and -0 in turn), every third negative.  The single special elements sit at column
    cols // 3, in the term of rank min(1, n - 1) unless said otherwise:
      nan            a NaN                          -> res_out NaN there, y NaN in the whole row
      inf            +inf                           -> res_out +inf there; ms = inf: y NaN there, 0 elsewhere
      inf_minus_inf  +inf in rank 0's term, -inf in the last rank's -> as nan
      overflow       (fp16) 60000 in the terms of ranks 0 and 1: finite terms whose sum rounds to inf -> as inf
      big            (bf16) 2^100: zq^2 exceeds FLT_MAX -> res_out finite, y = 0 in the whole row
      subnormal      every term and the residual below the smallest normal value, random signs
      neg_zero       every term and the residual -0     -> res_out -0, y zero"""
    rng = np.random.default_rng([seed, SPECIALS[dt].index(kind)])
    xs, res, gamma = inputs(seed, n, rows, cols, dt, residual)
    k, c = min(1, n - 1), cols // 3
    everywhere = xs + ([res] if residual else [])
    if kind == "nan":
        xs[k][row, c] = QNAN[dt]
    elif kind == "inf":
        xs[k][row, c] = INF[dt]
    elif kind == "inf_minus_inf":
        xs[0][row, c], xs[n - 1][row, c] = INF[dt], INF[dt] | 0x8000
    elif kind == "overflow":
        xs[0][row, c] = xs[1][row, c] = encode(np.float32([60000.0]), dt)[0]
    elif kind == "big":
        xs[k][row, c] = encode(np.float32([2.0 ** 100]), dt)[0]
    elif kind == "subnormal":
        for t in everywhere:
            t[row] = rng.integers(1, 1 << MANT[dt], cols, dtype=np.uint16) | (rng.integers(0, 2, cols, dtype=np.uint16) << 15)
    elif kind == "neg_zero":
        for t in everywhere:
            t[row] = 0x8000
    else:
        assert kind == "gamma", kind
        gamma[0::3] = 0
        gamma[3::6] = 0x8000
        gamma[1::3] |= 0x8000
    assert in_band(xs, res, dt)
    return xs, res, gamma


def ulps(got, want64, dt):  # |got - want| in units of the element type's spacing at `want`
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(want64), 2.0 ** EMIN[dt])))
        return np.abs(decode(got, dt).astype(np.float64) - want64) / np.exp2(e - MANT[dt])


class Guarded:
    """A [rows][cols] device tensor of the element type between two 64-byte runs of 0xA5."""
    PAD = 64

    def __init__(self, torch, rows, cols, dt, bits=None):
        nbytes = rows * cols * 2
        self.whole = torch.full((nbytes + 2 * self.PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        tdt = torch.float16 if dt == "fp16" else torch.bfloat16
        self.t = self.whole[self.PAD:self.PAD + nbytes].view(tdt).view(rows, cols)
        if bits is not None:
            self.t.view(torch.int16).copy_(torch.from_numpy(bits.view(np.int16)))

    def read(self):  # (patterns, guards intact)
        raw = self.whole.cpu().numpy()
        ok = bool((raw[:self.PAD] == 0xA5).all() and (raw[-self.PAD:] == 0xA5).all())
        return raw[self.PAD:-self.PAD].view(np.uint16).reshape(self.t.shape), ok


def check(ref, dt, got_y, got_res):
    """One rank's results against ref = model(...): (the failed checks, the worst y error in ulp over the
    elements whose reference is a number).  res_out: equal patterns, or NaN where the model has one (any NaN
    pattern); y: NaN exactly where the reference is NaN, elsewhere within 2 ulp of it, -0 counting as +0."""
    zq, y64 = ref
    bad = []
    if got_res is not None:
        wrong = int(((got_res != zq) & ~(is_nan(got_res, dt) & is_nan(zq, dt))).sum())
        bad += ["res_out differs from the model in %d elements" % wrong] if wrong else []
    due = np.isnan(y64)
    missing = int((due & ~is_nan(got_y, dt)).sum())
    bad += ["y is a number in %d elements whose reference is NaN" % missing] if missing else []
    err = np.where(due, 0.0, ulps(got_y, np.where(due, 0.0, y64), dt))
    worst = float(np.where(np.isfinite(err), err, np.inf).max())
    return bad + ([] if worst <= 2.0 else ["y is %.3f ulp from the fp64 reference" % worst]), worst


def judge(xs, res, gamma, dt, got_y, got_res, eps=EPS):
    """The failed checks of one rank's results (patterns; got_res None without a residual)."""
    return check(model(xs, res, gamma, dt, eps), dt, got_y, got_res)[0]


def run_on(ranks, fn, xs, res, gamma, dt, mode, eps=EPS, **shape):
    """One call of fn (all_reduce_rms_norm or all_reduce_rms_norm_pull of the InProcessRanks `ranks`) on the
    prepared patterns, mode "none" (res is None), "out_of_place" or "in_place": no device error, guards intact,
    every rank's results pass `check`, y equal on all ranks.  Prints the worst y error; returns rank 0's y."""
    import torch

    n, (rows, cols) = len(xs), xs[0].shape
    assert (res is None) == (mode == "none")
    g = Guarded(torch, 1, cols, dt, gamma.reshape(1, cols))
    x = [Guarded(torch, rows, cols, dt, xs[r]) for r in range(n)]
    y = x if mode == "in_place" else [Guarded(torch, rows, cols, dt) for _ in range(n)]
    r_in = r_out = None
    if mode != "none":
        r_in = [Guarded(torch, rows, cols, dt, res) for _ in range(n)]
        r_out = r_in if mode == "in_place" else [Guarded(torch, rows, cols, dt) for _ in range(n)]
    fn([b.t for b in x], [b.t for b in y], [g.t[0]] * n, r_in and [b.t for b in r_in], r_out and [b.t for b in r_out],
       eps=float(eps), **shape)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    ys, rs = [b.read() for b in y], [b.read() for b in r_out] if r_out else [(None, True)] * n
    ref, worst = model(xs, res, gamma, dt, eps), 0.0
    for r in range(n):
        assert ys[r][1] and rs[r][1], f"guard bytes of rank {r} overwritten"
        bad, w = check(ref, dt, ys[r][0], rs[r][0])
        worst = max(worst, w)
        assert not bad, (r, bad)
        assert np.array_equal(ys[r][0], ys[0][0]), f"y of rank {r} differs from rank 0's"
    print(f"{os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]}: {fn.__name__} n={n} {dt} {rows}x{cols} {mode} "
          f"eps={float(eps):g} {shape}: worst y error {worst:.3f} ulp")
    return ys[0][0]
