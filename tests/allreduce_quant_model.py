"""The quantised-wire AllReduce in numpy over 16-bit patterns: Q, D, the three steps, the block
bound against the fp64 sum, and inputs whose blocks cycle through: 0 a probe (two ranks hold a large block whose
element 1 cancels to a small value, a third a tiny block whose element 1 is 0.75 ulp of it: added after both large
terms it survives the fp32 add and tips Q(s) off a rounding tie, added before either it is lost; the roles move one
rank on from probe to probe, n >= 3); 1 random values, block magnitudes over twelve binades; 2 clamps (2^k, the values
just under 2^k and 2^(k + 1): 128 -> 127, just under 8 -> 6); 3 zeros on every rank."""
import numpy as np

import allreduce_rmsnorm_model as R

FORMATS = ("mxint8", "mxfp4")
DTYPES = R.DTYPES
K = {"mxint8": 2.0 ** -6, "mxfp4": 0.5}
CODE_BYTES = {"mxint8": 32, "mxfp4": 16}  # per block
E2M1 = np.float64([0, 0.5, 1, 1.5, 2, 3, 4, 6])


def dq(v32, fmt):
    """D(Q(v)) of fp32 blocks [B, 32], as fp32 (every product is exact in fp64 and in fp32)."""
    amax = np.abs(v32).max(axis=1)
    e32 = (amax.view(np.uint32) >> 23).astype(np.int64)[:, None]
    v = v32.astype(np.float64)
    if fmt == "mxint8":
        code = np.clip(np.rint(np.ldexp(v, 133 - e32)), -127, 127) + 0.0  # (an int8 has no -0)
        return np.ldexp(code, e32 - 133).astype(np.float32)
    E = np.maximum(e32 - 2, 0)
    mag = np.abs(np.ldexp(v, 127 - E))
    hi = np.clip(np.searchsorted(E2M1, mag, side="left"), 0, 7)
    lo = np.maximum(hi - 1, 0)
    up, down = E2M1[hi] - mag, mag - E2M1[lo]
    code = np.where((up < down) | ((up == down) & (hi % 2 == 0)), hi, lo)  # RNE on the code; above 6: 6
    return np.ldexp(np.copysign(E2M1[code], v), E - 127).astype(np.float32)


def terms(xs, dt, fmt, order=None, own_exact=False):
    """(x, c, s) as fp32 blocks.  order: the ranks in the order they are added (the definition: 0 .. n - 1);
    own_exact: the owner of a slice adds its own x unquantised (NOT the definition)."""
    n = len(xs)
    x32 = [R.decode(x, dt).reshape(-1, 32) for x in xs]
    c = [dq(x, fmt) for x in x32]
    S = -(-x32[0].shape[0] // n)
    for q in range(n if own_exact else 0):
        c[q][q * S:(q + 1) * S] = x32[q][q * S:(q + 1) * S]
    order = list(order or range(n))
    s = c[order[0]].copy()
    for r in order[1:]:
        s = s + c[r]  # fp32, RNE
    return x32, c, s


def model(xs, dt, fmt, **variant):  # out's patterns [count]
    return R.encode(dq(terms(xs, dt, fmt, **variant)[2], fmt).reshape(-1), dt)


def error_and_bound(xs, out, dt, fmt):
    """(|out - sum_r x_r| in fp64, the bound) per element: sum_r k amax_r + k amax_s per block, the n - 1 fp32
    roundings (2^-24 of at most sum_r |c_r| each) and one rounding to the element type."""
    n = len(xs)
    x32, c, s = terms(xs, dt, fmt)
    blockmax = lambda a: np.abs(a).astype(np.float64).max(axis=1, keepdims=True)
    got = R.decode(out, dt).astype(np.float64).reshape(-1, 32)
    bound = K[fmt] * (sum(blockmax(x) for x in x32) + blockmax(s)) + np.zeros_like(got)
    bound += (n - 1) * 2.0 ** -24 * sum(np.abs(a).astype(np.float64) for a in c)
    bound += np.maximum(np.abs(got) * 2.0 ** -(R.MANT[dt] + 1), 2.0 ** -25 if dt == "fp16" else 0.0)
    err = np.abs(got - sum(x.astype(np.float64) for x in x32))
    return err.reshape(-1), bound.reshape(-1)


def inputs(seed, n, count, dt, fmt):
    """The ranks' patterns [count], count % 32 == 0: the four kinds of block in turn, the probe first."""
    rng = np.random.default_rng([seed, n, count])
    B = count // 32
    x = np.zeros((n, B, 32), np.float32)
    kind = np.arange(B) % 4
    # 1: magnitudes 2^[-6, 6] per (rank, block), elements uniform inside
    x[:, kind == 1] = (np.exp2(rng.uniform(-6, 6, (n, B, 1))) * rng.uniform(-1, 1, (n, B, 32)))[:, kind == 1]
    # 2: small values and the three clamp values, k per (rank, block) in [-2, 2]
    pred = 1 - 2.0 ** -(R.MANT[dt] + 1)
    clamp = np.exp2(rng.integers(-2, 3, (n, B, 1))) * np.concatenate(
        [np.float64([1, pred, 2 * pred]), rng.uniform(-0.2, 0.2, 29)])[None, None, :]
    x[:, kind == 2] = clamp[:, kind == 2]
    # 0: the probe (module docstring); unit 4, so that the tiny term is an fp16 pattern
    big, e1, tiny = {"mxint8": (400, (-252, 256), 1.5 * 2.0 ** -22), "mxfp4": (24, (-6, 8), 1.5 * 2.0 ** -23)}[fmt]
    for j, k in enumerate(np.flatnonzero(kind == 0)):  # the j-th probe: the three roles on ranks j, j + 1, j + 2
        for i in range(2):
            x[(j + i) % n, k, 0], x[(j + i) % n, k, 1] = big, e1[i]
        if n > 2:
            x[(j + 2) % n, k, 1] = tiny
    return [R.encode(x[r].reshape(-1), dt) for r in range(n)]


def wrong_orders(n):
    """Orders an implementation might take instead: reversed, and the ring order of every rank but 0."""
    return [list(range(n))[::-1]] + [[(r + k) % n for k in range(n)] for r in range(1, n)]


def scratch_bytes(n, fmt, nblocks, W):
    """The bulk scratch that holds passes of W blocks per workgroup and no more: regions A and B of n images."""
    P = W * nblocks
    img = P * CODE_BYTES[fmt] + (P + 15) // 16 * 16
    return 2 * ((n * img + 255) // 256 * 256)
