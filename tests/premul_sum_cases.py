"""Reference, inputs, scalars and case tables of the PreMulSum tests (a helper, not collected).

The arithmetic is the definition in include/mscclpp_amd/pull_reduce_device.hpp, restated in numpy:
rank k's operand x_k and scalar s_k decode exactly to fp32; p_k = x_k * s_k is one np.float32 multiply;
acc = p_0, then acc = acc + p_k in rank order, one np.float32 add each; acc is rounded once to the
element type (pull_reduce_cases.round_to).  Arrays hold element BITS, one per rank; scalars are fp32
values the element type holds exactly (scalar_values rounds them first, as a caller must).

Every table case has two sets of scalars:
  * "special": distinct, finite, |s| <= 1, of both signs, one rank at exactly 1.0 and one at -0 (so
    at n = 2 the pair is {1.0, -0}: every product is then exact, the result is rank 0's or rank 1's
    operand, and what the case checks is WHOSE scalar multiplies whose operand and the signed zeros);
  * "generic": the same without 1.0 and 0, so that every product rounds (fp32) at every rank count.
Which scalar a rank gets rotates with the seed."""
import numpy as np

import oracle_lib as O
import pull_reduce_cases as P

PREMUL_SUM = 5
REDUCE, REDUCE_SCATTER, ALLREDUCE = P.COLLS
COLLS = P.COLLS
TYPES = (O.F16, O.BF16, O.F32)
NAMES = {O.F16: "f16", O.BF16: "bf16", O.F32: "f32"}
RANKS = (2, 3, 8)
COUNT = P.COUNT        # 4097
PLANTED = P.PLANTED    # positions [0, PLANTED) of a case with at least MIN_PLANT elements carry specials
MIN_PLANT = P.MIN_PLANT
SMALL_COUNTS = (1, 3)
NAN_CAP = 16
KINDS = ("special", "generic")

_OTHERS = (1.0 / 3.0, -0.7, 0.55, -0.123, 0.9, -0.0625, 0.271, -0.85)


def bits_dtype(code):
    return P.bits_dtype(code)


def scalar_bits(code, values):
    """The element-type bits of fp32 values, rounded to nearest even."""
    return P.round_to(code, np.asarray(values, np.float32))


def scalar_values(code, values):
    """fp32 values rounded to the element type (what a caller passes, decoded again)."""
    return P.decode(code, scalar_bits(code, values)).astype(np.float32)


def scalars(code, n, seed, kind="special"):
    """n per-rank scalars of the element type, as fp32 values."""
    base = ([1.0, -0.0] + list(_OTHERS[:n - 2])) if kind == "special" else list(_OTHERS[:n])
    k = seed % n
    s = scalar_values(code, base[k:] + base[:k])
    assert len(set(s.view(np.uint32).tolist())) == n and np.isfinite(s).all() and (np.abs(s) <= 1).all()
    assert np.signbit(s).any() and not np.signbit(s).all()
    return s


def fsdp_scalars(code, n):
    """Equal scalars 1 / (2 n): FSDP's gradient divide factor when it is not the group's size."""
    return scalar_values(code, [1.0 / (2 * n)] * n)


# ---- the reference ---------------------------------------------------------------------------
def product(code, x, s):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (P.decode(code, x).astype(np.float32) * np.float32(s)).astype(np.float32)


def fp32_sum(ps):
    with np.errstate(over="ignore", invalid="ignore"):
        acc = ps[0]
        for p in ps[1:]:
            acc = (acc + p).astype(np.float32)
    return acc


def reference(code, xs, ss):
    return P.round_to(code, fp32_sum([product(code, x, s) for x, s in zip(xs, ss)]))


# ---- what an implementation could compute instead (the CPU test proves the tables tell them apart)
def variant_same_scalar(code, xs, ss):
    """Every rank takes rank 0's scalar."""
    return reference(code, xs, [ss[0]] * len(xs))


def variant_fused(code, xs, ss):
    """The products are kept exact: acc = fma(x_k, s_k, acc).  (In float64 a product of two fp32
    values is exact; the sum is then rounded to fp32.)"""
    with np.errstate(over="ignore", invalid="ignore"):
        acc = product(code, xs[0], ss[0])
        for x, s in zip(xs[1:], ss[1:]):
            acc = (acc.astype(np.float64) + P.decode(code, x).astype(np.float64) * np.float64(s)).astype(np.float32)
    return P.round_to(code, acc)


def variant_scaled_afterwards(code, xs, ss):
    """The fp32 sum of the unscaled operands times rank 0's scalar."""
    with np.errstate(over="ignore", invalid="ignore"):
        return P.round_to(code, (P.float_sum(code, xs) * np.float32(ss[0])).astype(np.float32))


def variant_element_product(code, xs, ss):
    """The product is rounded to the element type (NCCL's half-precision multiply) before the fp32 sum."""
    ps = [P.decode(code, P.round_to(code, product(code, x, s))).astype(np.float32) for x, s in zip(xs, ss)]
    return P.round_to(code, fp32_sum(ps))


# ---- inputs ----------------------------------------------------------------------------------
def zero_rank(ss):
    """The rank whose scalar is +-0, or None."""
    z = np.flatnonzero(np.asarray(ss) == 0)
    return int(z[0]) if z.size else None


def plant(code, xs, ss):
    """Specials at positions [0, PLANTED): a NaN operand, inf x 0 (where a rank's scalar is 0; inf x s
    otherwise), and operands whose product with the rank's scalar is inexact in fp32 and lands on a
    rounding boundary of the sum, so that a fused multiply-add gives other bits (fp32 only: a product
    of two fp16 or two bf16 values of these magnitudes has at most 22 / 16 significant bits and is
    exact in fp32, so for those types no fused product can differ and none is planted)."""
    n, dt = len(xs), bits_dtype(code)
    one, sg, nan, inf = P.ONE[code], P.SIGN[code], P.NAN[code], P.INF[code]

    def put(pos, vals):
        for r in range(n):
            xs[r][pos] = dt(vals[r] & (2 ** (8 * xs[r].itemsize) - 1))

    put(0, [one, nan] + [one] * (n - 2))                      # a NaN operand
    z = zero_rank(ss)
    put(1, [inf if r == (0 if z is None else z) else one for r in range(n)])  # inf x 0 = NaN (generic: inf x s = +-inf)
    put(2, [sg] * n)                                          # -0 x s_k: the signs of the zero products
    put(3, [one] * n)                                         # the sum of the scalars themselves
    if code == O.F32:
        # 2^24 + 1 is not an fp32 value but x_k * s_k can carry such low bits: 0x3f800001 * s and its neighbours
        put(4, [0x3f800001 + 2 * r for r in range(n)])
        put(5, [0x4b000001 + r for r in range(n)])            # 2^23 + 1 + r: the products' low bits straddle ulps of the sum
        put(6, [0x3fffffff - r for r in range(n)])
    return xs


def inputs(code, n, count, seed, ss):
    """n arrays of `count` element bits: random finite patterns, with the specials planted when the
    case is long enough to hold them."""
    xs = P.random_bits(code, n, count, seed, finite=True)
    return plant(code, xs, ss) if count >= MIN_PLANT else xs


def mismatches(code, got, want):
    """Indices where got differs from want, bit for bit -- except that where the reference is NaN any
    NaN passes (the sign and payload of a generated NaN differ between x86 and the GPU)."""
    got, want = np.asarray(got), np.asarray(want)
    bad = got != want
    bad &= ~(P.is_nan_bits(code, want) & P.is_nan_bits(code, got))
    return np.flatnonzero(bad)


# ---- case tables -----------------------------------------------------------------------------
TABLE = [(code, n) for code in TYPES for n in RANKS]  # at COUNT elements, each with both kinds of scalars


def table_seed(code, n):
    return 7000 + TABLE.index((code, n))


def table_case(code, n, kind):
    """(xs, ss) of a table case."""
    seed = table_seed(code, n) + (500 if kind == "generic" else 0)
    ss = scalars(code, n, seed, kind)
    return inputs(code, n, COUNT, seed, ss), ss
