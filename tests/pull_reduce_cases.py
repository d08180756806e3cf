"""References, inputs and case tables of the ncclMax / ncclAvg tests (a helper, not collected).

The arithmetic is the definition in include/mscclpp_amd/pull_reduce_device.hpp, restated in numpy:
operands in rank order 0 .. n - 1; MAX selects raw element bits (`if isnan(acc) or x > acc: acc = x`);
float AVG is the fp32 sum in rank order times float32(1) / float32(n), rounded once to the element
type; integer AVG is the exact sum divided by n, truncating toward zero.  Arrays hold element BITS
(uint8 / uint16 / uint32), one per rank."""
import numpy as np

import oracle_lib as O

MAX, AVG = 2, 3
REDUCE, REDUCE_SCATTER, ALLREDUCE = 0, 1, 2
COLLS = (REDUCE, REDUCE_SCATTER, ALLREDUCE)
TYPES = (O.F16, O.BF16, O.F32, O.I32, O.U32, O.U8, O.E4M3, O.E5M2)
FLOAT_TYPES = (O.F16, O.BF16, O.F32, O.E4M3, O.E5M2)
NAMES = {O.F16: "f16", O.BF16: "bf16", O.F32: "f32", O.I32: "i32", O.U32: "u32", O.U8: "u8", O.E4M3: "e4m3",
         O.E5M2: "e5m2"}
BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32}
COUNT = 4097          # elements of the table cases: odd, no multiple of a 16-byte unit, several workgroups
PLANTED = 16          # positions [0, PLANTED) of a case with at least MIN_PLANT elements carry specials
MIN_PLANT = 64
UNITS = 2             # kPullReduceUnits (kernels/pull_reduce.hip)
SWEEP = 512 * UNITS * 16  # bytes one 512-lane workgroup covers per loop trip


def bits_dtype(code):
    return BITS[O.itemsize(code)]


# ---- decoding / encoding ---------------------------------------------------------------------
_FP8_TABLE = {}


def fp8_table(e5m2):
    """float32 value of every fp8 byte (the oracle's decode, the model of v_cvt_f32_fp8 / _bf8)."""
    if e5m2 not in _FP8_TABLE:
        _FP8_TABLE[e5m2] = np.array([O.fp8_decode(b, e5m2) for b in range(256)], np.float32)
    return _FP8_TABLE[e5m2]


def decode(code, bits):
    """Exact fp32 value of every element of a float type."""
    bits = np.asarray(bits)
    if code == O.F32:
        return bits.view(np.float32)
    if code == O.F16:
        return bits.view(np.float16).astype(np.float32)
    if code == O.BF16:
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return fp8_table(code == O.E5M2)[bits]


def bf16_round(r):
    """fp32 -> bf16 bits, round to nearest even; every NaN becomes 0x7fc0 with its sign."""
    u = np.asarray(r, np.float32).view(np.uint32)
    out = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(r)
    out[nan] = ((u[nan] >> 16) & 0x8000).astype(np.uint16) | 0x7fc0
    return out


def fp8_round(r, e5m2):
    """fp32 -> fp8 bits as fp8x4_encode: finite values saturate to +-448 / +-57344, then round to
    nearest even; NaN -> 0x7f with the sign; inf -> inf (e5m2) or NaN (e4m3, which has none)."""
    r = np.asarray(r, np.float32)
    top = 0x7b if e5m2 else 0x7e
    mags = fp8_table(e5m2)[: top + 1].astype(np.float64)  # ascending: codes 0 .. top
    a = np.minimum(np.abs(r.astype(np.float64)), mags[-1])
    hi = np.clip(np.searchsorted(mags, a, side="left"), 0, top)
    lo = np.maximum(hi - 1, 0)
    dlo, dhi = a - mags[lo], mags[hi] - a
    pick = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    out = pick.astype(np.uint8)
    out[np.isinf(r)] = 0x7c if e5m2 else 0x7f
    out[np.isnan(r)] = 0x7f
    return out | (np.signbit(r).astype(np.uint8) << 7)


def is_nan_bits(code, bits):
    return np.isnan(decode(code, bits))


# ---- the reference ---------------------------------------------------------------------------
def ref_max(code, xs):
    acc = np.array(xs[0], copy=True)
    if code in FLOAT_TYPES:
        fa = decode(code, acc).copy()
        for x in xs[1:]:
            fx = decode(code, x)
            with np.errstate(invalid="ignore"):
                take = np.isnan(fa) | (fx > fa)
            acc = np.where(take, x, acc)
            fa = np.where(take, fx, fa)
        return acc
    view = np.int32 if code == O.I32 else acc.dtype
    for x in xs[1:]:
        acc = np.where(np.asarray(x).view(view) > acc.view(view), x, acc)
    return acc


def float_sum(code, xs):
    """The fp32 sum in the order given, one fp32 add per operand."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = decode(code, xs[0]).astype(np.float32)
        for x in xs[1:]:
            s = (s + decode(code, x)).astype(np.float32)
    return s


def round_to(code, r):
    with np.errstate(over="ignore", invalid="ignore"):
        if code == O.F32:
            return np.asarray(r, np.float32).view(np.uint32).copy()
        if code == O.F16:
            return np.asarray(r, np.float32).astype(np.float16).view(np.uint16)
        if code == O.BF16:
            return bf16_round(r)
        return fp8_round(r, code == O.E5M2)


def ref_avg(code, xs):
    n = len(xs)
    if code in FLOAT_TYPES:
        inv_n = np.float32(1.0) / np.float32(n)
        with np.errstate(over="ignore", invalid="ignore"):
            r = (float_sum(code, xs) * inv_n).astype(np.float32)
        return round_to(code, r)
    wide = np.int64 if code == O.I32 else np.uint64
    view = np.int32 if code == O.I32 else xs[0].dtype
    s = np.zeros(len(xs[0]), wide)
    for x in xs:
        s = s + np.asarray(x).view(view).astype(wide)
    if code == O.I32:
        q = np.abs(s) // n * np.sign(s)  # toward zero
        return q.astype(np.int32).view(np.uint32)
    return (s // wide(n)).astype(xs[0].dtype)


def reference(code, op, xs):
    return ref_max(code, xs) if op == MAX else ref_avg(code, xs)


# ---- inputs ----------------------------------------------------------------------------------
def mix64(count, seed):
    """count 64-bit words of splitmix64 (own generator: the tables do not depend on numpy's)."""
    with np.errstate(over="ignore"):
        z = (np.arange(1, count + 1, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


EXP_MASK = {O.F16: (0x7c00, 0x0400), O.BF16: (0x7f80, 0x0080), O.F32: (0x7f800000, 0x00800000),
            O.E4M3: (0x78, 0x08), O.E5M2: (0x7c, 0x04)}
ONE = {O.F16: 0x3c00, O.BF16: 0x3f80, O.F32: 0x3f800000, O.E4M3: 0x38, O.E5M2: 0x3c}
SIGN = {O.F16: 0x8000, O.BF16: 0x8000, O.F32: 0x80000000, O.E4M3: 0x80, O.E5M2: 0x80}
INF = {O.F16: 0x7c00, O.BF16: 0x7f80, O.F32: 0x7f800000, O.E5M2: 0x7c}  # e4m3 has none
NAN = {O.F16: 0x7e01, O.BF16: 0x7fc1, O.F32: 0x7fc00001, O.E4M3: 0x7f, O.E5M2: 0x7e}
TOP = {O.F16: 0x7bff, O.BF16: 0x7f7f, O.F32: 0x7f7fffff, O.E4M3: 0x7e, O.E5M2: 0x7b}  # largest finite


def random_bits(code, n, count, seed, finite):
    dt = bits_dtype(code)
    xs = [(mix64(count, seed * 64 + r * 7919 + 1) >> np.uint64(17)).astype(dt) for r in range(n)]
    if finite and code in FLOAT_TYPES:
        mask, low = EXP_MASK[code]
        xs = [np.where((x & dt(mask)) == dt(mask), x & dt(~low & (2 ** (8 * x.itemsize) - 1)), x).astype(dt) for x in xs]
    return xs


def plant(code, op, xs):
    """Specials at positions [0, PLANTED) (only the first few are used; the rest stay random)."""
    n, dt = len(xs), bits_dtype(code)

    def put(pos, vals):
        for r in range(n):
            xs[r][pos] = dt(vals[r] & (2 ** (8 * xs[r].itemsize) - 1))

    if code in FLOAT_TYPES:
        one, sg, nan, top = ONE[code], SIGN[code], NAN[code], TOP[code]
        inf = INF.get(code, top)
        if op == MAX:
            put(0, [nan] + [one | sg] * (n - 1))                      # NaN on rank 0 only: the -1s win
            nans = {O.E4M3: [0x7f, 0xff] * 4, O.E5M2: [0x7d, 0x7e, 0x7f, 0xfd, 0xfe, 0xff, 0x7d, 0xfe]}
            put(1, nans[code][:n] if code in nans else [nan + r for r in range(n)])  # NaN everywhere, payloads differ
            put(2, [0, sg] + [one | sg] * (n - 2))                    # +0 before -0: +0
            put(3, [sg, 0] + [one | sg] * (n - 2))                    # -0 before +0: -0
            put(4, [one] * (n - 1) + [inf])                           # +inf (e4m3: 448) on the last rank
            put(5, [inf | sg] * (n - 1) + [top | sg])                 # -inf everywhere but the last
            put(6, [one, nan] + [0] * (n - 2))                        # NaN in the middle loses
        else:
            put(0, [one, nan] + [one] * (n - 2))                      # NaN
            put(1, [inf] + [one] * (n - 1))                           # inf (e4m3: a large finite sum)
            put(2, [inf, inf | sg] + [one] * (n - 2))                 # inf - inf = NaN (e4m3: 0)
            put(3, [sg] * n)                                          # -0
            put(4, [0x7bff if code == O.F16 else top] * n)            # |s| beyond the type's range
            put(5, [1] + [0] * (n - 1))                               # the smallest subnormal
            put(6, [1 | sg] + [1] * (n - 1))
            if code == O.BF16:
                # 131 * 2^-131 - 2^-133: rounded to bf16 first it is 131 * 2^-131, a tie once scaled into
                # the subnormals by a power of two (n = 2, 4, 8), where one rounding goes the other way
                put(7, [0x0183, 0x8001] + [0] * (n - 2))
    elif op == MAX:
        put(0, [0xfffffffb, 3] + [0] * (n - 2))                       # -5 vs 3: signed and unsigned disagree
        put(1, [0x80000000, 0x7fffffff] + [1] * (n - 2))
        put(2, [0] * (n - 1) + [0xffffffff])
    else:
        put(0, [0x7fffffff] * n)                                      # n x INT32_MAX (u8: n x 255)
        put(1, [0xfffffff9] + [0] * (n - 1))                          # -7 / n: trunc != floor
        put(2, [0xffffffff] * n)
        put(3, [0xfffffff9, 0xfffffffe] + [0] * (n - 2))              # -9 / n
    return xs


def inputs(code, op, n, count, seed):
    """n arrays of `count` element bits.  AVG: random finite patterns; MAX: unrestricted ones; both
    with the specials planted when the case is long enough to hold them."""
    xs = random_bits(code, n, count, seed, finite=(op == AVG))
    return plant(code, op, xs) if count >= MIN_PLANT else xs


def mismatches(code, op, got, want, planted, offset=0):
    """Indices where got differs from want, bit for bit -- except that where the AVG reference is
    NaN at a planted position any NaN will do (the sign and payload of a generated NaN differ
    between x86 and the GPU).  offset: the position of want[0] in the message the specials were
    planted in (a ReduceScatter block)."""
    got, want = np.asarray(got), np.asarray(want)
    bad = got != want
    k = max(0, min(PLANTED - offset, len(want)))
    if op == AVG and code in FLOAT_TYPES and planted and k:
        ok = is_nan_bits(code, want[:k]) & is_nan_bits(code, got[:k])
        bad[:k] &= ~ok
    return np.flatnonzero(bad)


# ---- case tables -----------------------------------------------------------------------------
RANKS = (2, 3, 8)
# (dtype, op, n) at COUNT elements, seed = index: the table the CPU test proves non-vacuous
TABLE = [(code, op, n) for code in TYPES for op in (MAX, AVG) for n in RANKS]


def table_seed(code, op, n):
    return 1000 + TABLE.index((code, op, n))


SIZE_TYPES = (O.F16, O.F32, O.U8)
# message bytes of the small-size cases (x collective x SIZE_TYPES x n in (3, 8)); one element is added per type
SMALL_BYTES = (12, 16, 20)
