"""References, inputs and case tables of the int64 / uint64 / int8 reduction tests (a helper, not
collected; modelled on pull_reduce_cases).

The arithmetic is the definition in include/mscclpp_amd/pull_reduce_device.hpp, restated in numpy:
SUM wraps at the element width; MIN / MAX compare signed (int64, int8) or unsigned (uint64) over the
whole element; AVG is the EXACT sum divided by n, truncating toward zero.  numpy has no 128-bit
integer, so the 64-bit AVG is computed per operand (q_k = x_k / n, r_k = x_k % n, truncating; Q = sum
of q_k, R = sum of r_k; Q += R / n, R %= n; a result whose Q and R disagree in sign moves one toward
zero) -- another route than the kernel's 96-bit sum, and test_int_reduce_cases checks it against
Python's integers.  Every operation is exact, so there is no tolerance anywhere.  Arrays hold element
BITS (uint64 / uint8), one per rank."""
import numpy as np

from pull_reduce_cases import mix64

I64, U64, I8 = 16, 17, 18  # MSCCLPP_AMD_I64 / _U64 / _I8
SUM, MIN, MAX, AVG = 0, 1, 2, 3
OPS = (SUM, MIN, MAX, AVG)
REDUCE, REDUCE_SCATTER, ALLREDUCE = 0, 1, 2
COLLS = (REDUCE, REDUCE_SCATTER, ALLREDUCE)
TYPES = (I64, U64, I8)
NAMES = {I64: "i64", U64: "u64", I8: "i8"}
OP_NAMES = {SUM: "sum", MIN: "min", MAX: "max", AVG: "avg"}
ITEMSIZE = {I64: 8, U64: 8, I8: 1}
BITS = {I64: np.uint64, U64: np.uint64, I8: np.uint8}
VALUE = {I64: np.int64, U64: np.uint64, I8: np.int8}  # how the bits compare
COUNT = 4097          # elements of the table cases: odd, an 8-byte (1-byte) tail, several workgroups
PLANTED = 16          # positions [0, PLANTED) of a case with at least MIN_PLANT elements carry specials
MIN_PLANT = 64
RANKS = (2, 3, 8)
SMALL_COUNTS = (1, 3)  # 3 x 8 bytes: one 16-byte unit and an 8-byte tail


def itemsize(code):
    return ITEMSIZE[code]


def bits_dtype(code):
    return BITS[code]


# ---- the reference ---------------------------------------------------------------------------
def ref_sum(code, xs):
    with np.errstate(over="ignore"):
        acc = np.array(xs[0], copy=True)
        for x in xs[1:]:
            acc = acc + x  # unsigned of the element width: wraps
    return acc


def ref_select(code, xs, larger, view=None):
    """MIN / MAX as a selection in rank order (`view`: compare as that type instead of the element's)."""
    view = view or VALUE[code]
    acc = np.array(xs[0], copy=True)
    for x in xs[1:]:
        take = x.view(view) > acc.view(view) if larger else x.view(view) < acc.view(view)
        acc = np.where(take, x, acc)
    return acc


def trunc_div(s, n):
    """s / n toward zero for a signed array: fmod's remainder has the dividend's sign, so s - r is no
    larger in magnitude than s (the smallest value included) and divides exactly."""
    n = s.dtype.type(n)
    return (s - np.fmod(s, n)) // n


def ref_avg(code, xs):
    n = len(xs)
    if code == I8:
        s = np.zeros(len(xs[0]), np.int32)
        for x in xs:
            s = s + x.view(np.int8).astype(np.int32)
        return trunc_div(s, n).astype(np.int8).view(np.uint8)
    with np.errstate(over="ignore"):
        if code == U64:
            big_q, big_r = np.zeros(len(xs[0]), np.uint64), np.zeros(len(xs[0]), np.uint64)
            for x in xs:
                big_q = big_q + x // np.uint64(n)
                big_r = big_r + x % np.uint64(n)
            return big_q + big_r // np.uint64(n)
        big_q, big_r = np.zeros(len(xs[0]), np.int64), np.zeros(len(xs[0]), np.int64)
        for x in xs:
            v = x.view(np.int64)
            big_q = big_q + trunc_div(v, n)
            big_r = big_r + np.fmod(v, np.int64(n))
        carry = trunc_div(big_r, n)
        big_q = big_q + carry
        big_r = big_r - carry * n
        big_q = big_q - ((big_q > 0) & (big_r < 0)).astype(np.int64) + ((big_q < 0) & (big_r > 0)).astype(np.int64)
        return big_q.view(np.uint64)


def wrapped_avg(code, xs):
    """What AVG is NOT: the wrapped sum divided by n."""
    n, s = len(xs), ref_sum(code, xs)
    if code == U64:
        return s // np.uint64(n)
    return trunc_div(s.view(VALUE[code]), n).view(BITS[code])


def reference(code, op, xs):
    if op == SUM:
        return ref_sum(code, xs)
    if op == AVG:
        return ref_avg(code, xs)
    return ref_select(code, xs, op == MAX)


def big_reference(code, op, vals):
    """One element in Python's integers: vals are the element bits of every rank; returns the bits."""
    width = 8 * ITEMSIZE[code]
    if code != U64:
        vals = [v - (1 << width) if v >> (width - 1) else v for v in vals]
    if op == SUM:
        r = sum(vals)
    elif op == AVG:
        s = sum(vals)
        r = abs(s) // len(vals) * (1 if s >= 0 else -1)
    else:
        r = max(vals) if op == MAX else min(vals)
    return r % (1 << width)


# ---- inputs ----------------------------------------------------------------------------------
def random_bits(code, n, count, seed):
    """Per rank `count` element bits.  64-bit: three elements of four are uniform over all 64 bits (sums
    wrap, and the high word decides every compare), one of four is shifted right by a random amount
    (arithmetically for int64): small magnitudes of both signs, equal high words."""
    xs = []
    for r in range(n):
        z = mix64(count, seed * 64 + r * 7919 + 1)
        if code == I8:
            xs.append((z >> np.uint64(17)).astype(np.uint8))
            continue
        sh = mix64(count, seed * 64 + r * 7919 + 2) % np.uint64(64)
        small = (z.view(np.int64) >> sh.astype(np.int64)).view(np.uint64) if code == I64 else z >> sh
        xs.append(np.where(np.arange(count) % 4 == 1, small, z).astype(np.uint64))
    return xs


HI = 7 << 32  # the high word of the planted pairs


def plant(code, op, xs):
    """Specials at positions [0, PLANTED) (only the first few are used; the rest stay random)."""
    n, dt = len(xs), BITS[code]
    mask = (1 << (8 * ITEMSIZE[code])) - 1

    def put(pos, vals):
        for r in range(n):
            xs[r][pos] = dt(vals[r] & mask)

    top, low = mask >> 1, (mask >> 1) + 1  # the largest and (as bits) the smallest signed value
    if op in (MIN, MAX):
        put(0, [-5, 3] + [1] * (n - 2))                               # -5 vs 3: signed and unsigned disagree
        put(1, [low, top] + [1] * (n - 2))
        if code != I8:
            put(2, [HI | 5, HI | 9] + [HI | 7] * (n - 2))             # pair A: equal high words; MAX is rank 1's
            put(3, [HI | 9, HI | 5] + [HI | 7] * (n - 2))             #         ... and MIN is rank 1's
            put(4, [1 << 32, 0xffffffff] + [0x80000000] * (n - 2))    # pair B: the low words order the other way
            put(5, [0xffffffff, 1 << 32] + [0x180000000] * (n - 2))
    elif op == SUM:
        if code == I8:
            for pos, b in enumerate((0x7f, 0xff, 0x7f, 0xff)):        # neighbouring bytes: a word-wide add carries across
                put(pos, [b, 1] + [0] * (n - 2))
        else:
            put(0, [0x00000000ffffffff, 1] + [0] * (n - 2))           # a carry out of the low word
            put(1, [mask, 1] + [0] * (n - 2))                         # a wrap at 2^64
            put(2, [top, 1] + [0] * (n - 2))
    else:
        put(0, [mask if code == U64 else top] * n)                    # n x the largest value: the sum needs 67 (11) bits
        put(1, [low] * n)                                             # n x INT64_MIN / -128 (uint64: n x 2^63)
        put(2, [-7] + [0] * (n - 1))                                  # -7 / n: trunc != floor (uint64: 2^64 - 7)
        put(3, [-7, -2] + [0] * (n - 2))                              # -9 / n
        put(4, [low, top] + [0] * (n - 2))
        put(5, [mask, 1] + [0] * (n - 2))                             # uint64: 2^64 / n exactly
    return xs


def inputs(code, op, n, count, seed):
    """n arrays of `count` element bits, the specials planted when the case is long enough to hold them."""
    xs = random_bits(code, n, count, seed)
    return plant(code, op, xs) if count >= MIN_PLANT else xs


def mismatches(got, want):
    """Indices where got differs from want, bit for bit."""
    return np.flatnonzero(np.asarray(got) != np.asarray(want))


# ---- case tables -----------------------------------------------------------------------------
# (dtype, op, n) at COUNT elements: the table the CPU test proves non-vacuous
TABLE = [(code, op, n) for code in TYPES for op in OPS for n in RANKS]


def table_seed(code, op, n):
    return 3000 + TABLE.index((code, op, n))
