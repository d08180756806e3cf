"""Case tables of the small-message LL path of the pull-reduce operations (kernels/pull_reduce_ll.hip), a
numpy restatement of its geometry and of a region's packet image, and the lanes that tell rank order
from own-first order (a helper, not collected).

The expected bits are those of the three existing references -- pull_reduce_cases (MAX / AVG of the
eight types), int_reduce_cases (int64 / uint64 / int8) and premul_sum_cases (PreMulSum) -- reached
through one interface here: a ROW is (family, dtype code, op), a case is (xs, ss) with xs the element
bits per rank and ss the per-rank scalars (None outside PreMulSum)."""
import numpy as np

import int_reduce_cases as I
import oracle_lib as O
import premul_sum_cases as S
import pull_reduce_cases as P

REDUCE, REDUCE_SCATTER, ALLREDUCE = P.COLLS
LL_COLLS = (REDUCE_SCATTER, ALLREDUCE)
SUM, MIN, MAX, AVG, PREMUL_SUM = 0, 1, 2, 3, 5
RANKS = (2, 3, 8)

ROWS = ([("pull", code, op) for code in P.TYPES for op in (MAX, AVG)] +
        [("int", code, op) for code in I.TYPES for op in I.OPS] +
        [("premul", code, PREMUL_SUM) for code in S.TYPES])
OP_NAMES = {SUM: "sum", MIN: "min", MAX: "max", AVG: "avg", PREMUL_SUM: "premulsum"}


def row_name(row):
    fam, code, op = row
    return f"{(I.NAMES if fam == 'int' else P.NAMES)[code]}-{OP_NAMES[op]}"


def itemsize(row):
    return I.itemsize(row[1]) if row[0] == "int" else O.itemsize(row[1])


def bits_dtype(row):
    return I.bits_dtype(row[1]) if row[0] == "int" else P.bits_dtype(row[1])


def is_float_sum(row):
    """AVG of a float type, or PreMulSum: the rows whose result depends on the operand order."""
    return row[0] == "premul" or (row[0] == "pull" and row[2] == AVG and row[1] in P.FLOAT_TYPES)


# ---- sizes -------------------------------------------------------------------------------------
# Bytes of a message (AllReduce) or of a per-rank block (ReduceScatter), per element size.  One element;
# an odd word count W (the lone trailing 8-byte packet: 12 bytes, W = 3); 1 .. 9 bytes of the one-byte
# types; 1, 2 and 3 elements of the 64-bit types; 6-byte blocks (a ReduceScatter's block starts are then
# not word-aligned); 65 and 129 units (two and three passes of a 1 x 64 grid; the one-, two- and
# four-byte sizes of 65 units have an odd W, those of 129 units of the one- and two-byte types a tail).
SIZES = {1: (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 516, 1030),
         2: (2, 6, 12, 514, 1030),
         4: (4, 12, 516, 1028),
         8: (8, 16, 24, 520, 1032)}
SEVERAL_PASSES = {1: (516, 1030), 2: (514, 1030), 4: (516, 1028), 8: (520, 1032)}
ONE_BY_64 = dict(nblocks=1, nthreads=64)     # the grid that covers SEVERAL_PASSES in 2 and 3 passes
WIDE_GRID = dict(nblocks=5, nthreads=64)     # wider than the unit count of every size up to 24 bytes


# The built-in cutover (kernels/pull_reduce_ll.hip): the largest byte count -- the message
# of an AllReduce, the per-rank block of a ReduceScatter -- that ncclAllReduce / ncclReduceScatter send to
# the LL path, per collective and MEASURED rank count; a rank count between two measured ones takes
# the next measured one above it.
BUILTIN_MAX = {(REDUCE_SCATTER, 2): 512 << 10, (REDUCE_SCATTER, 4): 512 << 10, (REDUCE_SCATTER, 8): 128 << 10,
               (ALLREDUCE, 2): 1 << 20, (ALLREDUCE, 4): 512 << 10, (ALLREDUCE, 8): 256 << 10}


def measured_ranks(n):
    return 2 if n <= 2 else 4 if n <= 4 else 8


def ll_words(nbytes, es):
    """32-bit words a message covers: bytes / 4 for 4- and 8-byte elements, (bytes + es) / 4 for 1- and
    2-byte ones, rounded up where that stops short of the message (the llWords rule)."""
    if es in (4, 8):
        return nbytes // 4
    w = (nbytes + es) // 4
    return w if w * 4 >= nbytes else (nbytes + 3) // 4


def geometry(n, nbytes, es, premul=False):
    """The kernel's geometry of one call: words, 16-byte units, where the scalar unit sits in a region,
    the region stride, the half size and the scratch the call needs."""
    w = ll_words(nbytes, es)
    units = (w + 1) // 2
    region = units * 16 + (16 if premul else 0)
    half = (n * region + 255) // 256 * 256
    return dict(W=w, units=units, scalar_at=units * 16, region=region, half=half, scratch=2 * half)


def default_grid(units):
    """(nblocks, nthreads) of a launch with nblocks = nthreads = 0: a function of the unit count alone."""
    nthreads = 256
    return max(1, min(128, (units + nthreads - 1) // nthreads)), nthreads


def region_image(payload, es, flag, scalar=None):
    """The bytes one source rank leaves in its region of a peer's half: payload (uint8, one message or
    block) as units {w0, flag, w1, flag}; an odd word count ends in the 8-byte packet {w0, flag} and
    the 8 bytes behind it are not written (0 here); tail bytes are zero-filled.  scalar: the fp32 bits
    of the rank's PreMulSum scalar, in one more unit {bits, flag, 0, flag}."""
    payload = np.asarray(payload, np.uint8)
    g = geometry(2, len(payload), es, scalar is not None)
    words = np.zeros(2 * g["units"], np.uint32)
    padded = np.zeros(4 * len(words), np.uint8)
    padded[:len(payload)] = payload
    words[:] = padded.view(np.uint32)
    img = np.zeros(g["region"] // 4, np.uint32)
    k = 4 * g["units"]
    img[0:k:4], img[1:k:4], img[2:k:4], img[3:k:4] = words[0::2], flag, words[1::2], flag
    if g["W"] % 2:
        img[k - 2:k] = 0  # the lone trailing packet: its second half is never written
    if scalar is not None:
        img[k:k + 4] = (scalar, flag, 0, flag)
    return img.view(np.uint8)


# ---- one interface over the three references -----------------------------------------------------
def make_case(row, n, count, seed):
    """(xs, ss): element bits per rank (count elements each) and the per-rank scalars or None."""
    fam, code, op = row
    if fam == "pull":
        return P.inputs(code, op, n, count, seed), None
    if fam == "int":
        return I.inputs(code, op, n, count, seed), None
    ss = S.scalars(code, n, seed, S.KINDS[seed % 2])
    return S.inputs(code, n, count, seed, ss), ss


def reference(row, xs, ss=None):
    fam, code, op = row
    if fam == "pull":
        return P.reference(code, op, xs)
    if fam == "int":
        return I.reference(code, op, xs)
    return S.reference(code, xs, ss)


def mismatches(row, got, want):
    """Indices where got differs from want, bit for bit -- except that where a float sum's reference is
    NaN any NaN passes (the sign and payload of a generated NaN differ between x86 and the GPU)."""
    fam, code, op = row
    got, want = np.asarray(got), np.asarray(want)
    bad = got != want
    if is_float_sum(row):
        bad &= ~(P.is_nan_bits(code, want) & P.is_nan_bits(code, got))
    return np.flatnonzero(bad)


# ---- rank order against own-first order ----------------------------------------------------------
# The committed inputs of the three case modules tell the two orders apart for MAX of the float types
# and for the fp32 AVG at n = 8 only; for the float sums this module plants lanes of its own.  Lane
# r - 2 (for every rank r >= 2): x_0 = B, x_1 = -B, x_r = eps, zeros elsewhere, with B + eps == B in
# fp32 and eps / n a non-zero value of the element type.  Rank order gives (B - B) + eps = eps (AVG:
# eps / n); own-first on rank r gives (eps + B) - B = 0.  PreMulSum takes every scalar as 0.5, so that
# every product is exact and the same argument holds with B / 2 and eps / 2.
ORDER_COUNT = 8  # elements of an order case: lanes 0 .. n - 3 are planted, the rest are zero
ORDER_B_EPS = {O.F16: (2.0 ** 15, 2.0 ** -10), O.BF16: (2.0 ** 15, 2.0 ** -10), O.E5M2: (2.0 ** 15, 2.0 ** -10),
               O.F32: (2.0 ** 24, 0.5)}
ORDER_ROWS = [row for row in ROWS if is_float_sum(row) and row[1] in ORDER_B_EPS]
ORDER_RANKS = (3, 8)


def order_case(row, n):
    """(xs, ss) of the order case of a float-sum row at n >= 3."""
    fam, code, op = row
    big, eps = ORDER_B_EPS[code]
    vals = np.zeros((n, ORDER_COUNT), np.float32)
    for r in range(2, n):
        vals[0, r - 2], vals[1, r - 2], vals[r, r - 2] = big, -big, eps
    xs = [P.round_to(code, vals[r]).astype(bits_dtype(row)) for r in range(n)]
    for r in range(n):
        assert np.array_equal(P.decode(code, xs[r]), vals[r])  # every planted value is exact in the type
    return xs, (S.scalar_values(code, [0.5] * n) if fam == "premul" else None)


def own_first(row, xs, ss, r):
    """The result had rank r's operand been taken first (the SUM LL8 kernel's order)."""
    order = [r] + [k for k in range(len(xs)) if k != r]
    return reference(row, [xs[k] for k in order], None if ss is None else [ss[k] for k in order])
