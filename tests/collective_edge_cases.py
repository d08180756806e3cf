"""Case tables, inputs and CPU expectations of tests/test_collective_edges_gpu.py (no GPU, no torch here):
ReduceScatter (the bulk kernel's MODE 1), AllGather (MODE 2) and Broadcast along the axes the earlier
tests hold fixed.  tests/test_collective_edge_cases.py proves on the CPU that the tables are not
vacuous, so a bad row fails there and not on the GPU box.

Groups: A launch shapes, B multi-pass, C every reduce type and op in MODE 1, D guards, views and the
in-place forms, E Broadcast shapes, F refusals, and the list the NCCL ABI workers run.

Inputs.  Every buffer of every call comes from numpy.random.default_rng((case id, call, rank)), so no
two buffers of a case share content and a wrong slice, a wrong peer or a stale read of the previous
call shows in (nearly) every lane.  Two families:
  bits    uniform random bit patterns of the element width (NaN, infinities, subnormals, negative and
          >= 2^31 integers), compared bit for bit with the oracle;
  finite  (F16, BF16, F32) random sign, magnitude m * 2^e with m uniform in [1, 2) and e uniform in
          [-6, 6], rounded to the type: no zeros, and 8 * 128 = 1024 overflows no type.  These are
          compared with a plain fp64 reference as well, no lane left out.

Judges of a reducing case: the oracle (O.allreduce_sliced, slice r in rank r's order), bit for bit;
and a reference that shares no code with it: numpy integers for I32 / U32, numpy's minimum for a
finite float MIN, and for a finite float SUM the fp64 sum with the recursive-summation bound
|got - ref| <= gamma * sum|x_i| + the smallest subnormal, gamma = (n-1)u / (1 - (n-1)u)."""
import zlib

import numpy as np

import kernel_edge_cases as K
import oracle_lib as O

RS, AG, BC = 1, 2, 3                      # ReduceScatter, AllGather (mscclppAmdCollectiveLaunch's codes), Broadcast
COLL_NAMES = {RS: "rs", AG: "ag", BC: "bc"}
ALGOS = ("fullmesh", "rsag")
ORDER = {"fullmesh": 0, "rsag": 1}        # sum order of the oracle: own then ascending / ring from own
FLOATS = (O.F16, O.BF16, O.F32)
PLAIN_TYPES = FLOATS + (O.I32, O.U32)     # the types with a plain reference besides the oracle
UNIT_ROUNDOFF = {O.F32: 2.0 ** -24, O.F16: 2.0 ** -11, O.BF16: 2.0 ** -8}
SMALLEST_SUBNORMAL = {O.F32: 2.0 ** -149, O.F16: 2.0 ** -24, O.BF16: 2.0 ** -133}
FINITE_EXP = (-6, 6)
GUARD = K.GUARD


def case_id(*row):
    """A stable integer per table row: the first element of every buffer's seed."""
    return zlib.crc32(repr(row).encode())


# ---- inputs ------------------------------------------------------------------------------------------
def uint_of(code):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32}[O.itemsize(code)]


def bits(code, count, cid, call, rank):
    rng = np.random.default_rng((cid, call, rank))
    return rng.integers(0, 2 ** (8 * O.itemsize(code)), count, dtype=np.uint64).astype(uint_of(code))


def encode(code, x):
    """fp64 -> the bit patterns of F16 / BF16 / F32, round to nearest even."""
    if code == O.F16:
        return x.astype(np.float16).view(np.uint16)
    w = x.astype(np.float32).view(np.uint32)
    if code == O.F32:
        return w
    return ((w + 0x7FFF + ((w >> 16) & 1)) >> 16).astype(np.uint16)


def decode(code, a):
    """Bit patterns of F16 / BF16 / F32 -> fp64 (exact)."""
    if code == O.F16:
        return a.view(np.float16).astype(np.float64)
    if code == O.BF16:
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return a.view(np.float32).astype(np.float64)


def finite(code, count, cid, call, rank):
    rng = np.random.default_rng((cid, call, rank))
    sign = rng.integers(0, 2, count) * 2.0 - 1.0
    m = 1.0 + rng.random(count)
    e = rng.integers(FINITE_EXP[0], FINITE_EXP[1] + 1, count)
    return encode(code, sign * np.ldexp(m, e))


def plant_edges(code, ins, call):
    """Float MIN: the pairings of K.inputs(edges=True) (NaN against numbers, +0 against -0, subnormals
    against each other, +-inf against numbers, +inf everywhere, NaN against -inf) planted on `ins`."""
    n, count = len(ins), ins[0].size
    src = K.inputs(code, n, count, seq=call, special=False, edges=True)
    for b in K.edge_bases(count):
        for r in range(n):
            ins[r][b:b + K.EDGE_LANES] = src[r][b:b + K.EDGE_LANES]
    return ins


def reduce_inputs(code, op, n, count, cid, call, family):
    """The n input buffers of one reducing call.  family "bits" or "finite"; a float MIN over bits
    gets the planted groups as well."""
    make = finite if family == "finite" else bits
    ins = [make(code, count, cid, call, r) for r in range(n)]
    if family == "bits" and op == O.MIN and code in FLOATS:
        plant_edges(code, ins, call)
    return ins


def families(code):
    """Input family of calls 0, 1, 2: the float types get one finite call for the plain reference."""
    return ("bits", "finite", "bits") if code in FLOATS else ("bits", "bits", "bits")


# ---- expectations --------------------------------------------------------------------------------------
def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def rs_expected(code, op, ins, block_bytes, order):
    """The oracle's reduced buffer (bytes): slice r, bytes [r * block, (r + 1) * block), is what rank r
    receives, summed in rank r's order."""
    nwords = as_bytes(ins[0]).size // 4
    return O.allreduce_sliced(code, op, ins, nwords, block_bytes // 4, order)[0].view(np.uint8)


def plain_int(code, op, ins):
    """I32 / U32 by numpy alone: SUM in int64 wrapped modulo 2^32, MIN by np.minimum.reduce."""
    st = np.stack([as_bytes(a).view(np.int32 if code == O.I32 else np.uint32) for a in ins])
    if op == O.SUM:
        return as_bytes((st.astype(np.int64).sum(axis=0) % (1 << 32)).astype(np.uint32))
    return as_bytes(np.minimum.reduce(st))


def plain_float_min(code, ins):
    """numpy's minimum of finite inputs (no NaN, no zero: equal values have equal bits)."""
    return as_bytes(encode(code, np.minimum.reduce(np.stack([decode(code, a) for a in ins]))))


def sum_reference(code, ins):
    """(fp64 sum, bound) per lane of a finite float SUM: gamma_{n-1} * sum|x_i| + the smallest
    subnormal, the recursive-summation bound, which holds for rounding per step and for a wider
    accumulator rounded once.  (The fp64 sum itself is exact: 8 terms of 24 bits within 2^-6 .. 2^7.)"""
    v = np.stack([decode(code, a) for a in ins])
    n, u = len(ins), UNIT_ROUNDOFF[code]
    gamma = (n - 1) * u / (1 - (n - 1) * u)
    return v.sum(axis=0), gamma * np.abs(v).sum(axis=0) + SMALLEST_SUBNORMAL[code]


def mismatches(code, got, exp):
    """Indices where the bytes `got` differ from `exp`; for F32, by words, and a lane whose expected
    value is a NaN must hold a NaN (as the AllReduce edge tests compare)."""
    if code == O.F32 and got.size % 4 == 0:
        g, e = got.view(np.uint32), exp.view(np.uint32)
        nan = (e & 0x7FFFFFFF) > 0x7F800000
        return np.nonzero(np.where(nan, (g & 0x7FFFFFFF) <= 0x7F800000, g != e))[0]
    return np.nonzero(got != exp)[0]


def plain_failures(code, op, ins, got):
    """Lanes of the bytes `got` that the plain reference rejects (none excluded); ins: the inputs of
    the lanes `got` covers.  Only for PLAIN_TYPES, and for floats only over finite inputs."""
    if code in (O.I32, O.U32):
        return np.nonzero(plain_int(code, op, ins).view(np.uint32) != got.view(np.uint32))[0]
    if op == O.MIN:
        return np.nonzero(plain_float_min(code, ins).view(uint_of(code)) != got.view(uint_of(code)))[0]
    ref, bound = sum_reference(code, ins)
    with np.errstate(invalid="ignore"):
        ok = np.abs(decode(code, got.view(uint_of(code))) - ref) <= bound
    return np.nonzero(~ok)[0]


def handshakes(coll, passes=1):
    """block_handshake calls per workgroup of one launch: ReduceScatter two per pass, AllGather one at
    entry and one per pass, Broadcast entry and exit."""
    return {RS: 2 * passes, AG: 1 + passes, BC: 2}[coll]


def bulk_grid(nblocks, nthreads):
    """The grid launchCollectiveBulk runs: 0 is its default, 64 workgroups of 512 lanes."""
    return nblocks or 64, nthreads or 512


def bcast_grid(nbytes, nblocks, nthreads):
    """launchBroadcast's: by default one workgroup per 256 KiB, 8 to 128 of them, 512 lanes."""
    want = (nbytes + (256 << 10) - 1) // (256 << 10)
    return nblocks or min(max(want, 8), 128), nthreads or 512


# ---- A: launch shapes ------------------------------------------------------------------------------
# 16 B: one workgroup has the only unit, the others only handshake (63 of the default 64); 64 KiB + 16 B:
# several T-strides per lane at 64 lanes on one workgroup, and a lone trailing unit.
A_BLOCKS = (16, 48, 4096 + 16, 65536 + 16)
A_TYPES = ((O.F16, O.SUM), (O.F32, O.SUM), (O.I32, O.MIN))
A_GRIDS = [(nb, nt) for nb in (1, 3, 0, K.MAX_CHANNELS) for nt in (64, 512)]
# In-process ranks share one device and every workgroup spins on its peers, so the launcher refuses a
# grid that cannot be resident at once: 256 x 512 lanes runs at 2 ranks only -- 512 workgroups, what
# the default 64 x 512 grid takes at 8 ranks, and what an MI355X holds (two per compute unit).  256 x 64
# lanes runs at every rank count.  Group F has 256 x 512 at 3 ranks as a refusal (ncclInvalidUsage).
A_MAX_WIDE_WORKGROUPS = 512


def _a_cases():
    cases = []
    for coll in (RS, AG):
        for algo in ALGOS:
            for n in (2, 3, 8):
                for gi, (nb, nt) in enumerate(A_GRIDS):
                    if bulk_grid(nb, nt)[1] == 512 and bulk_grid(nb, nt)[0] * n > A_MAX_WIDE_WORKGROUPS:
                        continue
                    # every block size on every grid; the three types rotate over (grid, block)
                    picks = tuple((blk,) + A_TYPES[(gi + bi + n) % 3] for bi, blk in enumerate(A_BLOCKS))
                    cases.append((coll, algo, n, nb, nt, picks))
    return cases


# (coll, algo, n, nblocks, nthreads, ((block bytes, dtype, op), ...)); three calls per block on one group
A_CASES = _a_cases()
A_SCRATCH = 1 << 20   # one pass at every row

# ---- B: multi-pass -----------------------------------------------------------------------------------
# (n, dtype, op, block bytes, scratch bytes, nblocks, nthreads)
B_CASES = [
    (8, O.F16, O.SUM, 2 * 8192 + 4096 + 16, 64 * K.KIB, 8, 256),  # 3 passes; the last: 4 full workgroups, one unit, 3 idle
    (7, O.F32, O.SUM, 2 * 9984 + 4992, 7 * 10000, 6, 256),        # the pass rounds to 9984 and does not divide the block
    (3, O.BF16, O.SUM, 3 * 960 + 112, 3000, 3, 64),               # 4 passes of 20 units per workgroup: below one wave
    (2, O.I32, O.MIN, 4 * 4096 + 48, 2 * 4096, 1, 512),           # 5 passes on one workgroup
]
B_REFUSED = (8, O.F16, 1024, 8 * 127, 8, 256)  # 127 bytes per rank region < one pass of 16 * 8 bytes

# ---- C: every reduce type and op in MODE 1 ---------------------------------------------------------------
C_TYPES = (O.F16, O.BF16, O.F32, O.I32, O.U32) + O.FP8_TYPES + (O.U8,) + O.B15_TYPES
C_BLOCK = 2064            # 129 units of 16 bytes per slice: 43 per workgroup on the grid below
C_GRID = (3, 256)
# (reduce code, op, algo, n)
C_CASES = [(code, op, algo, n) for code in C_TYPES for op in (O.SUM, O.MIN) for algo in ALGOS for n in (3, 8)]

# ---- D: guards, views and in-place ------------------------------------------------------------------------
D_BLOCK = 1040            # 65 units per rank block
D_BCAST = 4099            # bytes (of uint8; the F16 row takes one byte less): a 3-byte tail


def _d_cases():
    cases = []
    for algo in ALGOS:
        for n in (3, 8):
            cases += [(RS, algo, n, code, D_BLOCK, s, s) for code, s in ((O.F16, 0), (O.BF16, 2), (O.F32, 4))]
            cases += [(AG, algo, n, code, D_BLOCK, s, s) for code, s in ((O.F16, 0), (O.F16, 2), (O.F32, 4))]
            cases += [(AG, algo, n, O.U8, D_BLOCK, si, so) for si, so in ((1, 0), (0, 1), (1, 1))]
    for n in (3, 8):
        cases += [(BC, None, n, O.U8, D_BCAST, si, so) for si, so in ((0, 0), (1, 0), (0, 1), (1, 1))]
        cases.append((BC, None, n, O.F16, D_BCAST - 1, 2, 2))
    return cases


# (coll, algo, n, dtype, bytes (per-rank block; Broadcast: the buffer), shift of the input, of the output):
# both buffers start that many bytes past a 256-byte boundary inside one 0xA5 arena per rank
D_CASES = _d_cases()


def d_layout(in_bytes, out_bytes, in_shift, out_shift):
    """(input offset, output offset, arena bytes) from K.arena_layout for the larger buffer, the two
    shifts added: 252 guard bytes or more stay around either buffer."""
    i, o, total = K.arena_layout(max(in_bytes, out_bytes), 1, False)
    return i + in_shift, o + out_shift, total


# ---- E: Broadcast shapes -------------------------------------------------------------------------------------
E_SWEEP = 64 * 4 * 16     # one workgroup of 64 lanes: T * U units of 16 bytes per sweep (U = 4 in launchBroadcast)
# (n, bytes, nblocks, nthreads); every root 0..n-1 in turn on one group
E_CASES = [(n, nbytes, nb, nt) for n in (2, 3, 8) for nbytes in (1, 15, 16, 17, 4097) for nb in (1, 3, 0)
           for nt in (64, 512)] + \
          [(n, E_SWEEP * k + 16 + 3, 1, 64) for n in (2, 3, 8) for k in (1, 3)]  # whole sweeps, a partial one, a byte tail

# ---- F: refusals ----------------------------------------------------------------------------------------------
F_N = 3
F_BLOCK = 1024
# (what, arguments, code).  "coll": (coll, algo, block bytes, nblocks, nthreads); "bcast": (root, bytes)
F_CASES = [("coll", (coll, "fullmesh", F_BLOCK + 8, 0, 0), 5) for coll in (RS, AG)] + \
          [("coll", (coll, "rsag", 24, 3, 64), 5) for coll in (RS, AG)] + \
          [("coll", (coll, "rsag_zc", F_BLOCK, 0, 0), 4) for coll in (RS, AG)] + \
          [("coll", (coll, algo, F_BLOCK, K.MAX_CHANNELS + 1, 256), 4) for coll in (RS, AG) for algo in ALGOS] + \
          [("coll", (coll, "fullmesh", F_BLOCK, 4, nt), 4) for coll in (RS, AG) for nt in (32, 96, 576)] + \
          [("coll", (coll, "fullmesh", F_BLOCK, K.MAX_CHANNELS, 512), 5) for coll in (RS, AG)] + \
          [("bcast", (F_N, F_BLOCK), 4), ("bcast", (-1, F_BLOCK), 4), ("bcast", (0, 0), 4)]

# ---- through the NCCL ABI ---------------------------------------------------------------------------------------
ABI_RANKS = (2, 4)
ABI_BLOCK = 4096 + 48     # bytes per rank
ABI_OFFSET = 272          # bytes into the allocation of the out-of-place views (16-byte aligned, non-zero)
ABI_ODD = 259             # an odd byte offset for the uint8 views
ABI_SMALL = 8             # a per-rank block the bulk path refuses
ABI_REPLAYS = 3
# the keys every worker reports True for
ABI_CHECKS = ("ag_in_place", "rs_in_place_bf16_sum", "rs_in_place_f32_min", "ag_views", "rs_views", "bcast_odd",
              "ag_odd", "small_ag_refused", "small_rs_refused", "rs_after_refusal", "ag_after_refusal",
              "ar_after_refusal", "graph_ag_in_place")
