"""Case tables, inputs and CPU expectations of tests/test_kernel_edges_gpu.py (no GPU, no torch here).

The GPU file runs these tables; tests/test_kernel_edge_cases.py proves on the CPU, with the oracle and
the library's host-side queries, the conditions that keep them from being vacuous (a launch shape that
the launcher accepts, three passes or more, lanes that tell a wrong MIN apart, the self-reduce form a
caller's grid reaches), so a bad table entry fails there and not on the GPU box.

Groups: A launch shapes, B multi-pass bulk, C MIN and uint32, D guard bands and element-aligned
views, E the self-reduce on a caller's grid."""
import numpy as np

import oracle_lib as O

ITEM = {O.F16: 2, O.BF16: 2, O.F32: 4, O.I32: 4, O.U32: 4}
KIB = 1024
FLAG_SLOTS = 4096     # MSCCLPP_AMD_FLAG_SLOTS: the LL launchers' grid limit
MAX_CHANNELS = 256    # MSCCLPP_AMD_MAX_CHANNELS: the bulk launchers' grid limit
LL_ALGOS = ("packet", "allpair")
BULK_ALGOS = ("fullmesh", "rsag", "rsag_zc")
ALGOS = LL_ALGOS + BULK_ALGOS
GUARD = 0xA5


# ---- inputs and expectations ---------------------------------------------------------------------
def _edge_bits(dt):
    """(quiet NaN, +inf, -inf, -0, smallest subnormal, largest subnormal, sign bit) of a float type."""
    if dt == O.F16:
        return 0x7E00, 0x7C00, 0xFC00, 0x8000, 0x0001, 0x03FF, 0x8000
    if dt == O.BF16:
        return 0x7FC0, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x007F, 0x8000
    return 0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x007FFFFF, 0x80000000


EDGE_GROUPS, EDGE_LANES = 9, 8


def edge_bases(count):
    """First lanes of the planted groups: spread from lane 0 to the last lanes of the buffer, so they
    fall into several rank slices and into the ragged tail."""
    return [int(v) for v in np.linspace(0, count - EDGE_LANES, EDGE_GROUPS)]


def inputs(dt, n, count, seq=0, special=True, edges=False):
    """Per-rank inputs: O.lcg values; `special` overlays random bit patterns on a quarter of the lanes
    (NaN, inf, subnormals, negative and >= 2^31 integers); `edges` (float types) plants in nine groups of
    eight lanes the pairings a random overlay almost never makes: NaN against numbers, +0 against -0,
    subnormals against each other, +inf / -inf against numbers, +inf everywhere, NaN against -inf."""
    base = [O.lcg(dt, count, r, seq) for r in range(n)]
    ins = [a.copy() for a in base]
    if special:
        rng = np.random.default_rng(11 + seq)
        bits = 8 * ITEM[dt]
        for r in range(n):
            m = rng.random(count) < 0.25
            ins[r][m] = rng.integers(0, 2**bits, m.sum(), dtype=np.uint64).astype(ins[r].dtype)
    if edges:
        assert dt in (O.F16, O.BF16, O.F32) and count >= EDGE_GROUPS * EDGE_LANES
        nan, pinf, ninf, nzero, sub_lo, sub_hi, sign = _edge_bits(dt)
        for g, b in enumerate(edge_bases(count)):
            a, c = (g + seq) % n, (g + seq + 1) % n
            for r in range(n):
                ins[r][b:b + EDGE_LANES] = base[r][b:b + EDGE_LANES]  # plain numbers under the planted lanes
                ins[r][b + 1] = 0 if (r + g) % 2 == 0 else nzero
            ins[a][b + 0] = nan
            ins[a][b + 2], ins[c][b + 2] = sub_lo, sub_hi
            ins[a][b + 3] = pinf
            ins[a][b + 4] = ninf
            for r in range(n):
                ins[r][b + 5] = pinf
            ins[a][b + 6] = sub_hi | sign
            ins[a][b + 7], ins[c][b + 7] = nan, ninf
    return ins


def slice_bytes(n, nbytes):
    """Bytes of a rank's slice on the bulk paths (bulkScratchRequired: ceil(bytes / n) to 16 bytes)."""
    return ((nbytes + n - 1) // n + 15) // 16 * 16


def expected(algo, dt, op, ins, count, flag=1, half_bytes=1 << 20):
    """([rank] -> the result's nbytes bytes, [rank] -> scratch image in 32-bit words or None)."""
    n, nbytes = len(ins), count * ITEM[dt]
    if algo == "packet":
        outs, scr = O.allreduce_packet(dt, op, ins, count, flag, half_bytes)
    elif algo == "allpair":
        outs, scr = O.allreduce_allpairs(dt, op, ins, count, flag, half_bytes)
    else:
        nwords = (nbytes + 3) // 4
        padded = []
        for a in ins:
            w = np.zeros(nwords, np.uint32)
            w.view(np.uint8)[:nbytes] = a.view(np.uint8)
            padded.append(w)
        # sum orders of the reference: fullmesh own slice first then ascending, rsag / rsag_zc ring order
        outs = O.allreduce_sliced(dt, op, padded, nwords, slice_bytes(n, nbytes) // 4, 0 if algo == "fullmesh" else 1)
        scr = None
    return [o.view(np.uint8)[:nbytes] for o in outs], scr


def pipeline_expected(dt, op, ins, nbytes, n, R, T):
    """Oracle for allreduceRsAgPipeline (allreduce_rsag_pipeline.cu:85-222): 16-byte unit u is owned
    by slot (u mod n*C) div C (C = R*T*4 units) and summed in ring order from its owner (own,
    owner+1, ...; calVector(data, tmp) with tmp = own first)."""
    nw = (nbytes + 15) // 16 * 4
    padded = []
    for a in ins:
        w = np.zeros(nw, np.uint32)
        w.view(np.uint8)[:nbytes] = a.view(np.uint8)[:nbytes]
        padded.append(w)
    C = R * T * 4
    owner = ((np.arange(nw) // 4) % (n * C)) // C
    exp = np.zeros(nw, np.uint32)
    for o in range(n):
        order = [padded[(o + k) % n] for k in range(n)]
        seq = O.reduce_seq(dt, op, order)
        exp[owner == o] = seq[owner == o]
    return exp


# ---- A: launch shapes ----------------------------------------------------------------------------
def _ll16_shapes(n):
    p = n - 1
    grids = sorted({p, 3 * p, 2 * p + 1})  # 2p+1 is rounded down to 2p by the launcher (3 = 3p at 2 ranks)
    return [(nb, nt) for nt in (64, 192, 512) for nb in grids + [0]] + [(0, 0)]


def _ll16_cases():
    cases = []
    for n in (2, 3, 5, 8):
        for count in (37, 3000 * n + 3):          # below a wave; ragged, 12 passes at 64 lanes on n-1 workgroups
            cases += [(n, O.F16, count, nb, nt) for nb, nt in _ll16_shapes(n)]
    cases += [(5, O.BF16, 15003, nb, nt) for nb, nt in _ll16_shapes(5)]
    cases += [(8, O.F32, 12003, nb, nt) for nb, nt in _ll16_shapes(8)]
    return cases


# (n, dtype, count, nblocks, nthreads)
LL16_SHAPE_CASES = _ll16_cases()

# kBatchedPollUnits = kSentinelUnits = 8192 packet units per slice: step 3's sentinel starts at 8192,
# step 2 polls peer by peer from 8193.  (n, count, units per slice) -- the geometry rounds a slice to
# whole packets, so n*8192*4 - 4 still has 8192 units; n*8191*4 is the size below the sentinel.
LL16_THRESHOLD_CASES = [(n, count, units, 3 * (n - 1), nt)
                        for n in (2, 3)
                        for count, units in ((n * 8191 * 4, 8191), (n * 8192 * 4 - 4, 8192), (n * 8192 * 4, 8192),
                                             (n * 8192 * 4 + 4, 8193))
                        for nt in (64, 512)]

# ll16Defaults switches lanes (512 / 256 / 512) and blocks per peer at 32 KiB and 256 KiB: (n, nbytes)
LL16_DEFAULT_CASES = [(n, nbytes) for n in range(2, 9)
                      for nbytes in (KIB, 32 * KIB - 2, 32 * KIB, 256 * KIB - 2, 256 * KIB)]

# f16 counts: 1002 -> 501 words (odd: a lone trailing LL8 packet), 1003 -> 2 bytes in the last word,
# 8192 -> 16 KiB exactly.  (n, count, nblocks, nthreads)
LL8_COUNTS = (1002, 1003, 8192)
LL8_SHAPE_CASES = [(n, count, nb, nt) for n in (3, 8) for count in LL8_COUNTS for nb in (1, 3, 7, 0)
                   for nt in (64, 320, 512, 0)]

# (8 ranks x) 1001 f16: 16 of the default 64 workgroups have a unit, the others only handshake;
# 65536 + 11 bf16: ragged slices and a tail below one 16-byte unit.
# (n, dtype, count, nblocks, nthreads); nblocks 0 = the default 64
BULK_SHAPE_CASES = [(n, dt, count, nb, nt) for n in (3, 8) for dt, count in ((O.F16, 1001), (O.BF16, 65536 + 11))
                    for nb in (1, 3, 0) for nt in (64, 512)]

# (algo, nblocks, nthreads) the launchers refuse with ncclInvalidArgument (4) before any launch
REFUSED_SHAPES = [(a, 4, nt) for a in ALGOS for nt in (96, 32, 576, 1024)] + \
                 [(a, FLAG_SLOTS + 1, 256) for a in LL_ALGOS] + [(a, MAX_CHANNELS + 1, 256) for a in BULK_ALGOS]


def accepted_ll16_grid(n, nblocks):
    """Workgroups launchAllReduceLL runs for an explicit LL16 grid: rounded down to a multiple of n - 1."""
    return nblocks // (n - 1) * (n - 1)


# ---- B: multi-pass bulk ----------------------------------------------------------------------------
# (n, dtype, count, scratch bytes, nblocks, nthreads)
MULTIPASS_CASES = [
    (8, O.F16, (1 << 18) + 24, 64 * KIB, 8, 256),   # 9 passes of 8 KiB, the last of 16 bytes (one workgroup)
    (7, O.F32, 123457, 7 * 10000, 6, 256),          # the pass rounds to 9984, which does not divide the slice
    (3, O.BF16, 200001, 24 * KIB, 3, 64),
    (2, O.I32, 70001, 16 * KIB, 1, 512),
]
MULTIPASS_RS_AG_COUNT = 1 << 18  # the first row's ReduceScatter / AllGather: 512 KiB = 4096 * 16 * 8 bytes
MULTIPASS_REFUSED = (8, O.F16, 1 << 16, 8 * 127, 8, 256)  # 127 bytes per rank region < one 16 * 8-byte pass


def bulk_passes(n, nbytes, scratch, nblocks):
    """(pass bytes, passes) of bulkScratchRequired for a scratch of `scratch` bytes; pass 0: refused."""
    sl = slice_bytes(n, nbytes)
    cap = min(scratch // n, (0xFFFFFFFF - 64) // n)
    ps = sl if sl <= cap else cap // (16 * nblocks) * (16 * nblocks)
    return ps, (sl + ps - 1) // ps if ps else 0


# ---- C: MIN and uint32 -----------------------------------------------------------------------------
MIN_U32_TYPES = [(O.F16, O.MIN), (O.BF16, O.MIN), (O.F32, O.MIN), (O.I32, O.MIN), (O.U32, O.MIN), (O.U32, O.SUM)]
# shapes that are not the earlier tests' fixed ones (LL16 (n-1)*2 x 256, LL8 4 x 256, bulk 8 x 256)
MIN_U32_SHAPES = {"packet": lambda n: (2 * (n - 1) + 1, 192), "allpair": lambda n: (3, 320),
                  "fullmesh": lambda n: (3, 512), "rsag": lambda n: (3, 512), "rsag_zc": lambda n: (3, 512)}


def min_u32_count(algo, dt):
    """8192 + 3 elements per rank; the one-hop LL8 path stays below its 16 KiB."""
    return 8192 + 3 if algo != "allpair" else 16 * KIB // ITEM[dt] - 3


MIN_U32_CASES = [(algo, dt, op, n) for algo in ALGOS for dt, op in MIN_U32_TYPES for n in (3, 8)]


def is_float(dt):
    return dt in (O.F16, O.BF16, O.F32)


def float_classes(dt, a):
    """(nan, inf, zero, subnormal) lane masks of a float bit-pattern array."""
    a = a.astype(np.uint32)
    ebits, mbits = {O.F16: (0x7C00, 0x03FF), O.BF16: (0x7F80, 0x007F), O.F32: (0x7F800000, 0x007FFFFF)}[dt]
    e, m = a & ebits, a & mbits
    return (e == ebits) & (m != 0), (e == ebits) & (m == 0), (e == 0) & (m == 0), (e == 0) & (m != 0)


# ---- D: guard bands and element-aligned views -------------------------------------------------------
# one ragged size per type and one that is a multiple of 16 bytes: (dtype, count)
GUARD_SIZES = [(O.F16, 777), (O.BF16, 1001), (O.F32, 1001), (O.I32, 5), (O.F16, 2048)]
GUARD_CASES = [(algo, n, dt, count, view) for algo in ALGOS for n in (3, 8) for dt, count in GUARD_SIZES
               for view in (False, True)]


def arena_layout(nbytes, item, view):
    """(input offset, output offset, arena bytes): both buffers 256 bytes (+ one element for the view
    run: element-aligned, not 16-byte aligned) past a 256-byte boundary, 256 guard bytes or more around."""
    d = item if view else 0
    in_off = 256 + d
    out_off = (in_off + nbytes + 256 + 255) // 256 * 256 + 256 + d
    total = (out_off + nbytes + 256 + 255) // 256 * 256
    return in_off, out_off, total


# ---- E: the self-reduce on a caller's grid -------------------------------------------------------------
# (nbytes, nblocks, waves, grid, rounds, skew): the form selfReduceShape reaches
SELF_REDUCE_CASES = [
    (8 * KIB + 16, 2, 4, 2, 2, 1),        # 3 tiles: one workgroup idle in the last round
    (28 * KIB, 1, 4, 2, 4, 1),            # odd grid rounded to 2
    (64 * KIB + 1040, 2, 4, 2, 9, 2),     # ragged last tile, tiles consumed two rounds late
    (256 * KIB + 48, 6, 4, 6, 11, 2),
    # More workgroups than tiles: one round, which always takes the plain form (skew 0, default cache
    # policy), so the last `else` of launchSelfReduce (skew 0, nt) cannot be reached from any grid.
    (64 * KIB, 1024, 4, 1024, 1, 0),
    (2048 * KIB, 512, 4, 512, 1, 0),      # a caller's grid inside the band where the default takes 8 waves
    (4096 * KIB + 16, 1023, 4, 1024, 2, 1),
]
SELF_REDUCE_TYPES = [(O.F16, O.SUM), (O.BF16, O.MIN), (O.F32, O.SUM), (O.U32, O.MIN)]


def self_reduce_shape_rule(nbytes, nblocks):
    """(waves, grid, rounds, skew) as DESIGN.md and self_reduce.hip state the rule: 4 waves x 1 KiB per
    workgroup and round on the caller's grid (made even), skew 1 from two rounds, 2 from eight; the
    default grid takes 8-wave workgroups in one round above 1 MiB up to 4 MiB."""
    if nblocks <= 0 and (1 << 20) < nbytes <= (4 << 20):
        t8 = (nbytes + 8191) // 8192
        return 8, t8 + t8 % 2, 1, 0
    tiles = (nbytes + 4095) // 4096
    grid = nblocks if nblocks > 0 else min(tiles, 1024)
    grid += grid % 2
    rounds = (tiles + grid - 1) // grid
    return 4, grid, rounds, 2 if rounds >= 8 else 1 if rounds >= 2 else 0


def self_reduce_inputs(dt, nbytes, seq):
    """x, y of one call: lcg values with random bit patterns over half of the lanes, new for every call."""
    count = nbytes // ITEM[dt]
    x, y = O.lcg(dt, count, 0, seq).copy(), O.lcg(dt, count, 1, seq).copy()
    rng = np.random.default_rng(7 + seq)
    m = rng.random(count) < 0.5
    bits = 8 * ITEM[dt]
    x[m] = rng.integers(0, 2**bits, m.sum(), dtype=np.uint64).astype(x.dtype)
    y[m] = rng.integers(0, 2**bits, m.sum(), dtype=np.uint64).astype(y.dtype)
    return x, y
