"""Tables, layouts and expectations of tests/test_allreduce_abi_gpu.py (no GPU, no torch here):
ncclAllReduce across processes through the library's own selector -- in place, on views inside an
allocation, every element type the ABI maps, SUM / MIN, and sizes on each side of the selector's
thresholds.  tests/test_allreduce_abi_cases.py proves on the CPU that the tables are not vacuous.

Inputs, input families and the judges are collective_edge_cases's (bits / finite, the oracle bit for
bit, the plain numpy / fp64 reference); nothing of them is restated here.  What is new:

  rows(n)           the table every rank of an n-process group runs, in order, on one communicator
  layout(row)       where the send and receive views of a row sit inside their 0xA5 allocations
  oracle_outputs()  the expected bytes from the oracle of the algorithm that ran (the selector's answer,
                    mscclppAmdSelectAlgo, or the forced one)
  refusals(n)       overlapping send / receive ranges that every entry point must refuse

Groups: 1 threshold sizes, 2 every type, 3 buffer forms, 4 forced algorithms on views, 5 refusals."""
import collections

import numpy as np

import collective_edge_cases as C
import kernel_edge_cases as K
import oracle_lib as O

RANKS = (2, 3, 8)
KIB = 1024
# The sizes rows are placed around.  That the selector really changes its answer between them is not
# taken from here: the CPU test asks mscclppAmdSelectAlgo.
SMALL_EDGE, LARGE_EDGE = 16 * KIB, 1 << 20
MAX_MESSAGE = LARGE_EDGE + 16 * KIB   # eight ranks' spinning kernels stay co-resident on one GPU
GUARD_BYTES = 256
CALLS = 3                             # per row, back to back, no host synchronisation between them

# ncclDataType_t / ncclRedOp_t of the reduce types the ABI maps (include/mscclpp_amd/nccl.h)
NCCL_TYPE = {O.F16: 6, O.BF16: 9, O.F32: 7, O.I32: 2, O.U32: 3, O.U8: 1, O.E4M3: 10, O.E5M2: 11}
NCCL_OP = {O.SUM: 0, O.MIN: 3}
TYPE_NAMES = {O.F16: "f16", O.BF16: "bf16", O.F32: "f32", O.I32: "i32", O.U32: "u32", O.U8: "u8", O.E4M3: "e4m3",
              O.E5M2: "e5m2"}
OP_NAMES = {O.SUM: "sum", O.MIN: "min"}
SELECTED = {1: "packet", 2: "allpair", 3: "fullmesh"}    # mscclppAmdSelectAlgo's codes
SUM_ORDER = {"fullmesh": 0, "rsag": 1, "rsag_zc": 1}     # O.allreduce_sliced order kinds
FORCED = ("allpair", "packet", "fullmesh", "rsag", "rsag_zc", "rsag_pipeline")

# group, reduce type, op, message bytes, buffer form, forced algorithm (None: the selector)
Row = collections.namedtuple("Row", "group code op nbytes form algo")
# forms: "base" out of place at the start of two allocations, "inplace" send == recv at the start of
# one, "a" out of place at byte 272 of two allocations, "b" out of place inside one allocation,
# "c" in place at an element-aligned offset that is not 16-byte aligned
FORMS = ("base", "inplace", "a", "b", "c")
VIEW_OFFSET = 272
ODD_OFFSET = 259                      # uint8: element-aligned is any byte


def region_sizes(es):
    """One message size inside each selector region."""
    return (4 * KIB + es, 256 * KIB + es, LARGE_EDGE + 16 + es)


def threshold_sizes(es):
    return (es, SMALL_EDGE - es, SMALL_EDGE, SMALL_EDGE + es, LARGE_EDGE - es, LARGE_EDGE, LARGE_EDGE + es)


G1_TYPES = ((O.F16, O.SUM), (O.F32, O.SUM), (O.I32, O.MIN))
G2_TYPES = tuple(NCCL_TYPE)
G3_TYPES = ((O.F16, O.SUM), (O.BF16, O.MIN), (O.U8, O.SUM))
G4_TYPES = ((O.F16, O.SUM), (O.F32, O.SUM))


def rows(n):
    """The rows of an n-rank group (the same at every n; the row id carries n)."""
    out = []
    for code, op in G1_TYPES:
        for nbytes in threshold_sizes(O.itemsize(code)):
            out += [Row(1, code, op, nbytes, form, None) for form in ("base", "inplace")]
    for code in G2_TYPES:
        for op in (O.SUM, O.MIN):
            out += [Row(2, code, op, nbytes, "inplace", None) for nbytes in region_sizes(O.itemsize(code))]
    for code, op in G3_TYPES:
        for nbytes in region_sizes(O.itemsize(code)):
            out += [Row(3, code, op, nbytes, form, None) for form in ("a", "b", "c")]
    for algo in FORCED:
        for code, op in G4_TYPES:
            es = O.itemsize(code)
            nbytes = (8 if algo == "allpair" else 256) * KIB + es
            out += [Row(4, code, op, nbytes, form, algo) for form in ("b", "c")]
    return out


def row_name(row):
    return f"g{row.group}-{TYPE_NAMES[row.code]}-{OP_NAMES[row.op]}-{row.nbytes}-{row.form}-{row.algo or 'auto'}"


def row_id(n, row):
    return C.case_id("allreduce-abi", n, *row)


def parts(n, k):
    """rows(n) dealt into k lists of about equal cost (a process group runs one list; the first one
    runs the refusals of group 5 as well, which count as half a million elements here).  The cost of
    a row is the host's: the oracle and the references work element by element."""
    def cost(row):
        return row.nbytes // O.itemsize(row.code) + 32 * KIB   # a call costs its launch as well

    out, load = [[] for _ in range(k)], [1 << 19] + [0] * (k - 1)
    for row in sorted(rows(n), key=lambda r: -cost(r)):
        i = load.index(min(load))
        out[i].append(row)
        load[i] += cost(row)
    order = {row: i for i, row in enumerate(rows(n))}
    return [sorted(p, key=order.get) for p in out]


def row_families(row):
    """Input family of the three calls: collective_edge_cases.families, except that the pipelined
    RS+AG, which has no oracle, takes finite inputs only (the plain reference is its one judge)."""
    return ("finite",) * CALLS if row.algo == "rsag_pipeline" else C.families(row.code)


def row_inputs(n, row, call):
    return C.reduce_inputs(row.code, row.op, n, row.nbytes // O.itemsize(row.code), row_id(n, row), call,
                           row_families(row)[call])


def has_plain(row, call):
    """The plain reference judges I32 / U32 always and the float types on their finite call."""
    return row.code in (O.I32, O.U32) or (row.code in C.FLOATS and row_families(row)[call] == "finite")


def layout(row):
    """((send allocation, byte offset), (receive allocation, byte offset), [bytes of each allocation]).
    Every allocation is filled with 0xA5 and keeps 256 guard bytes or more behind (and, for the
    views, before) each buffer."""
    nb, es = row.nbytes, O.itemsize(row.code)
    if row.form == "base":
        return (0, 0), (1, 0), [nb + GUARD_BYTES] * 2
    if row.form == "inplace":
        return (0, 0), (0, 0), [nb + GUARD_BYTES]
    if row.form == "a":
        return (0, VIEW_OFFSET), (1, VIEW_OFFSET), [VIEW_OFFSET + nb + GUARD_BYTES] * 2
    if row.form == "b":
        i, o, total = K.arena_layout(nb, 1, False)
        return (0, i), (0, o), [total]
    off = ODD_OFFSET if es == 1 else VIEW_OFFSET + es
    return (0, off), (0, off), [off + nb + GUARD_BYTES]


# ---- expectations ---------------------------------------------------------------------------------
def selected(lib, n, nbytes, code):
    """The algorithm the library's selector names for this call."""
    return SELECTED[lib.mscclppAmdSelectAlgo(n, nbytes, code)]


def oracle_outputs(lib, algo, code, op, ins, nbytes, order=None):
    """[rank] -> the nbytes result bytes of `algo` by its oracle; None for rsag_pipeline, which has
    none.  order: another sum order of the sliced oracle than the algorithm's (the CPU test's probe)."""
    n, count = len(ins), nbytes // O.itemsize(code)
    if algo == "rsag_pipeline":
        return None
    if algo in ("packet", "allpair"):
        half = lib.mscclppAmdScratchRequired(2 if algo == "allpair" else 1, n, nbytes, code) // 2
        fn = O.allreduce_allpairs if algo == "allpair" else O.allreduce_packet
        outs = fn(code, op, ins, count, 1, half)[0]
    else:
        nwords = (nbytes + 3) // 4
        padded = []
        for a in ins:
            w = np.zeros(nwords, np.uint32)
            w.view(np.uint8)[:nbytes] = C.as_bytes(a)
            padded.append(w)
        outs = O.allreduce_sliced(code, op, padded, nwords, K.slice_bytes(n, nbytes) // 4,
                                  SUM_ORDER[algo] if order is None else order)
    return [o.view(np.uint8)[:nbytes] for o in outs]


def judge(row, call, ins, got, exp):
    """Wrong bytes / lanes of one rank's result `got` (bytes): against the oracle's `exp` where the
    algorithm has one, and against the plain reference where the row has one."""
    bad = 0
    if exp is not None:
        bad += int(C.mismatches(row.code, got.copy(), exp.copy()).size)
    if has_plain(row, call):
        bad += int(C.plain_failures(row.code, row.op, ins, got.copy()).size)
    return bad


# ---- group 5: refusals ------------------------------------------------------------------------------
# (entry point, reduce type, op, bytes: the message of an AllReduce, the per-rank block of a ReduceScatter)
Refusal = collections.namedtuple("Refusal", "what code op nbytes")
REFUSALS = (Refusal("allreduce", O.F16, O.SUM, 4 * KIB), Refusal("allreduce", O.F16, O.SUM, 256 * KIB),
            Refusal("reducescatter", O.F16, O.SUM, C.ABI_BLOCK))
REFUSAL_SHIFT = 16
REFUSED = 4                           # ncclInvalidArgument
AFTER_BLOCK = C.ABI_BLOCK             # the valid AllReduce / ReduceScatter / AllGather that follow


def refusal_layout(ref, rank, n):
    """(send offset, send bytes, receive offset, receive bytes, allocation bytes) inside one 0xA5
    allocation: AllReduce recv = send + 16 bytes; ReduceScatter recv = block (rank + 1) % n of send."""
    if ref.what == "allreduce":
        return GUARD_BYTES, ref.nbytes, GUARD_BYTES + REFUSAL_SHIFT, ref.nbytes, \
            GUARD_BYTES + REFUSAL_SHIFT + ref.nbytes + GUARD_BYTES
    return GUARD_BYTES, n * ref.nbytes, GUARD_BYTES + (rank + 1) % n * ref.nbytes, ref.nbytes, \
        GUARD_BYTES + n * ref.nbytes + GUARD_BYTES


def refusal_name(ref):
    return f"g5-{ref.what}-{ref.nbytes}-refused"


# the keys every worker reports True for besides its rows
AFTER_CHECKS = ("g5-allreduce-after", "g5-reducescatter-after", "g5-allgather-after")
