"""Case tables, inputs and CPU expectations of tests/test_executor_ops_gpu.py (no GPU, no torch here).

The GPU file runs these tables; tests/test_executor_plan.py proves on the CPU that every plan in
them is deadlock free in the oracle, that the oracle's integer results are the plain numpy answer
at these very sizes, and that the tables together reach every operation of the device switch and
every (reuse scratch, packet type, reduce operation) kernel variant."""
import json
import os

import numpy as np

import kernel_edge_cases as K
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")
GUARD = 0xA5
GUARD_BYTES = 256          # message offset in its arena; at least as many guard bytes follow it
ARENA_BYTES = 1 << 20      # one arena for the input and one for the output, per rank
DT = {"f16": O.F16, "bf16": O.BF16, "f32": O.F32, "i32": O.I32, "u32": O.U32, "e4m3": O.E4M3, "e5m2": O.E5M2,
      "u8": O.U8, "b15": O.B15}
WORD_DTYPES = ("i32", "u32", "f16", "bf16", "f32")
BYTE_DTYPES = ("e4m3", "e5m2", "u8", "b15")
NP_INT = {"i32": np.int32, "u32": np.uint32}
PACKET_REDUCES = {"repkt", "respkt", "recpkt", "recspkt"}
REUSE_THRESHOLD = 16384    # PREDEFINED_SCRATCH / scratch_chunks 4096: above it scratch offsets wrap
# reuse plan chunk sizes: below, at and above the threshold, and well above it; with unit_size 4096
# the first, third and fourth leave a partial last pipeline iteration
REUSE_CHUNKS = (16368, 16384, 16400, 40976)

_DOCS = {}


def doc(fname):
    if fname not in _DOCS:
        with open(os.path.join(PLANS, fname)) as f:
            _DOCS[fname] = json.load(f)
    return _DOCS[fname]


def all_ops(d):
    """Operation names of a plan, pipelines' inner operations included."""
    names = set()
    for g in d["gpus"]:
        for tb in g["threadblocks"]:
            for o in tb["ops"]:
                names.add(o["name"])
                names.update(i["name"] for i in o.get("ops", []))
    return names


def reduce_ops(d):
    return {o.get("reduce_op") for g in d["gpus"] for tb in g["threadblocks"] for top in tb["ops"]
            for o in [top] + top.get("ops", []) if "reduce_op" in o}


def is_min(d):
    return "min" in reduce_ops(d)


def _tbg_size(d):
    return max([o["tbg_info"]["tbg_size"] for g in d["gpus"] for tb in g["threadblocks"] for top in tb["ops"]
                for o in [top] + top.get("ops", []) if "tbg_info" in o] or [1])


def in_out_bytes(d, msg):
    """(input bytes, output bytes) of a message of `msg` bytes (the larger of the two buffers)."""
    n = len(d["gpus"])
    if d["collective"] == "allgather":
        return msg // n, msg
    if d["collective"] == "reducescatter":
        return msg, msg // n
    return msg, msg


def message_sizes(fname, pkt):
    """Message sizes (bytes of the chunked buffer) a plan is run at: the minimum, chunks x alignment;
    the sizes at which a threadblock's slice of a chunk is nthreads-1, nthreads and nthreads+1 units
    (16 bytes for Simple plans, one packet payload for LL plans; where the alignment is coarser than
    the unit the slice is rounded to it, down below nthreads and up above: LL16 at alignment 16 gets
    nthreads-2 and nthreads+2 packets); and an odd multiple, chunks x alignment x 1007.  The reuse
    plans take the chunk sizes around the wrap threshold instead."""
    d = doc(fname)
    g = d["gpus"][0]
    chunks, align, nt = max(g["input_chunks"], g["output_chunks"]), d["buffer_alignment"], d["num_threads_per_block"]
    if d["reuse_resources"]:
        return [chunks * c for c in REUSE_CHUNKS]
    unit = (8 if pkt == "LL16" else 4) if d["protocol"] == "LL" else 16
    T = _tbg_size(d)
    lo, mid, hi = (nt - 1) * unit // align * align, nt * unit, -(-(nt + 1) * unit // align) * align
    sizes = [chunks * align] + [chunks * T * s for s in (lo, mid, hi)] + [chunks * align * 1007]
    assert all(s % (chunks * align) == 0 and s <= ARENA_BYTES - 2 * GUARD_BYTES for s in sizes), (fname, sizes)
    return sizes


def make_inputs(dtype, n, nbytes, seq):
    """Per-rank input bytes: random values with random bit patterns over a quarter of the lanes (NaN,
    inf, subnormals, negative and >= 2^31 integers) and, for floats in buffers that hold them, the
    planted groups of tests/kernel_edge_cases.py (NaN against numbers, +0 against -0, subnormals,
    +-inf); plain LCG bytes for the one-byte types."""
    code = DT[dtype]
    count = nbytes // O.itemsize(code)
    if dtype in BYTE_DTYPES:
        return [O.lcg(code, count, r, seq).view(np.uint8).copy() for r in range(n)]
    edges = K.is_float(code) and count >= K.EDGE_GROUPS * K.EDGE_LANES
    return [a.view(np.uint8).copy() for a in K.inputs(code, n, count, seq=seq, special=True, edges=edges)]


def numpy_answer(d, dtype, ins):
    """The collective's result per rank, computed without the oracle: i32 / u32 only (wrapping sum,
    min, concatenation).  None where there is no such answer: other types, and `min` through the
    packet reductions, which start from zero words (as the reference's do)."""
    if dtype not in NP_INT:
        return None
    n, npdt = len(ins), NP_INT[dtype]
    coll = d["collective"]
    if coll == "allgather":
        return [np.concatenate(ins)] * n
    if coll == "get_offsets":  # [my input chunk 1, the peer's input chunk 0]
        h = ins[0].size // 2
        return [np.concatenate([ins[r][h:], ins[1 - r][:h]]) for r in range(2)]
    v = np.stack([a.view(npdt) for a in ins])
    if is_min(d):
        if all_ops(d) & PACKET_REDUCES:
            return None
        red = v.min(axis=0)
    else:
        red = v.view(np.uint32).sum(axis=0, dtype=np.uint64).astype(np.uint32)  # wraps like the device's add
    red = np.ascontiguousarray(red).view(np.uint8)
    if coll == "reducescatter":
        c = red.size // n
        return [red[r * c:(r + 1) * c] for r in range(n)]
    assert coll == "allreduce", coll
    return [red] * n


class Case:
    """One GPU case: `steps` = [(plan file, message bytes)] executed in order with fresh inputs."""

    def __init__(self, steps, dtype, pkt, tag=""):
        self.steps, self.dtype, self.pkt = steps, dtype, pkt
        names = []
        for f, _ in steps:
            if f[:-5] not in names:
                names.append(f[:-5])
        sizes = []
        for _, s in steps:
            if s not in sizes:
                sizes.append(s)
        self.id = "+".join(names) + "-" + "_".join(map(str, sizes)) + f"-{dtype}-{pkt}" + tag

    def nranks(self):
        return len(doc(self.steps[0][0])["gpus"])


def _plan_cases(fname, pkts, dtypes=WORD_DTYPES, calls=3):
    """i32 and u32 at every size; the float and byte types at the smallest, one threshold and the odd size."""
    out = []
    for pkt in pkts:
        sizes = message_sizes(fname, pkt)
        for dt in dtypes:
            pick = sizes if dt in NP_INT else [sizes[0], sizes[-2], sizes[-1]]
            out += [Case([(fname, s)] * calls, dt, pkt) for s in pick]
    return out


BOTH, LL16, LL8 = ("LL16", "LL8"), ("LL16",), ("LL8",)
ALL_DTYPES = WORD_DTYPES + BYTE_DTYPES


def _cases_2():
    c = []
    c += _plan_cases("allgather_get_n2.json", LL16)
    c += _plan_cases("get_offsets_n2.json", LL16, ("i32", "u32", "f16"))
    c += _plan_cases("reducescatter_rre_n2.json", LL16, ALL_DTYPES)
    c += _plan_cases("reducescatter_rre_min_n2.json", LL8)
    c += _plan_cases("reducescatter_rre_a4_n2.json", LL16)
    c += _plan_cases("allreduce_res_n2.json", LL8)
    c += _plan_cases("allreduce_relay_n2.json", BOTH)
    c += _plan_cases("allreduce_relay_min_n2.json", BOTH)
    c += _plan_cases("allreduce_reuse_n2.json", BOTH)
    c += _plan_cases("allreduce_reuse_min_n2.json", BOTH)
    c += _plan_cases("allreduce_rres_min_n2.json", LL16)
    c += _plan_cases("allreduce_put_min_n2.json", LL16)
    c += _plan_cases("allreduce_put_a4_n2.json", BOTH)
    c += _plan_cases("allreduce_put_min_a4_n2.json", LL8)
    c += _plan_cases("reducescatter_rre_min_a4_n2.json", LL8)
    c += _plan_cases("allreduce_pkt_a4_n2.json", LL8)
    c += _plan_cases("allreduce_pkt_a8_n2.json", BOTH)
    # i32 / u32 on the plans the older GPU file runs with floats only
    c += _plan_cases("allreduce_pkt_n2.json", BOTH, ("i32", "u32"))
    c += _plan_cases("allreduce_rres_n2.json", LL16, ("i32", "u32"))
    c += _plan_cases("allreduce_put_n2.json", LL16, ("i32", "u32"))
    # two message sizes in turn on the same buffers (A, B, A, B): the device plan cache and re-lowering
    for f, pkt in (("allreduce_relay_n2.json", "LL16"), ("allreduce_res_n2.json", "LL16"),
                   ("allreduce_reuse_n2.json", "LL8")):
        s = message_sizes(f, pkt)
        a, b = s[-1], s[1]
        c += [Case([(f, a), (f, b), (f, a), (f, b)], dt, pkt, "-abab") for dt in ("u32", "f16")]
    # a packet plan and a Simple plan in turn on one Executor: shared flag, tokens and wait counters
    p, q = "allreduce_relay_n2.json", "allreduce_res_n2.json"
    sp, sq = message_sizes(p, "LL16")[-1], message_sizes(q, "LL16")[-1]
    c += [Case([(p, sp), (q, sq), (p, sp), (q, sq)], dt, "LL16", "-pqpq") for dt in ("i32", "bf16")]
    return c


def _cases_4():
    c = []
    c += _plan_cases("allgather_get_n4.json", LL8)
    c += _plan_cases("reducescatter_rre_n4.json", LL16)
    c += _plan_cases("reducescatter_rre_min_n4.json", LL16)
    c += _plan_cases("allreduce_res_n4.json", LL16)
    c += _plan_cases("allreduce_relay_n4.json", BOTH, ALL_DTYPES)
    c += _plan_cases("allreduce_reuse_n4.json", BOTH)
    c += _plan_cases("allreduce_rres_min_n4.json", LL8)
    c += _plan_cases("allreduce_pkt_n4.json", BOTH, ("i32", "u32"))
    c += _plan_cases("allreduce_rres_n4.json", LL16, ("i32", "u32"))
    c += _plan_cases("allreduce_put_n4.json", LL16, ("i32", "u32"))
    return c


def _cases_8():
    c = []
    for f in ("allreduce_pkt_n8.json", "allgather_get_n8.json"):
        s = message_sizes(f, "LL16")
        c += [Case([(f, size)] * 3, dt, "LL16") for size in (s[0], s[-1]) for dt in ("i32", "u32", "f16")]
    return c


CASES = {2: _cases_2(), 4: _cases_4(), 8: _cases_8()}
# plans the older tests/test_executor_gpu.py executes (its CASES_2 / CASES_4 / CASES_REF)
OLDER_GPU_PLANS = ["allreduce_pkt_n2.json", "allreduce_rres_n2.json", "allreduce_put_n2.json", "allreduce_pkt_n4.json",
                   "allreduce_rres_n4.json", "allreduce_put_n4.json", "ref/allreduce_packet.json", "ref/allreduce.json"]


def gpu_plans():
    """Every plan file some GPU test executes."""
    return sorted({f for cs in CASES.values() for c in cs for f, _ in c.steps} | set(OLDER_GPU_PLANS))


def kernel_variants():
    """(reuse scratch, packet type, reduce operation) of every GPU case in the tables here."""
    return {(doc(f)["reuse_resources"], c.pkt, op) for cs in CASES.values() for c in cs for f, _ in c.steps
            for op in reduce_ops(doc(f))}


def run_oracle(case, first_flag):
    """The oracle's per-step (inputs, expected output bytes per rank, numpy answer or None) of a case
    whose first call is the executor's call number `first_flag`: one oracle object per plan, its
    flag set to the call number before every step."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import executor_oracle as E

    n = case.nranks()
    oracles, steps = {}, []
    for k, (fname, msg) in enumerate(case.steps):
        d = doc(fname)
        eo = oracles.setdefault(fname, E.ExecutorOracle(d, n))
        eo.flag = first_flag + k - 1
        ib, ob = in_out_bytes(d, msg)
        ins = make_inputs(case.dtype, n, ib, seq=first_flag + k)
        if d["inplace"]:
            bufs = [a.copy() for a in ins]
            res = eo.execute(bufs, bufs, case.dtype, packet=case.pkt)
            outs = [res[r][0] for r in range(n)]
        else:
            src = [a.copy() for a in ins]
            res = eo.execute(src, [np.full(ob, GUARD, np.uint8) for _ in range(n)], case.dtype, packet=case.pkt)
            assert all(np.array_equal(src[r], ins[r]) for r in range(n)), "the oracle changed an out-of-place input"
            outs = [res[r][1] for r in range(n)]
        steps.append((ins, outs, numpy_answer(d, case.dtype, ins)))
    return steps
