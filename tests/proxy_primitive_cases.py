"""Case tables and the plain model of the proxy-side device surface (tests/cpp/test_proxy_primitives.hip):
ProxyTrigger, FifoDeviceHandle::push / poll / sync, every overload of BasePortChannelDeviceHandle and
PortChannelDeviceHandle, and what ProxyService::handleTrigger / Connection::write make of their output.
No GPU, no torch.

  Group T  trigger images: one lane, one member, once, on a hand-built handle over a ring of 64 slots
  Group F  positions, laps and poll on hand-built rings of 2 .. 256 slots
  Group P  through this library's proxy (loopback, FIFO of 8, four arenas of 96 KiB, two semaphores)
  Group R  refusals that handleTrigger and Connection::write define

The model states the trigger's bit layout on its own (`encode`), replays a push sequence into a ring
image (`replay`) and moves bytes between arenas (`arenas_after`).  A case is one text line
"<idx> <op> <n> <v0> ... <vn-1>"; the meaning of v is in the builders below."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "idx group op v ref tag")

M64 = (1 << 64) - 1
NO_POS = M64

# ---- the trigger, from the bit layout ----------------------------------------------------------------
FIELD_BITS = dict(size=32, srcOffset=32, dstOffset=32, srcId=9, dstId=9, type=3, semaphoreId=10)


def fits(typ, dst_id, dst_off, src_id, src_off, size, sem):
    return (typ < 1 << 3 and dst_id < 1 << 9 and src_id < 1 << 9 and sem < 1 << 10 and dst_off < 1 << 32
            and src_off < 1 << 32 and size < 1 << 32)


def encode(typ, dst_id, dst_off, src_id, src_off, size, sem, commit=0):
    """fst = srcOffset << 32 | size; snd = dstOffset | srcId << 32 | dstId << 41 | type << 50 |
    semaphoreId << 53 | commit << 63.  Every field must fit: the model has no truncation of its own."""
    assert fits(typ, dst_id, dst_off, src_id, src_off, size, sem) and commit in (0, 1)
    fst = src_off << 32 | size
    snd = dst_off | src_id << 32 | dst_id << 41 | typ << 50 | sem << 53 | commit << 63
    return fst, snd


T_DATA, T_FLAG, T_SYNC = 1, 2, 4

# ---- ops ---------------------------------------------------------------------------------------------
PUT_FORMS = ["put", "put_same", "putWithSignal", "putWithSignal_same", "putWithSignalAndFlush",
             "putWithSignalAndFlush_same"]
FORM_TYPE = {"put": T_DATA, "put_same": T_DATA, "putWithSignal": T_DATA | T_FLAG,
             "putWithSignal_same": T_DATA | T_FLAG, "putWithSignalAndFlush": T_DATA | T_FLAG | T_SYNC,
             "putWithSignalAndFlush_same": T_DATA | T_FLAG | T_SYNC}
MEMBER_OPS = PUT_FORMS + ["signal", "flush", "push", "poll"]
PROXY_OPS = ["place", "order", "account", "laps", "refuse"]
FLUSH_OPS = ("flush", "putWithSignalAndFlush", "putWithSignalAndFlush_same")

# v[] of a member case
H = collections.namedtuple("H", "bound ring grid lanes active count step type dstId dstOff srcId srcOff size semId "
                                "tail flushDone")

OFFSETS = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
MEM_IDS = [0, 1, 255, 256, 511]
SEM_IDS = [0, 1, 511, 512, 1023]
DEFAULTS = dict(dstId=3, dstOff=0x123, srcId=5, srcOff=0x456, size=0x789, semId=9)
FLUSH_DONE = 1 << 20  # above every position a case can reach

ARENA = 96 << 10
WITNESS = 3 * ARENA
PROXY_FIFO = 8
N_MEM = 4
BOUND_DST, BOUND_SRC = 2, 1  # the PortChannelDeviceHandle of group P
FILL = 0xA5
WITNESS_FILL = 0x5A
ERR_BAD_GEOMETRY = 4
ERR_PROXY_FAILURE = 5

CASES = []


def _add(group, op, v, ref, tag):
    CASES.append(Case(len(CASES), group, op, tuple(int(x) for x in v), ref, tag))


def _member(group, op, tag, bound=0, ring=64, grid=1, lanes=1, active=None, count=1, step=0, type=0, tail=0,
            ref=True, **f):
    d = dict(DEFAULTS, **f)
    h = H(bound, ring, grid, lanes, grid * lanes if active is None else active, count, step, type, d["dstId"],
          d["dstOff"], d["srcId"], d["srcOff"], d["size"], d["semId"], tail, FLUSH_DONE if op in FLUSH_OPS else 0)
    _add(group, op, h, ref, tag)


ALL_AT_ONCE = [
    dict(dstOff=0xFFFFFFFF, srcOff=0x80000000, size=0x7FFFFFFF, dstId=511, srcId=256, semId=1023),
    dict(dstOff=0x80000000, srcOff=0xFFFFFFFF, size=0xFFFFFFFF, dstId=256, srcId=511, semId=512),
    dict(dstOff=0x7FFFFFFF, srcOff=1, size=0x80000000, dstId=255, srcId=1, semId=511),
    dict(dstOff=1, srcOff=0, size=1, dstId=1, srcId=0, semId=1),
    dict(dstOff=0, srcOff=0x7FFFFFFF, size=0, dstId=0, srcId=255, semId=0),
]
FIELD_VALUES = dict(dstOff=OFFSETS, srcOff=OFFSETS, size=OFFSETS, dstId=MEM_IDS, srcId=MEM_IDS, semId=SEM_IDS)


def _build_T():
    for op in PUT_FORMS:
        same = op.endswith("_same")
        for bound in (0, 1):
            who = "bound" if bound else "base"
            _member("T", op, f"{who}-defaults", bound=bound)
            for field, values in FIELD_VALUES.items():
                if same and field == "srcOff":
                    continue  # the common offset is dstOff
                for x in values:
                    _member("T", op, f"{who}-{field}={x:#x}", bound=bound, **{field: x})
            for i, combo in enumerate(ALL_AT_ONCE):
                _member("T", op, f"{who}-all{i}", bound=bound, **combo)
            # this library only: a value that does not fit is not pushed at all
            for field in ("dstOff", "size") if same else ("dstOff", "srcOff", "size"):
                _member("T", op, f"{who}-{field}=2^32", bound=bound, ref=False, **{field: 1 << 32})
    for op in ("signal", "flush"):
        for bound in (0, 1):
            who = "bound" if bound else "base"
            for x in [DEFAULTS["semId"]] + SEM_IDS:
                _member("T", op, f"{who}-semId={x:#x}", bound=bound, semId=x)
    for typ in range(1, 8):
        _member("T", "push", f"type={typ}-defaults", type=typ)
        for i, combo in enumerate(ALL_AT_ONCE):
            _member("T", "push", f"type={typ}-all{i}", type=typ, **combo)
    for field, values in FIELD_VALUES.items():
        for x in values:
            _member("T", "push", f"type=5-{field}={x:#x}", type=5, **{field: x})


SEQ_RINGS = {2: 1, 8: 3, 64: 37}  # ring size -> r, the partial last lap
LANE_SHAPES = [(1, 1, 1), (1, 63, 63), (1, 64, 64), (1, 65, 65), (3, 96, 256)]  # grid, lanes, active


def _ring_for(n):
    ring = 64
    while ring < n:
        ring *= 2
    return ring


def _build_F():
    for ring, r in SEQ_RINGS.items():
        for k in range(4):
            total = k * ring + r
            _member("F", "push", f"seq-ring{ring}-k{k}-r{r}", ring=ring, count=total, step=1, type=T_DATA, dstOff=0,
                    srcOff=0x80000000, tail=total)
    for grid, lanes, active in LANE_SHAPES:
        _member("F", "push", f"lanes-{active}", ring=_ring_for(active), grid=grid, lanes=lanes, active=active, step=1,
                type=T_DATA | T_FLAG, dstOff=0, srcOff=0x80000000)
    for grid, lanes, active in LANE_SHAPES[3:]:
        for op in PUT_FORMS:
            for bound in (0, 1):
                _member("F", op, f"lanes-{active}-{'bound' if bound else 'base'}", bound=bound, ring=_ring_for(active),
                        grid=grid, lanes=lanes, active=active, step=1, dstOff=0, srcOff=0x80000000)
    for head in (4, 5, 6):
        _member("F", "poll", f"tail5-fifoHead{head}", dstOff=head, tail=5)


# ---- group P -------------------------------------------------------------------------------------------
ALIGN_OFFSETS = [0, 1, 2, 4, 8, 12]
PLACE_SIZES = [0, 1, 15, 16, 17, 4099, (64 << 10) + 19]
PLACE_DST_BASES = [0x100, 0x200, 0x300, 0x400, 0x500, 0x1000, 0x3000]
ID_PAIRS = [(d, s) for d in range(N_MEM) for s in range(N_MEM) if d != s]


def _place(tag, bound, form, puts, split):
    v = [bound, PUT_FORMS.index(form), len(puts)] + list(split)
    for p in puts:
        v += list(p)
    _add("P", "place", v, False, tag)


def _build_P():
    pair_i = 0
    combos = [(f, b) for f in ("put", "putWithSignal", "putWithSignalAndFlush") for b in (0, 1)]
    same_combos = [(f, b) for f in ("put_same", "putWithSignal_same", "putWithSignalAndFlush_same") for b in (0, 1)]
    n = 0
    for dmod in ALIGN_OFFSETS:
        for smod in ALIGN_OFFSETS:
            runs = [combos[n % 6]]
            if dmod == smod:  # the common-offset overloads can only meet the diagonal
                runs.append(same_combos[ALIGN_OFFSETS.index(dmod)])
            n += 1
            for form, bound in runs:
                if bound:
                    dst, src = BOUND_DST, BOUND_SRC
                else:
                    dst, src = ID_PAIRS[pair_i % len(ID_PAIRS)]
                    pair_i += 1
                shift = 0 if form.endswith("_same") else 0x40
                puts = [(dst, base + dmod, src, base + shift + smod, size)
                        for base, size in zip(PLACE_DST_BASES, PLACE_SIZES)]
                split = [ARENA if a == src else 0 for a in range(N_MEM)]
                _place(f"d+{dmod}-s+{smod}-{form}-{'bound' if bound else 'base'}-{dst}<-{src}", bound, form, puts, split)
    # dstId == srcId over disjoint ranges: sources in the lower half, destinations in the upper
    half = ARENA // 2
    for a in range(N_MEM):
        dmod, smod = ALIGN_OFFSETS[a + 1], ALIGN_OFFSETS[(a + 3) % 6]
        puts = [(a, half + base + dmod, a, base + smod, size)
                for base, size in zip([0x100, 0x200, 0x300, 0x400, 0x500, 0x1000, 0x3000],
                                      [0, 1, 15, 16, 17, 4099, (16 << 10) + 3])]
        _place(f"same-id-{a}", 0, ("put", "putWithSignal", "putWithSignalAndFlush", "put")[a], puts,
               [half if x == a else 0 for x in range(N_MEM)])
    # data before signal: v = size, rounds, srcId, srcOff, srcStep, dstId0, dstOff, witnessStride
    for size in (16, 4099, (64 << 10) + 19):
        _add("P", "order", [size, 3, 0, 0x44, 4100, 1, 0x88, ARENA], False, f"order-{size}")
    # semaphore accounting: v = k, j, dstId, srcId
    for k, j in [(1, 0), (1, 1), (3, 0), (3, 2), (3, 3), (9, 0), (9, 4), (9, 9)]:
        _add("P", "account", [k, j, 2, 3], False, f"account-k{k}-j{j}")
    # laps under consumption and concurrent flushes: v = lanes, per, mode, dstId, srcId
    _add("P", "laps", [1, 5 * PROXY_FIFO + 3, 0, 1, 0], False, "laps-1x43")
    _add("P", "laps", [PROXY_FIFO, 6, 0, 1, 0], False, "laps-8x6")
    _add("P", "laps", [PROXY_FIFO, 1, 1, 1, 0], False, "flush-8-lanes")


GOOD_PUT = (2, 0x300, 0, 0x400, 32)
REFUSALS = {  # tag -> the refused put (dstId, dstOff, srcId, srcOff, size)
    "dst-id=count": (N_MEM, 0x100, 0, 0x200, 16),
    "src-id=count": (1, 0x100, N_MEM, 0x200, 16),
    "dst-one-byte-past": (1, ARENA - 16 + 1, 0, 0x200, 16),
    "src-one-byte-past": (1, 0x100, 0, ARENA - 16 + 1, 16),
}


def _build_R():
    for tag, bad in REFUSALS.items():
        _add("R", "refuse", list(bad) + list(GOOD_PUT), False, tag)


_build_T()
_build_F()
_build_P()
_build_R()


# ---- the case file -------------------------------------------------------------------------------------
def format_case(c):
    return f"{c.idx} {c.op} {len(c.v)} " + " ".join(str(x) for x in c.v)


def describe(c):
    return f"case {c.idx} [{c.group} {c.op} {c.tag}]: {format_case(c)}"


def write_case_file(path, for_reference=False):
    with open(path, "w") as f:
        for c in CASES:
            if not for_reference or c.ref:
                f.write(format_case(c) + "\n")


def parse_case_file(path):
    """-> [(idx, op, v)]"""
    out = []
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            v = tuple(int(x) for x in w[3:])
            assert len(v) == int(w[2]), line
            out.append((int(w[0]), w[1], v))
    return out


# ---- the model: members on a hand-built ring -----------------------------------------------------------
def member(c):
    assert c.op in MEMBER_OPS
    return H(*c.v)


def call_trigger(c, ordinal):
    """The trigger (7 fields) that call `ordinal` of a member case pushes; None when it pushes none."""
    h = member(c)
    off = h.dstOff + ordinal * h.step
    if c.op == "push":
        t = (h.type, h.dstId, off, h.srcId, h.srcOff, h.size, h.semId)
    elif c.op == "signal":
        t = (T_FLAG, 0, 0, 0, 0, 0, h.semId)
    elif c.op == "flush":
        t = (T_SYNC, 0, 0, 0, 0, 0, h.semId)
    elif c.op in PUT_FORMS:
        src_off = off if c.op.endswith("_same") else h.srcOff
        t = (FORM_TYPE[c.op], h.dstId, off, h.srcId, src_off, h.size, h.semId)
    else:
        return None
    return t if fits(*t) else None


def replay(ring_size, triggers, tail):
    """Push `triggers` (7-field tuples) in sequence into a zeroed ring: -> (ring [size, 2] uint64, head,
    tailCache, positions).  The commit bit of a slot is the lap parity of its position, lap 0 writing 1;
    a push at pos >= size + tailCache syncs on pos - size, which must already be below `tail`, and
    caches the tail it saw."""
    shift = ring_size.bit_length() - 1
    assert 1 << shift == ring_size
    ring = np.zeros((ring_size, 2), np.uint64)
    head = tail_cache = 0
    positions = []
    for t in triggers:
        pos = head
        head += 1
        if pos >= ring_size + tail_cache:
            assert pos - ring_size < tail, "the model never waits"
            tail_cache = tail
        commit = ((pos >> shift) & 1) ^ 1
        ring[pos & (ring_size - 1)] = encode(*t, commit=commit)
        positions.append(pos)
    return ring, head, tail_cache, positions


def expected_member(c):
    """-> dict(ring or None when the order is free, slots (multiset of (fst, snd)) , head, tail, tailCache,
    pos or None, err0)."""
    h = member(c)
    n = h.active * h.count
    if c.op == "poll":
        hit = h.dstOff < h.tail
        return dict(ring=np.zeros((h.ring, 2), np.uint64), head=0, tail=h.tail, tailCache=h.tail if hit else 0,
                    pos=[int(hit)], err0=0)
    trig = [call_trigger(c, i) for i in range(n)]
    if any(t is None for t in trig):  # this library refuses what does not fit: nothing is pushed
        assert all(t is None for t in trig)
        return dict(ring=np.zeros((h.ring, 2), np.uint64), head=0, tail=h.tail, tailCache=0, pos=[NO_POS] * n,
                    err0=ERR_BAD_GEOMETRY)
    ring, head, tail_cache, positions = replay(h.ring, trig, h.tail)
    e = dict(ring=ring, head=head, tail=h.tail, tailCache=tail_cache, err0=0,
             pos=positions if c.op == "push" else [NO_POS] * n)
    if h.active > 1:  # which lane got which position is free
        e["free"] = True
    return e


def judge_member(c, got):
    """got: dict(ring, head, tail, tailCache, pos, err) as parsed.  -> None or what differs."""
    h = member(c)
    e = expected_member(c)
    for k in ("head", "tail", "tailCache"):
        if got[k] != e[k]:
            return f"{k} {got[k]} != {e[k]}"
    if list(got["err"]) != [e["err0"], 0, 0, 0]:
        return f"error record {list(got['err'])} != {[e['err0'], 0, 0, 0]}"
    ring = got["ring"]
    if not e.get("free"):
        if got["pos"] != e["pos"]:
            return f"positions {got['pos'][:8]}.. != {e['pos'][:8]}.."
        bad = np.nonzero((ring != e["ring"]).any(axis=1))[0]
        if len(bad):
            s = int(bad[0])
            return (f"slot {s}: got ({int(ring[s, 0]):#x}, {int(ring[s, 1]):#x}), want "
                    f"({int(e['ring'][s, 0]):#x}, {int(e['ring'][s, 1]):#x})")
        return None
    # many lanes, one trigger each, all on lap 0 (the ring holds them all)
    n = h.active * h.count
    assert n <= h.ring
    if (ring[n:] != 0).any():
        return "a slot past the pushed ones is not zero"
    if c.op == "push":
        if sorted(got["pos"]) != list(range(n)):
            return "the returned positions are not a permutation of 0..N-1"
        for lane, pos in enumerate(got["pos"]):
            want = encode(*call_trigger(c, lane), commit=1)
            if (int(ring[pos, 0]), int(ring[pos, 1])) != want:
                return f"lane {lane} at position {pos}: slot ({int(ring[pos, 0]):#x}, {int(ring[pos, 1]):#x}) != {want}"
        return None
    if got["pos"] != e["pos"]:
        return "a void form wrote a position"
    have = sorted((int(a), int(b)) for a, b in ring[:n])
    want = sorted(encode(*call_trigger(c, i), commit=1) for i in range(n))
    if have != want:
        return f"the {n} used slots do not hold the {n} expected payloads (first got {have[0]}, want {want[0]})"
    return None


# ---- the model: arenas ----------------------------------------------------------------------------------
def pattern(idx, arena, nbytes):
    j = np.arange(nbytes // 4, dtype=np.uint64)
    x = ((j + 1) * 2654435761 + (idx * 4 + arena + 1) * 0x9E3779B9) & 0xFFFFFFFF
    x ^= x >> 15
    return x.astype("<u4").view(np.uint8)


def splits(c):
    s = [0] * N_MEM
    if c.op == "place":
        s = list(c.v[3:7])
    else:
        s[c.v[{"order": 2, "account": 3, "laps": 4, "refuse": 7}[c.op]]] = ARENA  # the source memory
    return s


def arenas_before(c):
    out = []
    for a, split in enumerate(splits(c)):
        m = np.full(ARENA, FILL, np.uint8)
        m[:split] = pattern(c.idx, a, ARENA)[:split]
        out.append(m)
    return out


def puts_of(c):
    """-> ([(dstId, dstOff, srcId, srcOff, size)] the proxy performs, triggers pushed, signals on A)."""
    v = c.v
    if c.op == "place":
        puts = [tuple(v[7 + 5 * p:12 + 5 * p]) for p in range(v[2])]
        return puts, len(puts) + 1, len(puts) if PUT_FORMS[v[1]] not in ("put", "put_same") else 0
    if c.op == "order":
        return [(v[5] + r, v[6], v[2], v[3] + r * v[4], v[0]) for r in range(v[1])], v[1] + 1, v[1]
    if c.op == "account":
        return [(v[2], 16 * i, v[3], 16 * (i + 7), 16) for i in range(v[0]) if i & 1], v[0] + 1, v[0]
    if c.op == "laps":
        cells = v[0] * v[1]
        return [(v[3], 16 * x, v[4], 16 * (x + 5), 16) for x in range(cells)], cells + (v[0] if v[2] else 1), 0
    assert c.op == "refuse"
    return [tuple(v[5:10])], 3, 0


def arenas_after(c):
    mem = arenas_before(c)
    src = [m.copy() for m in mem]
    for dst_id, dst_off, src_id, src_off, size in puts_of(c)[0]:
        mem[dst_id][dst_off:dst_off + size] = src[src_id][src_off:src_off + size]
    return mem


def witness_after(c):
    assert c.op == "order"
    v = c.v
    w = np.full(WITNESS, WITNESS_FILL, np.uint8)
    src = arenas_before(c)[v[2]]
    for r in range(v[1]):
        w[r * v[7]:r * v[7] + v[0]] = src[v[3] + r * v[4]:v[3] + r * v[4] + v[0]]
    return w


def judge_proxy(c, got):
    """got: dict(arenas, witness, err, handled, headBefore, head, sem (8 words), pos).  -> None or what differs."""
    puts, pushed, signals = puts_of(c)
    want_err = [ERR_PROXY_FAILURE if c.group == "R" else 0, 0, 0, 0]
    if list(got["err"]) != want_err:
        return f"error record {list(got['err'])} != {want_err}"
    for a, (have, want) in enumerate(zip(got["arenas"], arenas_after(c))):
        bad = np.nonzero(have != want)[0]
        if len(bad):
            b = int(bad[0])
            return f"arena {a} byte {b:#x}: got {int(have[b]):#x}, want {int(want[b]):#x} ({len(bad)} bytes differ)"
    if c.op == "order":
        bad = np.nonzero(got["witness"] != witness_after(c))[0]
        if len(bad):
            b = int(bad[0])
            return (f"witness byte {b:#x} (round {b // c.v[7]}): the data was not there when the signal was "
                    f"({len(bad)} bytes differ)")
    if got["handled"][1] - got["handled"][0] != pushed:
        return f"triggersHandled() rose by {got['handled'][1] - got['handled'][0]}, {pushed} triggers were pushed"
    if got["head"] - got["headBefore"] != pushed:
        return f"head rose by {got['head'] - got['headBefore']}, {pushed} triggers were pushed"
    before, after = got["sem"][:4], got["sem"][4:]
    if c.op == "account":
        k, j = c.v[0], c.v[1]
        if before != [0, 0, 0, 0] or after != [k, k, 0, 0]:
            return f"semaphore words (A inbound, A expected, B inbound, B expected) {before} -> {after}, want zeros -> {[k, k, 0, 0]}"
        if got["pos"] != [k - j]:
            return f"poll() was true {got['pos']} times, want {k - j}"
        return None
    want = [before[0] + signals, before[1] + signals, before[2], before[3]]
    if before[0] != before[1] or after != want:
        return f"semaphore words {before} -> {after}, want {want}"
    return None


# ---- the output file -------------------------------------------------------------------------------------
MAGIC = 0x3159584F52505644
RECORD_WORDS = 24


def parse_output(blob):
    """-> {idx: dict}"""
    head = np.frombuffer(blob, np.uint64, 4, 0)
    assert int(head[0]) == MAGIC and int(head[2]) == NO_POS
    out, off = {}, 32
    for _ in range(int(head[1])):
        r = [int(x) for x in np.frombuffer(blob, np.uint64, RECORD_WORDS, off)]
        off += 8 * RECORD_WORDS
        idx, slots, npos, narena = r[0:4]
        sizes = r[4:9]
        g = dict(handled=r[9:11], headBefore=r[11], head=r[12], tail=r[13], tailCache=r[14], sem=r[15:23])
        g["ring"] = np.frombuffer(blob, np.uint64, 2 * slots, off).reshape(slots, 2)
        off += 16 * slots
        g["pos"] = [int(x) for x in np.frombuffer(blob, np.uint64, npos, off)]
        off += 8 * npos
        mems = []
        for a in range(narena):
            mems.append(np.frombuffer(blob, np.uint8, sizes[a], off))
            off += sizes[a]
        g["arenas"], g["witness"] = mems[:4], mems[4] if narena > 4 else None
        g["err"] = [int(x) for x in np.frombuffer(blob, np.uint32, 4, off)]
        off += 16
        out[idx] = g
    assert off == len(blob), "trailing bytes"
    return out
