"""Case tables and the plain model of the device primitive matrix (tests/cpp/test_device_primitives.hip):
copy / put / get at every <Alignment, CopyRemainder>, the packet forms of LL16 and LL8, the packet
classes, read<T> / write<T> and the semaphore handles, at offsets, misalignments, remainders and lane
shapes.  numpy only: no GPU, no torch.

One case is one launch of the program's generic kernel over three arenas:
  L  the channel's src_ (local memory),  R  its dst_ (the "peer": a second allocation),
  K  its packetBuffer_ (uncached).
The handle's pointers are arena + GUARD, so every offset of a case is relative to GUARD bytes into
its arena, and the program dumps all three arenas whole after the launch: a stray write anywhere,
the guards included, is a difference.  `expected(case)` is the model: it builds the arenas as the
program's host side fills them and applies the primitive's definition with numpy slices.
"""
from collections import namedtuple

import numpy as np

GUARD = 256          # bytes before the handle's base and after the last byte a case may touch
MAX_ARENA = 160 << 10  # what the program allocates per arena (it checks every case against it)
FILL = 0xA5
FILL_WORD = 0xA5A5A5A5
BUDGET_TICKS = 2_000_000  # 20 ms of 10 ns ticks: every handle's wait bound
MAGIC = 0x314D495250564544  # "DEVPRIM1"

INIT_FILL, INIT_PATTERN, INIT_IMAGE = 0, 1, 2
ARENA_L, ARENA_R, ARENA_K, PAYLOAD = 0, 1, 2, 3

FIELDS = ("idx op p0 p1 grid lanes toff ooff nbytes flag sL sR sK iL iR iK imgoff imgcount stale ref group tags")
Case = namedtuple("Case", FIELDS)

SHAPES = ((1, 1), (1, 63), (1, 64), (1, 65), (1, 256), (1, 1000), (3, 192))
FLAGS = (1, 0x7FFFFFFF, 0xFFFFFFFF)

# ---- Group A ------------------------------------------------------------------------------------
COPY_OPS = ("copy", "put2", "put1", "get2", "get1")
ALIGNMENTS = (4, 8, 16)
MISALIGNMENTS = (0, 4, 8, 12)
COPY_BYTES = (0, 4, 8, 12, 16, 20, 36, 1020, 1024, 1028, 4100, 65540)
RAGGED_BYTES = (18, 1027)  # the last 1 to 3 bytes are not copied
BELOW_HEAD = ((4, 4), (4, 8), (12, 0))  # (misalignment, bytes): sizes below the 4-byte head
TARGET_OFF, ORIGIN_OFF = 0x130, 0x50

# ---- Group B ------------------------------------------------------------------------------------
PACKET_OPS = ("putPackets2", "putPackets1", "unpackPackets2", "unpackPackets1", "unpackPacket", "copyToPackets",
              "copyFromPackets")
UNIT_OPS = ("put_unit", "try_unit")  # ll16_ / ll8_: no reference spelling
PAYLOAD_BYTES = (0, 4, 8, 12, 1024, 1028, 4104)
UNIT_EXTRA_BYTES = (16, 48)  # one and three whole units (a unit is 16 payload bytes)
PACKET_OFF, DATA_OFF, SAME_OFF = 0x240, 0x50, 0x140

# ---- Group C / D / E ----------------------------------------------------------------------------
CLASS_OPS = ("pkt_ctor", "pkt_write3", "pkt_write64", "pkt_write2", "pkt_clear", "readOnce2", "readOnce3", "pkt_read")
RW_TYPES = {4: "uint32_t", 8: "uint64_t", 2: "uint2"}  # p0 -> T (uint2 is 8 bytes)
SEM_OPS = ("sem_d2d", "sem_base", "sem_h2d")
LIBRARY_ONLY_OPS = UNIT_OPS + ("readOnce3",) + SEM_OPS

OPS = COPY_OPS + PACKET_OPS + UNIT_OPS + CLASS_OPS + ("rw",) + SEM_OPS


def pattern(idx, arena, nwords, first=0):
    """Word j of arena `arena` of case `idx` (the program's pat()): a multiplicative hash, never the
    fill word and never a flag of the tables (asserted in test_device_primitive_cases.py)."""
    j = np.arange(first, first + nwords, dtype=np.uint64)
    x = ((j + 1) * 2654435761 + (idx * 4 + arena + 1) * 0x9E3779B9) & 0xFFFFFFFF
    x ^= x >> 15
    return x.astype(np.uint32)


def payload_per_packet(psize):
    return 8 if psize == 16 else 4


def round256(n):
    return (n + 255) // 256 * 256


def arena_size(off, extent):
    return round256(GUARD + off + extent + GUARD)


# ---- the model of copyHelper ----------------------------------------------------------------------
def copy_ranges(dst_addr, nbytes, A, R, clamp=True):
    """(head, body, tail, [(from, to)]) in 4-byte words and source-relative byte ranges written.
    clamp=False is the reference's arithmetic for bytes < head (it underflows: see DESIGN)."""
    n4 = nbytes // 4
    head = ((-dst_addr) % A) // 4
    if clamp:
        head = min(head, n4)
    elif head > n4:
        raise OverflowError("numInt - nFirstInt underflows")
    per = A // 4
    body = (n4 - head) // per
    tail = n4 - head - body * per
    if R:
        return head, body, tail, [(0, 4 * n4)]
    return head, body, tail, [(4 * head, 4 * head + A * body)]


def copy_roles(op):
    """(destination arena, source arena) of a Group A primitive."""
    return (ARENA_L, ARENA_R) if op.startswith("get") else (ARENA_R, ARENA_L)


def copy_geometry(case, bases=(0, 0, 0)):
    dst, _ = copy_roles(case.op)
    return copy_ranges(bases[dst] + GUARD + case.toff, case.nbytes, case.p0, bool(case.p1))


# ---- building the table ----------------------------------------------------------------------------
def _mk(cases, group, op, p0, p1, shape, toff, ooff, nbytes, flag, sizes, inits, imgoff=0, imgcount=0, stale=(),
        tags=()):
    ref = 0 if op in LIBRARY_ONLY_OPS or "below_head" in tags else 1
    cases.append(Case(len(cases), op, p0, p1, shape[0], shape[1], toff, ooff, nbytes, flag, sizes[0], sizes[1],
                      sizes[2], inits[0], inits[1], inits[2], imgoff, imgcount, tuple(stale), ref, group,
                      tuple(tags)))


def _group_a(cases):
    for op in COPY_OPS:
        two = op in ("copy", "put2", "get2")
        dst, src = copy_roles(op)
        inits = [INIT_FILL] * 3
        inits[src] = INIT_PATTERN
        for A in ALIGNMENTS:
            for R in (1, 0):
                rows = []
                for i, nb in enumerate(COPY_BYTES + RAGGED_BYTES):
                    rows.append((MISALIGNMENTS[i % 4], nb, SHAPES[(i + 2) % 7], ("ragged",) if nb % 4 else ()))
                for m in MISALIGNMENTS:
                    rows.append((m, 20, SHAPES[2], ()))
                    rows.append((m, 1028, SHAPES[6], ()))
                for shape in SHAPES:
                    rows.append((4, 1028, shape, ()))
                for m, nb in BELOW_HEAD:
                    rows.append((m, nb, SHAPES[2], ()))
                for m, nb, shape, tags in rows:
                    toff = TARGET_OFF + m
                    ooff = ORIGIN_OFF + m if two else toff
                    head_raw = ((-(GUARD + toff)) % A) // 4
                    tags = list(tags)
                    if nb // 4 < head_raw:
                        tags.append("below_head")
                    head, body, tail, _ = copy_ranges(GUARD + toff, nb, A, R)
                    if head + tail > 0:
                        tags.append("remainder")
                    if two:
                        tags.append("two_offsets")
                    s = arena_size(max(toff, ooff), nb)
                    _mk(cases, "A", op, A, R, shape, toff, ooff, nb, 0, (s, s, 2 * GUARD), inits, tags=tags)


def _group_b(cases):
    for psize in (16, 8):
        per = payload_per_packet(psize)
        for op in PACKET_OPS + UNIT_OPS:
            sizes = PAYLOAD_BYTES + (UNIT_EXTRA_BYTES if op in UNIT_OPS else ())
            rows = [(nb, SHAPES[(i + 1) % 7], FLAGS[i % 3]) for i, nb in enumerate(sizes)]
            rows += [(1028, shape, 1) for shape in SHAPES]
            rows += [(1024, SHAPES[3], f) for f in FLAGS]
            for nb, shape, flag in rows:
                same = op.endswith("1")
                poff, doff = (SAME_OFF, SAME_OFF) if same else (PACKET_OFF, DATA_OFF)
                if op in UNIT_OPS:
                    npk = nb // 16 * (32 // psize)
                else:
                    npk = nb // per
                # both arenas hold either offset, so a swap of the two lands inside the dump; a reader's
                # image has one valid packet more than the call may unpack, so a packet count rounded
                # up moves payload that the model leaves alone
                extra = 0 if op in UNIT_OPS else 1
                pk_arena = arena_size(max(poff, doff), (npk + extra) * psize)
                data_arena = arena_size(max(poff, doff), nb + 8)
                tags = ["two_offsets"] if op.endswith("2") else []
                if psize == 16 and nb % 8 == 4 and op not in UNIT_OPS:
                    tags.append("ll16_remainder")
                if op in ("putPackets2", "putPackets1"):
                    # packets go to the peer's memory (dst_), the data comes from src_
                    sz = (data_arena, pk_arena, 2 * GUARD)
                    inits = (INIT_PATTERN, INIT_FILL, INIT_FILL)
                    _mk(cases, "B", op, psize, 0, shape, poff, doff, nb, flag, sz, inits, tags=tags)
                elif op in ("copyToPackets", "put_unit"):
                    sz = (data_arena, 2 * GUARD, pk_arena)
                    inits = (INIT_PATTERN, INIT_FILL, INIT_FILL)
                    _mk(cases, "B", op, psize, 0, shape, poff, doff, nb, flag, sz, inits, tags=tags)
                else:
                    # readers: the image is in K before the launch, the data lands in L; try_unit
                    # stores its verdict per unit in R
                    sz = (data_arena, arena_size(0, 4 * (nb // 16)) if op == "try_unit" else 2 * GUARD, pk_arena)
                    inits = (INIT_FILL, INIT_FILL, INIT_IMAGE)
                    _mk(cases, "B", op, psize, 0, shape, poff, doff, nb, flag, sz, inits, imgoff=poff,
                        imgcount=npk + extra, tags=tags)


ONE = (1, 1)


def _group_c(cases):
    small = arena_size(PACKET_OFF, 64)
    for psize in (16, 8):
        for i, flag in enumerate(FLAGS):
            # constructor and the write forms: one lane, the value words come from L's pattern
            ops = ("pkt_ctor", "pkt_write3", "pkt_write64", "pkt_write2") if psize == 16 else ("pkt_ctor", "pkt_write3")
            for op in ops:
                _mk(cases, "C", op, psize, 0, ONE, PACKET_OFF + 16 * i, DATA_OFF + 8 * i, 8, flag,
                    (small, 2 * GUARD, small), (INIT_PATTERN, INIT_FILL, INIT_FILL))
            # clear(): the middle one of three packets
            _mk(cases, "C", "pkt_clear", psize, 0, ONE, PACKET_OFF + psize, 0, 0, flag, (2 * GUARD, 2 * GUARD, small),
                (INIT_FILL, INIT_FILL, INIT_IMAGE), imgoff=PACKET_OFF, imgcount=3)
            # readOnce on four host-written packets: both flags right, only flag1, only flag2, neither
            stale = (7, 9, 13, 15) if psize == 16 else (3, 7)  # LL8: packets 1 and 3 stale
            for op in ("readOnce2", "readOnce3") if psize == 16 else ("readOnce2",):
                _mk(cases, "C", op, psize, 0, ONE, PACKET_OFF, DATA_OFF, 0, flag, (small, 2 * GUARD, small),
                    (INIT_FILL, INIT_FILL, INIT_IMAGE), imgoff=PACKET_OFF, imgcount=4, stale=stale)
            # read(flag) on ready packets
            _mk(cases, "C", "pkt_read", psize, 0, SHAPES[1], PACKET_OFF, DATA_OFF, 5 * payload_per_packet(psize), flag,
                (small, 2 * GUARD, arena_size(PACKET_OFF, 5 * psize)), (INIT_FILL, INIT_FILL, INIT_IMAGE),
                imgoff=PACKET_OFF, imgcount=5)
        # the safety property on the hot kernels' form: one stale flag word of a unit, at each position
        for pos in (1, 3, 5, 7):
            _mk(cases, "C", "try_unit", psize, 0, SHAPES[2], PACKET_OFF, DATA_OFF, 32, FLAGS[pos % 3],
                (small, arena_size(0, 8), arena_size(PACKET_OFF, 64)), (INIT_FILL, INIT_FILL, INIT_IMAGE),
                imgoff=PACKET_OFF, imgcount=64 // psize, stale=(8 + pos,), tags=("stale_unit",))


def _group_d(cases):
    for T in RW_TYPES:
        for chan in (1, 0):
            for n, shape in ((1, ONE), (5, SHAPES[2]), (65, SHAPES[3])):
                # write<T> at index 11.., read<T> at index 150.. of R; the values read land in L
                s = arena_size(0, 8 * (150 + 65))
                _mk(cases, "D", "rw", T, chan, shape, 11, 150, n, 0, (arena_size(0, 8 * 65), s, 2 * GUARD),
                    (INIT_FILL, INIT_PATTERN, INIT_FILL))


def _group_e(cases):
    for op in SEM_OPS:
        _mk(cases, "E", op, 0, 0, ONE, 0, 0, 0, 0, (arena_size(0, 128), 2 * GUARD, 2 * GUARD),
            (INIT_FILL, INIT_FILL, INIT_FILL))


def build_cases():
    cases = []
    _group_a(cases)
    _group_b(cases)
    _group_c(cases)
    _group_d(cases)
    _group_e(cases)
    return cases


CASES = build_cases()


# ---- the case file ---------------------------------------------------------------------------------
def format_case(c):
    stale = list(c.stale) + [0] * (4 - len(c.stale))
    nums = [c.p0, c.p1, c.grid, c.lanes, c.toff, c.ooff, c.nbytes, c.flag, c.sL, c.sR, c.sK, c.iL, c.iR, c.iK, c.imgoff,
            c.imgcount, len(c.stale)] + stale + [c.ref]
    return f"{c.idx} {c.op} " + " ".join(str(x) for x in nums)


def parse_case(line):
    t = line.split()
    n = [int(x) for x in t[2:]]
    return dict(idx=int(t[0]), op=t[1], p0=n[0], p1=n[1], grid=n[2], lanes=n[3], toff=n[4], ooff=n[5], nbytes=n[6],
                flag=n[7], sL=n[8], sR=n[9], sK=n[10], iL=n[11], iR=n[12], iK=n[13], imgoff=n[14], imgcount=n[15],
                stale=tuple(n[17:17 + n[16]]), ref=n[21])


def case_file_lines(cases=None, for_reference=False):
    """The lines of the case file.  for_reference: only what the reference's headers can run -- no
    semaphore cases (its waits are unbounded), no ll*_unit forms or 3-argument readOnce (it has none),
    and no copy with bytes below the head (its copyHelper underflows there and copies out of bounds)."""
    cases = CASES if cases is None else cases
    return [format_case(c) for c in cases if c.ref or not for_reference]


def write_case_file(path, cases=None, for_reference=False):
    lines = case_file_lines(cases, for_reference)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)


# ---- the arenas before and after -------------------------------------------------------------------
def initial_arenas(c):
    out = []
    for a, (size, init) in enumerate(((c.sL, c.iL), (c.sR, c.iR), (c.sK, c.iK))):
        if init == INIT_FILL:
            w = np.full(size // 4, FILL_WORD, np.uint32)
        elif init == INIT_PATTERN:
            w = pattern(c.idx, a, size // 4)
        else:
            # poison in every slot: the case's flag with payload 0xA5A5A5A5 (LL16 and LL8 alike:
            # even words data, odd words flag), then the image, then the stale flag words
            w = np.full(size // 4, FILL_WORD, np.uint32)
            w[1::2] = c.flag
            first = (GUARD + c.imgoff) // 4
            P = pattern(c.idx, PAYLOAD, c.imgcount * payload_per_packet(c.p0) // 4)
            w[first:first + 2 * len(P):2] = P
            for s in c.stale:
                w[first + s] = (c.flag - 1) & 0xFFFFFFFF
        out.append(w.view(np.uint8).copy())
    return out


def _words(arena, off, n):
    """A uint32 view of n words at byte offset `off` from the handle's base."""
    return arena[GUARD + off:GUARD + off + 4 * n].view(np.uint32)


def _packets_from(P, psize, flag):
    img = np.empty(2 * len(P), np.uint32)
    img[0::2] = P
    img[1::2] = flag
    return img


def rw_value_words(T, n):
    """The words write<T> stores for lanes 0..n-1 (the program's rw_value())."""
    t = np.arange(n, dtype=np.uint32)
    if T == 4:
        return 0xC0DE0000 + t
    lo, hi = (3 * t + 1, 0xFACE0000 + t) if T == 8 else (0xAB000000 + t, 0xCD000000 + t)
    w = np.empty(2 * n, np.uint32)
    w[0::2], w[1::2] = lo, hi
    return w


SEM_D2D_EXPECT = (0, 0, 1, 1, 0, 4, 4, 5, 5, 5)  # poll, expected | poll, expected, poll | in, exp | in, exp | relaxed in
SEM_H2D_EXPECT = (1, 0, 2, 2)  # poll, poll, expected, inbound (token preset to 2, after one wait())


def expected(c, bases=(0, 0, 0), swap_offsets=False, flip_remainder=False, ll16_round_up=False, clamp=True):
    """The three arenas after the case.  The keyword arguments are the wrong models that
    test_device_primitive_cases.py holds the table against."""
    L, R, K = initial_arenas(c)
    ar = [L, R, K]
    toff, ooff = (c.ooff, c.toff) if swap_offsets else (c.toff, c.ooff)
    op = c.op
    if op in COPY_OPS:
        dst, src = copy_roles(op)
        Rm = bool(c.p1) != flip_remainder
        *_, ranges = copy_ranges(bases[dst] + GUARD + toff, c.nbytes, c.p0, Rm, clamp=clamp)
        for a, b in ranges:
            ar[dst][GUARD + toff + a:GUARD + toff + b] = ar[src][GUARD + ooff + a:GUARD + ooff + b]
        return ar
    psize = c.p0
    per = payload_per_packet(psize) if op != "rw" else 0
    if op in ("putPackets2", "putPackets1", "copyToPackets"):
        npk = -(-c.nbytes // per) if ll16_round_up else c.nbytes // per
        P = _words(L, ooff, npk * per // 4)
        dst = K if op == "copyToPackets" else R
        _words(dst, toff, 2 * len(P))[:] = _packets_from(P, psize, c.flag)
    elif op in ("unpackPackets2", "unpackPackets1", "unpackPacket", "copyFromPackets", "pkt_read"):
        npk = -(-c.nbytes // per) if ll16_round_up else c.nbytes // per
        img = _words(K, toff, npk * psize // 4)
        _words(L, ooff, npk * per // 4)[:] = img[0::2]
    elif op == "put_unit":
        P = _words(L, ooff, c.nbytes // 16 * 4)
        _words(K, toff, 2 * len(P))[:] = _packets_from(P, psize, c.flag)
    elif op == "try_unit":
        units = c.nbytes // 16
        img = _words(K, toff, 8 * units).copy()
        _words(L, ooff, 4 * units)[:] = img[0::2]
        _words(R, 0, units)[:] = (img[1::2].reshape(units, 4) == c.flag).all(axis=1)
    elif op in ("pkt_ctor", "pkt_write3", "pkt_write64", "pkt_write2"):
        v = _words(L, ooff, 2)
        _words(K, toff, psize // 4)[:] = _packets_from(v[:per // 4], psize, c.flag)
    elif op == "pkt_clear":
        _words(K, toff, psize // 4)[:] = 0
    elif op in ("readOnce2", "readOnce3"):
        img = _words(K, toff, 4 * psize // 4).reshape(4, psize // 4)
        ok = (img[:, 1::2] == c.flag).all(axis=1)
        ret = ok if op == "readOnce3" else ~ok  # the reference's helper is true while NOT ready
        rec = np.concatenate([ret[:, None].astype(np.uint32), img[:, 0::2]], axis=1)
        _words(L, ooff, rec.size)[:] = rec.reshape(-1)
    elif op == "rw":
        T, n = c.p0, c.nbytes
        wpe = 1 if T == 4 else 2
        _words(R, 4 * wpe * toff, wpe * n)[:] = rw_value_words(T, n)
        _words(L, 0, wpe * n)[:] = _words(R, 4 * wpe * ooff, wpe * n)
    elif op in ("sem_d2d", "sem_base"):
        _words(L, 0, 2 * len(SEM_D2D_EXPECT))[:] = np.array(SEM_D2D_EXPECT, np.uint64).view(np.uint32)
    elif op == "sem_h2d":
        _words(L, 0, 2 * len(SEM_H2D_EXPECT))[:] = np.array(SEM_H2D_EXPECT, np.uint64).view(np.uint32)
    else:
        raise ValueError(op)
    return ar


def touched_extents(c):
    """[(arena, first byte, end byte)] relative to the arena's start: what the primitive may read or
    write (the image and the poison packets are the whole K arena by construction)."""
    per = payload_per_packet(c.p0) if c.op != "rw" else 0
    if c.op in COPY_OPS:
        n = c.nbytes
        return [(ARENA_L, GUARD + min(c.toff, c.ooff), GUARD + max(c.toff, c.ooff) + n),
                (ARENA_R, GUARD + min(c.toff, c.ooff), GUARD + max(c.toff, c.ooff) + n)]
    if c.op == "rw":
        return [(ARENA_R, GUARD, GUARD + 8 * (max(c.toff, c.ooff) + c.nbytes)), (ARENA_L, GUARD, GUARD + 8 * c.nbytes)]
    if c.op in SEM_OPS:
        return [(ARENA_L, GUARD, GUARD + 8 * len(SEM_D2D_EXPECT))]
    if c.op in UNIT_OPS:
        return [(ARENA_L, GUARD + c.ooff, GUARD + c.ooff + c.nbytes // 16 * 16),
                (ARENA_R, GUARD, GUARD + (c.nbytes // 16 * 4 if c.op == "try_unit" else 0)),
                (ARENA_K, GUARD + c.toff, GUARD + c.toff + c.nbytes // 16 * 32)]
    pk = ARENA_R if c.op in ("putPackets2", "putPackets1") else ARENA_K
    npk = max(c.imgcount, c.nbytes // per, 1)
    data = 48 if c.op in ("readOnce2", "readOnce3") else c.nbytes
    return [(ARENA_L, GUARD + c.ooff, GUARD + c.ooff + data),
            (pk, GUARD + min(c.toff, c.imgoff or c.toff), GUARD + max(c.toff, c.imgoff) + npk * c.p0)]


# ---- the program's output ----------------------------------------------------------------------------
def parse_output(blob):
    """-> (bases, {idx: (err[4], [L, R, K])}) from the program's output file."""
    head = np.frombuffer(blob, np.uint64, 8, 0)
    assert int(head[0]) == MAGIC, hex(int(head[0]))
    ncases, bases = int(head[1]), tuple(int(x) for x in head[2:5])
    assert int(head[5]) == GUARD
    pos, out = 64, {}
    for _ in range(ncases):
        rec = np.frombuffer(blob, np.uint32, 8, pos)
        pos += 32
        idx, sizes, err = int(rec[0]), [int(x) for x in rec[1:4]], [int(x) for x in rec[4:8]]
        arenas = []
        for s in sizes:
            arenas.append(np.frombuffer(blob, np.uint8, s, pos))
            pos += s
        out[idx] = (err, arenas)
    assert pos == len(blob), (pos, len(blob))
    return bases, out


def region_of(c, arena, byte, bases=(0, 0, 0)):
    """Where a differing byte of `arena` fell: head, body, tail of a copy, inside the case's extent,
    or guard (everything else)."""
    if c.op in COPY_OPS:
        dst, _ = copy_roles(c.op)
        if arena == dst:
            head, body, tail, _ = copy_ranges(bases[dst] + GUARD + c.toff, c.nbytes, c.p0, True)
            rel = byte - GUARD - c.toff
            if 0 <= rel < 4 * head:
                return "head"
            if 4 * head <= rel < 4 * head + c.p0 * body:
                return "body"
            if 0 <= rel - 4 * head - c.p0 * body < 4 * tail:
                return "tail"
        return "guard"
    for a, lo, hi in touched_extents(c):
        if a == arena and lo <= byte < hi:
            return "extent"
    return "guard"


def first_difference(c, got, want, bases=(0, 0, 0)):
    """None, or a message naming the first differing byte, its region and the case line."""
    for a, name in enumerate("LRK"):
        if got[a].shape != want[a].shape:
            return f"arena {name}: {got[a].size} bytes dumped, {want[a].size} expected; case: {format_case(c)}"
        d = np.flatnonzero(got[a] != want[a])
        if d.size:
            b = int(d[0])
            return (f"arena {name} byte {b} (base{b - GUARD:+d}) in {region_of(c, a, b, bases)}: got "
                    f"0x{int(got[a][b]):02x}, want 0x{int(want[a][b]):02x}; {d.size} bytes differ; case: {format_case(c)}")
    return None
