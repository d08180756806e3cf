"""Cases, judges and the restated wire format of the small AllToAll / AllToAllv LL path
(kernels/alltoall_ll.hip).  Plain numpy slicing; nothing here touches a GPU.

A case is a matrix L[r][q] = bytes rank r sends rank q, laid out into `segs` with the meaning of
InProcessRanks.all_to_all: segs[r][p] = (src_off, dst_off, nbytes), rank r receives nbytes at dst_off of
its receive buffer from src_off of rank p's send buffer."""
import numpy as np

GUARD = 0xA5
RANKS = (2, 3, 4, 8)
# bytes per segment of the equal split: around one and two units, and one 256-lane workgroup's last unit +- 1
EQUAL_LENGTHS = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049)
# (bytes per segment, nblocks, nthreads): 200 units on 64 lanes (several strides, a partial last one, the
# last unit partial too), and one unit on four workgroups (three own nothing and still bump)
SHAPED = ((1597, 1, 64), (8, 4, 0))
SCRATCH_SIZES = (0, 1, 7, 8, 9, 2047, 2048, 2049, 1 << 20)


# ---- geometry, restated -------------------------------------------------------------------------
def wire_units(nbytes):
    return max(1, -(-nbytes // 8))


def geometry(n, max_seg):
    region = wire_units(max_seg) * 16
    half = (n * region + 255) // 256 * 256
    return {"units": wire_units(max_seg), "region": region, "half": half, "scratch": 2 * half}


def max_seg(L):
    return max(max(row) for row in L)


# ---- length matrices ----------------------------------------------------------------------------
def equal(n, nbytes):
    return [[nbytes] * n for _ in range(n)]


def v_tables(n):
    """name -> L.  Lengths straddle units (1..17), whole and partial, and differ in every row and column."""
    t = {}
    t["unequal"] = [[(5 * r + 3 * q) % 19 + 1 + (300 if (r + q) % n == 1 else 0) for q in range(n)] for r in range(n)]
    z = [[(7 * r + q) % 23 + 1 for q in range(n)] for r in range(n)]
    for r in range(n):
        z[r][(r + 1) % n] = 0  # zeros off the diagonal ...
    z[n - 1][n - 1] = 0  # ... and one empty self segment
    t["zeros"] = z
    zr = [[(3 * r + 5 * q) % 17 + 1 for q in range(n)] for r in range(n)]
    zr[0] = [0] * n  # rank 0 sends nothing
    t["zero_row"] = zr
    zc = [[(3 * r + 5 * q) % 17 + 1 for q in range(n)] for r in range(n)]
    for r in range(n):
        zc[r][n - 1] = 0  # rank n - 1 receives nothing
    t["zero_column"] = zc
    idle = [[(r + 2 * q) % 13 + 2 for q in range(n)] for r in range(n)]
    idle[1] = [0] * n
    for r in range(n):
        idle[r][1] = 0  # rank 1 sends and receives nothing, and still takes part
    t["idle_rank"] = idle
    return t


def layout(L, send_mis=None, recv_mis=None, permute=False, gap=0):
    """(segs, send_sizes, recv_sizes).  Send segments lie in peer order, receive segments in peer order or
    reversed (permute), `gap` guard bytes between neighbours; send_mis / recv_mis: functions (r, p) -> extra
    bytes in front of that segment, which set its start's misalignment."""
    n = len(L)
    send_off = [[0] * n for _ in range(n)]
    send_sizes, recv_sizes = [], []
    for r in range(n):
        at = 0
        for q in range(n):
            at += gap + (send_mis(r, q) if send_mis else 0)
            send_off[r][q] = at
            at += L[r][q]
        send_sizes.append(at + gap + 1)
    segs = [[None] * n for _ in range(n)]
    for r in range(n):
        at = 0
        for p in (reversed(range(n)) if permute else range(n)):
            at += gap + (recv_mis(r, p) if recv_mis else 0)
            segs[r][p] = (send_off[p][r], at, L[p][r])
            at += L[p][r]
        recv_sizes.append(at + gap + 1)
    return segs, send_sizes, recv_sizes


def misaligned(L):
    """Every start misalignment 0..7 on both sides, distinct on the two sides of a segment: the send start
    of r -> q is (r + q) % 8 past a multiple of 8, its receive start (r + q + 3) % 8."""
    n = len(L)
    pad = lambda at, want: (want - at) % 8  # noqa: E731
    send_at = [0] * n
    recv_at = [0] * n

    def send_mis(r, q):
        m = pad(send_at[r] + 3, (r + q) % 8)
        send_at[r] += 3 + m + L[r][q]
        return m

    def recv_mis(r, p):
        m = pad(recv_at[r] + 3, (r + p + 3) % 8)
        recv_at[r] += 3 + m + L[p][r]
        return m

    return layout(L, send_mis, recv_mis, gap=3)


def v_cases(n):
    """name -> (segs, send_sizes, recv_sizes): every AllToAllv table in a plain layout, and `unequal`
    permuted with gaps and with misaligned starts."""
    c = {name: layout(L, gap=2) for name, L in v_tables(n).items()}
    c["permuted_gaps"] = layout(v_tables(n)["unequal"], permute=True, gap=5)
    c["misaligned"] = misaligned(v_tables(n)["unequal"])
    return c


def lengths_of(segs):
    n = len(segs)
    return [[segs[q][r][2] for q in range(n)] for r in range(n)]


# ---- data and the judge -------------------------------------------------------------------------
def make_sends(segs, send_sizes, seed):
    """Random bytes (never the guard); the first byte of segment r -> q is r * 8 + q + 1, so even one-byte
    segments all differ."""
    n = len(segs)
    rng = np.random.default_rng(seed)
    sends = []
    for r in range(n):
        x = rng.integers(0, 255, send_sizes[r], dtype=np.uint8)
        x[x == GUARD] = 0x5A
        sends.append(x)
    for r in range(n):
        for p in range(n):
            off, _, ln = segs[r][p]
            if ln:
                sends[p][off] = p * 8 + r + 1
    return sends


def expected(segs, sends, recv_sizes):
    """The receive buffers after the call, started from GUARD everywhere."""
    n = len(segs)
    outs = [np.full(recv_sizes[r], GUARD, np.uint8) for r in range(n)]
    for r in range(n):
        for p in range(n):
            src, dst, ln = segs[r][p]
            outs[r][dst:dst + ln] = sends[p][src:src + ln]
    return outs


# ---- the packet image ---------------------------------------------------------------------------
def region_image(payload, flag):
    """The units of one segment: {w0, flag, w1, flag} per 8 payload bytes, the last one zero-filled, one
    arrival unit of zeros for an empty segment."""
    units = wire_units(len(payload))
    padded = np.zeros(units * 8, np.uint8)
    padded[:len(payload)] = payload
    img = np.empty((units, 4), np.uint32)
    w = padded.view(np.uint32).reshape(units, 2)
    img[:, 0], img[:, 2] = w[:, 0], w[:, 1]
    img[:, 1] = img[:, 3] = flag
    return img.reshape(-1).view(np.uint8)


def scratch_image(r, segs, sends, flag, scratch_bytes, arrival=True, stride=None):
    """Rank r's whole scratch after one call with `flag` on a GUARD-filled scratch.  arrival=False and
    `stride` model a kernel that drops the arrival unit or strides the regions wrongly."""
    n = len(segs)
    g = geometry(n, max_seg(lengths_of(segs)))
    stride = g["region"] if stride is None else stride
    img = np.full(scratch_bytes, GUARD, np.uint8)
    base = scratch_bytes // 2 if flag & 1 else 0
    for p in range(n):
        if p == r:
            continue
        src, _, ln = segs[r][p]
        if ln == 0 and not arrival:
            continue
        units = region_image(sends[p][src:src + ln], flag)
        at = base + p * stride
        img[at:at + len(units)] = units
    return img
