"""ncclSend / ncclRecv by a zero-copy pull (kernels/sendrecv.hip), in-process ranks: one launch
(blockIdx.y = rank) runs a table of operations.  Every comparison is byte-exact against torch slicing
on the device.  Every rank owns a send arena of random bytes and a receive arena of 0xA5; the
operations' buffers are slices of them with at least 64 bytes between two destinations, so the bytes
on both sides of every destination, and the whole arenas of ranks the table does not name, must still
read 0xA5 afterwards; send arenas must be unchanged and every rank's error word zero."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
SIZES = (1, 15, 16, 17, 4099, (256 << 10) + 19)


class Arenas:
    """ops: (src, dst, nbytes, src_misalignment, dst_misalignment) in table order."""

    def __init__(self, n, ops, gen):
        self.n, self.spec = n, ops
        sat, rat = [0] * n, [GUARD] * n
        self.place = []
        for src, dst, nbytes, so, do in ops:
            self.place.append((sat[src] + so, rat[dst] + do))
            sat[src] += (nbytes + so + 15) // 16 * 16 + 16
            rat[dst] += (nbytes + do + 15) // 16 * 16 + GUARD
        self.sends = [torch.zeros(max(sat[r], 16), dtype=torch.uint8, device="cuda") for r in range(n)]
        self.recvs = [torch.empty(rat[r] + GUARD, dtype=torch.uint8, device="cuda") for r in range(n)]
        self.gen = gen
        self.refill()

    def refill(self):
        for s in self.sends:
            s.copy_(torch.randint(0, 256, s.shape, dtype=torch.uint8, device="cuda", generator=self.gen))
        for r in self.recvs:
            r.fill_(FILL)
        self.keep = [s.clone() for s in self.sends]
        self.want = [torch.full_like(r, FILL) for r in self.recvs]
        for (src, dst, nbytes, _, _), (sa, ra) in zip(self.spec, self.place):
            self.want[dst][ra:ra + nbytes] = self.keep[src][sa:sa + nbytes]

    def table(self):
        return [(src, dst, self.sends[src][sa:sa + nbytes], self.recvs[dst][ra:ra + nbytes])
                for (src, dst, nbytes, _, _), (sa, ra) in zip(self.spec, self.place)]

    def check(self, recvs=None):
        for r in range(self.n):
            got = self.recvs[r] if recvs is None else recvs[r]
            assert torch.equal(got, self.want[r]), (r, int((got != self.want[r]).sum()))
            assert torch.equal(self.sends[r], self.keep[r]), r


def exchange(ranks, n, ops, seed, **shape):
    a = Arenas(n, ops, torch.Generator(device="cuda").manual_seed(seed))
    ranks.send_recv(a.table(), **shape)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    a.check()


def default_blocks(nbytes):
    import mscclpp_amd as m

    return m.lib().mscclppAmdSendRecvDefaultBlocks(nbytes)


def pattern(name, n, size):
    """The table of a pattern at one size (bytes), with no misalignment."""
    if name == "single":
        return [(n - 1, 0, size, 0, 0)]
    if name == "both_directions":
        return [(0, n - 1, size, 0, 0), (n - 1, 0, size + 3, 0, 0)]
    if name == "ring":
        # rank r sends to r + 1 and receives from r - 1.  One table serves the whole launch, each
        # transfer once: rank 0 finds its send before its receive, the others their receive first
        # (no order of a ring's edges puts every rank's send first; the one-view launches of
        # tests/test_sendrecv_multiprocess_gpu.py do, each in its own table)
        return [(r, (r + 1) % n, size + r, 0, 0) for r in range(n)]
    if name == "same_direction_twice":  # the second transfer uses more channels than the first, or fewer
        other = (256 << 10) + 19 if size <= (256 << 10) else 3 * (256 << 10) + 5
        assert default_blocks(other) != default_blocks(size)
        return [(0, 1, size, 0, 0), (0, 1, other, 0, 0)] if size % 2 else [(0, 1, other, 0, 0), (0, 1, size, 0, 0)]
    if name == "fan_in":
        return [(p, 0, size + p, 0, 0) for p in range(1, n)]
    raise KeyError(name)


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("name", ["single", "both_directions", "ring", "same_direction_twice", "fan_in"])
def test_table_patterns_exact(built, n, name):
    """Default grids (from each operation's byte count), every size on one set of ranks: the token
    counters advance from launch to launch."""
    import mscclpp_amd as m

    ranks = m.InProcessRanks(n, 1 << 16)
    for size in SIZES:
        exchange(ranks, n, pattern(name, n, size), 1000 * n + size)


def test_ring_tables_may_list_each_ranks_send_first(built):
    """The table of a ring as the ranks would issue it, concatenated: every rank's send stands before
    its receive, so every receive stands after the send it matches only for some ranks."""
    import mscclpp_amd as m

    n = 3
    ranks = m.InProcessRanks(n, 1 << 16)
    ops = [(r, (r + 1) % n, 4099 + r, 0, 0) for r in range(n)]  # the sends; each is also r + 1's receive
    exchange(ranks, n, ops, 5)
    exchange(ranks, n, list(reversed(ops)), 6)


@pytest.mark.parametrize("nblocks", [1, 2, 3, 8])
@pytest.mark.parametrize("nthreads", [64, 512])
def test_explicit_grids_exact(built, nblocks, nthreads):
    """An explicit grid for every operation: a ragged last sub-range (4099 = 3 x 1376 - 29), and
    workgroups whose share is empty (1, 15, 16 and 17 bytes over 2, 3 or 8 workgroups)."""
    import mscclpp_amd as m

    n = 3
    ranks = m.InProcessRanks(n, 1 << 16)
    for size in SIZES:
        exchange(ranks, n, pattern("ring", n, size), size + nblocks, nblocks=nblocks, nthreads=nthreads)
        exchange(ranks, n, pattern("single", n, size), size + nthreads, nblocks=nblocks, nthreads=nthreads)


@pytest.mark.parametrize("size", [17, 4099, (256 << 10) + 19])
@pytest.mark.parametrize("nblocks", [0, 3])
def test_every_pairing_of_start_offsets(built, size, nblocks):
    """Source and destination starts 0 / 1 / 2 / 4 / 8 bytes past a 16-byte boundary, all 25 pairings
    as 25 transfers of one pair and direction in one table (they count up on the channels they share)."""
    import mscclpp_amd as m

    n = 2
    ranks = m.InProcessRanks(n, 1 << 16)
    offs = (0, 1, 2, 4, 8)
    exchange(ranks, n, [(1, 0, size, so, do) for so in offs for do in offs], size + nblocks, nblocks=nblocks)


def test_ranks_the_table_does_not_name_are_untouched(built):
    import mscclpp_amd as m

    n = 8
    ranks = m.InProcessRanks(n, 1 << 16)
    before = [(t.clone(), e.clone()) for t, e in zip((m.device_view(b.ptr, b.nbytes) for b in ranks.tokens), ranks.expected)]
    exchange(ranks, n, [(5, 2, 4099, 1, 2), (2, 5, 33, 0, 8)], 77)  # (Arenas.check covers all 8 ranks' arenas)
    for r in (0, 1, 3, 4, 6, 7):
        assert torch.equal(m.device_view(ranks.tokens[r].ptr, ranks.tokens[r].nbytes), before[r][0]), r
        assert torch.equal(ranks.expected[r], before[r][1]), r
    # each side of the pair: one token in and one expectation per operation and channel, no more
    for r, q in ((2, 5), (5, 2)):
        tok = m.device_view(ranks.tokens[r].ptr, ranks.tokens[r].nbytes).view(torch.int64).view(m.MAX_RANKS, m.MAX_CHANNELS)
        exp = ranks.expected[r].view(m.MAX_RANKS, m.MAX_CHANNELS)
        assert torch.equal(tok, exp) and int(tok.sum()) == 2 and int(tok[q].sum()) == 2, (r, q)
        assert int(tok[q][0]) == 1 and int(tok[q][m.MAX_CHANNELS // 2]) == 1  # one per direction's first channel


def test_three_launches_back_to_back_on_the_same_buffers(built):
    """No host synchronisation between the launches: each launch's result is copied aside on the
    stream and the send arenas are rewritten right behind it."""
    import mscclpp_amd as m

    n = 3
    ranks = m.InProcessRanks(n, 1 << 16)
    a = Arenas(n, pattern("ring", n, (256 << 10) + 19) + [(0, 2, 4099, 1, 4)], torch.Generator(device="cuda").manual_seed(3))
    tab, got, wants = a.table(), [], []
    for _ in range(3):
        ranks.send_recv(tab, nblocks=3)
        got.append([r.clone() for r in a.recvs])
        wants.append((a.want, a.keep))
        a.refill()  # new data into the same send buffers, 0xA5 over the receive buffers
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    for g, (want, _) in zip(got, wants):
        for r in range(n):
            assert torch.equal(g[r], want[r]), (r, int((g[r] != want[r]).sum()))


def test_a_message_of_many_workgroups(built):
    import mscclpp_amd as m

    size = (5 << 20) + 3
    assert default_blocks(size) > 8
    ranks = m.InProcessRanks(2, 1 << 16)
    exchange(ranks, 2, [(0, 1, size, 0, 0), (1, 0, size - 1, 8, 8)], 11)
