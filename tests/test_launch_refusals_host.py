"""One table of malformed calls over every in-process launch entry point (mscclppAmd*Launch): each
must be refused with the pinned code before a device is touched.  The views are fakes, as in
test_reduce_host.py; nothing here needs a GPU.

Rows that are left out, because the entry point does not check the field and would go on to ask
the device (whose answer without a GPU is a 5 that means something else):
  * tokens, expected and peerTokens[q] on the five LL algorithms, which hand-shake through packet
    flags and take `flags`, `scratch` and `peerScratch[q]` instead (checked here in their place);
  * a view rank equal to nranks on the pipelined AllReduce, ReduceScatter, AllGather and Broadcast,
    which do not range-check a view's rank.
That is 5 x 15 + 4 = 79 rows beside the 917 the table holds (test_table_size keeps it under one in
five).  The expected codes are what the library returned before its launch entry points shared one
validator and one launch path; the table pins them.
"""
import pytest

N = 3
PTR = 1 << 20
NBYTES = 96  # whole 16-byte units per rank at 3 ranks (what the in-place and bulk forms require)
F32, I32 = 2, 3
SUM, MAX = 0, 2
BUDGET = 1000


def fake_views(n=N):
    import mscclpp_amd as m

    arr = (m.RankView * n)()
    for r in range(n):
        v = arr[r]
        for f in ("input", "output", "scratch", "tokens", "expected", "flags", "err", "pipeSems"):
            setattr(v, f, PTR)
        v.scratchBytes = 1 << 30
        v.rank = r
        for q in range(n):
            v.peerScratch[q] = v.peerOutput[q] = v.peerTokens[q] = v.peerInput[q] = PTR
    return arr


class Entry:
    """An entry point with its well-formed arguments.  fields / peers: what it wants non-null on
    every view (peers: for every rank q); root_fields / root_peers: on the root's view only;
    peers_at_root: entry [root] of the array, on every view.  limit: the largest nblocks taken;
    above: the smallest nblocks refused.  big: a byte count whose share of one of 8 workgroups
    exceeds one buffer descriptor (None: the collective has no such check)."""

    def __init__(self, name, call, fields, peers, limit, rank_checked, big=None, root=None, root_fields=(),
                 root_peers=(), peers_at_root=(), above=None, dup_checked=False):
        self.name, self.call, self.fields, self.peers = name, call, fields, peers
        self.limit, self.rank_checked, self.big, self.root = limit, rank_checked, big, root
        self.root_fields, self.root_peers, self.peers_at_root = root_fields, root_peers, peers_at_root
        self.above = above if above is not None else limit + 1
        self.dup_checked = dup_checked


def allreduce(algo, dtype):
    def call(arr, nviews, nranks, nbytes, nblocks, nthreads):
        import mscclpp_amd as m

        return m.lib().mscclppAmdAllReduceLaunch(algo, arr, nviews, nranks, nbytes, dtype, SUM, nblocks, nthreads,
                                                 BUDGET, None)

    return call


def collective(coll):
    def call(arr, nviews, nranks, nbytes, nblocks, nthreads):
        import mscclpp_amd as m

        return m.lib().mscclppAmdCollectiveLaunch(coll, 3, arr, nviews, nranks, nbytes, F32, SUM, nblocks, nthreads,
                                                  BUDGET, None)

    return call


ROOT = 1


def broadcast(arr, nviews, nranks, nbytes, nblocks, nthreads):
    import mscclpp_amd as m

    return m.lib().mscclppAmdBroadcastLaunch(arr, nviews, nranks, nbytes, ROOT, nblocks, nthreads, BUDGET, None)


def alltoall(arr, nviews, nranks, nbytes, nblocks, nthreads):
    import mscclpp_amd as m

    segs = (m.AllToAllSeg * (m.MAX_RANKS * m.MAX_RANKS))()
    for i in range(len(segs)):
        segs[i].len = nbytes
    return m.lib().mscclppAmdAllToAllLaunch(arr, nviews, nranks, segs, nblocks, nthreads, BUDGET, None)


def reduce(arr, nviews, nranks, nbytes, nblocks, nthreads):
    import mscclpp_amd as m

    return m.lib().mscclppAmdReduceLaunch(arr, nviews, nranks, nbytes, F32, SUM, ROOT, nblocks, nthreads, BUDGET, None)


def sendrecv(arr, nviews, nranks, nbytes, nblocks, nthreads):
    import mscclpp_amd as m

    ops = (m.SendRecvOp * 1)()
    ops[0].src, ops[0].dst, ops[0].send, ops[0].recv, ops[0].bytes = 0, 1, PTR, PTR, nbytes
    return m.lib().mscclppAmdSendRecvLaunch(arr, nviews, nranks, ops, 1, nblocks, nthreads, BUDGET, None)


def pull_reduce(coll):
    def call(arr, nviews, nranks, nbytes, nblocks, nthreads):
        import mscclpp_amd as m

        return m.lib().mscclppAmdPullReduceLaunch(arr, nviews, nranks, coll, nbytes, F32, MAX, ROOT, nblocks, nthreads,
                                                  BUDGET, None)

    return call


CHANNELS, SLOTS = 256, 4096  # MSCCLPP_AMD_MAX_CHANNELS, MSCCLPP_AMD_FLAG_SLOTS
HANDSHAKE = ("tokens", "expected", "err")
LL = dict(fields=("input", "output", "flags", "err", "scratch"), peers=("peerScratch",), limit=SLOTS,
          rank_checked=True, dup_checked=True)
BIG = 1 << 40

ENTRIES = [
    # the LL buckets are bounded as a whole (one descriptor per buffer), not per workgroup
    Entry("allreduce-packet", allreduce(1, F32), big=BIG, **LL),
    Entry("allreduce-allpair", allreduce(2, F32), big=BIG, **LL),
    Entry("allreduce-test-k2", allreduce(102, I32), big=BIG, **LL),
    # k6 / k7 round nblocks down to a multiple of the peer count first: 4097 launches 4096
    Entry("allreduce-test-k6", allreduce(106, I32), big=BIG, above=SLOTS + 2, **LL),
    Entry("allreduce-test-k7", allreduce(107, I32), big=BIG, above=SLOTS + 2, **LL),
    Entry("allreduce-fullmesh", allreduce(3, F32), ("input", "output", "flags", "scratch") + HANDSHAKE,
          ("peerScratch", "peerOutput", "peerTokens"), CHANNELS, True, dup_checked=True),
    Entry("allreduce-rsag", allreduce(4, F32), ("input", "output", "flags", "scratch") + HANDSHAKE,
          ("peerScratch", "peerOutput", "peerTokens"), CHANNELS, True, dup_checked=True),
    Entry("allreduce-rsag-zc", allreduce(5, F32), ("input", "output", "flags") + HANDSHAKE,
          ("peerOutput", "peerTokens", "peerInput"), CHANNELS, True, big=BIG, dup_checked=True),
    # chunks of whole 16-byte units: 3 << 40 passes that check and meets the descriptor limit
    Entry("allreduce-test-k5", allreduce(105, I32), ("input", "output", "flags") + HANDSHAKE,
          ("peerOutput", "peerTokens"), CHANNELS, True, big=3 << 40, dup_checked=True),
    # the reduce workgroups: even, 2..128 (129 is refused as odd, 130 as too many)
    Entry("allreduce-rsag-pipeline", allreduce(6, F32), ("input", "output", "scratch", "pipeSems") + HANDSHAKE,
          ("peerScratch", "peerTokens"), 128, False, above=130),
    Entry("reduce-scatter", collective(1), ("input", "output", "scratch") + HANDSHAKE,
          ("peerScratch", "peerTokens", "peerOutput"), CHANNELS, False),
    Entry("all-gather", collective(2), ("input", "output", "scratch") + HANDSHAKE,
          ("peerScratch", "peerTokens", "peerOutput"), CHANNELS, False),
    Entry("broadcast", broadcast, ("output",) + HANDSHAKE, ("peerTokens",), CHANNELS, False, big=BIG, root=ROOT,
          root_fields=("input",), peers_at_root=("peerInput",)),
    Entry("alltoall", alltoall, ("input", "output") + HANDSHAKE, ("peerTokens", "peerInput"), CHANNELS, True, big=BIG),
    Entry("reduce", reduce, ("input",) + HANDSHAKE, ("peerTokens",), CHANNELS, True, big=BIG, root=ROOT,
          root_fields=("output",), root_peers=("peerInput",)),
    Entry("sendrecv", sendrecv, HANDSHAKE, ("peerTokens",), CHANNELS // 2, True, big=BIG),
    Entry("pull-reduce", pull_reduce(0), ("input",) + HANDSHAKE, ("peerTokens",), CHANNELS, True, big=BIG, root=ROOT,
          root_fields=("output",), root_peers=("peerInput",), dup_checked=True),
    Entry("pull-reduce-scatter", pull_reduce(1), ("input", "output") + HANDSHAKE, ("peerTokens", "peerInput"), CHANNELS,
          True, big=BIG, dup_checked=True),
    Entry("pull-allreduce", pull_reduce(2), ("input", "output") + HANDSHAKE, ("peerTokens", "peerInput", "peerOutput"),
          CHANNELS, True, big=BIG, dup_checked=True),
]


def rows(e):
    """(what, expected code, thunk) for every malformed call of entry point e."""
    import mscclpp_amd as m

    def row(what, code, views=None, nviews=N, nranks=N, nbytes=NBYTES, nblocks=4, nthreads=64, null=False):
        arr = None if null else (views if views is not None else fake_views())
        return (what, code, lambda: e.call(arr, nviews, nranks, nbytes, nblocks, nthreads))

    def broken(what, code, edit, **kw):
        views = fake_views()
        edit(views)
        return row(what, code, views=views, **kw)

    def null_field(r, f):
        return lambda views: setattr(views[r], f, None)

    def null_peer(r, f, q):
        return lambda views: getattr(views[r], f).__setitem__(q, None)

    out = [
        row("null views", 4, null=True),
        row("nviews 0", 4, nviews=0),
        row("nviews 2 of 3 ranks", 4, nviews=2),
        row("nranks 1", 4, nviews=1, nranks=1),
        row("nranks MAX_RANKS + 1", 4, nviews=1, nranks=m.MAX_RANKS + 1),
    ]
    for r in range(N):
        for f in e.fields + (e.root_fields if r == e.root else ()):
            out.append(broken(f"view {r}: null {f}", 4, null_field(r, f)))
        for f in e.peers + (e.root_peers if r == e.root else ()):
            for q in range(N):
                out.append(broken(f"view {r}: null {f}[{q}]", 4, null_peer(r, f, q)))
        for f in e.peers_at_root:
            out.append(broken(f"view {r}: null {f}[root]", 4, null_peer(r, f, e.root)))
    if e.rank_checked:
        out.append(broken("view 2: rank == nranks", 4, lambda views: setattr(views[2], "rank", N)))
    if e.dup_checked:
        out.append(broken("views 0 and 2: the same rank", 4, lambda views: setattr(views[2], "rank", 0)))
    out.append(row(f"nblocks {e.above}", 4, nblocks=e.above))
    if e.above != e.limit + 1:
        out.append(row(f"nblocks {e.above + 1}", 4, nblocks=e.above + 1))
    for nthreads in (32, 96, 576, 1024):
        out.append(row(f"nthreads {nthreads}", 4, nthreads=nthreads))
    if e.big:
        out.append(row("over the descriptor limit", 5, nbytes=e.big, nblocks=8))
        out.append(row("over the limit, nthreads 96", 4, nbytes=e.big, nblocks=8, nthreads=96))
        out.append(row(f"over the limit, nblocks {e.above}", 4, nbytes=e.big, nblocks=e.above))
        out.append(broken("over the limit, null err", 4, null_field(0, "err"), nbytes=e.big, nblocks=8))
        out.append(row("over the limit, nviews 2", 4, nbytes=e.big, nblocks=8, nviews=2))
    return out


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])
def test_malformed_launch_is_refused_before_the_device(built, entry):
    wrong = [(what, code, got) for what, code, got in ((w, c, t()) for w, c, t in rows(entry)) if got != code]
    assert not wrong, wrong


def test_table_size(built):
    """The rows left out (module docstring) stay under one in five."""
    total = sum(len(rows(e)) for e in ENTRIES)
    left_out = 5 * (N * 2 + N * N) + 4
    assert left_out * 5 <= total + left_out, (left_out, total)
