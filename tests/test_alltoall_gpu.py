"""ncclAllToAll / ncclAllToAllv by a zero-copy pull (kernels/alltoall.hip), in-process ranks (one
launch, blockIdx.y = rank).  Every comparison is byte-exact against torch slicing on the device:
receive buffers start as 0xA5 and are 64 bytes longer than needed, so the guard and every gap
between receive segments must still read 0xA5 afterwards; send buffers must be unchanged and every
rank's error word zero."""
import ctypes
import random
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


def equal_split(n, blk):
    return [[(r * blk, p * blk, blk) for p in range(n)] for r in range(n)]


def exchange(ranks, n, segs, send_bytes, recv_bytes, gen, **shape):
    """One call with fresh random data; segs[r][p] = (src_off, dst_off, nbytes)."""
    sends = [torch.randint(0, 256, (send_bytes[r],), dtype=torch.uint8, device="cuda", generator=gen) for r in range(n)]
    whole = [torch.full((recv_bytes[r] + GUARD,), FILL, dtype=torch.uint8, device="cuda") for r in range(n)]
    keep = [s.clone() for s in sends]
    want = [torch.full_like(w, FILL) for w in whole]
    for r in range(n):
        for p in range(n):
            so, do, ln = segs[r][p]
            want[r][do:do + ln] = keep[p][so:so + ln]
    ranks.all_to_all(sends, [w[:recv_bytes[r]] for r, w in enumerate(whole)], segs, **shape)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    for r in range(n):
        assert torch.equal(whole[r], want[r]), (r, int((whole[r] != want[r]).sum()))
        assert torch.equal(sends[r], keep[r]), r


@pytest.mark.parametrize("n,blk", [(n, blk) for blk in (1, 15, 16, 4097, (1 << 20) + 3) for n in (2, 3, 8)] +
                         [(8, 6 << 20)])  # 48 MiB per rank once
def test_equal_split_exact(built, n, blk):
    """Odd blocks put every segment but the first on a misaligned start (the narrow path); three calls
    on one set of ranks advance the token counters."""
    import mscclpp_amd as m

    ranks = m.InProcessRanks(n, 1 << 16)
    gen = torch.Generator(device="cuda").manual_seed(blk * 8 + n)
    for _ in range(3):
        exchange(ranks, n, equal_split(n, blk), [n * blk] * n, [n * blk] * n, gen)


@pytest.mark.parametrize("blk", [4097, 1 << 20])
@pytest.mark.parametrize("nblocks", [1, 3, 0])
@pytest.mark.parametrize("nthreads", [64, 512])
def test_launch_shapes(built, blk, nblocks, nthreads):
    import mscclpp_amd as m

    n = 3
    ranks = m.InProcessRanks(n, 1 << 16)
    gen = torch.Generator(device="cuda").manual_seed(blk + 31 * nblocks + nthreads)
    exchange(ranks, n, equal_split(n, blk), [n * blk] * n, [n * blk] * n, gen, nblocks=nblocks, nthreads=nthreads)


def test_more_workgroups_than_units(built):
    """64 workgroups over segments of three 16-byte units: 61 workgroups own nothing, hand-shake all
    the same, and the call completes."""
    import mscclpp_amd as m

    n, blk = 3, 48
    ranks = m.InProcessRanks(n, 1 << 16)
    gen = torch.Generator(device="cuda").manual_seed(7)
    for _ in range(2):
        exchange(ranks, n, equal_split(n, blk), [n * blk] * n, [n * blk] * n, gen, nblocks=64, nthreads=64)


def v_table(n, es, seed, nblocks):
    """An AllToAllv exchange in bytes from a seeded counts matrix (elements of es bytes): zeros, a
    1-element segment, one larger than nblocks * 16 bytes, send segments in rank order with gaps,
    receive segments in a permuted order with gaps."""
    rng = random.Random(seed)
    cnt = [[rng.choice([0, 0, 1, 7, 33, 1000, 4099]) for _ in range(n)] for _ in range(n)]  # cnt[p][r]: p -> r
    cnt[0][1], cnt[1][0], cnt[2][1], cnt[1][1] = 0, 1, nblocks * 16 + 4099, 0
    sdis, send_bytes = [], []
    for p in range(n):
        at, row = rng.randrange(3), []
        for r in range(n):
            row.append(at)
            at += cnt[p][r] + rng.randrange(4)
        sdis.append(row)
        send_bytes.append(max(at, 1) * es)
    segs, recv_bytes = [], []
    for r in range(n):
        order = list(range(n))
        rng.shuffle(order)
        if order == sorted(order):
            order.reverse()
        at, rdis = rng.randrange(3), [0] * n
        for p in order:
            rdis[p] = at
            at += cnt[p][r] + 1 + rng.randrange(4)
        segs.append([(sdis[p][r] * es, rdis[p] * es, cnt[p][r] * es) for p in range(n)])
        recv_bytes.append(at * es)
    return segs, send_bytes, recv_bytes


@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_alltoallv_tables(built, n, es):
    import mscclpp_amd as m

    nblocks = 8
    segs, send_bytes, recv_bytes = v_table(n, es, 1000 * n + es, nblocks)
    lens = [s[2] for row in segs for s in row]
    assert 0 in lens and es in lens and max(lens) > nblocks * 16
    ranks = m.InProcessRanks(n, 1 << 16)
    gen = torch.Generator(device="cuda").manual_seed(n * 16 + es)
    exchange(ranks, n, segs, send_bytes, recv_bytes, gen, nblocks=nblocks)
    exchange(ranks, n, segs, send_bytes, recv_bytes, gen)  # the default shape


def test_offsets_past_4gib(built):
    """Blocks of 2 GiB + 16: rank 1's source offsets and every rank's second destination block lie
    past 2 GiB and run past 4 GiB."""
    import mscclpp_amd as m

    n, blk = 2, (2 << 30) + 16
    need = n * (2 * n * blk + GUARD) + 3 * n * blk  # the buffers, and the temporaries of the fill and the checks
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip("free device memory is short of %d GiB" % ((need >> 30) + 1))
    ranks = m.InProcessRanks(n, 1 << 16)
    sends = [(torch.arange(n * blk // 8, dtype=torch.int64, device="cuda") * (2 * r + 3)).view(torch.uint8)
             for r in range(n)]
    whole = [torch.full((n * blk + GUARD,), FILL, dtype=torch.uint8, device="cuda") for _ in range(n)]
    ranks.all_to_all(sends, [w[:n * blk] for w in whole])
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n, ranks.error_details()
    for r in range(n):
        for p in range(n):
            assert torch.equal(whole[r][p * blk:(p + 1) * blk], sends[p][r * blk:(r + 1) * blk]), (r, p)
        assert bool((whole[r][n * blk:] == FILL).all()), r
        fresh = (torch.arange(n * blk // 8, dtype=torch.int64, device="cuda") * (2 * r + 3)).view(torch.uint8)
        assert torch.equal(sends[r], fresh), r
        del fresh


def test_refusals_launch_nothing(built):
    import mscclpp_amd as m

    n, blk = 2, 4096
    ranks = m.InProcessRanks(n, 1 << 16)
    sends = [torch.zeros(n * blk, dtype=torch.uint8, device="cuda") for _ in range(n)]
    recvs = [torch.full((n * blk,), FILL, dtype=torch.uint8, device="cuda") for _ in range(n)]
    tokens = [m.device_view(t.ptr, t.nbytes).clone() for t in ranks.tokens]
    for shape in ({"nblocks": m.MAX_CHANNELS + 1}, {"nthreads": 32}, {"nthreads": 96}, {"nthreads": 1024}):
        with pytest.raises(m.MscclppError) as e:
            ranks.all_to_all(sends, recvs, **shape)
        assert e.value.code == 4, shape
    arr = ranks.views(sends, recvs)
    tab = (m.AllToAllSeg * (n * n))(*[m.AllToAllSeg(r * blk, p * blk, blk) for r in range(n) for p in range(n)])
    launch = m.lib().mscclppAmdAllToAllLaunch
    for nranks in (1, 9):
        assert launch(arr, 1, nranks, tab, 0, 0, 0, m.stream_ptr()) == 4, nranks
    assert launch(None, n, n, tab, 0, 0, 0, m.stream_ptr()) == 4
    assert launch(arr, n, n, None, 0, 0, 0, m.stream_ptr()) == 4
    for field in ("input", "output"):
        bad = ranks.views(sends, recvs)
        setattr(bad[1], field, None)
        assert launch(bad, n, n, tab, 0, 0, 0, m.stream_ptr()) == 4, field
    bad = ranks.views(sends, recvs)
    bad[0].peerInput[1] = None
    assert launch(bad, n, n, tab, 0, 0, 0, m.stream_ptr()) == 4
    torch.cuda.synchronize()
    for r in range(n):  # nothing ran: no byte received, no token moved
        assert bool((recvs[r] == FILL).all())
        assert torch.equal(m.device_view(ranks.tokens[r].ptr, ranks.tokens[r].nbytes), tokens[r])
    assert ranks.errors() == [0] * n


ERR_SEMAPHORE_TIMEOUT = 2
BUDGET_TICKS = 20_000_000  # 0.2 s at the 100 MHz s_memrealtime clock


def test_absent_peer_ends_in_error_word(built):
    """Rank 0 of a 2-rank AllToAll launched alone (tests/test_failure_detection_gpu.py): its entry
    handshake gives up after the budget, the kernel runs to its end and the error word names the
    channel and the peer."""
    import mscclpp_amd as m

    n, blk, nblocks = 2, 1 << 16, 2
    ranks = m.InProcessRanks(n, 1 << 16)
    sends = [torch.zeros(n * blk, dtype=torch.uint8, device="cuda") for _ in range(n)]
    recvs = [torch.zeros(n * blk, dtype=torch.uint8, device="cuda") for _ in range(n)]
    arr = ranks.views(sends, recvs)
    one = (m.RankView * 1)()
    one[0] = arr[0]
    tab = (m.AllToAllSeg * n)(*[m.AllToAllSeg(0, p * blk, blk) for p in range(n)])
    t0 = time.time()
    rc = m.lib().mscclppAmdAllToAllLaunch(one, 1, n, tab, nblocks, 256, BUDGET_TICKS, m.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    took = time.time() - t0
    err = ranks.error_details()[0]
    assert err[0] == ERR_SEMAPHORE_TIMEOUT, err
    # detail: channel | peer << 16, rank, tokens seen | wanted << 16
    assert err[1] >> 16 == 1 and (err[1] & 0xffff) < nblocks and err[2] == 0 and (err[3] >> 16) >= 1, err
    assert ranks.errors()[1] == 0
    assert took < 60, took
