"""The small AllToAll / AllToAllv LL kernel (kernels/alltoall_ll.hip) with n ranks of one collective in one
process on one GPU: outputs byte for byte against numpy slicing (alltoall_ll_cases), 0xA5 guards around
every receive buffer and between its segments, send buffers unchanged, and the packet image of the
scratch against the restated wire format."""
import numpy as np
import pytest
import torch

import alltoall_ll_cases as C

pytestmark = pytest.mark.gpu

SCRATCH = 1 << 17  # two halves of 8 regions of 4 KiB + the rounding: every case below fits


def _dev(a):
    return torch.from_numpy(a.copy()).cuda()


def _guarded(sizes):
    return [torch.full((s,), C.GUARD, dtype=torch.uint8, device="cuda") for s in sizes]


def _run(ranks, segs, ssz, rsz, seed, call="all_to_all_ll", **shape):
    """One call on fresh buffers; the outputs, guards, send buffers and error words are all judged."""
    n = ranks.n
    sends = C.make_sends(segs, ssz, seed)
    dsend, drecv = [_dev(x) for x in sends], _guarded(rsz)
    getattr(ranks, call)(dsend, drecv, segs=segs, **shape)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n
    want = C.expected(segs, sends, rsz)
    for r in range(n):
        got = drecv[r].cpu().numpy()
        bad = np.nonzero(got != want[r])[0]
        assert bad.size == 0, f"rank {r}: {bad.size} bytes differ, first at {bad[:8]}"
        assert np.array_equal(dsend[r].cpu().numpy(), sends[r]), f"send buffer of rank {r} changed"
    return sends, [d.cpu().numpy() for d in drecv]


@pytest.mark.parametrize("n", C.RANKS)
def test_equal_split_lengths(built, n):
    import mscclpp_amd as m

    ranks = m.InProcessRanks(n, SCRATCH)
    for k, nbytes in enumerate(C.EQUAL_LENGTHS):
        segs, ssz, rsz = C.layout(C.equal(n, nbytes), gap=1)
        _run(ranks, segs, ssz, rsz, 100 + k)
    for k, (nbytes, nblocks, nthreads) in enumerate(C.SHAPED):
        segs, ssz, rsz = C.layout(C.equal(n, nbytes), gap=1)
        _run(ranks, segs, ssz, rsz, 200 + k, nblocks=nblocks, nthreads=nthreads)


@pytest.mark.parametrize("n", C.RANKS)
def test_equal_split_default_table(built, n):
    """segs=None: block p of sends[q] lands as block q of recvs[p]."""
    import mscclpp_amd as m

    ranks = m.InProcessRanks(n, SCRATCH)
    blk = 24
    xs = [np.random.default_rng(7 + r).integers(0, 256, n * blk, dtype=np.uint8) for r in range(n)]
    dsend = [_dev(x) for x in xs]
    drecv = [torch.zeros(n * blk, dtype=torch.uint8, device="cuda") for _ in range(n)]
    ranks.all_to_all_ll(dsend, drecv)
    torch.cuda.synchronize()
    assert ranks.errors() == [0] * n
    for r in range(n):
        want = np.concatenate([xs[p][r * blk:(r + 1) * blk] for p in range(n)])
        assert np.array_equal(drecv[r].cpu().numpy(), want)


@pytest.mark.parametrize("n", C.RANKS)
def test_alltoallv_tables(built, n):
    import mscclpp_amd as m

    ranks = m.InProcessRanks(n, SCRATCH)
    for k, (name, (segs, ssz, rsz)) in enumerate(sorted(C.v_cases(n).items())):
        _run(ranks, segs, ssz, rsz, 300 + k)


@pytest.mark.parametrize("n", C.RANKS)
def test_large_small_large_on_stale_packets(built, n):
    """Call k + 2 lands on the half call k used: its stale packets (older flags, and units beyond the
    small call's regions) must never be taken for new ones."""
    import mscclpp_amd as m

    ranks = m.InProcessRanks(n, SCRATCH)
    for k, nbytes in enumerate((2049, 5, 2049, 3, 1597, 2049)):
        segs, ssz, rsz = C.layout(C.equal(n, nbytes), gap=1)
        _run(ranks, segs, ssz, rsz, 400 + k)
    segs, ssz, rsz = C.v_cases(n)["zeros"]
    for k in range(3):
        _run(ranks, segs, ssz, rsz, 410 + k)


@pytest.mark.parametrize("n", C.RANKS)
def test_alternates_with_the_other_ll_kernels(built, n):
    """all_to_all_ll, pull_reduce_ll and the LL8 SUM AllReduce share flags and scratch."""
    import mscclpp_amd as m

    ranks = m.InProcessRanks(n, SCRATCH)
    segs, ssz, rsz = C.v_cases(n)["unequal"]
    count = 333
    for k in range(3):
        _run(ranks, segs, ssz, rsz, 500 + k)
        xs = [np.random.default_rng(510 + 8 * k + r).integers(-1000, 1000, count).astype(np.int32) for r in range(n)]
        dx = [_dev(x) for x in xs]
        dy = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
        ranks.all_reduce(dx, dy, m.ALGO_ALLPAIR)
        dz = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
        ranks.pull_reduce_ll(m.PULL_ALLREDUCE, dx, dz, m.MAX)
        torch.cuda.synchronize()
        assert ranks.errors() == [0] * n
        for r in range(n):
            assert np.array_equal(dy[r].cpu().numpy(), np.sum(xs, axis=0, dtype=np.int32))
            assert np.array_equal(dz[r].cpu().numpy(), np.max(xs, axis=0))
    _run(ranks, segs, ssz, rsz, 520)


@pytest.mark.parametrize("n", C.RANKS)
@pytest.mark.parametrize("name", ["zeros", "misaligned"])
def test_packet_image(built, n, name):
    """One call on a 0xA5-prefilled scratch: the half of the call's parity holds exactly the modelled units
    (payload words, flag words, zero-filled tails, arrival units), every other byte is still 0xA5."""
    import mscclpp_amd as m

    segs, ssz, rsz = C.v_cases(n)[name]
    sb = C.geometry(n, C.max_seg(C.lengths_of(segs)))["scratch"] + 512
    assert m.alltoall_ll_scratch_required(n, C.max_seg(C.lengths_of(segs))) == sb - 512
    ranks = m.InProcessRanks(n, sb)
    for r in range(n):
        ranks.scratch_tensor(r, sb).fill_(C.GUARD)
    torch.cuda.synchronize()
    sends, _ = _run(ranks, segs, ssz, rsz, 600)
    for r in range(n):
        got = ranks.scratch_tensor(r, sb).cpu().numpy()
        want = C.scratch_image(r, segs, sends, 1, sb)  # the flags start at 1: the upper half
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"scratch of rank {r}: {bad.size} bytes differ, first at {bad[:8]}"
        assert (got[:sb // 2] == C.GUARD).all()  # the other half is untouched


@pytest.mark.parametrize("n", C.RANKS)
def test_pull_kernel_gives_the_same_bytes(built, n):
    import mscclpp_amd as m

    ranks = m.InProcessRanks(n, SCRATCH)
    cases = C.v_cases(n)
    cases["equal_2049"] = C.layout(C.equal(n, 2049), gap=1)
    for k, (name, (segs, ssz, rsz)) in enumerate(sorted(cases.items())):
        _, ll = _run(ranks, segs, ssz, rsz, 700 + k)
        _, pull = _run(ranks, segs, ssz, rsz, 700 + k, call="all_to_all")
        for r in range(n):
            assert np.array_equal(ll[r], pull[r]), (name, r)
