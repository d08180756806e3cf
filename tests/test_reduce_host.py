"""CPU checks of the native Reduce: the entry points exist at every layer, and the in-process
launcher refuses null, zero and out-of-range arguments before it touches a device."""
import subprocess


def test_reduce_symbols_and_methods_exist(built):
    import mscclpp_amd as m

    out = subprocess.run(["nm", "-D", "--defined-only", m.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"ncclReduce", "mscclppAmdReduceLaunch"} <= have
    L = m.lib()
    assert len(L.mscclppAmdReduceLaunch.argtypes) == 11 and len(L.ncclReduce.argtypes) == 8
    assert callable(m.InProcessRanks.reduce) and callable(m.Communicator.reduce)
    assert "reduce" in m.TRACE_PHASES
    assert L.ncclReduce(None, None, 1, 7, 0, 0, None, None) == 4  # null communicator: ncclInvalidArgument


def fake_views(n):
    import mscclpp_amd as m

    arr = (m.RankView * n)()
    for r in range(n):
        v = arr[r]
        v.input = v.output = v.tokens = v.expected = v.err = 1 << 20
        v.rank = r
        for q in range(n):
            v.peerInput[q] = v.peerTokens[q] = 1 << 20
    return arr


N, ROOT = 3, 1


def launch(arr, nviews=N, nranks=N, nbytes=64, dtype=2, op=0, root=ROOT, nblocks=0, nthreads=0):
    import mscclpp_amd as m

    return m.lib().mscclppAmdReduceLaunch(arr, nviews, nranks, nbytes, dtype, op, root, nblocks, nthreads, 1000, None)


def test_reduce_launch_rejects_bad_arguments_without_gpu(built):
    import mscclpp_amd as m

    arr = fake_views(N)
    assert launch(None) == 4  # no views
    assert launch(arr, nviews=0) == 4  # no view to run
    assert launch(arr, nviews=2) == 4  # views: one, or one per rank
    assert launch(arr, nviews=1, nranks=1, root=0) == 4  # one rank: nothing to reduce
    assert launch(arr, nviews=1, nranks=m.MAX_RANKS + 1) == 4
    for root in (-1, N):
        assert launch(arr, root=root) == 4, root
    assert launch(arr, nbytes=0) == 4
    # a byte count that splits an element: fp32, fp16; one byte of a 1-byte type is fine up to here
    assert launch(arr, nbytes=66, dtype=m.F32) == 4
    assert launch(arr, nbytes=63, dtype=m.F16) == 4
    for dtype in (-1, 15, 100):
        assert launch(arr, dtype=dtype) == 4, dtype
    for op in (-1, 2, 3):
        assert launch(arr, op=op) == 4, op
    for field in ("input", "tokens", "expected", "err"):
        for r in range(N):
            bad = fake_views(N)
            setattr(bad[r], field, None)
            assert launch(bad) == 4, (field, r)
    bad = fake_views(N)
    bad[0].peerTokens[2] = None
    assert launch(bad) == 4
    bad = fake_views(N)
    bad[ROOT].output = None  # the root's receive buffer
    assert launch(bad) == 4
    for q in range(N):
        bad = fake_views(N)
        bad[ROOT].peerInput[q] = None  # a send buffer the root reads
        assert launch(bad) == 4, q
    bad = fake_views(N)
    bad[2].rank = N
    assert launch(bad) == 4
    # launch shapes (checked before the device is asked anything)
    assert launch(arr, nblocks=m.MAX_CHANNELS + 1) == 4
    for nthreads in (32, 96, 576, 1024):
        assert launch(arr, nblocks=4, nthreads=nthreads) == 4, nthreads


def test_reduce_launch_over_the_descriptor_limit_is_invalid_usage(built):
    """A workgroup's range must fit one buffer descriptor (4 GiB): ncclInvalidUsage, checked after the
    arguments (a bad argument at that size is still 4) and before the device."""
    arr = fake_views(N)
    assert launch(arr, nbytes=1 << 40, nblocks=8, nthreads=64) == 5
    assert launch(arr, nbytes=1 << 40, nblocks=8, nthreads=64, root=N) == 4
    assert launch(arr, nbytes=1 << 40, nblocks=8, nthreads=64, dtype=15) == 4
