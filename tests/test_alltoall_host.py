"""CPU checks of the native AllToAll: the entry points exist at every layer, and the in-process
launcher refuses null, zero and out-of-range arguments before it touches a device."""
import ctypes
import subprocess


def test_alltoall_symbols_and_methods_exist(built):
    import mscclpp_amd as m

    out = subprocess.run(["nm", "-D", "--defined-only", m.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"ncclAllToAll", "ncclAllToAllv", "mscclppAmdAllToAllLaunch"} <= have
    L = m.lib()
    assert L.mscclppAmdAllToAllLaunch.argtypes is not None
    assert len(L.ncclAllToAll.argtypes) == 6 and len(L.ncclAllToAllv.argtypes) == 9
    assert callable(m.InProcessRanks.all_to_all)
    assert callable(m.Communicator.all_to_all) and callable(m.Communicator.all_to_all_v)
    assert ctypes.sizeof(m.AllToAllSeg) == 24
    assert L.ncclAllToAll(None, None, 1, 7, None, None) == 4  # null communicator
    assert L.ncclAllToAllv(None, None, None, None, None, None, 7, None, None) == 4


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


def test_alltoall_launch_rejects_bad_arguments_without_gpu(built):
    import mscclpp_amd as m

    L = m.lib()
    n = 2
    arr = fake_views(n)
    segs = (m.AllToAllSeg * (n * n))(*[m.AllToAllSeg(0, 0, 64) for _ in range(n * n)])
    launch = L.mscclppAmdAllToAllLaunch
    assert launch(None, n, n, segs, 0, 0, 1000, None) == 4  # no views
    assert launch(arr, n, n, None, 0, 0, 1000, None) == 4  # no segment table
    assert launch(arr, 0, n, segs, 0, 0, 1000, None) == 4  # no view to run
    assert launch(arr, 1, 1, segs, 0, 0, 1000, None) == 4  # one rank: nothing to exchange
    assert launch(arr, 1, 9, segs, 0, 0, 1000, None) == 4  # more ranks than MAX_RANKS
    assert launch(arr, 3, n, segs, 0, 0, 1000, None) == 4  # views: one, or one per rank
    for field in ("input", "output", "tokens", "expected", "err"):
        bad = fake_views(n)
        setattr(bad[1], field, None)
        assert launch(bad, n, n, segs, 0, 0, 1000, None) == 4, field
    for field in ("peerInput", "peerTokens"):
        bad = fake_views(n)
        getattr(bad[0], field)[1] = None
        assert launch(bad, n, n, segs, 0, 0, 1000, None) == 4, field
    bad = fake_views(n)
    bad[1].rank = n
    assert launch(bad, n, n, segs, 0, 0, 1000, None) == 4
    # launch shapes (checked before the device is asked anything)
    assert launch(arr, n, n, segs, m.MAX_CHANNELS + 1, 0, 1000, None) == 4
    for nthreads in (32, 96, 1024):
        assert launch(arr, n, n, segs, 4, nthreads, 1000, None) == 4, nthreads
    # a workgroup's share of a segment must fit one buffer descriptor (4 GiB): ncclInvalidUsage
    huge = (m.AllToAllSeg * (n * n))(*[m.AllToAllSeg(0, 0, 1 << 40) for _ in range(n * n)])
    assert launch(arr, n, n, huge, 8, 64, 1000, None) == 5
