"""CPU checks of the native Send / Recv: the entry points exist at every layer, the in-process
launcher refuses null, zero and out-of-range arguments before it touches a device, and the group
calls nest."""
import ctypes
import subprocess


def test_sendrecv_symbols_and_methods_exist(built):
    import mscclpp_amd as m

    out = subprocess.run(["nm", "-D", "--defined-only", m.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"ncclSend", "ncclRecv", "ncclGroupStart", "ncclGroupEnd", "mscclppAmdSendRecvLaunch",
            "mscclppAmdSendRecvDefaultBlocks"} <= have
    L = m.lib()
    assert len(L.mscclppAmdSendRecvLaunch.argtypes) == 9
    assert len(L.ncclSend.argtypes) == 6 and len(L.ncclRecv.argtypes) == 6
    assert callable(m.InProcessRanks.send_recv)
    assert callable(m.Communicator.send) and callable(m.Communicator.recv) and callable(m.Communicator.group)
    assert ctypes.sizeof(m.SendRecvOp) == 32
    assert L.ncclSend(None, 1, 7, 0, None, None) == 4  # null communicator
    assert L.ncclRecv(None, 1, 7, 0, None, None) == 4


def test_default_blocks_depend_on_the_byte_count_alone(built):
    import mscclpp_amd as m

    nb = m.lib().mscclppAmdSendRecvDefaultBlocks
    assert nb(1) == 1 and nb(128 << 10) == 1 and nb((128 << 10) + 1) == 2 and nb((256 << 10) + 19) == 3
    got = [nb(1 << k) for k in range(0, 41)]
    assert got == sorted(got) and max(got) <= 128 and min(got) >= 1


def fake_views(n):
    import mscclpp_amd as m

    arr = (m.RankView * n)()
    for r in range(n):
        v = arr[r]
        v.tokens = v.expected = v.err = 1 << 20
        v.rank = r
        for q in range(n):
            v.peerTokens[q] = 1 << 20
    return arr


def ops_of(*ops):
    import mscclpp_amd as m

    return (m.SendRecvOp * len(ops))(*[m.SendRecvOp(*o) for o in ops])


def test_sendrecv_launch_rejects_bad_arguments_without_gpu(built):
    import mscclpp_amd as m

    L = m.lib()
    n, P = 3, 1 << 20
    arr = fake_views(n)
    good = ops_of((0, 1, P, P, 64), (2, 0, P, P, 4099))
    launch = L.mscclppAmdSendRecvLaunch
    assert launch(None, n, n, good, 2, 0, 0, 1000, None) == 4  # no views
    assert launch(arr, n, n, None, 2, 0, 0, 1000, None) == 4  # no table
    assert launch(arr, 0, n, good, 2, 0, 0, 1000, None) == 4  # no view to run
    assert launch(arr, 2, n, good, 2, 0, 0, 1000, None) == 4  # views: one, or one per rank
    assert launch(arr, 1, 1, good, 2, 0, 0, 1000, None) == 4  # one rank: nobody to send to
    assert launch(arr, 1, 9, good, 2, 0, 0, 1000, None) == 4  # more ranks than MAX_RANKS
    assert launch(arr, n, n, good, 0, 0, 0, 1000, None) == 4  # an empty table
    many = ops_of(*[(0, 1, P, P, 64)] * (m.SENDRECV_MAX_OPS + 1))
    assert launch(arr, n, n, many, m.SENDRECV_MAX_OPS + 1, 0, 0, 1000, None) == 4  # more than the table holds
    for field in ("tokens", "expected", "err"):
        bad = fake_views(n)
        setattr(bad[1], field, None)
        assert launch(bad, n, n, good, 2, 0, 0, 1000, None) == 4, field
    bad = fake_views(n)
    bad[0].peerTokens[2] = None
    assert launch(bad, n, n, good, 2, 0, 0, 1000, None) == 4
    bad = fake_views(n)
    bad[1].rank = n
    assert launch(bad, n, n, good, 2, 0, 0, 1000, None) == 4
    for op in ((1, 1, P, P, 64),  # to oneself
               (-1, 1, P, P, 64), (0, n, P, P, 64), (n, 0, P, P, 64), (0, -1, P, P, 64),  # ranks out of range
               (0, 1, None, P, 64), (0, 1, P, None, 64),  # null buffers
               (0, 1, P, P, 0)):  # nothing to move
        assert launch(arr, n, n, ops_of((2, 0, P, P, 16), op), 2, 0, 0, 1000, None) == 4, op
    # one view: its own operations are checked as above; the receiver needs both pointers, the sender none
    assert launch(arr, 1, n, ops_of((1, 0, None, P, 64)), 1, 0, 0, 1000, None) == 4
    assert launch(arr, 1, n, ops_of((1, 0, P, None, 64)), 1, 0, 0, 1000, None) == 4
    # launch shapes (checked before the device is asked anything)
    assert launch(arr, n, n, good, 2, 129, 0, 1000, None) == 4
    for nthreads in (32, 96, 576, 1024):
        assert launch(arr, n, n, good, 2, 4, nthreads, 1000, None) == 4, nthreads
    # a workgroup's sub-range must fit one buffer descriptor (4 GiB): ncclInvalidUsage
    huge = ops_of((0, 1, P, P, 64), (1, 2, P, P, 1 << 40))
    assert launch(arr, n, n, huge, 2, 8, 64, 1000, None) == 5
    assert launch(arr, n, n, huge, 2, 0, 64, 1000, None) == 5  # the default grid is too small for it as well


def test_group_calls_nest_and_return_success(built):
    import mscclpp_amd as m

    L = m.lib()
    assert L.ncclGroupEnd() == 0  # at depth 0: nothing to end
    assert L.ncclGroupStart() == 0 and L.ncclGroupStart() == 0
    assert L.ncclGroupEnd() == 0 and L.ncclGroupEnd() == 0
    assert L.ncclGroupEnd() == 0
    with m.Communicator.group():
        with m.Communicator.group():
            pass
    # a call refused inside a group is refused at once and leaves the group usable
    assert L.ncclGroupStart() == 0
    assert L.ncclSend(None, 1, 7, 0, None, None) == 4
    assert L.ncclGroupEnd() == 0
