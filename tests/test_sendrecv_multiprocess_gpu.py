"""ncclSend / ncclRecv and their groups through the NCCL ABI, one rank per process (placed by
mp_util): the sender posts an IPC export of its buffer through the bootstrap, the receiver imports it
and pulls.  Everything is byte-exact against what every rank can recompute for any other, receive
buffers carry 0xA5 guards on both sides, and every worker runs under the collect() watchdog from its
first call."""
import multiprocessing as mp
import os
import traceback

import mp_util
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
INTERNAL_ERROR, INVALID_ARGUMENT, INVALID_USAGE = 3, 4, 5


def _pattern(torch, rank, count, dtype, salt=0):
    """What `rank` sends: element i = a value every rank can recompute for any other rank."""
    x = (torch.arange(count, dtype=torch.int64, device="cuda") * 7 + 1000 * rank + salt) % 30011
    return x.to(dtype)


class _Guarded:
    """A receive buffer of `count` elements with GUARD bytes of 0xA5 on both sides."""

    def __init__(self, torch, count, dtype):
        self.torch = torch
        self.nbytes = count * torch.empty((), dtype=dtype).element_size()
        self.whole = torch.full((self.nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.buf = self.whole[GUARD:GUARD + self.nbytes].view(dtype)

    def reset(self):
        self.whole.fill_(FILL)

    def holds(self, want):
        t = self.torch
        return bool(t.equal(self.buf, want)) and bool((self.whole[:GUARD] == FILL).all()) and \
            bool((self.whole[GUARD + self.nbytes:] == FILL).all())


def _spawn(target, n, timeout=180, *extra):
    import mscclpp_amd as m

    uid = m.Communicator.unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, n, uid, q) + extra) for r in range(n)]
    for p in procs:
        p.start()
    return mp_util.collect(procs, q, n, timeout)


def _setup(rank, n, uid):
    os.environ.setdefault("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "10000")
    import torch

    import mscclpp_amd as m

    mp_util.place_rank(rank, n)
    return torch, m, m.Communicator(rank, n, uid)


def _pair_worker(rank, n, uid, q):
    try:
        torch, m, comm = _setup(rank, n, uid)
        res = {}
        peer = 1 - rank
        count = 4099
        # ungrouped: rank 0 sends then receives, rank 1 receives then sends (two kernels per rank)
        for name, dtype in (("f16", torch.float16), ("i64", torch.int64)):
            send = _pattern(torch, rank, count, dtype)
            recv = _Guarded(torch, count, dtype)
            if rank == 0:
                comm.send(send, peer)
                comm.recv(recv.buf, peer)
            else:
                comm.recv(recv.buf, peer)
                comm.send(send, peer)
            torch.cuda.synchronize()
            res[name] = recv.holds(_pattern(torch, peer, count, dtype)) and \
                bool(torch.equal(send, _pattern(torch, rank, count, dtype)))
        # grouped: both ranks list their send first; one kernel per rank
        big = (256 << 10) // 4 + 5  # three workgroups' worth, and no multiple of 16 bytes
        send = _pattern(torch, rank, big, torch.float32, 1)
        recv = _Guarded(torch, big, torch.float32)
        with comm.group():
            comm.send(send, peer)
            comm.recv(recv.buf, peer)
        torch.cuda.synchronize()
        res["grouped"] = recv.holds(_pattern(torch, peer, big, torch.float32, 1))
        # the same buffers again: the import of the peer's allocation is still open
        comm.barrier()
        before = m.ipc_stats()[0]
        recv.reset()
        send.copy_(_pattern(torch, rank, big, torch.float32, 2))
        with comm.group():
            comm.send(send, peer)
            comm.recv(recv.buf, peer)
        torch.cuda.synchronize()
        res["again"] = recv.holds(_pattern(torch, peer, big, torch.float32, 2))
        res["no_new_mapping"] = m.ipc_stats()[0] == before
        comm.barrier()
        # one rank groups two sends of different sizes (and channel counts), the peer receives them
        # with two ungrouped calls: the k-th send meets the k-th receive
        a, b = 17, 3 * (256 << 10) // 4 + 1
        if rank == 0:
            sa, sb = _pattern(torch, 0, a, torch.int32, 3), _pattern(torch, 0, b, torch.int32, 4)
            with comm.group():
                comm.send(sa, peer)
                comm.send(sb, peer)
            torch.cuda.synchronize()
            res["two_sends"] = bool(torch.equal(sa, _pattern(torch, 0, a, torch.int32, 3)))
        else:
            ra, rb = _Guarded(torch, a, torch.int32), _Guarded(torch, b, torch.int32)
            comm.recv(ra.buf, peer)
            comm.recv(rb.buf, peer)
            torch.cuda.synchronize()
            res["two_sends"] = ra.holds(_pattern(torch, 0, a, torch.int32, 3)) and \
                rb.holds(_pattern(torch, 0, b, torch.int32, 4))
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def test_send_recv_between_two_ranks(built):
    n = 2
    got = _spawn(_pair_worker, n)
    for rank in range(n):
        res = got[rank]
        assert res.pop("err") == 0, (rank, got[rank])
        assert not [k for k, ok in res.items() if not ok], (rank, res)


def _ring_worker(rank, n, uid, q):
    try:
        torch, m, comm = _setup(rank, n, uid)
        res = []
        nxt, prv = (rank + 1) % n, (rank - 1) % n
        for it, count in enumerate((1, 4099, (256 << 10) + 19)):
            send = _pattern(torch, rank, count, torch.uint8, it)
            recv = _Guarded(torch, count, torch.uint8)
            with comm.group():  # every rank lists its send first: ungrouped, this ring would deadlock
                comm.send(send, nxt)
                comm.recv(recv.buf, prv)
            torch.cuda.synchronize()
            res.append(recv.holds(_pattern(torch, prv, count, torch.uint8, it)))
        res.append(comm.device_error())
        comm.barrier()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def test_grouped_ring_of_three(built):
    n = 3
    got = _spawn(_ring_worker, n)
    for rank in range(n):
        assert got[rank] == [True, True, True, 0], (rank, got[rank])


def _stream_order_worker(rank, n, uid, q):
    try:
        torch, m, comm = _setup(rank, n, uid)
        res = []
        peer = 1 - rank
        count = 1 << 19
        send = torch.empty(count, dtype=torch.float32, device="cuda")
        recv = _Guarded(torch, count, torch.float32)
        for it in range(3):
            # the send buffer is still being produced on this rank's stream when the exchange is
            # queued behind it, and is overwritten by the next stream operation right after it: the
            # peer must read it after the producer and before the overwrite
            fresh = _pattern(torch, rank, count, torch.float32, it)
            recv.reset()
            torch.cuda._sleep(20_000_000)
            send.copy_(fresh)
            with comm.group():
                comm.send(send, peer)
                comm.recv(recv.buf, peer)
            send.fill_(-1.0)
            torch.cuda.synchronize()
            res.append(recv.holds(_pattern(torch, peer, count, torch.float32, it)))
        res.append(comm.device_error())
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def test_send_waits_for_the_producer_and_holds_off_the_overwrite(built):
    """"Ready" is posted by the sender's kernel, behind the producer on its stream; the sender's kernel
    ends only at the receiver's "done", so the overwrite behind it comes after the pull
    (tests/test_alltoall_multiprocess_gpu.py, test_alltoall_waits_for_the_peers_stream)."""
    n = 2
    got = _spawn(_stream_order_worker, n)
    for rank in range(n):
        assert got[rank] == [True, True, True, 0], (rank, got[rank])


def _mixed_worker(rank, n, uid, q):
    try:
        torch, m, comm = _setup(rank, n, uid)
        res = []
        peer = 1 - rank
        cnt = 1 << 20
        x = torch.full((cnt,), float(rank + 1), dtype=torch.float16, device="cuda")
        per = 4099
        a2a_send = _pattern(torch, rank, n * per, torch.int32)
        b = _pattern(torch, rank, 12345, torch.float32)
        p2p = (256 << 10) // 4 + 7
        for it in range(2):
            y = torch.full_like(x, -1.0)
            comm.all_reduce(x, y, algo="fullmesh")
            s1 = _pattern(torch, rank, p2p, torch.int32, 10 + it)
            r1 = _Guarded(torch, p2p, torch.int32)
            with comm.group():
                comm.send(s1, peer)
                comm.recv(r1.buf, peer)
            a2a_recv = torch.full((n * per,), -1, dtype=torch.int32, device="cuda")
            comm.all_to_all(a2a_send, a2a_recv)
            bc = torch.empty_like(b)
            comm.broadcast(b, bc, root=n - 1)
            s2 = _pattern(torch, rank, 33, torch.int32, 20 + it)
            r2 = _Guarded(torch, 33, torch.int32)
            if rank == 0:
                comm.send(s2, peer)
                comm.recv(r2.buf, peer)
            else:
                comm.recv(r2.buf, peer)
                comm.send(s2, peer)
            y2 = torch.empty_like(x)
            comm.all_reduce(x, y2, algo="fullmesh")
            torch.cuda.synchronize()
            total = n * (n + 1) / 2
            a2a_want = torch.cat([_pattern(torch, p, n * per, torch.int32)[rank * per:(rank + 1) * per] for p in range(n)])
            res.append(bool((y == total).all()) and bool((y2 == total).all()) and
                       r1.holds(_pattern(torch, peer, p2p, torch.int32, 10 + it)) and
                       r2.holds(_pattern(torch, peer, 33, torch.int32, 20 + it)) and
                       bool(torch.equal(a2a_recv, a2a_want)) and
                       bool(torch.equal(bc, _pattern(torch, n - 1, 12345, torch.float32))))
        res.append(comm.device_error())
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def test_mixed_sequence_keeps_token_channels_in_step(built):
    """all_reduce (fullmesh) -> grouped exchange -> all_to_all -> broadcast -> ungrouped exchange ->
    all_reduce on one communicator, twice: Send / Recv share the token channels with the collectives."""
    n = 2
    got = _spawn(_mixed_worker, n)
    for rank in range(n):
        assert got[rank] == [True, True, 0], (rank, got[rank])


KEPT_CAP = 64  # ncclComm::kP2pKept: imports of one peer's send allocations a receiver keeps open


def _kept_cap_worker(rank, n, uid, q):
    try:
        import time

        torch, m, comm = _setup(rank, n, uid)
        count, nbuf = 256, KEPT_CAP + 2
        res = {"wrong": [], "closed": []}
        if rank == 0:
            # one hipMalloc per send buffer (torch's allocator would carve them from one segment,
            # i.e. one import at the receiver)
            bufs = [m.DeviceBuffer(count * 4, uncached=False) for _ in range(nbuf)]
            sends = [m.device_view(b.ptr, count * 4).view(torch.float32) for b in bufs]
            for i, s in enumerate(sends):
                s.copy_(_pattern(torch, 0, count, torch.float32, i))
        recv = _Guarded(torch, count, torch.float32)

        def transfer(i):
            if rank == 0:
                comm.send(sends[i], 1)
            else:
                recv.reset()
                comm.recv(recv.buf, 0)
            torch.cuda.synchronize()
            if rank == 1 and not recv.holds(_pattern(torch, 0, count, torch.float32, i)):
                res["wrong"].append(i)

        def retired_close():
            deadline = time.perf_counter() + 1.0
            while True:
                awaiting = comm.registration_stats()[2]  # (each look closes what has completed)
                if awaiting == 0 or time.perf_counter() > deadline:
                    return awaiting == 0

        for i in range(nbuf):
            transfer(i)
            if i >= KEPT_CAP:  # the 65th and the 66th allocation each evicted the least recently used import
                res["closed"].append(retired_close())
        # buffers 0 and 1 were evicted; their mappings may still be closing when they are imported again
        for i in (0, 1):
            transfer(i)
        res["closed"].append(retired_close())
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        if rank == 0:
            del sends
            for b in bufs:
                b.free()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def test_recv_imports_beyond_the_kept_cap(built):
    """66 send allocations from one peer against the receiver's cap of 64 kept imports: every transfer
    is exact, the evicted imports close once their launches have completed (the retired-mapping count
    reaches 0), and the evicted buffers arrive exact when sent again."""
    n = 2
    got = _spawn(_kept_cap_worker, n)
    for rank in range(n):
        assert got[rank] == {"wrong": [], "closed": [True, True, True], "err": 0}, (rank, got[rank])


def _refusals_worker(rank, n, uid, q):
    try:
        import time

        torch, m, comm = _setup(rank, n, uid)
        res = {}
        peer = 1 - rank

        def code_of(call):
            try:
                call()
                return 0
            except m.MscclppError as e:
                return e.code

        dev = torch.zeros(64, dtype=torch.float32, device="cuda")
        # rank 0 sends from host memory, which cannot be exported: both ranks refuse, promptly
        t0 = time.time()
        if rank == 0:
            res["host_memory"] = code_of(lambda: comm.send(torch.zeros(64, dtype=torch.float32), peer))
        else:
            res["host_memory"] = code_of(lambda: comm.recv(dev, peer))
        res["prompt"] = time.time() - t0 < 5.0
        comm.barrier()
        recv = _Guarded(torch, 64, torch.float32)
        if rank == 0:
            comm.send(_pattern(torch, 0, 64, torch.float32), peer)
        else:
            comm.recv(recv.buf, peer)
        torch.cuda.synchronize()
        res["valid_after"] = rank == 0 or recv.holds(_pattern(torch, 0, 64, torch.float32))
        res["peer_out_of_range"] = [code_of(lambda: comm.send(dev, n)), code_of(lambda: comm.recv(dev, -1))]
        res["own_rank"] = [code_of(lambda: comm.send(dev, rank)), code_of(lambda: comm.recv(dev, rank))]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dev.mul_(1.0)
            cur = torch.cuda.current_stream()
            res["capture"] = [code_of(lambda: comm.send(dev, peer, stream=cur)),
                              code_of(lambda: comm.recv(dev, peer, stream=cur))]
        torch.cuda.synchronize()
        comm.barrier()
        res["err"] = comm.device_error()
        del g
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def test_refusals(built):
    """A sender whose buffer cannot be exported is ncclInvalidArgument on BOTH ranks, promptly and
    with no launch, and the next valid transfer works; a peer out of range is ncclInvalidArgument, the
    own rank ncclInternalError (not carried, no vendor library), a capturing stream ncclInvalidUsage."""
    n = 2
    got = _spawn(_refusals_worker, n)
    for rank in range(n):
        assert got[rank] == {"host_memory": INVALID_ARGUMENT, "prompt": True, "valid_after": True,
                             "peer_out_of_range": [INVALID_ARGUMENT] * 2, "own_rank": [INTERNAL_ERROR] * 2,
                             "capture": [INVALID_USAGE] * 2, "err": 0}, (rank, got[rank])
