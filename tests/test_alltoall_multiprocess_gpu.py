"""ncclAllToAll / ncclAllToAllv through the NCCL ABI, one rank per process (placed by mp_util): the
send buffers are IPC-registered per allocation and pulled from; everything is byte-exact against
torch slicing, receive buffers carry 0xA5 guards, and every worker runs under the collect()
watchdog from its first call."""
import multiprocessing as mp
import os
import traceback

import mp_util
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
INVALID_ARGUMENT = 4


def _pattern(torch, rank, count, dtype, salt=0):
    """What `rank` sends: element i = a value every rank can recompute for any other rank."""
    x = (torch.arange(count, dtype=torch.int64, device="cuda") * 7 + 1000 * rank + salt) % 30011
    return x.to(dtype)


def _guarded(torch, nbytes):
    whole = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[:nbytes]


def _a2a_expect(torch, rank, n, per, dtype, salt=0):
    return torch.cat([_pattern(torch, p, n * per, dtype, salt)[rank * per:(rank + 1) * per] for p in range(n)])


def _v_counts(n):
    """cnt[p][r]: elements p sends to r; uneven, with zeros."""
    return [[0 if (p + 2 * r) % 4 == 1 else 13 + 1000 * p + 77 * r for r in range(n)] for p in range(n)]


def _v_exchange(torch, comm, rank, n, dtype, salt, send_buf=None):
    """One AllToAllv: send segments in rank order with a gap of 3 elements, receive segments in
    reverse rank order with a gap of 5.  Returns True when every byte is as expected.  The buffers
    are allocated at the largest rank's size on every rank (the used part differs), so every rank's
    allocator stays in the same state for the equal-sized collectives around this call."""
    cnt = _v_counts(n)
    es = torch.empty((), dtype=dtype).element_size()

    def sdispls(p):
        d, at = [], 2
        for r in range(n):
            d.append(at)
            at += cnt[p][r] + 3
        return d, at

    def rdispls(r):
        d, at = [0] * n, 1
        for p in reversed(range(n)):
            d[p] = at
            at += cnt[p][r] + 5
        return d, at

    sd, stot = sdispls(rank)
    smax = max(sdispls(p)[1] for p in range(n))
    if send_buf is None:
        send_buf = torch.empty(smax, dtype=dtype, device="cuda")
    send_buf[:smax].copy_(_pattern(torch, rank, smax, dtype, salt))
    send = send_buf[:stot]
    rd, at = rdispls(rank)
    whole, _ = _guarded(torch, max(rdispls(r)[1] for r in range(n)) * es)
    recv8 = whole[:at * es]
    want = torch.full_like(whole, FILL)
    for p in range(n):
        seg = _pattern(torch, p, smax, dtype, salt)[sdispls(p)[0][rank]:][:cnt[p][rank]]
        want[rd[p] * es:(rd[p] + cnt[p][rank]) * es] = seg.view(torch.uint8)
    keep = send_buf[:smax].clone()
    comm.all_to_all_v(send, cnt[rank], sd, recv8.view(dtype), [cnt[p][rank] for p in range(n)], rd)
    torch.cuda.synchronize()
    return bool(torch.equal(whole, want)) and bool(torch.equal(send_buf[:smax].view(torch.uint8), keep.view(torch.uint8)))


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


def _dropin_worker(rank, n, uid, q):
    try:
        torch, m, comm = _setup(rank, n, uid)
        res = {}
        per = 4099
        for name, dtype in (("f16", torch.float16), ("i64", torch.int64)):
            es = torch.empty((), dtype=dtype).element_size()
            send = _pattern(torch, rank, n * per, dtype)
            whole, recv8 = _guarded(torch, n * per * es)
            comm.all_to_all(send, recv8.view(dtype))
            torch.cuda.synchronize()
            want = torch.cat([_a2a_expect(torch, rank, n, per, dtype).view(torch.uint8),
                              torch.full((GUARD,), FILL, dtype=torch.uint8, device="cuda")])
            res[name] = bool(torch.equal(whole, want)) and bool(torch.equal(send, _pattern(torch, rank, n * per, dtype)))
            # again on the same buffers: the registration of the send buffer is cached
            before = comm.registration_exchanges()[:2]
            whole.fill_(FILL)
            comm.all_to_all(send, recv8.view(dtype))
            torch.cuda.synchronize()
            res[name + "_again"] = bool(torch.equal(whole, want))
            res[name + "_cached"] = comm.registration_exchanges()[:2] == before
        res["v_f16"] = _v_exchange(torch, comm, rank, n, torch.float16, 5)
        res["v_i64"] = _v_exchange(torch, comm, rank, n, torch.int64, 9)
        # which buffer goes with which changes between calls: rank 0 sends once from another buffer,
        # the others from the one the call before paired with rank 0's first; then rank 0 goes back
        held = torch.empty(1 << 19, dtype=torch.int32, device="cuda")
        other = m.DeviceBuffer(1 << 21, uncached=False)  # an allocation of its own, not a block of torch's
        fresh = m.device_view(other.ptr, 1 << 21).view(torch.int32)
        res["v_held"] = _v_exchange(torch, comm, rank, n, torch.int32, 11, send_buf=held)
        res["v_diverged"] = _v_exchange(torch, comm, rank, n, torch.int32, 12, send_buf=fresh if rank == 0 else held)
        res["v_back"] = _v_exchange(torch, comm, rank, n, torch.int32, 13, send_buf=held)
        # a sub-tensor at a non-zero offset of one allocation, sent twice
        per = 1000
        big = _pattern(torch, rank, 3 * n * per + 40, torch.float32)
        sub = big[24:24 + n * per]
        whole, recv8 = _guarded(torch, n * per * 4)
        comm.all_to_all(sub, recv8.view(torch.float32))
        allocs = comm.registration_exchanges()[0]
        comm.all_to_all(sub, recv8.view(torch.float32))
        torch.cuda.synchronize()
        want = torch.cat([_pattern(torch, p, 3 * n * per + 40, torch.float32)[24 + rank * per:24 + (rank + 1) * per]
                          for p in range(n)])
        res["sub"] = bool(torch.equal(whole[:n * per * 4].view(torch.float32), want)) and \
            bool((whole[n * per * 4:] == FILL).all()) and comm.registration_exchanges()[0] == allocs
        res["err"] = comm.device_error()
        comm.barrier()
        comm.destroy()
        del fresh
        other.free()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("n", [2, 3])
def test_dropin_alltoall_and_alltoallv(built, n):
    got = _spawn(_dropin_worker, n)
    for rank in range(n):
        res = got[rank]
        assert res.pop("err") == 0, (rank, got[rank])
        assert not [k for k, ok in res.items() if not ok], (rank, res)


def _stream_order_worker(rank, n, uid, q):
    try:
        torch, m, comm = _setup(rank, n, uid)
        res = []
        per = 1 << 18
        send = torch.empty(n * per, dtype=torch.float32, device="cuda")
        whole, recv8 = _guarded(torch, n * per * 4)
        recv = recv8.view(torch.float32)
        for it in range(3):
            # the send buffer is still being produced on this rank's stream when the collective is
            # queued behind it, and is overwritten by the next stream operation right after it: the
            # peers must read it after the producer and before the overwrite
            fresh = _pattern(torch, rank, n * per, torch.float32, it)
            whole.fill_(FILL)
            torch.cuda._sleep(20_000_000)
            send.copy_(fresh)
            comm.all_to_all(send, recv)
            send.fill_(-1.0)
            torch.cuda.synchronize()
            ok = bool(torch.equal(recv, _a2a_expect(torch, rank, n, per, torch.float32, it)))
            res.append(ok and bool((whole[n * per * 4:] == FILL).all()))
        res.append(comm.device_error())
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def test_alltoall_waits_for_the_peers_stream(built):
    """The entry handshake orders the pull after the peers' producers, the exit handshake the
    peers' next stream operation after the pull (tests/test_comm_multiprocess_gpu.py,
    test_collectives_wait_for_the_peers_stream)."""
    n = 2
    got = _spawn(_stream_order_worker, n)
    for rank in range(n):
        assert got[rank] == [True, True, True, 0], (rank, got[rank])


def _mixed_worker(rank, n, uid, q):
    try:
        torch, m, comm = _setup(rank, n, uid)
        res = []
        cnt = 1 << 20
        x = torch.full((cnt,), float(rank + 1), dtype=torch.float16, device="cuda")
        y = torch.empty_like(x)
        per = 4099
        send = _pattern(torch, rank, n * per, torch.int32)
        recv = torch.empty(n * per, dtype=torch.int32, device="cuda")
        b = _pattern(torch, rank, 12345, torch.float32)
        for it in range(2):
            y.fill_(-1.0)
            comm.all_reduce(x, y, algo="fullmesh")
            recv.fill_(-1)
            comm.all_to_all(send, recv)
            bc = torch.empty_like(b)
            comm.broadcast(b, bc, root=n - 1)
            okv = _v_exchange(torch, comm, rank, n, torch.int32, it)
            y2 = torch.empty_like(x)
            comm.all_reduce(x, y2, algo="fullmesh")
            torch.cuda.synchronize()
            total = n * (n + 1) / 2
            res.append(bool((y == total).all()) and bool((y2 == total).all()) and okv and
                       bool(torch.equal(recv, _a2a_expect(torch, rank, n, per, torch.int32))) and
                       bool(torch.equal(bc, _pattern(torch, n - 1, 12345, torch.float32))))
        res.append(comm.device_error())
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def test_mixed_sequence_keeps_token_channels_in_step(built):
    """all_reduce (fullmesh) -> all_to_all -> broadcast -> all_to_all_v -> all_reduce on one
    communicator: the collectives share the token channels."""
    n = 2
    got = _spawn(_mixed_worker, n)
    for rank in range(n):
        assert got[rank] == [True, True, 0], (rank, got[rank])


def _graph_worker(rank, n, uid, q):
    try:
        torch, m, comm = _setup(rank, n, uid)
        res = []
        per = 1 << 16
        send = _pattern(torch, rank, n * per, torch.float32)
        whole, recv8 = _guarded(torch, n * per * 4)
        recv = recv8.view(torch.float32)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            comm.all_to_all(send, recv, stream=s)  # eager once: registers the send buffer
        s.synchronize()
        res.append(bool(torch.equal(recv, _a2a_expect(torch, rank, n, per, torch.float32))))
        comm.barrier()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            comm.all_to_all(send, recv, stream=torch.cuda.current_stream())
        for it in (1, 2):
            send.copy_(_pattern(torch, rank, n * per, torch.float32, it))
            whole.fill_(FILL)
            torch.cuda.synchronize()
            comm.barrier()  # every rank's new data is in place before any replay reads it
            g.replay()
            torch.cuda.synchronize()
            res.append(bool(torch.equal(recv, _a2a_expect(torch, rank, n, per, torch.float32, it))) and
                       bool((whole[n * per * 4:] == FILL).all()))
            comm.barrier()
        res.append(comm.device_error())
        del g
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def test_alltoall_graph_capture_replays(built):
    n = 2
    got = _spawn(_graph_worker, n)
    for rank in range(n):
        assert got[rank] == [True, True, True, 0], (rank, got[rank])


def _errors_worker(rank, n, uid, q):
    try:
        import time

        torch, m, comm = _setup(rank, n, uid)
        res = {}
        send = _pattern(torch, rank, 64, torch.float32)
        recv = torch.zeros(64, dtype=torch.float32, device="cuda")
        # rank 0 says it sends 5 to rank 1; rank 1 expects 4
        sc = [3, 5] if rank == 0 else [2, 6]
        rc = [3, 2] if rank == 0 else [4, 6]
        t0 = time.time()
        try:
            comm.all_to_all_v(send, sc, [0, 8], recv, rc, [0, 8])
            res["mismatch"] = 0
        except m.MscclppError as e:
            res["mismatch"] = e.code
        res["prompt"] = time.time() - t0 < 5.0
        comm.barrier()
        rc = [3, 2] if rank == 0 else [5, 6]
        comm.all_to_all_v(send, sc, [0, 8], recv, rc, [0, 8])
        torch.cuda.synchronize()
        other = _pattern(torch, 1 - rank, 64, torch.float32)
        mine_from = {0: (send[0:3], other[0:2]), 1: (other[8:13], send[8:14])}[rank]
        res["valid_after"] = bool(torch.equal(recv[0:rc[0]], mine_from[0])) and \
            bool(torch.equal(recv[8:8 + rc[1]], mine_from[1]))
        try:
            comm.all_to_all(send, send)
            res["inplace"] = 0
        except m.MscclppError as e:
            res["inplace"] = e.code
        try:
            comm.all_to_all(send[:32], send[16:48])  # overlapping ranges of one allocation
            res["overlap"] = 0
        except m.MscclppError as e:
            res["overlap"] = e.code
        comm.barrier()
        res["err"] = comm.device_error()
        comm.destroy()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))


def test_argument_errors_agree_across_ranks(built):
    """A count mismatch in AllToAllv is ncclInvalidArgument on BOTH ranks, promptly and with no
    launch (neither rank is left waiting for the other); the next valid call works; in-place and
    overlapping AllToAll is refused."""
    n = 2
    got = _spawn(_errors_worker, n)
    for rank in range(n):
        assert got[rank] == {"mismatch": INVALID_ARGUMENT, "prompt": True, "valid_after": True,
                             "inplace": INVALID_ARGUMENT, "overlap": INVALID_ARGUMENT, "err": 0}, (rank, got[rank])
