"""GPU parity of the collective kernels along the axes the earlier tests hold fixed (tables and CPU
expectations in kernel_edge_cases.py, checked on the CPU by test_kernel_edge_cases.py):

  A  launch shapes: lanes 64..512, grids from one workgroup (per peer) to the defaults, LL16 grids the
     launcher rounds down, the LL16 slice-size thresholds, refusals by return code;
  B  the bulk paths with a scratch so small that a slice takes 3..18 passes;
  C  MIN and uint32 at n = 3 and 8 with NaN / inf / +-0 / subnormal lanes;
  D  guard bands around the outputs, untouched inputs, and buffers that are element-aligned only;
  E  the 1-GPU self-reduce on a caller's grid (skew-1 and skew-2 forms at KiB sizes).

Every comparison is bit-exact against the CPU oracle (for f32, a lane whose expected value is a NaN
must hold a NaN); inputs are new for every call; after every call every rank's error word is 0 and
every flag slot holds the next flag (the bulk kernels use no flags: theirs stay untouched)."""
import numpy as np
import pytest
import torch

import kernel_edge_cases as K
import oracle_lib as O

pytestmark = pytest.mark.gpu

TORCH = {O.F16: torch.float16, O.BF16: torch.bfloat16, O.F32: torch.float32, O.I32: torch.int32, O.U32: torch.int32}


def _dev(arr, dt):
    t = torch.from_numpy(arr.view(np.int16 if arr.dtype == np.uint16 else np.int32).copy())
    return t.view(TORCH[dt]).cuda()


def _bytes(t):
    return t.cpu().contiguous().view(torch.uint8).numpy()


def _accum(dt):
    return O.U32 if dt == O.U32 else None  # uint32 runs over int32 tensors with the reduce-type code


def _cmp(got_bytes, exp_bytes, dt, what=""):
    if dt == O.F32 and got_bytes.size % 4 == 0:
        g, e = got_bytes.view(np.uint32), exp_bytes.view(np.uint32)
        nan = (e & 0x7FFFFFFF) > 0x7F800000
        bad = np.nonzero(g[~nan] != e[~nan])[0]
        assert bad.size == 0, f"{what}: {bad.size} word mismatches, first {bad[:8]}"
        assert np.all((g[nan] & 0x7FFFFFFF) > 0x7F800000), what
    else:
        bad = np.nonzero(got_bytes != exp_bytes)[0]
        assert bad.size == 0, f"{what}: {bad.size} byte mismatches, first {bad[:8]}"


def _check_state(ranks, want_flag):
    assert ranks.errors() == [0] * ranks.n, ranks.error_details()
    flags = torch.stack(ranks.flags).cpu().numpy()
    assert np.all(flags == want_flag), f"flag slots {np.unique(flags)} instead of {want_flag}"


def _ranks(m, algo, n, nbytes, dt, bulk_scratch=None):
    code = m.ALGO_NAMES[algo]
    if algo in K.LL_ALGOS:
        sb = max(m.scratch_required(code, n, nbytes, dt), 1 << 16)
        return m.InProcessRanks(n, sb), sb
    bulk = bulk_scratch or max(n * K.slice_bytes(n, nbytes), 1 << 20)  # one pass unless the test says otherwise
    return m.InProcessRanks(n, 1 << 16, bulk_scratch_bytes=bulk), 0


def _run_calls(m, algo, n, dt, count, nblocks, nthreads, op=O.SUM, edges=False, bulk_scratch=None, in_place_call=False):
    """Three calls (flags 1, 2, 3) with new inputs each; outputs, flag-1 scratch image (LL paths), error
    words and flag slots checked after every call; optionally a fourth call in place."""
    code = m.ALGO_NAMES[algo]
    nbytes = count * K.ITEM[dt]
    ranks, sb = _ranks(m, algo, n, nbytes, dt, bulk_scratch)
    ll = algo in K.LL_ALGOS
    for call in range(4 if in_place_call else 3):
        flag = call + 1
        ins = K.inputs(dt, n, count, seq=call, special=True, edges=edges)
        dins = [_dev(a, dt) for a in ins]
        douts = dins if call == 3 else [torch.zeros_like(d) for d in dins]
        ranks.all_reduce(dins, douts, code, op=op, nblocks=nblocks, nthreads=nthreads, accum=_accum(dt))
        torch.cuda.synchronize()
        _check_state(ranks, flag + 1 if ll else 1)
        exp, scr = K.expected(algo, dt, op, ins, count, flag, sb // 2)
        for r in range(n):
            _cmp(_bytes(douts[r]), exp[r], dt, f"call {call} rank {r}")
        if ll and call == 0:  # packet image of the flag-1 half: flag words and data words
            for r in range(n):
                got = ranks.scratch_tensor(r, sb).cpu().numpy()
                _cmp(got, scr[r].view(np.uint8), dt, f"scratch image of rank {r}")


# ---- A: launch shapes ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,dt,count,nblocks,nthreads", K.LL16_SHAPE_CASES,
                         ids=lambda v: str(v))
def test_ll16_launch_shapes(built, n, dt, count, nblocks, nthreads):
    import mscclpp_amd as m

    _run_calls(m, "packet", n, dt, count, nblocks, nthreads)


@pytest.mark.parametrize("n,count,units,nblocks,nthreads", K.LL16_THRESHOLD_CASES)
def test_ll16_slice_thresholds(built, n, count, units, nblocks, nthreads):
    """8191 / 8192 / 8193 packet units per slice: step 3 without and with its sentinel wait, step 2
    polling all peers at once and peer by peer."""
    import mscclpp_amd as m

    _run_calls(m, "packet", n, O.F16, count, nblocks, nthreads)


@pytest.mark.parametrize("n,nbytes", K.LL16_DEFAULT_CASES)
def test_ll16_default_shapes(built, n, nbytes):
    """The shape the product picks (ll16Defaults) on either side of its 32 KiB and 256 KiB switches."""
    import mscclpp_amd as m

    _run_calls(m, "packet", n, O.F16, nbytes // 2, 0, 0)


@pytest.mark.parametrize("n,count,nblocks,nthreads", K.LL8_SHAPE_CASES)
def test_ll8_launch_shapes(built, n, count, nblocks, nthreads):
    import mscclpp_amd as m

    _run_calls(m, "allpair", n, O.F16, count, nblocks, nthreads)


@pytest.mark.parametrize("algo", K.BULK_ALGOS)
@pytest.mark.parametrize("n,dt,count,nblocks,nthreads", K.BULK_SHAPE_CASES, ids=lambda v: str(v))
def test_bulk_launch_shapes(built, algo, n, dt, count, nblocks, nthreads):
    import mscclpp_amd as m

    _run_calls(m, algo, n, dt, count, nblocks, nthreads)


def test_refused_launch_shapes(built):
    """Lanes that are no multiple of 64 or above 512, and grids above the slot / channel limits, are
    ncclInvalidArgument before any launch: outputs, flags and error words stay as they were."""
    import mscclpp_amd as m

    n, count = 3, 1024
    for algo, nb, nt in K.REFUSED_SHAPES:
        ranks, _ = _ranks(m, algo, n, count * 2, O.F16)
        ins = [torch.ones(count, dtype=torch.float16, device="cuda") for _ in range(n)]
        outs = [torch.zeros_like(t) for t in ins]
        with pytest.raises(m.MscclppError) as e:
            ranks.all_reduce(ins, outs, m.ALGO_NAMES[algo], nblocks=nb, nthreads=nt)
        assert e.value.code == 4, (algo, nb, nt)
        torch.cuda.synchronize()
        _check_state(ranks, 1)
        assert all(not bool(o.any()) for o in outs), (algo, nb, nt)


# ---- B: multi-pass bulk --------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["fullmesh", "rsag"])
@pytest.mark.parametrize("n,dt,count,scratch,nblocks,nthreads", K.MULTIPASS_CASES, ids=lambda v: str(v))
def test_bulk_multipass(built, algo, n, dt, count, scratch, nblocks, nthreads):
    """A scratch of a third of the slices or less: pass rounding to 16 * nblocks bytes, a partial last
    pass, workgroups without a unit that still handshake, the scratch reused pass after pass; three
    calls out of place and one in place."""
    import mscclpp_amd as m

    _run_calls(m, algo, n, dt, count, nblocks, nthreads, bulk_scratch=scratch, in_place_call=True)


@pytest.mark.parametrize("algo", ["fullmesh", "rsag"])
def test_bulk_multipass_reduce_scatter_all_gather(built, algo):
    """ReduceScatter and AllGather of the first row (8 passes of 8 KiB per slice)."""
    import mscclpp_amd as m

    n, dt, _, scratch, nblocks, nthreads = K.MULTIPASS_CASES[0]
    count, item = K.MULTIPASS_RS_AG_COUNT, K.ITEM[dt]
    block = count // n
    code = m.ALGO_NAMES[algo]
    ranks = m.InProcessRanks(n, 1 << 16, bulk_scratch_bytes=scratch)
    for call in range(3):
        ins = K.inputs(dt, n, count, seq=call, special=True)
        dins = [_dev(a, dt) for a in ins]
        douts = [torch.zeros(block, dtype=TORCH[dt], device="cuda") for _ in range(n)]
        ranks.collective(1, dins, douts, algo=code, nblocks=nblocks, nthreads=nthreads)
        torch.cuda.synchronize()
        _check_state(ranks, 1)
        exp, _ = K.expected(algo, dt, O.SUM, ins, count)  # slice r in rank r's order, as the AllReduce
        for r in range(n):
            _cmp(_bytes(douts[r]), exp[0][r * block * item:(r + 1) * block * item], dt, f"reduce-scatter rank {r}")
        gathered = [torch.zeros(count, dtype=TORCH[dt], device="cuda") for _ in range(n)]
        ranks.collective(2, douts, gathered, algo=code, nblocks=nblocks, nthreads=nthreads)
        torch.cuda.synchronize()
        _check_state(ranks, 1)
        for r in range(n):
            _cmp(_bytes(gathered[r]), exp[0], dt, f"all-gather rank {r}")


def test_bulk_scratch_below_one_pass_is_refused(built):
    import mscclpp_amd as m

    n, dt, count, scratch, nblocks, nthreads = K.MULTIPASS_REFUSED
    for algo in ("fullmesh", "rsag"):
        ranks = m.InProcessRanks(n, 1 << 16, bulk_scratch_bytes=scratch)
        ins = [torch.ones(count, dtype=TORCH[dt], device="cuda") for _ in range(n)]
        outs = [torch.zeros_like(t) for t in ins]
        with pytest.raises(m.MscclppError) as e:
            ranks.all_reduce(ins, outs, m.ALGO_NAMES[algo], nblocks=nblocks, nthreads=nthreads)
        assert e.value.code == 5
        torch.cuda.synchronize()
        assert ranks.errors() == [0] * n and all(not bool(o.any()) for o in outs)


# ---- C: MIN and uint32 -----------------------------------------------------------------------------
@pytest.mark.parametrize("algo,dt,op,n", K.MIN_U32_CASES, ids=lambda v: str(v))
def test_min_and_u32(built, algo, dt, op, n):
    import mscclpp_amd as m

    nblocks, nthreads = K.MIN_U32_SHAPES[algo](n)
    _run_calls(m, algo, n, dt, K.min_u32_count(algo, dt), nblocks, nthreads, op=op, edges=K.is_float(dt))


# ---- D: guard bands and element-aligned views -------------------------------------------------------
@pytest.mark.parametrize("algo,n,dt,count,view", K.GUARD_CASES, ids=lambda v: str(v))
def test_guard_bands_and_views(built, algo, n, dt, count, view):
    """Input and output carved out of one 0xA5 arena per rank, 256 bytes past a 256-byte boundary (view:
    one element more, so element-aligned but not 16-byte aligned, as a slice of a tensor is).  After
    every call the outputs are bit-exact and every arena byte outside the output is as it was: guards
    and inputs.  The fourth call runs in place."""
    import mscclpp_amd as m

    code = m.ALGO_NAMES[algo]
    item = K.ITEM[dt]
    nbytes = count * item
    in_off, out_off, total = K.arena_layout(nbytes, item, view)
    ranks, sb = _ranks(m, algo, n, nbytes, dt)
    ll = algo in K.LL_ALGOS
    for call in range(4):
        in_place = call == 3
        ins = K.inputs(dt, n, count, seq=call, special=True)
        host = []
        for r in range(n):
            a = np.full(total, K.GUARD, np.uint8)
            a[(out_off if in_place else in_off):][:nbytes] = ins[r].view(np.uint8)
            host.append(a)
        arenas = [torch.from_numpy(a).cuda() for a in host]
        douts = [a[out_off:out_off + nbytes].view(TORCH[dt]) for a in arenas]
        dins = douts if in_place else [a[in_off:in_off + nbytes].view(TORCH[dt]) for a in arenas]
        assert all(t.data_ptr() % 16 == (item if view else 0) for t in dins + douts)
        ranks.all_reduce(dins, douts, code, nblocks=0, nthreads=0)
        torch.cuda.synchronize()
        _check_state(ranks, call + 2 if ll else 1)
        exp, _ = K.expected(algo, dt, O.SUM, ins, count, call + 1, sb // 2)
        for r in range(n):
            got = arenas[r].cpu().numpy()
            _cmp(got[out_off:out_off + nbytes], exp[r], dt, f"call {call} rank {r}")
            got[out_off:out_off + nbytes] = host[r][out_off:out_off + nbytes]
            bad = np.nonzero(got != host[r])[0]
            assert bad.size == 0, f"call {call} rank {r}: {bad.size} bytes outside the output changed, first {bad[:8]}"


# ---- E: the self-reduce on a caller's grid -------------------------------------------------------------
@pytest.mark.parametrize("dt,op", K.SELF_REDUCE_TYPES, ids=lambda v: str(v))
@pytest.mark.parametrize("nbytes,nblocks,waves,grid,rounds,skew", K.SELF_REDUCE_CASES)
def test_self_reduce_on_callers_grid(built, dt, op, nbytes, nblocks, waves, grid, rounds, skew):
    """mscclppAmdSelfReduceLL16 with nblocks > 0: output and packet image bit-exact, every flag slot
    bumped, and nothing written around the output or after the 2 * nbytes packet buffer."""
    import mscclpp_amd as m

    assert m.self_reduce_shape(nbytes, nblocks) == (waves, 1, grid, skew)
    pad = 256
    pk = m.DeviceBuffer(2 * nbytes + 2 * pad)  # the packet buffer sits inside a larger allocation
    pk_all = m.device_view(pk.ptr, 2 * nbytes + 2 * pad)
    pk_all.fill_(K.GUARD)
    flags = torch.ones(m.FLAG_SLOTS, dtype=torch.int32, device="cuda")
    err = torch.zeros(16, dtype=torch.int32, device="cuda")
    for flag in (1, 2, 3):
        x, y = K.self_reduce_inputs(dt, nbytes, flag)
        xd, yd = _dev(x, dt), _dev(y, dt)
        arena = torch.full((nbytes + 2 * pad,), K.GUARD, dtype=torch.uint8, device="cuda")
        out = arena[pad:pad + nbytes].view(TORCH[dt])
        m.self_reduce_ll16(xd, yd, pk.ptr + pad, out, flags, err, op=op, nblocks=nblocks, accum=_accum(dt))
        torch.cuda.synchronize()
        assert int(err[0].item()) == 0
        assert bool(torch.all(flags == flag + 1))
        exp_pk, exp_out = O.self_reduce(dt, op, x, y, flag)
        got = arena.cpu().numpy()
        _cmp(got[pad:pad + nbytes], exp_out.view(np.uint8), dt, f"flag {flag} output")
        assert np.all(got[:pad] == K.GUARD) and np.all(got[pad + nbytes:] == K.GUARD)
        got_pk = pk_all.cpu().numpy()
        assert np.array_equal(got_pk[pad:pad + 2 * nbytes].view(np.uint32), exp_pk)  # LL16 flag and data words
        assert np.all(got_pk[:pad] == K.GUARD) and np.all(got_pk[pad + 2 * nbytes:] == K.GUARD)
        assert np.array_equal(_bytes(xd), x.view(np.uint8)) and np.array_equal(_bytes(yd), y.view(np.uint8))
    pk.free()


def test_self_reduce_grid_above_limit_is_refused(built):
    import mscclpp_amd as m

    x = torch.zeros(4096, dtype=torch.float16, device="cuda")
    out = torch.zeros_like(x)
    pk = m.DeviceBuffer(2 * 8192)
    flags = torch.ones(m.FLAG_SLOTS, dtype=torch.int32, device="cuda")
    err = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(m.MscclppError) as e:
        m.self_reduce_ll16(x, x, pk.ptr, out, flags, err, nblocks=1025)
    assert e.value.code == 4
    torch.cuda.synchronize()
    assert bool(torch.all(flags == 1)) and not bool(out.any())
    pk.free()
