"""The tables of alltoall_ll_cases are not vacuous and its judges tell a right kernel from the wrong
ones they are meant to catch; the scratch requirement is the restated geometry; the host layer of the LL
AllToAll refuses what it must (mscclppAmdAllToAllLLLaunch with fake views: nothing touches a device); the
rule follows MSCCLPP_AMD_A2A_LL_MAX_BYTES."""
import os
import subprocess
import sys

import numpy as np
import pytest

import alltoall_ll_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the tables ---------------------------------------------------------------------------------
def test_equal_lengths_hold_every_shape_the_kernel_treats_differently():
    assert C.RANKS == (2, 3, 4, 8)
    assert {1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049} == set(C.EQUAL_LENGTHS)
    units = {b: C.wire_units(b) for b in C.EQUAL_LENGTHS}
    assert units[8] == 1 and units[9] == 2 and units[2048] == 256 and units[2049] == 257  # a second workgroup
    (b0, nb0, nt0), (b1, nb1, nt1) = C.SHAPED
    assert C.wire_units(b0) == 200 and b0 % 8 and 200 > 3 * nb0 * nt0 and 200 % (nb0 * nt0)
    assert C.wire_units(b1) == 1 and nb1 == 4
    assert C.wire_units(0) == 1  # the arrival unit


@pytest.mark.parametrize("n", C.RANKS)
def test_v_tables_are_what_their_names_say(n):
    t = C.v_tables(n)
    assert set(t) == {"unequal", "zeros", "zero_row", "zero_column", "idle_rank"}
    u = t["unequal"]
    assert len({x for row in u for x in row}) > 2 and all(x > 0 for row in u for x in row)
    assert u != [list(c) for c in zip(*u)] or n == 2  # not symmetric: send and receive lengths differ
    z = t["zeros"]
    assert all(z[r][(r + 1) % n] == 0 for r in range(n)) and z[n - 1][n - 1] == 0 and any(x for row in z for x in row)
    assert not any(t["zero_row"][0]) and all(any(row) for row in t["zero_row"][1:])
    assert not any(row[n - 1] for row in t["zero_column"]) and all(any(row[:n - 1]) for row in t["zero_column"])
    idle = t["idle_rank"]
    assert not any(idle[1]) and not any(row[1] for row in idle)
    if n > 2:
        assert all(idle[r][q] for r in range(n) for q in range(n) if r != 1 and q != 1)
    for L in t.values():
        assert 0 < C.max_seg(L) <= 4096


@pytest.mark.parametrize("n", C.RANKS)
def test_layouts(n):
    cases = C.v_cases(n)
    assert set(cases) == set(C.v_tables(n)) | {"permuted_gaps", "misaligned"}
    for name, (segs, ssz, rsz) in cases.items():
        L = C.lengths_of(segs)
        for r in range(n):
            # inside the buffers, receive segments disjoint with the gap between them
            spans = sorted((dst, dst + ln) for _, dst, ln in segs[r])
            assert spans[0][0] >= 2 and spans[-1][1] < rsz[r]
            assert all(a[1] + 2 <= b[0] for a, b in zip(spans, spans[1:])), (name, r)
            for p in range(n):
                src, _, ln = segs[r][p]
                assert ln == L[p][r] and src + ln < ssz[p]
    segs = cases["permuted_gaps"][0]
    assert all(segs[r][0][1] > segs[r][n - 1][1] for r in range(n))  # the receive order is reversed
    segs = C.misaligned(C.v_tables(8)["unequal"])[0]
    send_mis = {segs[r][p][0] % 8 for r in range(8) for p in range(8)}
    recv_mis = {segs[r][p][1] % 8 for r in range(8) for p in range(8)}
    assert send_mis == recv_mis == set(range(8))
    assert all(segs[r][p][0] % 8 != segs[r][p][1] % 8 for r in range(8) for p in range(8))


@pytest.mark.parametrize("n", C.RANKS)
def test_every_segment_differs_and_the_judge_is_not_vacuous(n):
    for name, (segs, ssz, rsz) in list(C.v_cases(n).items()) + [("equal1", C.layout(C.equal(n, 1)))]:
        sends = C.make_sends(segs, ssz, 5)
        assert all((x != C.GUARD).all() for x in sends)
        pieces = [sends[p][s:s + ln].tobytes() for r in range(n) for p in range(n) for s, _, ln in [segs[r][p]] if ln]
        assert len(pieces) == len(set(pieces)), name
        want = C.expected(segs, sends, rsz)
        for r in range(n):
            covered = sum(ln for _, _, ln in segs[r])
            assert int((want[r] != C.GUARD).sum()) == covered < rsz[r]  # guards everywhere else
        # a kernel that reads a segment one byte off its start is told apart
        for r in range(n):
            for p in range(n):
                src, dst, ln = segs[r][p]
                if ln:
                    shifted = [list(row) for row in segs]
                    shifted[r][p] = (src + 1, dst, ln)
                    assert not np.array_equal(C.expected(shifted, sends, rsz)[r], want[r]), (name, r, p)


def test_region_image():
    img = C.region_image(np.arange(1, 13, dtype=np.uint8), 7).view(np.uint32)
    assert img.tolist() == [0x04030201, 7, 0x08070605, 7, 0x0c0b0a09, 7, 0, 7]  # whole units, zero-filled tail
    img = C.region_image(np.arange(1, 6, dtype=np.uint8), 9).view(np.uint32)
    assert img.tolist() == [0x04030201, 9, 0x00000005, 9]
    img = C.region_image(np.zeros(0, np.uint8), 3).view(np.uint32)
    assert img.tolist() == [0, 3, 0, 3]  # the arrival unit of an empty segment


@pytest.mark.parametrize("n", (3, 8))
def test_scratch_image_tells_the_wrong_kernels_apart(n):
    segs, ssz, rsz = C.v_cases(n)["zeros"]
    sends = C.make_sends(segs, ssz, 6)
    g = C.geometry(n, C.max_seg(C.lengths_of(segs)))
    sb = g["scratch"] + 512
    for r in range(n):
        img = C.scratch_image(r, segs, sends, 1, sb)
        assert (img[:sb // 2] == C.GUARD).all() and (img[sb // 2:] != C.GUARD).any()  # flag 1: the upper half
        assert (img[sb // 2 + r * g["region"]:sb // 2 + (r + 1) * g["region"]] == C.GUARD).all()  # no self packets
        assert not np.array_equal(img, C.scratch_image(r, segs, sends, 1, sb, arrival=False))
        assert not np.array_equal(img, C.scratch_image(r, segs, sends, 1, sb, stride=g["region"] + 16))
        assert not np.array_equal(img, C.scratch_image(r, segs, sends, 3, sb))
        even = C.scratch_image(r, segs, sends, 2, sb)
        assert (even[sb // 2:] == C.GUARD).all() and (even[:sb // 2] != C.GUARD).any()


# ---- the host layer --------------------------------------------------------------------------------
def test_symbols_and_methods_exist(built):
    import mscclpp_amd as m

    out = subprocess.run(["nm", "-D", "--defined-only", m.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"mscclppAmdAllToAllLLLaunch", "mscclppAmdAllToAllLLScratchRequired", "mscclppAmdAllToAllTakesLL",
            "mscclppAmdCommAllToAllLLCount"} <= have
    assert len(m.lib().mscclppAmdAllToAllLLLaunch.argtypes) == 8
    assert callable(m.InProcessRanks.all_to_all_ll) and callable(m.Communicator.a2a_ll_count)
    assert callable(m.alltoall_takes_ll) and callable(m.alltoall_ll_scratch_required)


def test_scratch_requirement_is_the_restated_geometry(built):
    import mscclpp_amd as m

    for n in range(2, 9):
        for b in C.SCRATCH_SIZES:
            assert m.alltoall_ll_scratch_required(n, b) == C.geometry(n, b)["scratch"], (n, b)
    assert C.geometry(2, 0)["scratch"] == 512 and C.geometry(8, 1 << 20)["scratch"] == 2 * 8 * (2 << 20)
    assert m.alltoall_ll_scratch_required(1, 64) == 0 and m.alltoall_ll_scratch_required(9, 64) == 0
    assert m.alltoall_ll_scratch_required(8, 1 << 32) == 0  # a half beyond one descriptor


N = 3
SCRATCH = 1 << 16


def fake_views(n, scratch_bytes=SCRATCH):
    import mscclpp_amd as m

    arr = (m.RankView * n)()
    for r in range(n):
        v = arr[r]
        v.input = v.output = v.scratch = v.flags = v.err = 1 << 20
        v.scratchBytes = scratch_bytes
        v.rank = r
        for q in range(n):
            v.peerScratch[q] = 1 << 20
    return arr


def table(L, nviews=None):
    """The LL table of the views of ranks 0 .. nviews - 1 for the length matrix L (offsets packed)."""
    import mscclpp_amd as m

    n = len(L)
    nviews = n if nviews is None else nviews
    tab = (m.AllToAllLLSeg * (nviews * n))()
    for r in range(nviews):
        for q in range(n):
            tab[r * n + q] = m.AllToAllLLSeg(sum(L[r][:q]), L[r][q], sum(L[p][r] for p in range(q)), L[q][r])
    return tab


def launch(arr, tab, nviews=N, nranks=N, nblocks=0, nthreads=0):
    import mscclpp_amd as m

    return m.lib().mscclppAmdAllToAllLLLaunch(arr, nviews, nranks, tab, nblocks, nthreads, 1000, None)


def test_launch_rejects_bad_arguments_without_gpu(built):
    import mscclpp_amd as m

    arr, tab = fake_views(N), table(C.equal(N, 64))
    assert launch(None, tab) == 4
    assert launch(arr, None) == 4
    assert launch(arr, tab, nviews=0) == 4
    assert launch(arr, tab, nviews=N + 1) == 4
    assert launch(arr, tab, nviews=1, nranks=1) == 4
    assert launch(arr, tab, nviews=1, nranks=m.MAX_RANKS + 1) == 4
    for field in ("input", "output", "scratch", "flags", "err"):
        for r in range(N):
            bad = fake_views(N)
            setattr(bad[r], field, None)
            assert launch(bad, tab) == 4, (field, r)
    bad = fake_views(N)
    bad[0].peerScratch[2] = None
    assert launch(bad, tab) == 4
    bad = fake_views(N)
    bad[1].flags = (1 << 20) + 4  # the flag refresh stores 16 bytes at a time
    assert launch(bad, tab) == 4
    bad = fake_views(N)
    bad[2].rank = N
    assert launch(bad, tab) == 4
    bad = fake_views(N)
    bad[2].rank = 0  # a rank twice
    assert launch(bad, tab) == 4
    # what one view sends, the receiving view expects -- also of itself
    for r, q in ((0, 1), (2, 0), (1, 1)):
        wrong = table(C.equal(N, 64))
        wrong[r * N + q].sendLen = 65
        assert launch(arr, wrong) == 4, (r, q)
        wrong = table(C.equal(N, 64))
        wrong[r * N + q].recvLen = 0
        assert launch(arr, wrong) == 4, (r, q)
    assert launch(arr, tab, nblocks=m.FLAG_SLOTS + 1) == 4
    for nthreads in (32, 96, 576, 1024):
        assert launch(arr, tab, nblocks=4, nthreads=nthreads) == 4, nthreads


def test_launch_with_too_little_scratch_is_invalid_usage(built):
    """Checked after the arguments (a bad argument is still 4) and before the device."""
    import mscclpp_amd as m

    L = C.equal(N, 100)
    L[2][0] = 4096  # one large segment sets every region
    need = m.alltoall_ll_scratch_required(N, 4096)
    assert need == C.geometry(N, 4096)["scratch"] > 0
    assert launch(fake_views(N, need - 256), table(L)) == 5
    assert launch(fake_views(N, 0), table(L)) == 5
    uneven = fake_views(N, need)
    uneven[1].scratchBytes = need + 256
    assert launch(uneven, table(L)) == 5
    wrong = table(L)
    wrong[1].recvLen += 1
    assert launch(fake_views(N, need - 256), wrong) == 4
    assert launch(fake_views(N, need - 256), table(L), nblocks=4, nthreads=96) == 4
    assert launch(fake_views(N, 1 << 30), table(C.equal(N, 1 << 32))) == 5  # a size the path does not carry


# ---- the rule --------------------------------------------------------------------------------------
VAR = "MSCCLPP_AMD_A2A_LL_MAX_BYTES"


def takes_in_a_process(value, queries):
    """mscclppAmdAllToAllTakesLL in a process of its own with the variable set to `value`, or unset for
    None (the library reads it once)."""
    code = f"import mscclpp_amd as m; print([int(m.alltoall_takes_ll(n, b)) for n, b in {queries!r}])"
    env = {k: v for k, v in os.environ.items() if k != VAR}
    if value is not None:
        env[VAR] = value
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True, check=True)
    return [int(x) for x in out.stdout.strip().splitlines()[-1].strip("[]").split(",")]


def test_builtin_rule_is_monotone_and_bounded(built):
    sizes = [1 << k for k in range(3, 21)]
    q = [(n, b) for n in range(1, 10) for b in [0] + sizes + [(1 << 20) + 1, 1 << 21]]
    got = dict(zip(q, takes_in_a_process(None, q)))
    for n in range(1, 10):
        assert not got[(n, 0)] and not got[(n, (1 << 20) + 1)] and not got[(n, 1 << 21)]
        row = [got[(n, b)] for b in sizes]
        assert row == sorted(row, reverse=True), (n, row)  # once refused, every larger size is refused
        if n in (1, 9):
            assert not any(row)


def test_variable_zero_disables_the_path(built):
    q = [(n, b) for n in (2, 4, 8) for b in (1, 8, 4096)]
    assert takes_in_a_process("0", q) == [0] * len(q)


def test_variable_sets_the_bound(built):
    q = [(n, b) for n in (2, 3, 8) for b in (0, 1, 4096, 4097)] + [(1, 8), (9, 8)]
    assert takes_in_a_process("4096", q) == [0, 1, 1, 0] * 3 + [0, 0]


def test_variable_is_clamped_to_1mib(built):
    q = [(n, b) for n in (2, 8) for b in (1 << 20, (1 << 20) + 1)]
    assert takes_in_a_process(str(1 << 30), q) == [1, 0] * 2
