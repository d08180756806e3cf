"""mscclppAmdAllReduceRmsNormPullLaunch's refusals without a GPU (made-up addresses), and a size the LL entry
point refuses passing the host-only argument check."""
import ctypes

import pytest

N, A = 3, 1 << 21  # three ranks; buffers 2 MiB apart from address A on
X, Y, RES, RO, GAMMA = 0, 1, 2, 3, 4


def call(check=False, a=A, rows=4, cols=64, dtype=0, nthreads=0, nblocks=0, ptrs=None, peer_ro=True, **view_fields):
    """The code of a launch (or of the host-only check) whose view r has buffer b at A * (8 + 8 * r + b), but for
    ptrs[(r, b)]; a: the spacing."""
    import mscclpp_amd as m

    at = {(r, b): a * (8 + 8 * r + b) for r in range(N) for b in range(5)}
    at.update(ptrs or {})
    arr = (m.RankView * N)()
    for r in range(N):
        v = arr[r]
        v.input, v.output, v.rank = at[(r, X)], at[(r, Y)], r
        v.tokens = v.expected = v.err = A
        for q in range(N):
            v.peerTokens[q], v.peerInput[q], v.peerOutput[q] = A, at[(q, X)], at[(q, Y)]
        for k, val in view_fields.items():
            setattr(v, k, val)
    col = lambda b: (ctypes.c_void_p * N)(*[at[(r, b)] for r in range(N)])
    if check:
        return m.lib().mscclppAmdAllReduceRmsNormPullCheck(arr, N, N, col(RES), col(RO), col(GAMMA), rows, cols, dtype,
                                                           nblocks, nthreads)
    pro = (ctypes.c_void_p * (N * m.MAX_RANKS))()
    for r in range(N):
        for q in range(N):
            pro[r * m.MAX_RANKS + q] = at[(q, RO)]
    return m.lib().mscclppAmdAllReduceRmsNormPullLaunch(arr, N, N, col(RES), col(RO), pro if peer_ro else None, col(GAMMA),
                                                        rows, cols, dtype, 1e-5, nblocks, nthreads, 1000, None)


@pytest.mark.parametrize("bad", [
    dict(rows=0), dict(cols=0), dict(cols=4), dict(cols=68), dict(cols=8200, nthreads=256), dict(cols=16392, nthreads=512),
    dict(cols=2056, nthreads=64), dict(dtype=2), dict(dtype=-1), dict(nthreads=96), dict(nblocks=257),
    dict(ptrs={(1, X): None}), dict(ptrs={(1, Y): None}), dict(ptrs={(2, GAMMA): None}),
    dict(ptrs={(0, GAMMA): A * 12 + 8}), dict(ptrs={(0, X): A * 8 + 8}),  # 8-byte aligned is not enough
    dict(ptrs={(0, RES): None}), dict(ptrs={(0, RO): None}), dict(ptrs={(r, RES): None for r in range(N)}),
    dict(peer_ro=False),
    dict(ptrs={(0, Y): A * 8 + 16}),       # y overlaps x without being x
    dict(ptrs={(0, RO): A * 8}),           # res_out is x
    dict(ptrs={(0, GAMMA): A * 9 + 64}),   # gamma inside y
    dict(ptrs={(1, Y): A * 8}),            # rank 1 writes rank 0's x
    dict(tokens=None), dict(err=None), dict(rank=3),
    dict(rows=65, cols=8192, dtype=2),     # the LL entry point's size refusal does not come first: there is none
], ids=str)
def test_refused_as_invalid_argument(built, bad):
    assert call(**bad) == 4


def test_the_argument_check_has_no_byte_cap(built):
    in_place = {(r, b + 1): A * (8 + 8 * r + b) for r in range(N) for b in (X, RES)}
    assert call(check=True) == 0 and call(check=True, ptrs=in_place) == 0
    assert call(check=True, rows=65, cols=8192) == 0  # above the LL path's 1 MiB
    assert call(check=True, a=1 << 36, rows=1 << 20, cols=16384) == 0  # 32 GiB per buffer: the addresses are made up
    assert call(check=True, rows=65, cols=8192, dtype=2) == 4 and call(check=True, cols=4) == 4
    # one workgroup for 3 x 2^18 rows of 32 KiB: its rows exceed one descriptor
    assert call(check=True, a=1 << 36, rows=3 << 18, cols=16384, nblocks=1) == 5
    assert call(check=True, a=1 << 36, rows=3 << 18, cols=16384, nblocks=4) == 0
