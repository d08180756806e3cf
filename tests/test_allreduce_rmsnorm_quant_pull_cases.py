"""mscclppAmdAllReduceRmsNormQuantPullLaunch's own refusals without a GPU (made-up addresses) through the host-only
check: what it adds to the pull entry point's -- cols % 16, q and scale present, aligned and overlapping nothing."""
import ctypes

import pytest

N, A = 3, 1 << 21  # three ranks; buffers 2 MiB apart from address A on
X, Q, RES, RO, GAMMA, SCALE = range(6)
at0 = lambda r, b: A * (8 + 8 * r + b)  # view r's buffer b


def call(launch=False, rows=4, cols=64, dtype=1, ptrs=None, peer_scale=True):
    """The code of the host-only check (or of a launch) whose view r has buffer b at at0(r, b), but for ptrs[(r, b)]."""
    import mscclpp_amd as m

    at = {**{(r, b): at0(r, b) for r in range(N) for b in range(6)}, **(ptrs or {})}
    arr = (m.RankView * N)()
    for r in range(N):
        v = arr[r]
        v.input, v.output, v.rank = at[(r, X)], at[(r, Q)], r
        v.tokens = v.expected = v.err = A
        for q in range(N):
            v.peerTokens[q], v.peerInput[q], v.peerOutput[q] = A, at[(q, X)], at[(q, Q)]
    col = lambda b: (ctypes.c_void_p * N)(*[at[(r, b)] for r in range(N)])
    if not launch:
        return m.lib().mscclppAmdAllReduceRmsNormQuantPullCheck(arr, N, N, col(RES), col(RO), col(GAMMA), col(SCALE), rows,
                                                                cols, dtype, 0, 0)
    peers = lambda b: (ctypes.c_void_p * (N * m.MAX_RANKS))(*[at[(q, b)] if q < N else None
                                                              for _ in range(N) for q in range(m.MAX_RANKS)])
    return m.lib().mscclppAmdAllReduceRmsNormQuantPullLaunch(arr, N, N, col(RES), col(RO), peers(RO), col(GAMMA), col(SCALE),
                                                             peers(SCALE) if peer_scale else None, rows, cols, dtype, 1e-5,
                                                             0, 0, 1000, None)


@pytest.mark.parametrize("bad", [
    dict(cols=24), dict(cols=8), dict(cols=2056),   # whole units of x, but rows of q that are not whole 16-byte units
    dict(ptrs={(1, Q): None}), dict(ptrs={(2, SCALE): None}), dict(ptrs={(0, Q): at0(0, Q) + 8}),
    dict(ptrs={(0, SCALE): at0(0, SCALE) + 2}), dict(ptrs={(0, Q): at0(0, X)}),  # ...; q is x: no in-place form
    dict(ptrs={(0, Q): at0(0, X) + 496}),           # q begins inside x's last bytes
    dict(ptrs={(1, Q): at0(1, RO) - 240}),          # q's last 16 bytes are res_out's first
    dict(ptrs={(0, SCALE): at0(0, Q) + 252}),       # scale begins in q's last dword
    dict(ptrs={(2, SCALE): at0(0, GAMMA) + 124}),   # rank 2's scale in rank 0's gamma
    dict(ptrs={(1, Q): at0(0, Q) + 128}),           # two ranks' q overlap
    dict(ptrs={(1, SCALE): at0(2, SCALE) + 12}),    # two ranks' scales share a dword
    dict(launch=True, peer_scale=False), dict(rows=0), dict(dtype=2),  # (the last two: the pull entry point's stay)
], ids=str)
def test_refused_as_invalid_argument(built, bad):
    assert call(**bad) == 4


def test_good_calls_pass(built):
    in_place = {(r, RO): at0(r, RES) for r in range(N)}
    assert call() == 0 and call(ptrs=in_place) == 0 and call(dtype=0) == 0
    assert call(rows=65, cols=8192) == 0
    assert call(ptrs={(0, SCALE): at0(0, Q) + 256, (1, Q): at0(1, X) + 512}) == 0  # adjacent is not overlapping
