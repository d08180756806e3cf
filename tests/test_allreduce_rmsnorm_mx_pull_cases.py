"""mscclppAmdAllReduceRmsNormMxPullLaunch's own refusals without a GPU (made-up addresses) through the host-only
check: what it adds to the pull entry point's -- cols % 32, the format, q and scale present and overlapping nothing."""
import ctypes

import pytest

N, A = 3, 1 << 21  # three ranks; buffers 2 MiB apart from address A on
X, Q, RES, RO, GAMMA, SCALE = range(6)
at0 = lambda r, b: A * (8 + 8 * r + b)  # view r's buffer b


def call(rows=4, cols=64, dtype=1, fmt=0, ptrs=None):
    """The code of the host-only check whose view r has buffer b at at0(r, b), but for ptrs[(r, b)]."""
    import mscclpp_amd as m

    at = {**{(r, b): at0(r, b) for r in range(N) for b in range(6)}, **(ptrs or {})}
    arr = (m.RankView * N)()
    for r in range(N):
        arr[r].input, arr[r].output, arr[r].rank = at[(r, X)], at[(r, Q)], r
    col = lambda b: (ctypes.c_void_p * N)(*[at[(r, b)] for r in range(N)])
    return m.lib().mscclppAmdAllReduceRmsNormMxPullCheck(arr, N, N, col(RES), col(RO), col(GAMMA), col(SCALE), rows, cols,
                                                         dtype, fmt, 0, 0)


@pytest.mark.parametrize("bad", [
    dict(cols=48), dict(cols=16), dict(fmt=2), dict(fmt=-1), dict(rows=0), dict(dtype=2),  # (the last two: the pull check's)
    dict(ptrs={(1, Q): None}), dict(ptrs={(2, SCALE): None}), dict(ptrs={(0, Q): at0(0, Q) + 8}),
    dict(ptrs={(0, Q): at0(0, X)}), dict(ptrs={(0, Q): at0(0, X) + 496}),  # q is x; q begins inside x's last bytes
    dict(fmt=1, ptrs={(1, Q): at0(1, RO) - 112}),            # MXFP4: q's last 16 of 128 bytes are res_out's first
    dict(ptrs={(0, SCALE): at0(0, Q) + 255}),                # scale begins in q's last byte
    dict(fmt=1, ptrs={(0, SCALE): at0(0, Q) + 127}),         # ... of MXFP4's 128
    dict(ptrs={(2, SCALE): at0(0, GAMMA) - 7}),              # rank 2's 8 scale bytes end in rank 0's gamma
    dict(ptrs={(1, SCALE): at0(2, SCALE) + 7}),              # two ranks' scales share a byte
], ids=str)
def test_refused_as_invalid_argument(built, bad):
    assert call(**bad) == 4


@pytest.mark.parametrize("fmt", [0, 1])
def test_good_calls_pass(built, fmt):
    in_place = {(r, RO): at0(r, RES) for r in range(N)}
    qbytes = 256 >> fmt
    assert call(fmt=fmt) == 0 and call(fmt=fmt, ptrs=in_place) == 0 and call(fmt=fmt, dtype=0) == 0
    assert call(fmt=fmt, rows=65, cols=8192) == 0
    # adjacent is not overlapping; a scale at an odd address
    assert call(fmt=fmt, ptrs={(0, SCALE): at0(0, Q) + qbytes, (1, Q): at0(1, X) + 512, (2, SCALE): at0(2, SCALE) + 3}) == 0
    assert call(fmt=fmt, ptrs={(1, SCALE): at0(2, SCALE) + 8, (0, SCALE): at0(0, Q) - 8}) == 0
