"""mscclppAmdAllReduceRmsNormQuantLaunch's own refusals without a GPU (made-up addresses) through the host-only check:
what it adds to the LL entry point's -- the format, cols % 32 in the MX formats, q and scale present, aligned and
overlapping nothing -- and that entry point's size cap in bytes of x."""
import ctypes

import pytest

N, A = 3, 1 << 21  # three ranks; buffers 2 MiB apart from address A on
X, Q, RES, RO, GAMMA, SCALE = range(6)
MXFP8, MXFP4, FP8_ROW = range(3)
at0 = lambda r, b: A * (8 + 8 * r + b)  # view r's buffer b


def call(rows=4, cols=64, dtype=1, fmt=MXFP8, ptrs=None):
    """The code of the host-only check whose view r has buffer b at at0(r, b), but for ptrs[(r, b)]."""
    import mscclpp_amd as m

    at = {**{(r, b): at0(r, b) for r in range(N) for b in range(6)}, **(ptrs or {})}
    arr = (m.RankView * N)()
    for r in range(N):
        arr[r].input, arr[r].output, arr[r].rank = at[(r, X)], at[(r, Q)], r
    col = lambda b: (ctypes.c_void_p * N)(*[at[(r, b)] for r in range(N)])
    return m.lib().mscclppAmdAllReduceRmsNormQuantCheck(arr, N, N, col(RES), col(RO), col(GAMMA), col(SCALE), rows, cols,
                                                        dtype, fmt, 0, 0)


@pytest.mark.parametrize("bad", [
    dict(fmt=3), dict(fmt=-1), dict(cols=48, fmt=MXFP8), dict(cols=48, fmt=MXFP4), dict(cols=6, fmt=FP8_ROW),
    dict(ptrs={(1, Q): None}), dict(ptrs={(2, SCALE): None}), dict(ptrs={(0, Q): at0(0, Q) + 2}),
    dict(fmt=FP8_ROW, ptrs={(1, SCALE): at0(1, SCALE) + 2}),
    dict(ptrs={(0, Q): at0(0, X)}), dict(fmt=FP8_ROW, ptrs={(0, Q): at0(0, X) + 508}),  # q is x; q begins in x's last bytes
    dict(fmt=MXFP4, ptrs={(1, Q): at0(1, RO) - 124}),       # MXFP4: q's last 4 of 128 bytes are res_out's first
    dict(ptrs={(0, SCALE): at0(0, Q) + 255}),                # scale begins in q's last byte
    dict(fmt=FP8_ROW, ptrs={(0, SCALE): at0(0, Q) + 252}),   # ... the row scales in q's last dword
    dict(ptrs={(2, SCALE): at0(0, GAMMA) - 7}),              # rank 2's 8 scale bytes end in rank 0's gamma
    dict(ptrs={(1, SCALE): at0(2, SCALE) + 7}),              # two ranks' scales share a byte
], ids=str)
def test_refused_as_invalid_argument(built, bad):
    assert call(**bad) == 4


@pytest.mark.parametrize("fmt", [MXFP8, MXFP4, FP8_ROW])
def test_good_calls_pass_and_the_cap_is_in_bytes_of_x(built, fmt):
    in_place = {(r, RO): at0(r, RES) for r in range(N)}
    qbytes, sbytes = 256 >> (fmt == MXFP4), 16 if fmt == FP8_ROW else 8
    assert call(fmt=fmt) == 0 and call(fmt=fmt, ptrs=in_place) == 0 and call(fmt=fmt, dtype=0) == 0
    assert call(fmt=fmt, rows=64, cols=8192) == 0 and call(fmt=fmt, rows=65, cols=8192) == 5  # 1 MiB of x, and past it
    # buffers that touch without overlapping
    assert call(fmt=fmt, ptrs={(0, SCALE): at0(0, Q) + qbytes, (1, Q): at0(1, X) + 512}) == 0
    assert call(fmt=fmt, ptrs={(1, SCALE): at0(2, SCALE) + sbytes, (0, SCALE): at0(0, Q) - sbytes}) == 0


def test_what_depends_on_the_format(built):
    assert call(cols=48, fmt=FP8_ROW) == 0 and call(cols=4, fmt=FP8_ROW) == 0
    assert call(fmt=MXFP8, ptrs={(2, SCALE): at0(2, SCALE) + 3}) == 0 and call(fmt=MXFP4, ptrs={(2, SCALE): at0(2, SCALE) + 1}) == 0
