"""mscclppAmdAllReduceRmsNormLaunch's refusals and the scratch requirement without a GPU (made-up addresses)."""
import ctypes

import pytest

N, A = 3, 1 << 21  # three ranks; buffers 2 MiB apart from address A on
X, Y, RES, RO, GAMMA = 0, 1, 2, 3, 4


def launch(rows=4, cols=64, dtype=0, nthreads=0, nblocks=0, scratch_bytes=1 << 24, ptrs=None, **view_fields):
    """The code of a launch whose view r has buffer b at A * (8 + 8 * r + b), but for ptrs[(r, b)]."""
    import mscclpp_amd as m

    at = {(r, b): A * (8 + 8 * r + b) for r in range(N) for b in range(5)}
    at.update(ptrs or {})
    arr = (m.RankView * N)()
    for r in range(N):
        v = arr[r]
        v.input, v.output = at[(r, X)], at[(r, Y)]
        v.scratch = v.flags = v.err = A
        v.scratchBytes, v.rank = scratch_bytes, r
        for q in range(N):
            v.peerScratch[q] = A
        for k, val in view_fields.items():
            setattr(v, k, val)
    col = lambda b: (ctypes.c_void_p * N)(*[at[(r, b)] for r in range(N)])
    return m.lib().mscclppAmdAllReduceRmsNormLaunch(arr, N, N, col(RES), col(RO), col(GAMMA), rows, cols, dtype, 1e-5,
                                                    nblocks, nthreads, 1000, None)


@pytest.mark.parametrize("bad", [
    dict(rows=0), dict(cols=0), dict(cols=66), dict(cols=8196, nthreads=256), dict(cols=16388, nthreads=512),
    dict(cols=2052, nthreads=64), dict(dtype=2), dict(dtype=-1), dict(nthreads=96), dict(nblocks=4097),
    dict(ptrs={(1, X): None}), dict(ptrs={(1, Y): None}), dict(ptrs={(2, GAMMA): None}),
    dict(ptrs={(0, GAMMA): A * 12 + 4}), dict(ptrs={(0, X): A * 8 + 2}),
    dict(ptrs={(0, RES): None}), dict(ptrs={(0, RO): None}), dict(ptrs={(r, RES): None for r in range(N)}),
    dict(ptrs={(0, Y): A * 8 + 8}),        # y overlaps x without being x
    dict(ptrs={(0, RO): A * 8}),           # res_out is x
    dict(ptrs={(0, GAMMA): A * 9 + 64}),   # gamma inside y
    dict(ptrs={(1, Y): A * 8}),            # rank 1 writes rank 0's x
    dict(flags=A + 4), dict(scratch=None), dict(err=None),
], ids=str)
def test_refused_as_invalid_argument(built, bad):
    assert launch(**bad) == 4


def test_refused_as_invalid_usage_and_the_scratch_requirement(built):
    import mscclpp_amd as m

    need = m.all_reduce_rms_norm_scratch_required(N, 4, 64, m.BF16)
    assert need == 2 * ((N * 4 * 16 * 16 + 255) // 256 * 256)  # two halves of N regions of rows * cols / 4 units
    assert m.all_reduce_rms_norm_scratch_required(8, 64, 8192, m.F16) == 32 << 20
    for n, rows, cols, dt in ((1, 4, 64, 0), (9, 4, 64, 0), (2, 0, 64, 0), (2, 4, 62, 0), (2, 4, 64, m.F32),
                              (2, 65, 8192, 0), (2, 1, 16388, 0)):
        assert m.all_reduce_rms_norm_scratch_required(n, rows, cols, dt) == 0
    assert launch(scratch_bytes=need - 256) == 5
    assert launch(rows=65, cols=8192) == 5  # above 1 MiB
    assert launch(rows=65, cols=8192, dtype=2) == 4  # an argument refusal comes first
    assert launch(scratch_bytes=0, ptrs={(r, b + 1): A * (8 + 8 * r + b) for r in range(N) for b in (X, RES)}) == 5


def test_python_refuses_tensors_that_do_not_fit(built):
    import mscclpp_amd as m
    import torch

    x, g = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(64, dtype=torch.bfloat16)
    strided = torch.zeros(4, 128, dtype=torch.bfloat16)[:, :64]
    for bad in ((x, x, None, None, g[:32]), (x, x, None, None, g.float()), (strided, strided, None, None, g),
                (x, x[1:], None, None, g), (x, x, x.float(), x, g), (x[0], x[0], None, None, g)):
        with pytest.raises(m.MscclppError):
            m._rms_norm_tensors(*bad)
    m._rms_norm_tensors(x, x, x, x, g)
