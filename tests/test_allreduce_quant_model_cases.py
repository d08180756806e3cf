"""The numpy model of the quantised-wire AllReduce on the GPU tests' inputs (no GPU): it stays inside the error bound
against the fp64 sum, and the inputs tell the definition from a wrong summation order and from an own contribution
left unquantised -- otherwise the bit-for-bit GPU cases would show nothing about either."""
import numpy as np
import pytest

import allreduce_quant_model as Q


@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("dt", Q.DTYPES)
@pytest.mark.parametrize("n", [2, 3, 8])
def test_model_on_the_test_inputs(n, dt, fmt):
    for count in (32, 32 * (n + 1), 32 * (64 * n + 5)):
        xs = Q.inputs(1, n, count, dt, fmt)
        out = Q.model(xs, dt, fmt)
        err, bound = Q.error_and_bound(xs, out, dt, fmt)
        assert (err <= bound).all(), (count, float((err - bound).max()))
        if n > 2 and count > 32 * (n + 1):  # (two terms have one order; the probes' roles need blocks to go round)
            for order in Q.wrong_orders(n):
                assert not np.array_equal(Q.model(xs, dt, fmt, order=order), out), (count, order)
        if count > 32:  # (the probe's values are their own codes)
            assert not np.array_equal(Q.model(xs, dt, fmt, own_exact=True), out), count
    assert Q.K["mxint8"] == 2.0 ** -6 and Q.K["mxfp4"] == 0.5
