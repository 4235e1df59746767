"""Every firfilt kernel against the direct form's per-output error bound
(tests/fir_bound.py), however the caller cuts the stream (`-m gpu`).

The normwise checks of the rest of the suite divide the largest error by the
largest output of the whole stream, so a quiet region that is entirely wrong
still scores 1e-12.  Here every output is held to (T + 8) 2^-23 A[n] against
a float64 convolution, A[n] the sum of |h||x| that output sees; outputs whose
inputs are all zero must be exactly zero.  The same bound on every kernel is
what makes the result independent of the call size: envelopes with bursts,
exact-zero gaps and level steps run
  (a) as one device call,
  (b) as device calls of 8191 samples,
  (c) as two calls, the loud samples reaching the second only through the
      carried history,
  (d) in place,
and through the host-pointer execute_block, all against the same y64.
"""
import numpy as np
import pytest

import fir_bound as FB
import liquidmi as LQ
import oracle_lib as O
from test_gpu_edges import _pattern

pytestmark = pytest.mark.gpu

FILTERS = pytest.mark.parametrize("f", FB.FILTERS, ids=FB.filter_id)


def _filt(c):
    g = LQ.FirFilt(c.t, c.h)
    g.set_scale(c.s)
    return g


def _run_dev(c, cuts=(), in_place=False):
    """The stream through execute_block_dev, one call per piece."""
    g = _filt(c)
    x = c.x
    bx = LQ.DeviceBuffer.from_array(x)
    by = bx if in_place else LQ.DeviceBuffer(x.nbytes)
    edges = [0] + list(cuts) + [len(x)]
    for a, b in zip(edges[:-1], edges[1:]):
        g.execute_block_dev(bx.p + a * x.itemsize, b - a, by.p + a * x.itemsize)
    g.synchronize()
    return by.to_array(x.dtype, len(x))


@pytest.mark.parametrize("name", FB.ENVELOPES)
@FILTERS
def test_firfilt_bound_one_call(f, name):
    c = FB.case(f[0], f[1], name)
    c.check(_run_dev(c))


@pytest.mark.parametrize("name", FB.ENVELOPES)
@FILTERS
def test_firfilt_bound_calls_of_8191(f, name):
    c = FB.case(f[0], f[1], name)
    c.check(_run_dev(c, cuts=range(8191, len(c.x), 8191)))


@FILTERS
def test_firfilt_bound_carried_history(f):
    c = FB.carried_case(*f)
    c.check(_run_dev(c, cuts=(FB.carried_split(f[1])[0],)))


@FILTERS
def test_firfilt_bound_in_place(f):
    c = FB.case(f[0], f[1], "burst")
    c.check(_run_dev(c, in_place=True))


@FILTERS
def test_firfilt_bound_host_pointers(f):
    c = FB.case(f[0], f[1], "stairs")
    c.check(_filt(c).execute_block(c.x))


@pytest.mark.parametrize("small", [False, True], ids=["2p98", "2m58"])
def test_firfilt_bound_extreme_range(small):
    # 129 equal taps of 2^13 on a constant 2^98: the direct sum is finite
    # (3.3e35) where nfft sum|h| |x| is not; the mirror, 2^-13 on 2^-58, sits
    # at the small end of the ranges the kernels guard
    c = FB.overflow_case(small)
    y = _run_dev(c)
    ref = O.FirFilt(O.CRCF, c.h).execute_block(c.x)
    assert np.array_equal(_pattern(y), _pattern(ref)), "non-finite pattern differs from the oracle"
    c.check(y)
