"""fftfilt's overlap-save kernels against an error bound local to a window
(tests/fftfilt_bound.py), however the caller cuts the stream (`-m gpu`).

An output may err by (8 lg + 8) 2^-23 |s| sum|h| times the 2-norm of the
inputs within nfft - 1 samples of it, and where those are all zero it must be
exactly zero: a segment that picks up a loud neighbour's content or rounding
noise -- through a register or LDS value the persistent loop keeps from its
previous segment, through the history job, through the first / last-segment
special cases -- fails, where the normwise checks of the rest of the suite
see 6e-8.  The bound is loose, so each run's worst ratio to it must also stay
within 4 x the oracle's on the same case (oracle at n = nfft / 2); both are
printed.

Each row names its kernel and asserts the transform size behind it
(lqk_fftfilt_nfft) and, for the 8192-point kernel, the alignment that picks
the paired or the unpaired form.  The burst and gaps streams run
  (a) as one device call,
  (b) as device calls cut at 40, L + 7 and 2L + 1 + nfft,
  (c) in place (x == y: the copy path),
  (d) through execute() with the object's n = max(h_len - 1, 64) and n = nfft / 2,
and all of it once more at three workgroups, where one workgroup walks from
a loud segment into a quiet one three segments on.  The rows past the
transforms run the direct FIR engine and are held to the direct form's
per-output bound (tests/fir_bound.py).
"""
import numpy as np
import pytest

import fftfilt_bound as FFB
import fir_bound as FB
import liquidmi as LQ

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 3], ids=["full-grid", "three-workgroups"])
def workgroups(request):
    LQ.set_max_workgroups(request.param)
    try:
        yield request.param
    finally:
        LQ.set_max_workgroups(0)


@pytest.fixture
def gpu_small_calls():
    """execute() on the GPU whatever its size"""
    old = LQ.get_small_calls()
    LQ.set_small_calls(False)
    try:
        yield
    finally:
        LQ.set_small_calls(old)


def _obj(c, n):
    g = LQ.FftFilt(c.h, n, t=c.t)
    g.set_scale(FB.scale_of(c.t))
    return g


def _run_dev(c, cuts=(), off=0, in_place=False):
    """The stream through execute_block_dev, one call per piece, x and y
    `off` bytes past a 16-byte boundary."""
    g = _obj(c, max(c.hlen - 1, 64))
    x, esz, n = c.x, c.x.itemsize, len(c.x)
    bx = LQ.DeviceBuffer(x.nbytes + 32)
    by = bx if in_place else LQ.DeviceBuffer(x.nbytes + 32)
    assert bx.p % 16 == 0 and by.p % 16 == 0
    LQ.lib().liquid_mi355x_memcpy_h2d(bx.p + off, LQ.ptr(x), x.nbytes)
    edges = [0] + list(cuts) + [n]
    for a, b in zip(edges[:-1], edges[1:]):
        g.execute_block_dev(bx.p + off + a * esz, b - a, by.p + off + a * esz)
    LQ.lib().liquid_mi355x_device_synchronize()
    yb = np.empty(x.nbytes + 32, np.uint8)
    LQ.lib().liquid_mi355x_memcpy_d2h(LQ.ptr(yb), by.p, yb.nbytes)
    return yb[off:off + x.nbytes].view(x.dtype).copy()


def _run_execute(c, n):
    """execute() on blocks of the object's n; the stream zero padded to whole blocks"""
    g = _obj(c, n)
    x = np.concatenate([c.x, np.zeros((-len(c.x)) % n, c.x.dtype)])
    return np.concatenate([g.execute(x[a:a + n]) for a in range(0, len(x), n)])[: len(c.x)]


def _cases(row, name):
    t, hlen = row[0], row[1]
    return [FFB.case(t, hlen, name, short) for short in ((False, True) if FFB.nfft_of(t, hlen) == 8192 else (False,))]


def _check(c, y, what):
    if c.nfft == 0:
        return c.check_direct(y, FB.scale_of(c.t))
    return c.check(y, FB.scale_of(c.t), FFB.oracle_worst(c.t, c.hlen, c.name, c.short), what)


def _assert_kernel(row):
    t, hlen, kernel, mode = row
    nfft = LQ.fftfilt_nfft(t, hlen)
    assert nfft == FFB.nfft_of(t, hlen)
    assert kernel == {0: "direct", 4096: "k_fftfilt_r16<%s>" % ("true" if t == "rrrf" else "false"),
                      8192: "k_fftfilt8k<%s>" % ("false" if mode == "off8" else "true")}[nfft]


@pytest.mark.parametrize("name", FFB.ENVELOPES)
@pytest.mark.parametrize("row", FFB.ROWS, ids=FFB.row_id)
def test_fftfilt_bound_device_calls(row, name, workgroups):
    """(a), (b), (c)"""
    _assert_kernel(row)
    off = 8 if row[3] == "off8" else 0
    for c in _cases(row, name):
        assert (c.x.itemsize == 8) or off == 0
        tag = "wg=%d n=%d " % (workgroups, len(c.x))
        _check(c, _run_dev(c, off=off), tag + "one call")
        _check(c, _run_dev(c, FFB.cuts(c.t, c.hlen), off=off), tag + "cut")
        _check(c, _run_dev(c, off=off, in_place=True), tag + "in place")
        _check(c, _run_dev(c, FFB.cuts(c.t, c.hlen), off=off, in_place=True), tag + "in place, cut")


@pytest.mark.parametrize("name", FFB.ENVELOPES)
@pytest.mark.parametrize("row", [r for r in FFB.ROWS if r[3] is None], ids=FFB.row_id)
def test_fftfilt_bound_execute(row, name, workgroups, gpu_small_calls):
    """(d): every execute() a kernel launch"""
    _assert_kernel(row)
    c = FFB.case(row[0], row[1], name)
    # create() needs n >= h_len - 1: the 4098-tap direct row runs its smallest n only
    for n in sorted({max(c.hlen - 1, 64), max(c.hlen - 1, FFB.span_of(c.t, c.hlen) // 2)}):
        _check(c, _run_execute(c, n), "wg=%d execute n=%d" % (workgroups, n))


@pytest.mark.parametrize("name", FFB.ENVELOPES)
@pytest.mark.parametrize("row", [r for r in FFB.ROWS if max(r[1] - 1, 64) * r[1] <= 65536 and r[3] is None],
                         ids=FFB.row_id)
def test_fftfilt_bound_execute_small_calls_on_the_host(row, name):
    """(d) in the small-call mode: n h_len <= 65536 is computed on the host as
    the direct convolution, the history mirrored; a device call in between
    hands the history over both ways."""
    c = FFB.case(row[0], row[1], name)
    old = LQ.get_small_calls()
    LQ.set_small_calls(True)
    try:
        n = max(c.hlen - 1, 64)
        g = _obj(c, n)
        x = np.concatenate([c.x, np.zeros((-len(c.x)) % n, c.x.dtype)])
        out = []
        for k, a in enumerate(range(0, len(x), n)):
            out.append(g.execute_block(x[a:a + n]) if k % 5 == 3 else g.execute(x[a:a + n]))
        _check(c, np.concatenate(out)[: len(c.x)], "host execute n=%d" % n)
    finally:
        LQ.set_small_calls(old)
