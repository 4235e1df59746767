"""tests/fftfilt_bound.py on the CPU: the oracle meets the window-local bound on
every row, the cases are what the GPU tests need them to be, and the checker
(both assertions) is pinned.  No GPU.
"""
import numpy as np
import pytest

import fftfilt_bound as FFB
import fir_bound as FB
import liquidmi as LQ
import oracle_lib as O

# the transform rows, one per (type, taps)
TROWS = sorted({(t, h) for t, h, k, _ in FFB.ROWS if k != "direct"})
TR = pytest.mark.parametrize("f", TROWS, ids=FB.filter_id)


@pytest.mark.parametrize("name", FFB.ENVELOPES)
@TR
def test_oracle_meets_the_bound(f, name):
    """At n = nfft / 2 (the figure the GPU tests compare with), at n = 64
    where the filter allows it, and on the shorter stream of the 8192-point rows."""
    t, hlen = f
    c = FFB.case(t, hlen, name)
    w = FFB.oracle_worst(t, hlen, name)
    assert 0 < w < 0.01   # rigorous but loose
    if hlen <= 65:
        c.check(FFB.oracle_stream(O, c, 64, 0.7), 0.7, what="oracle n=64")
    if c.nfft == 8192:
        assert 0 < FFB.oracle_worst(t, hlen, name, True) < 0.01


def test_rows_name_the_transform_the_library_takes():
    for t, hlen, kernel, mode in FFB.ROWS:
        nfft = LQ.fftfilt_nfft(t, hlen)
        assert nfft == FFB.nfft_of(t, hlen)
        assert nfft == {"k_fftfilt_r16<true>": 4096, "k_fftfilt_r16<false>": 4096, "k_fftfilt8k<true>": 8192,
                        "k_fftfilt8k<false>": 8192, "direct": 0}[kernel]
        assert ("<true>" in kernel and nfft == 4096) == (t == "rrrf" and nfft == 4096)
        # new samples per segment, as the kernels form them (k_fftfilt.hip)
        if nfft:
            assert FB.seg_len(hlen) == nfft - (hlen - 1 if nfft == 4096 else (hlen - 1 + 1) & ~1)
    assert LQ.fftfilt_nfft("rrrf", 2049) == 4096 and LQ.fftfilt_nfft("crcf", 4097) == 8192


@pytest.mark.parametrize("row", FFB.ROWS, ids=FFB.row_id)
def test_cases_are_what_they_say(row):
    t, hlen = row[0], row[1]
    span, L = FFB.span_of(t, hlen), FB.seg_len(hlen)
    for short in ((False, True) if FFB.nfft_of(t, hlen) == 8192 else (False,)):
        n = FFB.stream_len(t, hlen, short)
        assert n == 2 * L + 5 * span + 777 - short and n <= 55_000
        for name, floor in (("burst", 1e-5), ("gaps", 0.0)):
            e = FFB.envelope(name, t, hlen, short)
            assert len(e) == n and np.count_nonzero(e == 1.0) == 40 + 100 + 2 + 3
            assert np.all(e[[0, 39, L - 50, L + 49, 2 * L - 1, 2 * L, n - 3, n - 1]] == 1.0)
            assert np.all(e[[40, L - 51, L + 50, 2 * L - 2, 2 * L + 1, n - 4]] == floor)
        a, b, c3 = FFB.cuts(t, hlen)
        assert a == 40 and L < b < 2 * L and 2 * L + 1 + span == c3 < n - span
        assert (a < hlen - 1) == (hlen > 41)
        # gaps: at least nfft outputs whose bound is exactly 0; burst: at least
        # nfft whose bound is below 1e-3 of the largest
        g, bu = FFB.case(t, hlen, "gaps", short), FFB.case(t, hlen, "burst", short)
        nz = np.count_nonzero(g.bound1 == 0)
        assert nz >= span and np.all(g.y1[g.bound1 == 0] == 0)
        if not short:
            assert nz == {4096: 13063, 8192: 25351}[span]
        assert np.count_nonzero(bu.bound1 < 1e-3 * np.max(bu.bound1)) >= span
        assert np.all(bu.bound1 > 0)
    assert FFB.stream_len(t, hlen) % 2 == 1   # the full stream is odd, the short one even


def test_window_norm_is_exact_where_it_matters():
    x = np.zeros(30000, np.complex64)
    x[100:140] = 1 + 1j
    x[25000] = 3e-6
    W = FFB.window_norm(x, 4096)
    assert np.all(W[140 + 4095:25000 - 4095] == 0) and W[140 + 4094] > 0 and W[25000 - 4095] > 0
    assert abs(W[0] - np.sqrt(80.0)) < 1e-12 and abs(W[25000 + 4095] - 3e-6) < 1e-12
    assert np.all(W[25000 + 4096:] == 0)


# ------------------------------------------------------------- the checker, pinned
PIN_ROWS = pytest.mark.parametrize("f", [("rrrf", 45), ("crcf", 512), ("cccf", 2049), ("crcf", 2050)],
                                   ids=FB.filter_id)


def _good(c):
    """The oracle's stream: passes both assertions against its own worst ratio."""
    y = FFB.oracle_stream(O, c, c.nfft // 2, 0.7)
    w = FFB.oracle_worst(c.t, c.hlen, c.name, c.short)
    c.check(y, 0.7, w, what="unharmed")
    return y, w


@pytest.mark.parametrize("name", FFB.ENVELOPES)
@PIN_ROWS
def test_checker_fails_on_rounding_noise_of_the_loud_level_in_a_quiet_segment(f, name):
    """A quiet segment (number 5: its window holds nothing loud) gets 2^-24
    max |y| added to its L outputs -- what leaks when a loud segment's rounding
    noise reaches it.  Normwise that is 6e-8."""
    c = FFB.case(f[0], f[1], name)
    y, w = _good(c)
    z = y.copy()
    z[5 * c.L:6 * c.L] += np.float32(2.0 ** -24 * np.max(np.abs(y)))
    with pytest.raises(AssertionError):
        c.check(z, 0.7, w, what="noise")


@pytest.mark.parametrize("name", FFB.ENVELOPES)
@PIN_ROWS
def test_checker_fails_on_a_quiet_segment_overwritten_with_the_loud_one_three_before(f, name):
    c = FFB.case(f[0], f[1], name)
    y, w = _good(c)
    z = y.copy()
    z[5 * c.L:6 * c.L] = y[2 * c.L:3 * c.L]
    with pytest.raises(AssertionError):
        c.check(z, 0.7)   # the first assertion alone


def test_checker_fails_on_a_tiny_value_where_zero_is_due():
    c = FFB.case("crcf", 512, "gaps")
    y, w = _good(c)
    k = int(np.flatnonzero(c.bound1 == 0)[7])
    z = y.copy()
    z[k] = 1e-30
    r = c.report(z, 0.7)
    assert r["failing"] == 1 and r["nonzero_zeros"] == 1 and r["index"] == k
    with pytest.raises(AssertionError):
        c.check(z, 0.7, w)
    z[k] = -0.0   # either sign of zero passes
    c.check(z, 0.7, w)


def test_checker_fails_on_nan():
    c = FFB.case("rrrf", 45, "burst")
    y, w = _good(c)
    z = y.copy()
    z[20000] = np.nan
    assert c.report(z, 0.7)["nonfinite"] == 1
    with pytest.raises(AssertionError):
        c.check(z, 0.7, w)
