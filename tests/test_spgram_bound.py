"""tests/spgram_bound.py on the CPU: the oracle meets the bin-local bound on
every row, the streams are what the GPU tests need them to be (dynamic range,
bursts on their seams, calls with 64, 1 and 0 transforms), the rows reach
every kernel of the reduction by the launches' own decisions, and the checker
is pinned.  No GPU.
"""
import numpy as np
import pytest

import liquidmi as LQ
import oracle_lib as O
import spgram_bound as SB

ROWS = pytest.mark.parametrize("row", SB.ROWS, ids=SB.row_id)


@ROWS
def test_oracle_meets_the_bound_and_the_case_is_what_it_says(row):
    mode, real, nfft, W, T, alpha, cuts, name = row
    c = SB.case(row)
    w = SB.oracle_worst(c)
    assert 0 < w < 0.5            # rigorous but loose (0.04 to 0.15 on the long estimates)
    TC, G = LQ.spgram_chunk(), LQ.spgram_fold_group()
    assert (TC, G) == (64, 64)    # the rows' transform counts are chosen around these
    # transform counts
    if mode == "estimate":
        assert c.T == T and len(c.x) <= 2_200_000
        delay = nfft // 4
        assert (len(c.x) % delay != 0) == (T % 2 == 1) and c.ends[-1] == len(c.x) - 1
    else:
        per_call = SB.transforms_of_calls(W, c.calls)
        assert per_call[:2] == [2, T] and (per_call[2:] == [64, 1, 0, 1] if cuts else len(per_call) == 2)
        assert c.T == sum(per_call)
        assert np.all(c.a[:2] == 1.0) and np.all(c.a[2:] == np.float32(alpha))
        if cuts:
            assert c.calls[4][0] < W // 2
    # the stream
    if name == "tone":
        span = 10 * np.log10(np.max(c.psd64) / np.min(c.psd64))
        print("span %.1f dB" % span)
        if alpha != 0.0:         # alpha = 0 keeps the second transform's psd, taken inside the onset
            assert span >= 100.0
            k = int(np.argmax(c.psd64))
            assert k == (nfft // 4 + 1 + nfft // 2) % nfft or (real and k == (-(nfft // 4 + 1) + nfft // 2) % nfft)
    else:
        e = c.energy
        quiet = np.median(e)
        loud = [c.T - 1]
        seams = [t + (2 if mode == "accumulate" else 0) for t in SB.SEAMS]
        for t in seams:
            if t + 1 < c.T:
                loud += [t, t + 1]          # both sides of the seam
        for f in c.first[1:-1]:
            if 0 < f < c.T:
                loud += [f]                 # the first transform of a call: history and input
        assert quiet < 1e-6 and all(e[t] > 1e6 * quiet for t in loud), (quiet, [(t, e[t]) for t in loud])
        if mode == "accumulate":            # the main call's chunk seam is between its transforms 63 and 64
            assert seams[0] - c.first[1] == TC - 1 and seams[1] - c.first[1] == TC * G - 1
        else:
            assert seams == [TC - 1, TC * G - 1]
    assert np.all(c.bound > 0) and np.all(np.isfinite(c.bound))
    # the margin's yardstick: the oracle's ratio on the case, or, where psd is the last transform
    # of the tone alone, its worst over the last eight (the case among them), still loose
    assert SB.single_transform(row) == (mode == "accumulate" and alpha == 1.0 and name == "tone")
    if SB.single_transform(row):
        assert w <= SB.margin_oracle(row, c) < 0.05


def test_rows_reach_every_kernel_of_the_reduction():
    """From the launches' own decisions (liquid_mi355x_spgram_route, _chunk,
    _fold_group, _batch_samples): a change of dispatch that orphans a kernel
    fails here."""
    seen = {(SB.row_path(r)[0], SB.row_path(r)[1], r[0]) for r in SB.ROWS}
    fused = ["fused<float2,HALF,TR>", "fused<float,HALF,lds>", "fused<float2,full,lds>", "fused<float,full,lds>"]
    for path in ["plain"] + fused:
        for levels in (1, 2):
            for mode in ("estimate", "accumulate"):
                assert (path, levels, mode) in seen, (path, levels, mode)
    assert {p for p, _, _ in seen} == set(["plain"] + fused)
    assert [LQ.spgram_route(False, 1024, W) for W in SB.FUSED_W] == [fused[0], fused[0], fused[2], fused[2]]
    assert [LQ.spgram_route(True, 1024, W) for W in SB.FUSED_W] == [fused[1], fused[1], fused[3], fused[3]]
    assert LQ.spgram_route(False, 1024, 512, (1 << 27) - 1) != "plain" and LQ.spgram_route(False, 1024, 512, 1 << 27) == "plain"
    assert LQ.spgram_route(False, 512, 512) == "plain" and LQ.spgram_route(True, 2048, 301) == "plain"
    # the fold: one level up to 64 chunks of 64, two beyond
    assert SB.fold_levels(4096) == 1 and SB.fold_levels(4097) == 2 and SB.fold_levels(64) == 1
    # every named window at every named count, in both modes
    for W in SB.FUSED_W:
        for real in (False, True):
            for T in SB.FUSED_T:
                for mode in ("estimate", "accumulate"):
                    assert any(r[:5] == (mode, real, 1024, W, T) for r in SB.ROWS), (mode, real, W, T)
    # the second batch and the launch-geometry rows (test_gpu_spgram_bound.py)
    cap = LQ.spgram_batch_samples()
    assert cap == 1 << 25 and cap // 4096 == 8192 < SB.SECOND_BATCH_N == (1 << 13) + 5
    assert cap // 4 >= SB.GATHER_N == 70000 > 65535 and cap // 2 >= SB.CHUNKS_N == (1 << 22) + (1 << 12)
    assert -(-SB.CHUNKS_N // LQ.spgram_chunk()) > 65536


def test_two_sample_closed_form_is_the_general_reference():
    """The second-batch row's reference (spectra of a two-sample window in
    closed form) against reference() and against the oracle, at 77 transforms."""
    nfft, calls = 64, [(40, 0.3), (37, 0.05)]
    win, x, psd, bound, T = SB.two_sample_case(nfft, calls, 5)
    assert T == 77 and np.max(np.abs(x)) > 0.5 and np.all(np.isfinite(bound)) and np.all(bound > 0)
    w64 = SB.scaled_window(win, nfft)
    ends, a, first = SB.accumulate_plan(2, calls)
    assert first == [0, 40, 77] and np.all(a[:40] == 1.0) and np.all(a[40:] == np.float32(0.05))
    c, c_init = SB.weights(a)
    p2, b2, _ = SB.reference(x, 2, w64, nfft, ends, c, 3.0 * (T - np.arange(T)) + 8.0, c_init, 3.0 * T + 8.0)
    assert np.allclose(psd, p2, rtol=1e-12, atol=0) and np.allclose(bound, b2 + SB.conv(p2), rtol=1e-12, atol=0)
    A, B = SB.two_sample_terms(x, w64, ends[5:6])
    X = SB._spectra(x, 2, w64, nfft, ends[5:6])[0][0]
    assert np.allclose(X, A + B * np.exp(-2j * np.pi * np.arange(nfft) / nfft), rtol=0, atol=1e-15)
    g = O.Spgram(nfft, win)
    g.accumulate_psd(x[:40], 0.3)
    g.accumulate_psd(x[40:], 0.05)
    y = g.write_accumulation()
    assert SB.check_lin(y, psd, bound, "oracle, two-sample window") < 0.1
    z = y.copy()
    z[7] = 10 * np.log10(10 ** (y[7] / 10.0) + 2.0 * bound[7])
    with pytest.raises(AssertionError):
        SB.check_lin(z, psd, bound, "twice the bound in one bin")
    # the row itself: both launch batches carry weight
    ends, a, first = SB.accumulate_plan(2, [(SB.SECOND_BATCH_N, 0.3), (SB.SECOND_BATCH_N, 0.05)])
    c, _ = SB.weights(a)
    assert len(ends) == 2 * 8197 and c[-6] > 1e-2 and c[-5] > 1e-2      # either side of transform 8192 of the call


def test_launch_geometry_cases_are_what_they_say():
    """The oracle meets the bound on the 70000-transform and the 65600-chunk
    cases; bursts on their seams."""
    for c, n, nfft in ((SB.gather_case(), SB.GATHER_N, 4), (SB.chunks_case(), SB.CHUNKS_N, 2)):
        assert c.T == n == len(c.x) and c.nfft == c.W == nfft and np.all(c.ends == np.arange(n))
        assert 0 < SB.oracle_worst(c) < 0.01
        loud = np.abs(c.x) > 0.01
        assert loud[63] and loud[4095] and loud[n - 1] and np.count_nonzero(loud) < 4 * nfft
        assert np.all(c.bound > 0)


# ------------------------------------------------------------- the checker, pinned
PIN = [r for r in SB.ROWS if r[4] in (65, 257) and r[2] in (64, 1024) and r[3] in (48, 512) and not r[1]
       and r[5] in (None, 0.05)]


def _db(lin):
    return 10.0 * np.log10(lin)


@pytest.mark.parametrize("row", PIN, ids=SB.row_id)
def test_checker_fails_on_twice_the_bound_in_one_quiet_bin(row):
    c = SB.case(row)
    good = _db(c.psd64)
    c.check(good, None, "the reference itself")
    k = int(np.argmin(c.psd64))
    z = c.psd64.copy()
    z[k] += 2.0 * c.bound[k]
    r = c.report(_db(z))
    assert r["failing"] == 1 and r["bin"] == k and 1.9 < r["worst"] < 2.1
    with pytest.raises(AssertionError):
        c.check(_db(z))
    if row[7] == "tone":      # linear power normwise, the suite's other comparison, sees nothing
        assert 2.0 * c.bound[k] / np.max(c.psd64) < 1e-6


@pytest.mark.parametrize("row", PIN, ids=SB.row_id)
def test_checker_fails_on_the_margin_and_on_non_finite(row):
    c = SB.case(row)
    y = SB.run_object(O.Spgram(c.nfft, c.window, c.real), c)
    w = SB.oracle_worst(c)
    c.check(y, w, "oracle against itself")
    lin = 10.0 ** (y.astype(np.float64) / 10.0)
    k = int(np.argmin(c.bound))
    z = lin.copy()
    z[k] = c.psd64[k] + 5.0 * w * c.bound[k]       # inside the bound, outside 4 x the oracle
    assert c.report(_db(z))["failing"] == 0
    with pytest.raises(AssertionError):
        c.check(_db(z), w)
    for bad in (np.nan, np.inf, -np.inf):
        z = y.copy()
        z[3] = bad
        with pytest.raises(AssertionError):
            c.check(z, w)


def test_checker_fails_on_the_margin_where_psd_is_one_transform():
    """The yardstick over the last eight transforms still rejects 5 x itself in
    one bin, inside the bound."""
    row = ("accumulate", False, 64, 48, 4097, 1.0, False, "tone")
    assert row in SB.ROWS and SB.single_transform(row)
    c = SB.case(row)
    m = SB.margin_oracle(row, c)
    y = SB.run_object(O.Spgram(c.nfft, c.window, c.real), c)
    c.check(y, m, "oracle")
    k = int(np.argmax(c.psd64))      # the peak bin, where the dB value's rounding sits
    z = 10.0 ** (y.astype(np.float64) / 10.0)
    z[k] = c.psd64[k] + 5.0 * m * c.bound[k]
    assert c.report(_db(z))["failing"] == 0
    with pytest.raises(AssertionError):
        c.check(_db(z), m)


def test_checker_fails_when_a_chunk_is_dropped_or_weighted_as_a_full_one():
    """The two bookkeeping errors the long rows are there for, made on the
    reference: the last, shorter chunk left out of an estimate, and an
    accumulate's last chunk decayed as a full one."""
    row = ("estimate", False, 64, 48, 65, None, False, "bursts")
    c = SB.case(row)
    P = np.abs(SB._spectra(c.x, c.W, c.w64, c.nfft, c.ends)[0]) ** 2
    with pytest.raises(AssertionError):
        c.check(_db(np.roll(np.sum(P[:64], axis=0) / 65, 32)))
    row = ("accumulate", False, 64, 48, 65, 0.05, False, "bursts")
    c = SB.case(row)
    P = np.abs(SB._spectra(c.x, c.W, c.w64, c.nfft, c.ends)[0]) ** 2
    a = float(np.float32(0.05))
    p = P[1]
    for t in range(2, 67):
        p = (1 - a) * p + a * P[t]
    c.check(_db(np.roll(p, 32)), None, "the recursion in float64")
    p = P[1]
    for t in range(2, 66):
        p = (1 - a) * p + a * P[t]
    p = (1 - a) ** 64 * p + a * P[66]      # len = 1 treated as len = 64
    with pytest.raises(AssertionError):
        c.check(_db(np.roll(p, 32)))


def test_window_scale_matches_the_library_and_the_oracle():
    """execute() of an impulse returns the scaled window's last tap, rotated, in every bin:
    checked on the oracle here, on the GPU in test_gpu_spgram_bound.py."""
    for nfft, W in ((64, 48), (1024, 301)):
        win = SB.kaiser_window(W)
        w64 = SB.scaled_window(win, nfft)
        assert abs(np.sum(w64 ** 2) - 2.0 * W / nfft * 1.0) < 1e-5 * 2.0 * W / nfft     # rms(w) = sqrt(2 / nfft)
        g = O.Spgram(nfft, win)
        g.write(np.array([1.0], np.complex64))
        X = g.execute()
        assert np.max(np.abs(np.abs(X) - w64[-1])) <= 2.0 ** -22 * w64[-1]
