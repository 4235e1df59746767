"""tests/fft_bound.py on the CPU: the oracle meets the row-local bounds, the
batches are what the GPU tests need them to be, every row names the kernels
the library takes, and the checkers are pinned.  No GPU.
"""
import numpy as np
import pytest

import fft_bound as FB
import liquidmi as LQ
import oracle_lib as O
from test_gpu_persistent import FFT_G
from test_oracle import r2r_np

ORACLE_ROWS = [r for r in FB.POW2_ROWS if r[0] <= FB.ORACLE_MAX_N]


@pytest.mark.parametrize("kind", FB.KINDS)
@pytest.mark.parametrize("row", ORACLE_ROWS, ids=FB.row_id)
def test_oracle_meets_the_power_of_two_bound(row, kind):
    """Both directions; rigorous but loose: the oracle sits well inside."""
    n, _, rows, _ = row
    for d in (+1, -1):
        w = FB.oracle_worst(n, kind, rows, d)
        assert w < 0.1
        assert n == 1 or w > 0


@pytest.mark.parametrize("kind", FB.EXACT)
@pytest.mark.parametrize("n", [2, 64, 1024, 65536])
def test_oracle_meets_the_bound_on_exact_structure(n, kind):
    c = FB.case(n, kind, 5)
    c.check(FB.oracle_rows(O, c.X, +1), +1, what="oracle")


@pytest.mark.parametrize("row", [r for r in FB.OTHER_ROWS if r[0] <= 12288], ids=FB.row_id)
def test_oracle_meets_the_other_bounds(row):
    """Direct-DFT and Bluestein sizes: the oracle runs another algorithm, so
    the ratio is printed, the bound asserted."""
    n, _, rows, _ = row
    c = FB.case(n, "noise", min(FB.n_rows(n, rows), 9))
    for d in (+1, -1):
        c.check(FB.oracle_rows(O, c.X, d), d, what="oracle")


def test_bluestein_factor_is_what_the_docstring_derives():
    for n in (17, 1000, 2049):
        M = FB.bluestein_M(n)
        mx, nrm = FB.chirp_spectrum(n)
        assert M >= 2 * n - 1 > M // 2
        assert abs(nrm - np.sqrt(M * (2 * n - 1))) < 1e-6 * nrm      # Parseval: |b_j| = 1 on 2n - 1 entries
        assert np.sqrt(2 * n - 1) <= mx <= 2 * n - 1
        assert FB.row_factor(n) > 4 * np.log2(M) * np.sqrt(M * (2 * n - 1))      # the ||B||_2 term alone
    assert FB.row_factor(1024) == 48 * 32 and FB.row_factor(15) == 19 * np.sqrt(15)


def test_rows_name_the_kernels_the_library_takes():
    for n, route, rows, loops in FB.POW2_ROWS + FB.OTHER_ROWS:
        assert LQ.fft_route(n, True) == route, n
        # only the two largest one-pass kernels look at the alignment
        assert (LQ.fft_route(n, False) == route) == (n not in (8192, 16384)), n
        if loops and n & (n - 1) == 0:
            assert n in FFT_G and FB.group(n) == FFT_G[n]
        if "bluestein M=" in route:     # its M-point transforms run a looping kernel of FFT_G
            M = FB.bluestein_M(n)
            assert route == "bluestein M=%d" % M and M in FFT_G and FB.group(n) == FFT_G[M]
            assert LQ.fft_route(M).split("<")[0] in ("fftsmall", "fftr16")
    for n, route in FB.OFF8_ROWS:
        assert LQ.fft_route(n, False) == route
    # every family the route can return has a row
    names = {LQ.fft_route(n, a).split(" ")[0].split("<")[0].split("/")[0]
             for n, *_ in FB.POW2_ROWS + FB.OTHER_ROWS for a in (True, False)}
    assert names == set(LQ.FFT_FAMILIES) - {"refused"}
    # and every instantiation: the sizes each family takes
    assert {n for n, r, *_ in FB.POW2_ROWS if r.startswith("k_fft_batch")} == {2, 4, 8, 16}
    assert {n for n, r, *_ in FB.POW2_ROWS if r.startswith("fftsmall")} == {32, 64, 128}
    assert {n for n, r, *_ in FB.POW2_ROWS if r.startswith("fftr16")} == {256, 512, 2048}
    cols = {p for _, r, *_ in FB.POW2_ROWS for p in r.split(" ") if p.startswith("cols_r")}
    assert cols == {"cols_r<%d>" % k for k in (1, 2, 8, 16)}     # cols_r<4>: n = 2^19, 2^20 (test_gpu_parity) and 3 2^17 here
    assert any("cols_r<4>" in r for _, r, *_ in FB.OTHER_ROWS)
    assert any("cols_s<8>" in r for _, r, *_ in FB.OTHER_ROWS)
    # the thresholds between the families, from the launch's own decision
    assert LQ.fft_route(16384).startswith("fft16384") and LQ.fft_route(32768).startswith("four_step")
    assert LQ.fft_route(16) == "k_fft_batch<16>" and LQ.fft_route(17) == "bluestein M=64"
    assert LQ.fft_route(2048 + 0) == "fftr16<8>" and LQ.fft_route(2049).startswith("bluestein_fused M=8192")
    assert LQ.fft_route(2048 - 1) == "bluestein M=4096"
    assert LQ.fft_route(1 << 24).startswith("four_step 4096x4096") and LQ.fft_route((1 << 24) + 1) == "refused"
    assert LQ.fft_route((1 << 23) + 1) == "refused" and LQ.fft_route(0) == "refused"


@pytest.mark.parametrize("row", FB.POW2_ROWS + FB.OTHER_ROWS, ids=FB.row_id)
def test_batches_are_what_they_say(row):
    n, _, rows, loops = row
    G, B = FB.group(n), FB.n_rows(n, rows)
    if rows is None:
        assert B == 3 * G * 2 + G + 1
    lv, Z = FB.levels(n, B), FB.zero_rows(n, B)
    if B >= 3:
        assert 1 in Z and Z[0] < G + (G == 1) * 2     # inside the first group (its own row when G = 1)
    if B >= 5:
        assert len(Z) == 2 and Z[1] // G == 3          # group 3: the second of workgroup 0 of three
        assert G == 1 or Z[1] % G == 1
    if B >= 2:
        assert np.count_nonzero(lv == 1.0) >= 1 and np.count_nonzero(lv == FB.QUIET) >= 1
    if n <= 16384:                                      # the large rows: the other inputs on the GPU only
        for kind in FB.KINDS + FB.EXACT:
            X = FB.case(n, kind, rows).X
            assert X.shape == (B, n) and X.dtype == np.complex64
            nrm = np.sqrt(np.sum(np.abs(X.astype(np.complex128)) ** 2, axis=1))
            assert np.all((nrm == 0) == (lv == 0))
            bnd = FB.case(n, kind, rows).bound
            assert np.all((bnd == 0) == (lv == 0))
            q, f = nrm[lv == FB.QUIET], nrm[lv == 1.0]
            if len(q) and (kind in ("ones", "impulse", "tone") or (kind == "noise" and n >= 64)):
                assert np.max(q) < 2.0 ** -15 * np.min(f)
    if n >= 64 and n <= 16384:
        X = FB.case(n, "tone", rows).X.astype(np.complex128)
        S = np.abs(np.fft.fft(X[0])) ** 2
        assert np.argmax(S) == n // 3 and np.max(S) / np.median(S) > 10 ** 9     # over 90 dB in one row
        Xb = FB.case(n, "burst", rows).X
        assert np.count_nonzero(np.abs(Xb[0]) > 1e-4) <= n // 64


# ------------------------------------------------------------- the checker, pinned
PIN = pytest.mark.parametrize("n", [16, 64, 1024, 4096, 32768])


def _good(n, kind="noise"):
    rows = dict((r[0], r[2]) for r in FB.POW2_ROWS)[n]
    c = FB.case(n, kind, rows)
    y = FB.oracle_rows(O, c.X, +1)
    w = FB.oracle_worst(n, kind, rows, +1)
    c.check(y, +1, w, what="unharmed")
    return c, y, w


def _quiet_row(c):
    return int(np.flatnonzero(FB.levels(c.n, c.rows) == FB.QUIET)[0])


@PIN
def test_checker_fails_on_twice_the_bound_in_one_bin_of_one_quiet_row(n):
    """Normwise over the batch that is 2^-17 of nothing: 1e-10."""
    c, y, w = _good(n)
    b = _quiet_row(c)
    z = y.copy()
    z[b, n // 2] += np.complex64(2.0 * c.bound[b])
    r = FB.report(z, c.y64(+1), c.bound)
    assert r["failing"] == [b] and 1.5 < r["worst"] < 2.5
    with pytest.raises(AssertionError):
        c.check(z, +1)
    assert np.max(np.abs(z - y)) / np.max(np.abs(y)) < 1e-6   # what a normwise check would see


@PIN
def test_checker_fails_on_a_quiet_row_with_a_loud_rows_rounding_noise(n):
    """Passes the bound's first assertion or not; the margin catches it:
    2^-24 max |Y| added to a quiet row."""
    c, y, w = _good(n)
    b = _quiet_row(c)
    z = y.copy()
    z[b] += np.float32(2.0 ** -24 * np.max(np.abs(y)))
    with pytest.raises(AssertionError):
        c.check(z, +1, w)


@PIN
def test_checker_fails_on_a_tiny_value_in_a_zero_row(n):
    c, y, w = _good(n)
    b = FB.zero_rows(n, c.rows)[0]
    assert np.all(y[b] == 0)
    z = y.copy()
    z[b, 1] = 1e-30
    r = FB.report(z, c.y64(+1), c.bound)
    assert r["failing"] == [b] and r["nonzero_zeros"] == 1
    with pytest.raises(AssertionError):
        c.check(z, +1, w)
    z[b, 1] = -0.0
    c.check(z, +1, w)


def test_checker_fails_on_nan_and_on_swapped_rows():
    c, y, w = _good(1024)
    z = y.copy()
    z[2, 5] = np.nan
    assert FB.report(z, c.y64(+1), c.bound)["nonfinite"] == 1
    with pytest.raises(AssertionError):
        c.check(z, +1, w)
    z = y.copy()
    z[[0, 4]] = z[[4, 0]]
    with pytest.raises(AssertionError):
        c.check(z, +1)


# ------------------------------------------------------------------ real-to-real
def _r2r_ref(typ, X):
    return np.stack([r2r_np(typ, x) for x in X])


@pytest.mark.parametrize("n", FB.R2R_SIZES)
def test_r2r_bound_and_checker(n):
    """The float32 rounding of the float64 formula meets the bound with room;
    one ulp more in a quiet row does not."""
    X = FB.r2r_input(n)
    assert np.all(X[2] == 0) and np.max(np.abs(X[1])) <= FB.QUIET * 0.5 and np.max(np.abs(X[0])) > (0.01 if n < 3 else 0.3)
    for typ in FB.R2R_TYPES:
        Y64 = _r2r_ref(typ, X)
        bnd = FB.r2r_bound(X, Y64)
        assert np.all(bnd[2] == 0) and np.all(Y64[2] == 0)
        y = Y64.astype(np.float32)
        r = FB.r2r_check(y, Y64, bnd, "rounded float64 type %d n=%d" % (typ, n))
        assert r["worst"] <= 1.0
        z = y.copy()
        k = int(np.argmax(np.abs(y[1])))
        z[1, k] = np.nextafter(np.nextafter(z[1, k], np.float32(np.inf)), np.float32(np.inf))
        with pytest.raises(AssertionError):
            FB.r2r_check(z, Y64, bnd, "two ulps off")
        z = y.copy()
        z[2, 0] = 1e-30
        with pytest.raises(AssertionError):
            FB.r2r_check(z, Y64, bnd, "nonzero zero")
