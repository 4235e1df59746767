"""The FFT plan API's kernels against error bounds local to each row
(tests/fft_bound.py), one row per kernel the dispatch reaches (`-m gpu`).

Every batch holds full-scale rows, rows at 2^-17 and rows of zeros -- one
inside the first group of rows a workgroup transforms together, one inside
the group a workgroup of three walks to second -- and each row of the batch is
held to a bound in its own 2-norm: (4 lg n + 8) 2^-23 sqrt(n) ||x_b||_2 for the
powers of two, the Bluestein and direct-DFT bounds derived in fft_bound.py for
the rest, exact zeros for a row of zeros.  On noise, a bin-centred tone over a
1e-5 floor and a burst over that floor the worst ratio must also stay within
4 x the oracle's on the same batch (n up to 2^17); an impulse and an all-ones
row get the bound only.  Each row asserts through liquid_mi355x_fft_route, the
launch's own decision, that it reaches the kernels it names.  Everything runs
through fft_execute_batch_dev, in place and out of place, forward and
backward, at the full grid and, where the kernel loops, at three workgroups.

The real-to-real transforms (all eight types) are held to one rounding of the
float64 formula.  Two launches put 70000 rows on grid.y; the kernels stride
over what the launch caps (csrc/lq_device.h: LQ_GRID_Y_MAX), and the values
are asserted like any other row's.
"""
import time

import numpy as np
import pytest

import fft_bound as FB
import liquidmi as LQ
from test_oracle import r2r_np

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 3], ids=["full-grid", "three-workgroups"])
def workgroups(request):
    LQ.set_max_workgroups(request.param)
    try:
        yield request.param
    finally:
        LQ.set_max_workgroups(0)


def _run(X, direction, in_place, off=0, r2r=None):
    """fft_execute_batch_dev over the rows of X; rows `off` bytes past a 16-byte boundary."""
    L = LQ.lib()
    rows, n = X.shape
    bx = LQ.DeviceBuffer(X.nbytes + 32)
    by = bx if in_place else LQ.DeviceBuffer(X.nbytes + 32)
    assert bx.p % 16 == 0 and by.p % 16 == 0
    L.liquid_mi355x_memcpy_h2d(bx.p + off, LQ.ptr(X), X.nbytes)
    q = L.fft_create_plan(n, None, None, direction, 0) if r2r is None else L.fft_create_plan_r2r_1d(n, None, None, r2r, 0)
    try:
        L.fft_execute_batch_dev(q, bx.p + off, by.p + off, rows)
        L.liquid_mi355x_device_synchronize()
    finally:
        L.fft_destroy_plan(q)
    Y = np.empty_like(X)
    L.liquid_mi355x_memcpy_d2h(LQ.ptr(Y), by.p + off, Y.nbytes)
    bx.free()
    by.free()
    return Y


def _oracle(n, kind, rows, d):
    return FB.oracle_worst(n, kind, rows, d) if n & (n - 1) == 0 and n <= FB.ORACLE_MAX_N and kind in FB.KINDS else None


def _row_runs(n, kind, rows, wg, off=0):
    c = FB.case(n, kind, rows)
    for d in (+1, -1):
        for in_place in (True, False):
            what = "wg=%d %s%s" % (wg, "in place" if in_place else "out of place", " off8" if off else "")
            c.check(_run(c.X, d, in_place, off), d, _oracle(n, kind, rows, d), what)


SMALL = [r for r in FB.POW2_ROWS + FB.OTHER_ROWS if r[0] <= 1 << 17 or r[0] == 12288]
LARGE = [r for r in FB.POW2_ROWS + FB.OTHER_ROWS if r not in SMALL]


@pytest.mark.parametrize("kind", FB.KINDS + FB.EXACT)
@pytest.mark.parametrize("row", SMALL, ids=FB.row_id)
def test_fft_rows_hold_their_own_bound(row, kind):
    """At the full grid."""
    n, route, rows, loops = row
    assert LQ.fft_route(n, True) == route and LQ.get_max_workgroups() == 0
    _row_runs(n, kind, rows, 0)


@pytest.fixture
def three_workgroups():
    LQ.set_max_workgroups(3)
    try:
        yield 3
    finally:
        LQ.set_max_workgroups(0)


@pytest.mark.parametrize("kind", FB.KINDS + FB.EXACT)
@pytest.mark.parametrize("row", [r for r in SMALL if r[3]], ids=FB.row_id)
def test_fft_rows_hold_their_own_bound_at_three_workgroups(row, kind, three_workgroups):
    """The kernels that loop: each of three workgroups walks two or three groups of rows."""
    n, route, rows, loops = row
    assert LQ.fft_route(n, True) == route
    _row_runs(n, kind, rows, three_workgroups)


@pytest.mark.parametrize("kind", FB.KINDS)
@pytest.mark.parametrize("row", FB.OFF8_ROWS, ids=FB.row_id)
def test_fft_rows_on_8_byte_loads(row, kind, workgroups):
    n, route = row
    assert LQ.fft_route(n, False) == route
    _row_runs(n, kind, None, workgroups, off=8)


@pytest.mark.parametrize("row", LARGE, ids=FB.row_id)
def test_fft_large_rows_hold_their_own_bound(row):
    """n = 2^21 (two rows: full scale and 2^-17), 2^23 (one row, 64 MB) and
    3 2^17 (M = 2^20; full scale, zeros, 2^-17): noise forward in place and
    out of place, a tone backward in place."""
    n, route, rows, _ = row
    assert LQ.fft_route(n, True) == route
    for kind, d, in_place in (("noise", +1, True), ("noise", +1, False), ("tone", -1, True)):
        c = FB.case(n, kind, rows)
        t0 = time.time()
        Y = _run(c.X, d, in_place)
        t1 = time.time()
        c.check(Y, d, None, "%s, %.2f s with copies" % ("in place" if in_place else "out of place", t1 - t0))


# ------------------------------------------------------------------ real-to-real
def _r2r_ref(typ, X):
    return np.stack([r2r_np(typ, x) for x in X])


@pytest.mark.parametrize("typ", FB.R2R_TYPES)
@pytest.mark.parametrize("n", FB.R2R_SIZES)
def test_r2r_rows_hold_one_rounding_of_the_float64_formula(n, typ):
    """Three rows (full scale, 2^-17, zeros), in place (the staged copy) and out of place."""
    X = FB.r2r_input(n)
    Y64 = _r2r_ref(typ, X)
    bnd = FB.r2r_bound(X, Y64)
    for in_place in (True, False):
        FB.r2r_check(_run(X, 0, in_place, r2r=typ), Y64, bnd,
                     "type %d n=%d %s" % (typ, n, "in place" if in_place else "out of place"))


# ------------------------------------------------------------------ launch geometry
def test_fft_70000_rows_of_17_points():
    """Bluestein with M = 64: k_bs_pre, k_bs_mul and k_bs_post carry the batch
    on grid.y, capped at 65535 and strided over.  Every row against its bound."""
    n, rows = 17, FB.BIG_BATCH
    assert LQ.fft_route(n) == "bluestein M=64"
    c = FB.case(n, "noise", rows)
    assert np.count_nonzero(c.bound[65535:]) > 2000 and c.bound[FB.zero_rows(n, rows)[1]] == 0
    c.check(_run(c.X, +1, True), +1, None, "70000 rows in place")


def test_r2r_70000_rows_of_3_points():
    n, rows = 3, FB.BIG_BATCH
    X = FB.r2r_input(n, rows)
    for typ in (11, 20):
        i, k = np.arange(n)[:, None], np.arange(n)[None, :]
        K = np.cos(np.pi * (k + 0.5) * i / n) if typ == 11 else np.sin(np.pi * (k + 1) * (i + 1) / (n + 1))
        Y64 = 2.0 * X.astype(np.float64) @ K.T
        assert np.allclose(Y64[:3], _r2r_ref(typ, X[:3]), rtol=0, atol=1e-15)
        FB.r2r_check(_run(X, 0, True, r2r=typ), Y64, FB.r2r_bound(X, Y64), "type %d, 70000 rows in place" % typ)
