"""tests/interp_bound.py on the CPU: the oracle meets the bound on every row
and cut (the bound is reachable), the envelopes are what they say, the route
table is the launch's own, and the checker is pinned -- it fails on the faults
the GPU tests are there to catch.  No GPU.
"""
import numpy as np
import pytest

import interp_bound as IB
import liquidmi as LQ
import oracle_lib as O

TYPES = {"rrrf": O.RRRF, "crcf": O.CRCF, "cccf": O.CCCF}
ROWS = pytest.mark.parametrize("row", IB.ROWS, ids=IB.row_id)


def _oracle(c, cuts=()):
    o = O.FirInterp(TYPES[c.t], c.M, c.h)
    edges = [0] + list(cuts) + [len(c.x)]
    return np.concatenate([o.execute_block(c.x[a:b]) for a, b in zip(edges[:-1], edges[1:])])


def _oracle_pfb(c):
    o = O.FirPfb(TYPES[c.t], c.M, c.h)
    o.set_scale(c.s)
    y = np.zeros(len(c.x) * c.M, c.x.dtype)
    for t, v in enumerate(c.x):
        o.push(v)
        for i in range(c.M):
            y[t * c.M + i] = o.execute(i)
    return y


@pytest.mark.parametrize("name", IB.ENVELOPES)
@ROWS
def test_oracle_meets_the_bound_however_cut(row, name):
    c = IB.case(row[0], row[1], row[2], name)
    for cuts in ((), IB.CUTS, (IB.CARRIED_CUT,), range(7, IB.N, 7)):
        r = c.check(_oracle(c, cuts))
        assert r["worst"] < 0.5   # room: a kernel at the bound is not this computation
        if name == "gaps":
            assert r["nonzero_zeros"] == 0


@ROWS
def test_oracle_meets_the_bound_on_carried_history(row):
    c = IB.case(row[0], row[1], row[2], "carried")
    assert c.check(_oracle(c, (IB.CARRIED_CUT,)))["worst"] < 0.5


@pytest.mark.parametrize("row", IB.PFB_ROWS, ids=IB.row_id)
def test_oracle_firpfb_meets_the_bound(row):
    t, M, hlen, s, _ = row
    if t == "cccf":
        s = abs(s)   # the oracle's scale is real; the complex one runs on the GPU, against its own y64
    c = IB.case(t, M, hlen, "burst", s, True)
    assert c.L == hlen // M
    assert c.check(_oracle_pfb(c))["worst"] < 0.5


@ROWS
def test_envelopes_are_what_they_say(row):
    t, M, hlen, _ = row
    L = IB.taps_per_phase(M, hlen)
    assert M * (L - 1) < hlen <= M * L
    loud = [0, 1, 2, 60, 64, 255, 256, 300, 512 - L, 511, IB.N - 2, IB.N - 1]
    quiet = [3, 59, 65, 254, 257, 299, 301, 511 - L, 512, IB.N - 3]
    for name, floor in (("burst", 1e-5), ("gaps", 0.0)):
        e = IB.envelope(name, L)
        assert len(e) == IB.N == 3 * 256 + 77 and IB.N % 2 == 1
        assert np.all(e[loud] == 1.0) and np.all(e[quiet] == floor)
        assert np.count_nonzero(e == 1.0) == 3 + 5 + 2 + 1 + L + 2
        c = IB.case(t, M, hlen, name)
        assert np.all(c.x[e == 0] == 0) and np.max(np.abs(c.x[e == floor])) <= max(floor, 1e-30)
    # gaps: outputs whose L inputs are all zero have A == 0 exactly, and there are many
    c = IB.case(t, M, hlen, "gaps")
    assert np.count_nonzero(c.A == 0) > len(c.A) // 2
    assert np.all(c.y64[c.A == 0] == 0)
    # carried: nothing loud from the cut on, something loud within L - 1 before it
    e = IB.envelope("carried", L)
    assert np.all(e[IB.CARRIED_CUT:] == 1e-5) and e[IB.CARRIED_CUT - 1] == 1.0


def test_cuts_start_shorter_than_the_history():
    assert IB.CUTS == (1, 64, 65, 320) and IB.CARRIED_CUT == 500
    assert max(IB.taps_per_phase(M, h) for _, M, h, _ in IB.ROWS) - 1 > 1


def test_route_table_is_the_launch_decision():
    for t, M, hlen, route in IB.ROWS:
        assert LQ.firinterp_route(t, M, IB.taps_per_phase(M, hlen)) == route, (t, M, hlen)
    for t, M, hlen in IB.UNALIGNED_ROWS:
        L = IB.taps_per_phase(M, hlen)
        assert LQ.firinterp_route(t, M, L, True) != 0 and LQ.firinterp_route(t, M, L, False) == 0
    for t, M, hlen, _, route in IB.PFB_ROWS:
        assert LQ.firinterp_route(t, M, IB.taps_per_phase(M, hlen, True)) == route
    # every class is reached, and the LDS edges are where the rows say
    assert {r[3] for r in IB.ROWS} == {0, 8, 12, 16, 20, 24, 32}
    assert LQ.firinterp_route("crcf", 30, 8) == 8 and LQ.firinterp_route("crcf", 31, 8) == 0
    assert LQ.firinterp_route("rrrf", 61, 8) == 8 and LQ.firinterp_route("rrrf", 62, 8) == 0
    assert LQ.firinterp_route("crcf", 32, 2) == 0   # the suite's older "(32, 2)" row: plain, by LDS
    assert LQ.firinterp_route("rrrf", 64, 2) == 0 and LQ.firinterp_route("rrrf", 65, 2) == 0


def test_max_taps_is_the_plain_kernels_lds():
    # (256 + L) samples within the kernels' dynamic LDS budget of 159 KB
    for t, esz in (("rrrf", 4), ("crcf", 8), ("cccf", 8)):
        L = LQ.firinterp_max_taps(t)
        assert (256 + L) * esz <= 159 * 1024 < (256 + L + 1) * esz


# ------------------------------------------------------------- the checker, pinned
def _good(c):
    y = _oracle(c)
    assert c.report(y)["failing"] == 0
    return y


@pytest.mark.parametrize("row", [IB.ROWS[2], IB.ROWS[4], IB.ROWS[12]], ids=IB.row_id)
def test_checker_fails_on_swapped_phases_in_a_quiet_stretch(row):
    c = IB.case(row[0], row[1], row[2], "burst")
    y = _good(c).reshape(-1, c.M).copy()
    q = slice(100, 200)   # floor-level inputs: 1e-5 of the stream's largest output
    y[q, 0], y[q, 1] = y[q, 1].copy(), y[q, 0].copy()
    y = y.reshape(-1)
    assert np.max(np.abs(y - c.y64)) < 1e-4 * np.max(np.abs(c.y64))   # a normwise 1e-5-of-range check sees ~nothing
    with pytest.raises(AssertionError):
        c.check(y)
    assert c.report(y)["failing"] >= 100


@pytest.mark.parametrize("name", IB.ENVELOPES)
@pytest.mark.parametrize("row", [IB.ROWS[0], IB.ROWS[5]], ids=IB.row_id)
def test_checker_fails_on_a_wave_repeated_from_the_wave_before(row, name):
    c = IB.case(row[0], row[1], row[2], name)
    y = _good(c).copy()
    w = 64 * c.M
    for k in (1, 2):   # wave 1 from wave 0 (loud into quiet); wave 2 from wave 1 (quiet into quiet)
        z = y.copy()
        z[k * w:(k + 1) * w] = y[(k - 1) * w:k * w]
        with pytest.raises(AssertionError):
            c.check(z)


def test_checker_fails_on_a_tiny_value_where_zero_is_due():
    c = IB.case("crcf", 4, 45, "gaps")
    y = _good(c).copy()
    k = int(np.flatnonzero(c.A == 0)[5])
    y[k] = 1e-30
    r = c.report(y)
    assert r["failing"] == 1 and r["nonzero_zeros"] == 1 and r["index"] == k
    with pytest.raises(AssertionError):
        c.check(y)


def test_checker_fails_on_nan():
    c = IB.case("rrrf", 5, 100, "burst")
    y = _good(c).copy()
    y[1234] = np.nan
    assert c.report(y)["nonfinite"] == 1
    with pytest.raises(AssertionError):
        c.check(y)
