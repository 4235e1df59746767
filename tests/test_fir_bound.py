"""The oracle meets the per-output firfilt bound (tests/fir_bound.py) on every
case the GPU tests run: the bound is reachable by the reference computation,
and the checker is pinned -- it passes the direct form and catches the errors
a transform leaves on quiet outputs.  The same for the decimator: the oracle's
FirDecim on the small versions of the cases of tests/test_gpu_persistent.py,
and the checker against a repeated tile.  No GPU."""
import numpy as np
import pytest

import fir_bound as FB
import oracle_lib as O

TYPES = {"rrrf": O.RRRF, "crcf": O.CRCF, "cccf": O.CCCF}


def _oracle(c, cuts=()):
    o = O.FirFilt(TYPES[c.t], c.h)
    o.set_scale(c.s)
    return np.concatenate([o.execute_block(p) for p in np.split(c.x, list(cuts))])


@pytest.mark.parametrize("name", FB.ENVELOPES)
@pytest.mark.parametrize("f", FB.FILTERS, ids=FB.filter_id)
def test_oracle_meets_bound(f, name):
    c = FB.case(f[0], f[1], name)
    assert len(c.x) == 3 * FB.seg_len(f[1]) + 777
    c.check(_oracle(c))


@pytest.mark.parametrize("f", FB.FILTERS, ids=FB.filter_id)
def test_oracle_meets_bound_carried_history(f):
    c = FB.carried_case(*f)
    n1, n2 = FB.carried_split(f[1])
    assert n2 >= 8192 and np.max(np.abs(c.x[n1:])) < 1e-5 and np.max(np.abs(c.x[n1 - 300:n1])) > 0.4
    c.check(_oracle(c, cuts=(n1,)))


@pytest.mark.parametrize("small", [False, True], ids=["2p98", "2m58"])
def test_oracle_meets_bound_extreme_range(small):
    c = FB.overflow_case(small)
    y = _oracle(c)
    assert np.all(np.isfinite(y))
    if not small:
        assert abs(y[-1] - 129 * 2.0 ** 111) <= 1e-6 * 129 * 2.0 ** 111   # 3.3e35
    c.check(y)


DECIM_CASES = [(t, M, hlen) for M, hlen in FB.DECIM_ROWS for t in ("rrrf", "crcf", "cccf")] + [FB.DECIM_PLAIN]


@pytest.mark.parametrize("name", ["burst", "gaps"])
@pytest.mark.parametrize("f", DECIM_CASES, ids=lambda f: "%s-M%d-h%d" % f)
def test_oracle_decim_meets_bound(f, name):
    """The small versions of the decimator cases: one call, calls of 100
    outputs, and two calls cut where the loud burst stays in the history."""
    t, M, hlen = f
    nout, cut = FB.DECIM_SMALL
    c = FB.decim_case(t, M, hlen, name, nout, cut)
    assert len(c.x) == nout * M and np.max(np.abs(c.x[cut * M:(cut + 1) * M + 40])) <= 1e-5
    assert np.max(np.abs(c.x[cut * M - 300:cut * M])) > 0.4
    for cuts in ((), range(100, nout, 100), (cut,)):
        o = O.FirDecim(TYPES[t], M, c.h)
        c.check(np.concatenate([o.execute_block(p) for p in np.split(c.x, [k * M for k in cuts])]))


def test_decim_reference_and_envelope_are_what_they_say():
    r = np.random.default_rng(5)
    for t, M, hlen in (("rrrf", 3, 7), ("crcf", 4, 4), ("cccf", 5, 23), ("crcf", 1, 6)):
        h, x = FB.signal(t, hlen, "pin", np.ones(40 * M + 2))
        y64, A = FB.decim_reference(t, h, x, M)
        assert len(y64) == (40 * M + 2) // M and len(A) == len(y64)
        for o in r.integers(0, 40, 12):
            k = np.arange(min(hlen, o * M + 1))
            assert abs(y64[o] - np.sum(h[k].astype(np.complex128) * x[o * M - k])) <= 1e-15 * A[o]
            a = np.sum(np.abs(h[k].astype(np.complex128)) * np.abs(x[o * M - k].astype(np.complex128)))
            assert abs(A[o] - a) <= 1e-15 * A[o]
    M, nout, cut = 8, 70001 + 143, 2500
    e = FB.decim_envelope("gaps", M, nout, cut)
    a, b = 256 * M, 512 * M
    assert len(e) == nout * M and set(np.unique(e)) == {0.0, 1.0}
    assert e[a] == 1.0 and e[a + 1] == 0.0 and e[b - 1] == 1.0 and e[b - 2] == 0.0
    assert e[3 * a] == 0.0 and e[3 * a + 1] == 1.0 and e[2 * b - 2] == 1.0 and e[2 * b - 1] == 0.0
    assert e[5 * a - 1] == 0.0 and e[5 * a] == 1.0 and e[5 * a + 1] == 0.0
    mid = (nout // 512 // 2) * b
    assert mid % b == 0 and list(e[mid - 2:mid + 2]) == [0.0, 1.0, 1.0, 0.0]
    assert e[cut * M - 1] == 1.0 and np.all(e[cut * M:cut * M + 2000] == 0.0) and e[-1] == 1.0
    assert np.array_equal(FB.decim_envelope("burst", M, nout, cut) == 1.0, e == 1.0)


def test_checker_catches_a_decimator_tile_fault():
    # what a persistent loop that repeats or drops a tile leaves: one tile's
    # outputs taken from the tile before, and a quiet tile filled from a loud one
    t, M, hlen = "crcf", 8, 128
    nout, cut = FB.DECIM_SMALL
    c = FB.decim_case(t, M, hlen, "burst", nout, cut)
    y = O.FirDecim(TYPES[t], M, c.h).execute_block(c.x)
    c.check(y)
    bad = y.copy()
    bad[1024:1536] = y[512:1024]
    r = FB.report(t, hlen, bad, c.y64, c.A)
    assert r["failing"] > 400 and r["worst"] > 100
    bad = y.copy()
    bad[700] = y[701]   # two quiet neighbours swapped for one another
    assert FB.report(t, hlen, bad, c.y64, c.A)["failing"] == 1


def test_envelopes_are_what_they_say():
    L = FB.seg_len(129)
    assert L == 3968 and FB.seg_len(2049) == 2048 and FB.seg_len(2050) == 6142 and FB.seg_len(2051) == 6142
    b, g = FB.envelope("burst", 129), FB.envelope("gaps", 129)
    loud = np.flatnonzero(b == 1.0)
    assert len(loud) == 40 + 300 + 100 + 1 and loud[-1] == 2 * L + 1000 and b[L - 50] == 1.0 and b[L + 50] == 1e-5
    assert np.array_equal(b == 1.0, g == 1.0) and np.all(g[b != 1.0] == 0.0)
    s = FB.envelope("stairs", 129)
    assert [s[400 * i] for i in range(12)] == [1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, 1e-1]
    t = FB.envelope("two-level-3", 129)
    assert t[0] == 1.0 and t[L // 2 - 1] == 1.0 and t[L // 2] == 0.125 and t[L - 1] == 0.125 and t[L] == 1.0
    assert np.all(FB.envelope("flat", 129) == 1.0)


def test_checker_catches_what_a_transform_leaves():
    # the oracle's output, then the two defects of a transform's rounding
    # noise: an output that must be exactly zero at 1e-7, and a quiet output
    # off by a loud neighbour's float32 rounding
    c = FB.case("crcf", 129, "gaps")
    y = _oracle(c)
    z = np.flatnonzero(c.A == 0)
    assert len(z) > 9000 and np.all(y[z] == 0)
    bad = y.copy()
    bad[z[5]] = 1e-7
    r = FB.report(c.t, c.hlen, bad, c.y64, c.A)
    assert r["failing"] == 1 and r["nonzero_zeros"] == 1 and r["index"] == z[5] and r["worst"] == np.inf
    bad[z[5]] = -0.0   # either sign of zero passes
    assert FB.report(c.t, c.hlen, bad, c.y64, c.A)["failing"] == 0
    with pytest.raises(AssertionError, match="1 outputs that must be zero"):
        bad[z[7]] = 1e-30
        c.check(bad)

    c = FB.case("crcf", 129, "burst")
    y = _oracle(c)
    q = 1000   # sees only 1e-5-level inputs
    assert c.A[q] < 1e-3 * np.max(c.A)
    bad = y.copy()
    bad[q] += np.float32(2.0 ** -24 * np.max(np.abs(y)))
    r = FB.report(c.t, c.hlen, bad, c.y64, c.A)
    assert r["failing"] == 1 and r["index"] == q and r["worst"] > 10 and r["nonzero_zeros"] == 0
    bad = y.copy()
    bad[q + 1] = np.inf
    r = FB.report(c.t, c.hlen, bad, c.y64, c.A)
    assert r["failing"] == 1 and r["nonfinite"] == 1
