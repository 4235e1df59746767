"""The oracle meets the per-output firfilt bound (tests/fir_bound.py) on every
case the GPU tests run: the bound is reachable by the reference computation,
and the checker is pinned -- it passes the direct form and catches the errors
a transform leaves on quiet outputs.  No GPU."""
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
