"""The oracle meets the frame-local channelizer bound (tests/pfb_bound.py) on
every case the GPU tests run, in one call and in the ragged calls: the bound is
reachable by the reference computation, its worst ratio is printed per shape,
and every output that must be zero is.  The checker is pinned: it passes the
float64 model rounded to float32 and the oracle, and it catches what the
normwise metric of the rest of the suite lets through.  No GPU."""
import numpy as np
import pytest

import golden_io as G
import pfb_bound as PB

ROWS = pytest.mark.parametrize("r", PB.ROWS, ids=PB.row_id)


@pytest.mark.parametrize("name", PB.ENVELOPES)
@ROWS
def test_oracle_meets_bound(r, name):
    c = PB.case(r, name)
    assert c.nb == 3 * r.S + 2 * (2 * PB.window_blocks(r)) + 5
    y, rep = c.oracle()
    print("pfb_bound oracle %s %s: worst ratio %.4g" % (PB.row_id(r), name, rep["worst"]))
    assert rep["failing"] == 0 and rep["nonfinite"] == 0 and rep["nonzero_zeros"] == 0
    assert 0 < rep["worst"] < 1
    assert G.nrm_err(y, c.y64) < 1e-6          # the model is the oracle's computation
    if r.kind == "pfb2":                       # (the firpfbch oracle has one block per call as it is)
        c.check(PB.oracle_run(r, c.h, c.x, PB.cuts(r)), "oracle, ragged calls")


@ROWS
def test_streams_are_what_they_say(r):
    nb, wl, n = PB.n_blocks(r), PB.window_blocks(r), PB.nin(r)
    s = PB.stretches(r.S, wl, nb, r.an)
    b, g = PB.envelope("burst", r), PB.envelope("gaps", r)
    assert len(b) == nb * n and set(np.unique(b)) == {1e-5, 1.0} and set(np.unique(g)) == {0.0, 1.0}
    assert np.array_equal(b == 1.0, g == 1.0)
    loud = (g.reshape(nb, n) == 1.0)
    for k in ("first", "before", "after", "straddle", "last", "window", "single"):
        assert np.all(loud[s[k][0]:s[k][1]]), k
    assert s["first"] == (0, 1) and s["last"] == (nb - 1, nb) and s["before"][1] == min(r.S, nb)
    assert s["after"][0] == r.S + 1 and s["straddle"] == (2 * r.S - 1, 2 * r.S + 2)
    assert s["window"][1] - s["window"][0] == wl
    for k in ("window", "single") + (("mid", "sample") if r.an else ()):   # a quiet block on either side
        assert not loud[s[k][0] - 1].any() and not loud[s[k][1]].any(), k
    if r.an:
        a = s["sample"][0]
        assert np.count_nonzero(loud[a]) == 1 and loud[a, n // 2]
        a = s["mid"][0]
        if n >= 4:   # (M = 2 and 4 have no middle of a block to speak of)
            assert not loud[a, 0] and loud[a, -1] and loud[a + 1, 0] and not loud[a + 1, -1]
    if r.S >= 32 and r.mode != "few":      # room to be far from anything: a window's length either side
        for k in ("window", "single"):
            assert not loud[s[k][0] - wl:s[k][0]].any() and not loud[s[k][1]:s[k][1] + wl].any(), k
    # the ragged calls: both parities, one cut right after the loud window stretch
    cuts = PB.cuts(r)
    assert s["window"][1] in cuts and cuts == sorted(set(cuts)) and 0 < cuts[0] and cuts[-1] < nb
    assert {a & 1 for a in [0] + cuts} == {0, 1}
    if r.mode == "few":
        assert max(np.diff([0] + cuts + [nb])) <= 16 and max(np.diff([0] + PB.few_cuts(r) + [nb])) <= 16
    elif r.S >= 32:                         # the call after the stretch is quiet throughout
        k = cuts.index(s["window"][1])
        assert not loud[cuts[k]:cuts[k + 1]].any() and cuts[k + 1] - cuts[k] > wl


def test_rows_cover_the_dispatch():
    ids = [PB.row_id(r) for r in PB.ROWS]
    assert len(set(ids)) == len(ids)
    an2 = {(r.M, r.q) for r in PB.PFB2_AN}
    assert an2 >= {(2, 1), (8, 2), (12, 3), (4, 1), (64, 9), (1024, 9), (64, 2), (128, 4), (256, 2), (512, 3),
                   (1024, 2), (1024, 4), (1024, 3), (256, 8), (8192, 2), (2048, 2), (4096, 2)}
    assert {(r.M, r.q) for r in PB.PFB2_AN if r.mode == "few"} == {(1024, 2), (1024, 4)}
    assert [(r.M, r.q) for r in PB.PFB2_AN if r.mode == "unaligned"] == [(1024, 4)]
    assert [(r.M, r.q) for r in PB.PFB2_SYN] == [(12, 3), (64, 4), (256, 2), (512, 4), (1024, 2), (1024, 4), (4096, 2)]
    for rows in (PB.PFB_AN, PB.PFB_SYN):
        assert {(r.M, r.q) for r in rows if not r.mode} == {(10, 5), (64, 8), (256, 4), (1024, 4), (1024, 8), (4096, 4)}
        assert {r.M for r in rows if r.mode == "few"} == {1024}
    for an in (True, False):
        assert [(r.M, r.q) for r in PB.PFB_CCCF if r.an == an] == [(64, 4), (256, 4), (4096, 4)]
    assert np.iscomplexobj(PB.taps(PB.PFB_CCCF[0])) and PB.taps(PB.PFB_AN[0]).dtype == np.float32
    h = PB.taps(PB.PFB2_AN[6])
    assert h.dtype == np.float32 and len(h) == 2 * 64 * 2 + 1 and abs(np.sum(h.astype(np.float64)) - 64) < 1e-4


def test_models_follow_the_definitions():
    """The vectorised models against the sums written out, on a few outputs."""
    g = np.random.default_rng(11)
    r = PB.Row("pfb", True, "cccf", 6, 3, 1, None)
    h, x = PB.taps(r), PB.signal(r, "burst")
    y64, _ = PB.pfb_analyzer_model(h, x, 6, 3)
    for b in g.integers(0, PB.n_blocks(r), 6):
        v = np.zeros(6, np.complex128)
        for i in range(6):
            for n in range(3):
                if b - n >= 0:
                    v[i] += complex(h[i + n * 6]) * complex(x[(b - n) * 6 + 5 - i])
        assert np.allclose(y64[b], np.fft.fft(v[::-1]), rtol=0, atol=1e-14)
    r = PB.Row("pfb2", False, "crcf", 8, 2, 1, None)
    h, X = PB.taps(r), PB.signal(r, "burst")
    y64, _ = PB.pfb2_synthesizer_model(h, X, 8, 2)
    z = np.fft.ifft(X.astype(np.complex128).reshape(-1, 8), axis=1) * 4
    for f in g.integers(0, PB.n_blocks(r), 8):
        for i in range(4):
            c, s = i + (f & 1) * 4, 0
            for n in range(4):
                if f - 2 * n >= 0:
                    s += float(h[i + n * 8]) * z[f - 2 * n, c]
                if f - 1 - 2 * n >= 0:
                    s += float(h[i + 4 + n * 8]) * z[f - 1 - 2 * n, c]
            assert abs(y64[f, i] - s) < 1e-13


def _quiet_and_loud(c):
    """Two adjacent quiet frames with content (level under 1e-3 of the
    loudest frame's) and the loudest frame."""
    lv = c.frame_level()
    q = np.flatnonzero((lv[:-1] < 1e-3 * lv.max()) & (lv[1:] < 1e-3 * lv.max()) & (lv[:-1] > 0) & (lv[1:] > 0))
    return int(q[len(q) // 2]), int(np.argmax(lv))


PINNED = [PB.PFB2_AN[6], PB.PFB2_SYN[1]]    # firpfbch2 analyzer (64, 2), synthesizer (64, 4)


@pytest.mark.parametrize("r", PINNED, ids=PB.row_id)
def test_checker_is_pinned(r):
    c = PB.case(r, "burst")
    no = PB.nout(r)
    c.check(c.y64.astype(np.complex64), "model rounded to float32")
    y, rep = c.oracle()
    assert rep["failing"] == 0
    fr = y.reshape(c.nb, no)
    q, loud = _quiet_and_loud(c)
    assert np.max(np.abs(fr[q])) < 1e-3 * np.max(np.abs(fr[loud]))

    # the gap, stated as a test: 1e-6 of a loud frame leaked into a quiet one
    # passes the normwise metric of the parity tests and fails here
    bad = fr.copy()
    bad[q] += np.complex64(1e-6) * fr[loud]
    assert G.nrm_err(bad.reshape(-1), y) < 1e-5 and G.nrm_err(bad.reshape(-1), c.y64) < 1e-5
    rep = PB.report(bad.reshape(-1), c.y64, c.bound)
    assert rep["failing"] > no // 2 and rep["worst"] > 100 and q * no <= rep["index"] < (q + 1) * no
    with pytest.raises(AssertionError, match="outputs fail"):
        c.check(bad.reshape(-1), "leak")

    bad = fr.copy()                          # two adjacent quiet frames swapped
    bad[[q, q + 1]] = fr[[q + 1, q]]
    rep = PB.report(bad.reshape(-1), c.y64, c.bound)
    assert rep["failing"] > no and rep["worst"] > 1000

    bad = y.copy()
    bad[q * no + 3] = np.nan
    rep = PB.report(bad, c.y64, c.bound)
    assert rep["failing"] == 1 and rep["nonfinite"] == 1 and rep["worst"] == np.inf

    # a frame that must be zero
    c = PB.case(r, "gaps")
    y, rep = c.oracle()
    z = np.flatnonzero(c.bound == 0)
    assert rep["failing"] == 0 and rep["zeros"] == len(z) and len(z) >= 20 * no and np.all(y[z] == 0)
    bad = y.copy()
    bad[z[5]] = 1e-30
    rep = PB.report(bad, c.y64, c.bound)
    assert rep["failing"] == 1 and rep["nonzero_zeros"] == 1 and rep["index"] == z[5] and rep["worst"] == np.inf
    with pytest.raises(AssertionError, match="1 outputs that must be zero"):
        c.check(bad, "1e-30 in a zero frame")
    bad[z[5]] = -0.0                         # either sign of zero passes
    assert PB.report(bad, c.y64, c.bound)["failing"] == 0
