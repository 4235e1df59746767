"""The oracle meets the frame-local channelizer bound (tests/pfb_bound.py) on
every case the GPU tests run, in one call and in the ragged calls: the bound is
reachable by the reference computation, its worst ratio is printed per shape,
and every output that must be zero is.  The checker is pinned: it passes the
float64 model rounded to float32 and the oracle, and it catches what the
normwise metric of the rest of the suite lets through.

The second half holds the rows to the launches: every call of every row takes
the route the row names and walks runs of the row's S blocks
(liquidmi.firpfbch2_route / firpfbch_route, the launches' own decision, which
needs no GPU), the rows reach every route there is, the run formulas are what
they were before their workgroup targets became adjustable, and the limit and
the chunk knob change what they say they change.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_io as G
import liquidmi as LQ
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
    assert (16, 2) in an2                      # k_pfb2_an<16>
    assert [(r.M, r.q) for r in PB.PFB2_SYN] == [(12, 3), (64, 4), (256, 2), (512, 4), (1024, 2), (1024, 4), (4096, 2),
                                                 (64, 1), (12, 5)]
    for rows in (PB.PFB_AN, PB.PFB_SYN):
        assert {(r.M, r.q) for r in rows if not r.mode} == {(10, 5), (64, 8), (256, 4), (1024, 4), (1024, 8), (4096, 4),
                                                           (2048, 4)}
        assert {r.M for r in rows if r.mode == "few"} == {1024}
    assert [(r.M, r.q) for r in PB.PFB_AN if r.mode == "unaligned"] == [(1024, 4)]
    for an in (True, False):
        assert [(r.M, r.q) for r in PB.PFB_CCCF if r.an == an] == [(64, 4), (256, 4), (4096, 4), (1024, 4), (10, 5)]
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


# ------------------------------------------------------------------ routes
def query(r, n, parity=0, host=False, x16=None, y16=True):
    """The launch's decision for a call of n blocks of row r's object."""
    typ = LQ.LIQUID_ANALYZER if r.an else LQ.LIQUID_SYNTHESIZER
    x16 = r.mode != "unaligned" if x16 is None else x16
    if r.kind == "pfb2":
        return LQ.firpfbch2_route(typ, r.M, r.q, n, parity, x16, y16, host)
    return LQ.firpfbch_route(r.t, typ, r.M, r.q, n, x16, y16, host)


def check_row_routes(r):
    """Every call of every way takes its route; the row's S is the run."""
    seen = set()
    for name, at, host in PB.ways(r):
        for a, n in PB.pieces(r, at):
            got = query(r, n, a & 1, host)
            assert got.route == PB.piece_route(r, n, host), (PB.row_id(r), name, a, n, got)
            assert got.chunks == 1
            seen.add(got.route)
    whole = query(r, 16 if r.mode == "few" else PB.n_blocks(r))
    assert whole.route == r.route, (PB.row_id(r), whole)
    if r.mode == "few" and not r.an:          # one group of the workgroup's two: the seams are the calls'
        assert whole.workgroups == 1 and whole.run == 2 * r.S, (PB.row_id(r), whole)
    else:
        assert whole.run == r.S, (PB.row_id(r), whole)
        assert PB.n_blocks(r) > 3 * r.S           # the seams at S and 2S lie inside the stream
    return seen


# Routes no row needs to reach, each with its reason.
ONLY_TWO_PASS = ()     # none: LQ_*_TWO_PASS sends the fused sizes to routes other sizes take anyway
ONLY_2_31_BYTES = ()   # none: past 2^31 bytes the ladders fall to routes smaller calls take anyway


def check_complete(rows):
    seen = set()
    for r in rows:
        seen |= check_row_routes(r)
    every = LQ.channelizer_routes()
    assert len(set(every)) == len(every) == 42
    assert seen | set(ONLY_TWO_PASS) | set(ONLY_2_31_BYTES) == set(every), (
        "no row reaches %s; rows name the unknown %s" % (sorted(set(every) - seen), sorted(seen - set(every))))


@ROWS
def test_rows_take_their_routes(r):
    check_row_routes(r)


def test_rows_reach_every_route():
    check_complete(PB.ROWS)


def test_route_assertions_are_pinned():
    """A row that names a neighbouring route fails, and so does the
    completeness test once a route has lost its rows."""
    for r, other in ((PB.PFB2_AN[8], "pfb2_an512"), (PB.PFB2_AN[11], "pfb2_an1024_unpaired"),
                     (PB.PFB_SYN[8], "pfb_fft+syn_elem"), (PB.PFB_CCCF[0], "pfb_an_small")):
        check_row_routes(r)
        with pytest.raises(AssertionError):
            check_row_routes(r._replace(route=other))
    with pytest.raises(AssertionError):      # the comment said 64 blocks, the kernel walks 128
        check_row_routes(PB.PFB2_AN[16]._replace(S=64))
    for gone in ("pfb2_two_pass_elem", "pfb_an_run+fft", "pfb2_an1024_few_signal", "pfb_an1024_unpaired"):
        left = [r for r in PB.ROWS if gone not in {PB.piece_route(r, n, host) for _, at, host in PB.ways(r)
                                                     for _, n in PB.pieces(r, at)}]
        assert 0 < len(left) < len(PB.ROWS)
        with pytest.raises(AssertionError, match="no row reaches"):
            check_complete(left)


def test_queries_refuse_what_no_object_has():
    A = LQ.LIQUID_ANALYZER
    for bad in ((A, 7, 2, 10), (A, 0, 2, 10), (A, 64, 0, 10), (A, 64, 2, 0), (5, 64, 2, 10), (A, 16386, 2, 4)):
        with pytest.raises(ValueError):
            LQ.firpfbch2_route(*bad)
    for bad in (("crcf", A, 0, 2, 10), ("crcf", A, 64, 0, 10), ("crcf", A, 64, 2, 0), ("crcf", 5, 64, 2, 10)):
        with pytest.raises(ValueError):
            LQ.firpfbch_route(*bad)
    assert LQ.lib().liquid_mi355x_firpfbch_route(0, A, 64, 2, 10, 1, 1, 0, None, None, None) == -1   # rrrf
    assert LQ.lib().liquid_mi355x_channelizer_route_name(42) is None
    assert LQ.lib().liquid_mi355x_channelizer_route_name(-1) is None
    # an output that is not 16-byte aligned leaves the M = 1024 fast forms
    assert LQ.firpfbch2_route(A, 1024, 4, 200, y_aligned16=False).route == "pfb2_poly+fft"
    assert LQ.firpfbch_route("crcf", A, 1024, 4, 200, y_aligned16=False).route == "pfb_an_run+fft"
    # the signalling form: a host call whose output fits the completion buffer
    assert LQ.firpfbch2_route(A, 1024, 4, 8, host_call=True).route == "pfb2_an1024_few_signal"
    assert LQ.firpfbch2_route(A, 1024, 4, 9, host_call=True).route == "pfb2_an1024_few"
    assert LQ.firpfbch2_route(A, 1024, 4, 8, host_call=False).route == "pfb2_an1024_few"
    assert LQ.firpfbch2_route(A, 1024, 4, 17, host_call=True).route == "pfb2_an1024"


def test_operands_of_2_31_bytes():
    """Either side of the 32-bit offset limit of the fused forms; nothing runs."""
    A, S = LQ.LIQUID_ANALYZER, LQ.LIQUID_SYNTHESIZER
    assert LQ.firpfbch_route("crcf", A, 4096, 4, 65535).route == "pfb_an4096"
    assert LQ.firpfbch_route("crcf", A, 4096, 4, 65536).route == "pfb_an_run+fft"
    assert LQ.firpfbch_route("cccf", S, 4096, 4, 65535).route == "pfb_syn4096_c"
    assert LQ.firpfbch_route("cccf", S, 4096, 4, 65536).route == "pfb_fft+syn_run_c"
    assert LQ.firpfbch_route("crcf", A, 256, 4, 2 ** 20 - 1).route == "pfb_an_fused"
    assert LQ.firpfbch_route("crcf", A, 256, 4, 2 ** 20).route == "pfb_an_run+fft"
    assert LQ.firpfbch_route("crcf", S, 64, 4, 2 ** 25 - 1).route == "pfb_syn_small"      # (elements, not bytes)
    assert LQ.firpfbch_route("crcf", S, 64, 4, 2 ** 25).route == "pfb_fft+syn_run"
    assert LQ.firpfbch2_route(S, 4096, 2, 65535).route == "pfb2_syn4096"
    assert LQ.firpfbch2_route(S, 4096, 2, 65536).route == "pfb2_two_pass_run"
    assert LQ.firpfbch2_route(S, 512, 2, 2 ** 22 - 1).route == "pfb2_syn_fused"
    assert LQ.firpfbch2_route(S, 512, 2, 2 ** 22).route == "pfb2_two_pass_run"
    # the analyzers cut the call before the limit: the same route at any length
    for M, m, route, chunk in ((4096, 2, "pfb2_an4096", 2 ** 15), (256, 2, "pfb2_an256", 2 ** 19),
                               (1024, 4, "pfb2_an1024", 2 ** 18), (1024, 3, "pfb2_poly+fft", 2 ** 17)):
        for n, k in ((chunk, 1), (chunk + 1, 2), (3 * chunk, 3), (3 * chunk + 1, 4)):
            got = LQ.firpfbch2_route(A, M, m, n)
            assert (got.route, got.chunks) == (route, k), (M, m, n, got)
    assert LQ.firpfbch_route("crcf", A, 1024, 8, 2 ** 17).chunks == 1
    assert LQ.firpfbch_route("crcf", A, 1024, 8, 2 ** 17 + 1).chunks == 2


def test_two_pass_switches_show_in_the_query():
    """LQ_PFB2_TWO_PASS / LQ_PFB_TWO_PASS are read once per process."""
    code = ("import liquidmi as LQ\n"
            "A, S = LQ.LIQUID_ANALYZER, LQ.LIQUID_SYNTHESIZER\n"
            "print(LQ.firpfbch2_route(A, 256, 2, 500).route, LQ.firpfbch2_route(A, 4096, 2, 500).route,\n"
            "      LQ.firpfbch2_route(S, 512, 4, 500).route, LQ.firpfbch2_route(S, 4096, 1, 500).route,\n"
            "      LQ.firpfbch_route('crcf', A, 64, 8, 500).route, LQ.firpfbch_route('cccf', S, 4096, 4, 500).route,\n"
            "      LQ.firpfbch2_route(A, 1024, 4, 500).route, LQ.firpfbch_route('crcf', S, 1024, 4, 500).route)\n")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.abspath(LQ.__file__)))
    plain = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
    assert plain.split() == ["pfb2_an256", "pfb2_an4096", "pfb2_syn_fused", "pfb2_syn4096", "pfb_an_small",
                             "pfb_syn4096_c", "pfb2_an1024", "pfb_syn1024"]
    env.update(LQ_PFB2_TWO_PASS="1", LQ_PFB_TWO_PASS="1")
    two = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
    assert two.split() == ["pfb2_poly+fft", "pfb2_poly+fft", "pfb2_two_pass_run", "pfb2_two_pass_elem",
                           "pfb_an_run+fft", "pfb_fft+syn_run_c", "pfb2_an1024", "pfb_syn1024"]


# ------------------------------------------------------------------ run formulas
# The formulas as they stood with literal workgroup targets, restated: with no
# limit set the query (and so the launch) must give exactly these.
def _cd(a, b):
    return -(-a // b)


def _rows8(rows, T, extra):
    S = _cd(_cd(rows, T), 8) * 8
    S8 = rows // (8 * T) * 8
    if extra and S8 >= 32 and rows - T * S8 <= S8 // 4:
        S = S8
    return max(S, 32)


def ref_pfb2_an(M, m, nb, p0):
    rows = ((p0 + nb - 1) >> 1) - ((p0 - 1) >> 1) + 1
    if M == 1024 and m in (2, 4):
        ng = (p0 + nb - 1) // 16 - p0 // 16 + 1
        gpw = max(4, _cd(ng, 256))
        return 16 * gpw, _cd(ng, gpw)
    if 2 * m <= 8 and M in (256, 512):
        S = _rows8(rows, 1024, True)
    elif 2 * m <= 8 and M == 2048:
        S = _rows8(rows, 256, True)
    elif 2 * m <= 8 and M == 4096:
        S = max(32, _cd(rows, 256))
    elif 2 * m <= 8 and M in (64, 128):
        S = _rows8(rows, 2048, False)
        return 2 * S, _cd(_cd(rows, S), 256 // M)
    else:
        nsl = max(1, M // 256)
        S = max(8 * m, _cd(rows * nsl, 2048))
        return 2 * S, _cd(rows, S) * nsl
    return 2 * S, _cd(rows, S)


def ref_blocks(nb, T, step, least, Q=1):
    S = max(least, _cd(_cd(nb, T), step) * step)
    return S, _cd(_cd(nb, S), Q)


def ref_groups(nb, least):
    ng = _cd(nb, 16)
    gpw = max(least, _cd(ng, 256))
    return 16 * gpw, _cd(ng, gpw)


def _sizes(top):
    """Block counts either side of every break point a formula can have
    below `top': multiples of its target times its step, in rows and blocks."""
    c = {1, 2, 3, 17, 100, top - 1, top}
    for T in (256, 1024, 2048):
        for k in (1, 2, 4, 6, 8, 16, 24, 32, 33, 34, 35, 36, 40, 48, 64, 66, 72, 96, 128, 256):
            for u in (1, 2, 16, 32):
                for q in (0, 1, 4, 5):            # (the short extra run: a quarter of S8 past T runs)
                    c.add(T * k * u + q * k * u // 4)
    return sorted({n + d for n in c for d in range(-4, 5) if 17 <= n + d <= top})


def test_run_formulas_unchanged_without_a_limit():
    assert LQ.get_max_workgroups() == 0 and LQ.get_channelizer_chunk() == 0
    A, S = LQ.LIQUID_ANALYZER, LQ.LIQUID_SYNTHESIZER
    n = 0
    for M, m in ((256, 2), (512, 3), (2048, 2), (4096, 4), (64, 2), (128, 4), (1024, 2), (1024, 4), (1024, 3), (256, 8),
                 (8192, 2), (64, 7)):
        top = min(2 ** 18, 2 ** 27 // M)             # one chunk
        for nb in _sizes(top):
            for p0 in (0, 1):
                got = LQ.firpfbch2_route(A, M, m, nb, p0)
                assert (got.run, got.workgroups) == ref_pfb2_an(M, m, nb, p0), (M, m, nb, p0, got)
                n += 1
    cases = [(lambda nb: LQ.firpfbch2_route(S, 4096, 2, nb), lambda nb: ref_blocks(nb, 256, 3, 33), 2 ** 16 - 1),
             (lambda nb: LQ.firpfbch2_route(S, 256, 2, nb), lambda nb: ref_blocks(nb, 1024, 16, 64), 2 ** 20),
             (lambda nb: LQ.firpfbch2_route(S, 1024, 4, nb), lambda nb: ref_groups(nb, 2), 2 ** 20),
             (lambda nb: LQ.firpfbch_route("crcf", A, 256, 4, nb), lambda nb: ref_blocks(nb, 1024, 16, 32), 2 ** 20 - 1),
             (lambda nb: LQ.firpfbch_route("cccf", A, 4096, 4, nb), lambda nb: ref_blocks(nb, 256, 1, 32), 2 ** 16 - 1),
             (lambda nb: LQ.firpfbch_route("crcf", A, 64, 8, nb), lambda nb: ref_blocks(nb, 2048, 16, 32, 4), 2 ** 20),
             (lambda nb: LQ.firpfbch_route("crcf", A, 128, 8, nb), lambda nb: ref_blocks(nb, 2048, 16, 32, 2), 2 ** 20),
             (lambda nb: LQ.firpfbch_route("crcf", A, 1024, 4, nb), lambda nb: ref_groups(nb, 2), 2 ** 17),
             (lambda nb: LQ.firpfbch_route("crcf", S, 512, 4, nb), lambda nb: ref_blocks(nb, 1024, 16, 64), 2 ** 20),
             (lambda nb: LQ.firpfbch_route("crcf", S, 4096, 4, nb), lambda nb: ref_blocks(nb, 256, 3, 33), 2 ** 16 - 1),
             (lambda nb: LQ.firpfbch_route("cccf", S, 64, 4, nb), lambda nb: ref_blocks(nb, 2048, 16, 64, 4), 2 ** 20),
             (lambda nb: LQ.firpfbch_route("crcf", S, 1024, 8, nb), lambda nb: ref_groups(nb, 2), 2 ** 20)]
    for k, (fn, ref, top) in enumerate(cases):
        for nb in _sizes(top):
            got = fn(nb)
            assert (got.run, got.workgroups) == ref(nb), (k, nb, got)
            n += 1
    print("pfb_bound run formulas: %d sizes agree with the literal targets" % n)
    # the full-size shapes of tests/test_gpu_fullsize.py, as DESIGN.md records them
    assert LQ.firpfbch2_route(A, 2048, 2, 2 ** 16)[1:] == (256, 257, 1)       # 256 runs of 128 rows + 1 row
    assert LQ.firpfbch2_route(A, 256, 2, 2 ** 19)[1:] == (512, 1025, 1)
    assert LQ.firpfbch2_route(A, 1024, 4, 2 ** 18)[1:] == (1024, 256, 1)


def test_limit_lengthens_the_runs():
    A, S = LQ.LIQUID_ANALYZER, LQ.LIQUID_SYNTHESIZER
    before = LQ.firpfbch2_route(A, 256, 2, 600)
    assert before[1:] == (64, 10, 1)
    try:
        LQ.set_max_workgroups(3)
        assert LQ.firpfbch2_route(A, 256, 2, 574) == ("pfb2_an256", 192, 3, 1)        # 288 rows: 3 runs of 96
        assert LQ.firpfbch2_route(A, 256, 2, 600) == ("pfb2_an256", 192, 4, 1)        # 301 rows: 3 x 96 + 13
        assert LQ.firpfbch2_route(A, 256, 2, 199, 0) == ("pfb2_an256", 64, 4, 1)      # 101 rows: 3 x 32 + 5
        assert LQ.firpfbch2_route(A, 2048, 2, 199, 0) == ("pfb2_an2048", 64, 4, 1)
        assert LQ.firpfbch2_route(A, 1024, 4, 600) == ("pfb2_an1024", 16 * 13, 3, 1)  # 38 groups
        assert LQ.firpfbch2_route(S, 4096, 2, 300) == ("pfb2_syn4096", 102, 3, 1)
        assert LQ.firpfbch_route("crcf", A, 64, 8, 300) == ("pfb_an_small", 112, 1, 1)  # 3 sets, 4 to a workgroup
        assert LQ.firpfbch_route("crcf", S, 1024, 4, 600) == ("pfb_syn1024", 16 * 13, 3, 1)
        assert LQ.firpfbch2_route(A, 16, 2, 600) == ("pfb2_direct", 64, 10, 1)        # no run to lengthen
    finally:
        LQ.set_max_workgroups(0)
    assert LQ.firpfbch2_route(A, 256, 2, 600) == before


def test_chunk_knob():
    A = LQ.LIQUID_ANALYZER
    assert LQ.get_channelizer_chunk() == 0
    for bad in (1, 2, 32, 62, 63, 65, 66, 80, 100, 127, 2 ** 27 + 32):
        with pytest.raises(ValueError):
            LQ.set_channelizer_chunk(bad)
        assert LQ.get_channelizer_chunk() == 0
    try:
        for ok in (64, 96, 128, 4096):
            LQ.set_channelizer_chunk(ok)
            assert LQ.get_channelizer_chunk() == ok
            for r, n in ((PB.PFB2_AN[11], 3 * ok + 1), (PB.PFB2_AN[8], 2 * ok), (PB.PFB2_AN[16], 2 * ok + 1),
                         (PB.PFB_AN[3], 5 * ok)):
                got = query(r, n)
                assert got.route == r.route and got.chunks == -(-n // ok), (PB.row_id(r), n, got)
                assert (got.run, got.workgroups) == query(r, ok)[1:3]
            # launches that do not cut their calls
            assert query(PB.PFB2_AN[4], 1000).chunks == 1 and query(PB.PFB2_SYN[4], 1000).chunks == 1
            assert query(PB.PFB_AN[2], 1000).chunks == 1 and query(PB.PFB_CCCF[6], 1000).chunks == 1
        LQ.set_channelizer_chunk(2 ** 27)            # past the defaults: the defaults stay
        assert LQ.firpfbch2_route(A, 1024, 4, 2 ** 18 + 1).chunks == 2
        assert LQ.firpfbch2_route(A, 8192, 2, 2 ** 14 + 1).chunks == 2
    finally:
        LQ.set_channelizer_chunk(0)
    assert LQ.get_channelizer_chunk() == 0 and LQ.firpfbch2_route(A, 1024, 4, 1000).chunks == 1
