"""The resamplers' per-output bound is reachable and the checker is pinned (CPU).

The oracle -- the reference's own float32 arithmetic -- must meet the bound
of tests/resamp_bound.py on every row and stream, with the folded-coefficient
term off (it forms no folded coefficient), and the models must give the
oracle's output counts exactly.  Then the oracle's output is damaged the way
a kernel with a stale tile, a slipped bank, a lost history or a wrong
BOUNDARY window would damage it: each damaged stream must fail the bound,
and the ones quiet enough to pass the normwise 1e-5 that every older
resampler test asserts must pass it (the test says which).
"""
import numpy as np
import pytest

import resamp_bound as RB

NRM = 1e-5


@pytest.mark.parametrize("kind", RB.KINDS)
@pytest.mark.parametrize("row", RB.ROWS + [RB.SILENT], ids=repr)
def test_oracle_meets_the_bound(row, kind):
    c = RB.case(row.name, kind)
    y = c.oracle([row.cut] if row.cut else None)
    assert len(y) == len(c.y64) == len(c.b)
    r = c.check(y, fold=0.0, label="oracle")
    print("r_oracle %s %s %.4f nrm %.3g" % (row.name, kind, r["worst"], RB.nrm_err(y, c.y64)))
    if row.rate <= row.npfb:
        assert c.nout(row.n) == len(y)
    if kind == "gaps":
        assert np.count_nonzero(c.A == 0) > 0 and np.all(y[c.A == 0] == 0)
        assert np.array_equal(c.A == 0, c.Af == 0)


def test_oracle_meets_the_bound_periodic_row():
    c = RB.case(RB.PERIODIC.name, "burst")
    y = c.oracle()
    assert len(y) == len(c.y64)
    r = c.check(y, label="oracle")
    print("r_oracle %s burst %.4f" % (RB.PERIODIC.name, r["worst"]))


def test_rows_reach_every_kernel_and_class():
    """Every row takes the kernel and class it names (the tile property
    asserts it against the library's own launch decision, no GPU call), and
    together the rows reach every route the query can return; the tiles of
    k_resamp3 differ between rows, so no stream is built for another's seams."""
    import liquidmi as LQ
    for row in RB.ROWS + [RB.PERIODIC, RB.SILENT]:
        assert row.tile > 0
        print("route %s: %s, tile %d" % (row.name, row.route, row.tile))
    assert {r.route for r in RB.ROWS} == set(LQ.RESAMP_ROUTES)
    assert RB.ROW["r3-fast"].tile < 2 * RB.ROW["r3-fast"].m + 1      # a tile shorter than the window
    assert RB.ROW["r3-env"].tile == RB.ROW["r3-rrrf"].tile and RB.ROW["r4-up"].tile == 256
    assert RB.ROW["rs-fast"].tile == 2048 and RB.ROW["generic"].tile == 256
    # the periodic row's one call is long enough for the periodic plan, and
    # a short first call at the same shape takes the same kernel
    assert RB.PERIODIC.n >= 1 << 16 and RB.PERIODIC.query(100) == RB.PERIODIC.query()
    for name, m, _, _ in RB.R2_ROWS:
        for mode in range(5):
            want = "filter" if mode == RB.FILTER else ("tiled_b" if m <= 16 else "tiled")
            c = RB.case2(name, mode, "gaps")
            assert LQ.resamp2_route(mode, m, c.x.nbytes) == (want, 256 if mode == RB.FILTER else RB.R2_TILE)
    assert LQ.resamp2_route(RB.INTERP, 4, 1 << 31) == ("tiled", RB.R2_TILE)   # past 2^31 bytes of input


def test_streams_put_edges_on_the_seams():
    """Every seam position the builder names carries a level edge on it or
    one sample either side, and the call cut and the stream's end are loud."""
    for row in RB.ROWS:
        c = RB.case(row.name, "gaps")
        loud = np.abs(c.x) > 0
        edge = np.flatnonzero(loud[1:] != loud[:-1]) + 1      # first sample of a new level
        seams = RB.seam_inputs(row, c.idx, row.n)
        assert len(seams) >= 3, row
        for p in seams:
            assert np.min(np.abs(edge - p)) <= 1, (row, p)
        if row.cut:
            assert loud[row.cut - 1] and not loud[row.cut]
        assert loud[-1] and not loud[0]
        for kind in RB.KINDS:      # room for the per-sample calls between the first loud-to-quiet edge and the cut
            assert 0 < RB.case(row.name, kind).drop <= row.cut - 8 - 2 * row.m - 2, (row, kind)


# ------------------------------------------------------------------ mutations
def _model32(c, win=None, mu=None, x=None):
    y64, _, _ = RB.resamp_reference(c.x if x is None else x, c.h, c.row.m, c.row.npfb,
                                    c.mu if mu is None else mu, c.win if win is None else win)
    return y64.astype(np.complex64)


def _tiles(c):
    """(loud, quiet): 256-output tiles by their largest A."""
    nt = len(c.A) // 256
    top = c.A[:nt * 256].reshape(nt, 256).max(1)
    return int(np.argmax(top)), int(np.argmin(np.where(top > 0, top, np.inf)))


def _mut_leak(c, y):
    """1e-6 of a loud tile added to a quiet one (a stale LDS window)."""
    loud, quiet = _tiles(c)
    y[quiet * 256:quiet * 256 + 256] += np.complex64(1e-6) * y[loud * 256:loud * 256 + 256]


def _mut_bank(c, y):
    """the bank index one too high for one tile of a quiet stretch"""
    _, quiet = _tiles(c)
    s = slice(quiet * 256, quiet * 256 + 256)
    b0, b1, i0, i1 = (a.copy() for a in c.win)
    b0[s] = np.minimum(b0[s] + 1, c.row.npfb - 1)
    b1[s] = np.minimum(b1[s] + 1, c.row.npfb - 1)
    y[s] = _model32(c, win=(b0, b1, i0, i1))[s]


def _mut_history(c, y):
    """the call that starts at `cut` finds zeros for its history"""
    cut = c.row.cut
    x = c.x.copy()
    x[:cut] = 0
    k0, k1 = c.nout(cut), c.nout(cut + 2 * c.row.m + 2)
    y[k0:k1] = _model32(c, x=x)[k0:k1]


def _mut_boundary(c, y):
    """a BOUNDARY output takes both banks on the newest window"""
    b0, b1, i0, i1 = c.win
    bnd = c.b < 0
    assert bnd.any()
    y[bnd] = _model32(c, win=(b0, b1, i1, i1))[bnd]


def _mut_nonzero(c, y):
    """one output that must be zero is 1e-30"""
    k = int(np.flatnonzero(c.A == 0)[7])
    y[k] = 1e-30


# mutation, stream, whether the damaged stream must still pass the normwise 1e-5
MUTATIONS = [(_mut_leak, "burst", True), (_mut_leak, "gaps", True), (_mut_bank, "burst", True),
             (_mut_history, "burst", False), (_mut_history, "stairs", None), (_mut_boundary, "burst", None),
             (_mut_boundary, "stairs", None), (_mut_nonzero, "gaps", True)]


@pytest.mark.parametrize("mut,kind,passes_nrm", MUTATIONS, ids=["%s-%s" % (m.__name__[5:], k) for m, k, _ in MUTATIONS])
@pytest.mark.parametrize("name", ["r4-up", "r3-npfb37"])
def test_mutations_fail_the_bound(name, mut, kind, passes_nrm):
    """passes_nrm True: the damage is below what the normwise 1e-5 of the
    older tests can see (leak, bank slip in a quiet tile, a non-zero zero);
    False: it is not (the history of a call that follows a loud burst); None:
    whichever it is, it is printed (BOUNDARY outputs are one in npfb and each
    is off by a whole sample's worth, which 1e-5 sees on some rows)."""
    c = RB.case(name, kind)
    good = c.oracle([c.row.cut])
    assert RB.report(good, c.y64, c.A, c.row.T)["failing"] == 0
    y = good.copy()
    mut(c, y)
    assert not np.array_equal(y, good)
    e = RB.nrm_err(y, good)
    r = RB.report(y, c.y64, c.A, c.row.T, c.Af, RB.FOLD)
    print("mutation %s on %s %s: normwise %.3g (%s 1e-5), %d outputs fail the bound, worst %.3g x"
          % (mut.__name__[5:], name, kind, e, "passes" if e < NRM else "fails", r["failing"], r["worst"]))
    assert r["failing"] > 0
    if passes_nrm is not None:
        assert (e < NRM) == passes_nrm


# ------------------------------------------------------------------ resamp2
@pytest.mark.parametrize("kind", RB.KINDS)
@pytest.mark.parametrize("mode", range(5), ids=RB.MODE_NAMES)
@pytest.mark.parametrize("name", [r[0] for r in RB.R2_ROWS])
def test_resamp2_oracle_meets_the_bound(name, mode, kind):
    c = RB.case2(name, mode, kind)
    y = c.oracle()
    assert len(y) == len(c.y64) == c.ncalls * RB.NOUT[mode]
    r = c.check(y, "oracle")
    print("r_oracle resamp2 %s %s %s %.4f" % (name, RB.MODE_NAMES[mode], kind, r["worst"]))
    if mode in (RB.INTERP, RB.SYNTHESIZER):
        assert np.count_nonzero(~np.isnan(c.ex.real)) == c.ncalls


@pytest.mark.parametrize("mode", range(5), ids=RB.MODE_NAMES)
def test_resamp2_mutations_fail(mode):
    """A window one call late (the outputs of a tile shifted by one call) and
    a leak of 1e-6 of the loud stretch before the tile seam into the quiet
    one after it: both pass the normwise 1e-5 on the burst stream or are
    printed, both fail the bound; a delay tap one ulp off fails bit-exactness."""
    c = RB.case2("m4", mode, "burst")
    good = c.oracle()
    no = RB.NOUT[mode]
    a = (2 * RB.R2_TILE + 200) * no
    y = good.copy()
    y[a:a + 256 * no] += np.complex64(1e-6) * good[(2 * RB.R2_TILE - 20) * no:(2 * RB.R2_TILE - 20) * no + 256 * no].max()
    e = RB.nrm_err(y, good)
    r = c.report(y)
    print("resamp2 %s leak: normwise %.3g, %d fail" % (RB.MODE_NAMES[mode], e, r["failing"]))
    assert e < NRM and r["failing"] > 0
    y = good.copy()
    s = slice(RB.R2_TILE * no, (RB.R2_TILE + 64) * no)
    y[s] = good[RB.R2_TILE * no - no:(RB.R2_TILE + 64) * no - no]
    r = c.report(y)
    print("resamp2 %s late window: normwise %.3g, %d fail" % (RB.MODE_NAMES[mode], RB.nrm_err(y, good), r["failing"]))
    assert r["failing"] > 0
    if mode in (RB.INTERP, RB.SYNTHESIZER):
        y = good.copy()
        k = int(np.flatnonzero(~np.isnan(c.ex.real) & (np.abs(good) > 0.1))[0])
        y[k] = np.nextafter(y[k].real, np.float32(2)) + 1j * y[k].imag
        r = c.report(y)
        assert r["failing"] == 0 and r["inexact"] == 1


# ------------------------------------------------------------------ msresamp2, msresamp
MS2 = [(typ, ns) for typ in (0, 1) for ns in (1, 2, 4)]


@pytest.mark.parametrize("kind", RB.KINDS)
@pytest.mark.parametrize("typ,ns", MS2)
def test_msresamp2_oracle_meets_the_cascaded_bound(typ, ns, kind):
    """T the sum of the stages', A carried through their modulus filters:
    first order, so the oracle staying under it is what holds the model."""
    c = RB.ms2case("crcf", typ, ns, kind)
    y = c.oracle()
    assert len(y) == len(c.y64) == (c.ncalls * c.M if typ == 0 else c.ncalls)
    r = c.check(y, "oracle")
    print("r_oracle msresamp2 typ %d ns %d %s %.4f (T = %d)" % (typ, ns, kind, r["worst"], c.T))
    assert r["worst"] <= 1.0


@pytest.mark.parametrize("kind", RB.KINDS)
@pytest.mark.parametrize("t,rate", [r[:2] for r in RB.MS_ROWS])
def test_msresamp_oracle_meets_the_cascaded_bound(t, rate, kind):
    c = RB.mscase(t, rate, kind)
    y = c.oracle([c.cut])
    assert len(y) == len(c.y64)
    r = c.check(y, "oracle")
    print("r_oracle msresamp %s %g %s %.4f (T = %d, %d stages)" % (t, rate, kind, r["worst"], c.T, c.ns))
    assert r["worst"] <= 1.0
    if kind == "gaps":
        assert np.count_nonzero(c.A == 0) > 0


@pytest.mark.parametrize("kind", RB.KINDS)
@pytest.mark.parametrize("As,hm", RB.MS_HB_ROWS)
def test_msresamp_oracle_meets_the_cascaded_bound_at_every_fused_stage_length(As, hm, kind):
    route, tile, got = RB.ms_query("crcf", RB.MS_HB_RATE, RB.MS_HB_N, As)
    c = RB.mshbcase(As, kind)
    assert (route, got) == ("resamp4/up", hm) and tile == 256 - ((2 * hm - 1 + 3) & ~3) and c.stages[-1][0] == hm
    y = c.oracle([c.cut])
    assert len(y) == len(c.y64)
    r = c.check(y, "oracle")
    print("r_oracle msresamp As %g (stage m %d) %s %.4f (T = %d)" % (As, hm, kind, r["worst"], c.T))
    assert r["worst"] <= 1.0


def test_msresamp_rows_reach_the_fused_and_the_unfused_chain():
    """The stage designs restate the library's (the fused stage's m is the
    query's), and the rows reach the fused launch -- its tile shorter by the
    stage's halo -- and the unfused chains."""
    for t, rate, n, cut, hm in RB.MS_ROWS:
        route, tile, got = RB.ms_query(t, rate, n)
        c = RB.mscase(t, rate, "gaps")
        print("msresamp %s %g: %s tile %d fused m %d, stages %s" % (t, rate, route, tile, got, [m for m, _ in c.stages]))
        assert got == hm
        if hm:
            assert c.typ == 0 and c.stages[-1][0] == hm and route == "resamp4/up"
            assert tile == 256 - ((2 * hm - 1 + 3) & ~3)
        assert (c.typ == 1) == (rate < 1) and (c.n % c.M != 0 and c.cut % c.M != 0 if c.typ == 1 else True)


def test_msresamp_mutation_fails_the_cascaded_bound():
    """1e-6 of the loudest 256 outputs added to the quietest: passes the
    normwise 1e-5, fails the cascaded bound."""
    c = RB.mscase("crcf", 2.6, "burst")
    good = c.oracle()
    nt = len(c.A) // 256
    top = c.A[:nt * 256].reshape(nt, 256).max(1)
    loud, quiet = int(np.argmax(top)), int(np.argmin(top))
    y = good.copy()
    y[quiet * 256:quiet * 256 + 256] += np.complex64(1e-6) * good[loud * 256:loud * 256 + 256]
    e, r = RB.nrm_err(y, good), c.report(y)
    print("msresamp leak: normwise %.3g, %d outputs fail" % (e, r["failing"]))
    assert e < NRM and r["failing"] > 0
