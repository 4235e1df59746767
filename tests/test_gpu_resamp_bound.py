"""Every resampler kernel against the per-output bound of tests/resamp_bound.py.

Each row of resamp_bound.ROWS is one kernel and rate class; a test first
asserts that the dispatch takes it (liquid_mi355x_resamp_route, computed by
the launch's own decision), then runs the burst, gaps and stairs streams --
their level edges on that kernel's seams -- through the library one way:

    one        one host call
    ragged     calls of 1, 3 and 5 inputs, cuts one either side of a tile
               seam, a cut right after the loud burst that ends at `cut`
    mixed      per-sample execute() calls (the host path) interleaved with
               block calls: loud samples pushed by execute() reach the next
               block call through the history, and a block call's loud tail
               reaches the execute() calls after it
    aligned    device pointers, the output pointer 16-byte aligned
    off8       ... and 8 bytes off
    reset      after reset() behind a loud stream (the gaps stream's head must
               then come out as exact zeros)
    wg3        at set_max_workgroups(3): every wave walks many tiles, so the
               windows prefetched a tile ahead are the ones used

and asserts the bound on every output, the exact output count, and
r_gpu <= 4 r_oracle, the margin the channelizer tests use.  r_oracle is the
oracle's worst ratio to (T + 8) 2^-23 A on the same stream.  r_gpu is the
worst ratio to that same term of what is left of an output's error once the
folded coefficient's derived allowance, 0.5 2^-23 A_fold, is taken off
(resamp_bound.excess): the allowance is an absolute amount the derivation
grants, the rest has to stay within four times the oracle's.  Measured
without taking it off, one row passes 4x -- k_resamp4 at r = 3.7, 5.3x on the
gaps stream, 6.1x on burst: a BOUNDARY output at mu = 0.99 whose one loud
sample sits where bank 0's tap is the prototype's zero crossing (h[576] at
fc = 0.25, 64 banks), so A = (1 - mu) |h[575]| |x| while the folded
coefficient fma(mu, h[576] - h[575], h[575]) carries the rounding of the
difference, mu u |h[575]| |x| = 0.5 2^-23 A_fold, 1.4 times the whole
(T + 8) term there.  No row is exempt, from the bound or from the margin.
resamp2's three kernels get the same treatment in all five modes, with the
delay taps bit for bit.
"""
import numpy as np
import pytest

import liquidmi as LQ
import resamp_bound as RB

pytestmark = pytest.mark.gpu

WAYS = ["one", "ragged", "mixed", "aligned", "off8", "reset", "wg3"]
MARGIN = 4.0


def _blocks(g, x, edges):
    out = [g.execute_block(x[a:b]).copy() for a, b in zip(edges[:-1], edges[1:]) if b > a]
    return np.concatenate(out) if out else np.zeros(0, x.dtype)


def _ragged_edges(c):
    """1, 3, 5, one either side of the first and of a later tile seam, the
    end of the loud burst at `cut`; for k_resamp4 the seams are outputs, so
    the cut goes to the input that emits the tile's first output."""
    row, n = c.row, c.row.n
    if row.seam == "out":
        seams = [int(c.idx[k]) for k in (256, 1024, 2048) if k < len(c.idx)]
    else:
        seams = [j * row.tile for j in (1, 4, 9) if j * row.tile < n]
    e = {0, 1, 4, 9, n}
    for s in seams:
        e.update((s - 1, s + 1))
    if row.cut:
        e.add(row.cut)
    return sorted(v for v in e if 0 <= v <= n)


def _dev(g, x, off_bytes, cap):
    dx = LQ.DeviceBuffer.from_array(x)
    dy = LQ.DeviceBuffer(cap * x.itemsize + 32)
    assert dy.p % 16 == 0
    ny = g.execute_block_dev(dx.p, len(x), dy.p + off_bytes)
    g.synchronize()
    y = np.empty(ny, x.dtype)
    LQ.lib().liquid_mi355x_memcpy_d2h(LQ.ptr(y), dy.p + off_bytes, y.nbytes)
    return y


def _mixed(g, x, d, L, cut):
    """block up to a loud-to-quiet edge | the L + 2 quiet samples after it by
    execute() | block | the last 8 loud samples before cut by execute() |
    block, which starts quiet"""
    out = [g.execute_block(x[:d]).copy()]
    out += [g.execute(v) for v in x[d:d + L + 2]]
    out.append(g.execute_block(x[d + L + 2:cut - 8]).copy())
    out += [g.execute(v) for v in x[cut - 8:cut]]
    out.append(g.execute_block(x[cut:]).copy())
    return np.concatenate(out)


def _run(c, way):
    row, x = c.row, c.x
    cap = len(c.y64) + 16
    with row.environ():
        g = LQ.Resamp(row.rate, row.m, row.fc, row.As, row.npfb, t=row.t)
        if way == "one":
            return g.execute_block(x).copy()
        if way == "ragged":
            return _blocks(g, x, _ragged_edges(c))
        if way == "mixed":
            L, n, cut, d = 2 * row.m, row.n, row.cut, c.drop
            assert 0 < d and d + L + 2 <= cut - 8
            was = LQ.get_small_calls()
            LQ.set_small_calls(True)         # execute() computes on the host
            try:
                return _mixed(g, x, d, L, cut)
            finally:
                LQ.set_small_calls(was)
        if way in ("aligned", "off8"):
            return _dev(g, x, 0 if way == "aligned" else 8, cap)
        if way == "reset":
            loud = np.ones(700, x.dtype) * 0.4
            g.execute_block(loud)
            g.reset()
            return g.execute_block(x).copy()
        if way == "wg3":
            LQ.set_max_workgroups(3)
            try:
                return _dev(g, x, 0, cap)
            finally:
                LQ.set_max_workgroups(0)
    raise ValueError(way)


@pytest.fixture(scope="module")
def r_oracle():
    """Worst ratio of the oracle per (row, stream), to the bound without the
    fold term; computed once."""
    memo = {}

    def get(c):
        key = (c.row.name, c.kind)
        if key not in memo:
            memo[key] = RB.report(c.oracle(), c.y64, c.A, c.row.T)["worst"]
        return memo[key]
    return get


def _held(c, y, way, r_oracle):
    assert len(y) == len(c.y64), "%s %s %s: %d outputs, the schedule has %d" % (c.row.name, c.kind, way, len(y), len(c.y64))
    full = c.check(y, fold=RB.FOLD, label=way)["worst"]
    rg = RB.excess(y, c.y64, c.A, c.Af, c.row.T)
    ro = r_oracle(c)
    print("r_gpu %s %s %s %.4f (of the whole bound %.4f) r_oracle %.4f ratio %.2f"
          % (c.row.name, c.kind, way, rg, full, ro, rg / ro))
    assert rg <= MARGIN * ro, (c.row.name, c.kind, way, rg, ro)


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("row", RB.ROWS, ids=repr)
def test_resamp_bound(row, way, r_oracle):
    assert row.query() == (row.route, row.tile)
    for kind in RB.KINDS:
        c = RB.case(row.name, kind)
        _held(c, _run(c, way), way, r_oracle)


@pytest.mark.parametrize("way", ["aligned", "off8", "wg3"])
def test_resamp_bound_periodic_plan(way, r_oracle):
    """One call of 2^16 + 5003 inputs builds the periodic plan (r = 1.5: it
    repeats every 256 outputs, so the call wraps it several hundred times and
    every burst lies across wraps)."""
    row = RB.PERIODIC
    assert row.query() == (row.route, row.tile) and row.n >= 1 << 16
    c = RB.case(row.name, "burst")
    _held(c, _run(c, way), way, r_oracle)


@pytest.mark.parametrize("kind", RB.KINDS)
def test_resamp_bound_call_without_outputs(kind, r_oracle):
    """r = 0.3: the loud burst's last input is a block call of its own that
    emits nothing (no launch: the history update alone); the quiet call after
    it sees the burst only through that history."""
    row = RB.SILENT
    assert row.query() == (row.route, row.tile)
    c = RB.case(row.name, kind)
    cut = row.cut
    assert cut - 1 not in set(c.idx.tolist())
    if kind != "stairs":
        assert abs(c.x[cut - 1]) > 1e-3 and abs(c.x[cut]) < 1e-4
    for dev in (False, True):
        g = LQ.Resamp(row.rate, row.m, row.fc, row.As, row.npfb, t=row.t)
        if dev:
            y = np.concatenate([_dev(g, c.x[a:b], 0, len(c.y64) + 16) for a, b in ((0, cut - 1), (cut - 1, cut), (cut, row.n))])
        else:
            parts = [g.execute_block(c.x[a:b]).copy() for a, b in ((0, cut - 1), (cut - 1, cut), (cut, row.n))]
            assert len(parts[1]) == 0
            y = np.concatenate(parts)
        _held(c, y, "silent-dev" if dev else "silent", r_oracle)


# ------------------------------------------------------------------ resamp2
R2_WAYS = ["one", "ragged", "mixed", "aligned", "off8", "clear"]


def _r2_out(mode, y):
    return np.stack(y, 1).ravel() if mode == RB.FILTER else y


def _r2_dev(g, c, off_bytes):
    mode, n = c.mode, c.ncalls
    dx = LQ.DeviceBuffer.from_array(c.x)
    esz = c.x.itemsize
    per = 1 if mode == RB.FILTER else RB.NOUT[mode]
    dy0, dy1 = LQ.DeviceBuffer(n * per * esz + 32), LQ.DeviceBuffer(n * esz + 32)
    g.run_dev(mode, dx.p, n, dy0.p + off_bytes, dy1.p + off_bytes if mode == RB.FILTER else None)
    g.synchronize()
    y0 = np.empty(n * per, c.x.dtype)
    LQ.lib().liquid_mi355x_memcpy_d2h(LQ.ptr(y0), dy0.p + off_bytes, y0.nbytes)
    if mode != RB.FILTER:
        return y0
    y1 = np.empty(n, c.x.dtype)
    LQ.lib().liquid_mi355x_memcpy_d2h(LQ.ptr(y1), dy1.p + off_bytes, y1.nbytes)
    return np.stack([y0, y1], 1).ravel()


def _r2_run(c, way):
    mode, per, n = c.mode, RB.NIN[c.mode], c.ncalls
    g = LQ.Resamp2(c.m, c.f0, 60.0, t=c.t)
    x = c.x

    def block(a, b):
        return _r2_out(mode, g.run(mode, x[a * per:b * per]))

    def single(i):
        if mode == RB.FILTER:
            return np.array(g.call(mode, x[i]), x.dtype)
        return g.call(mode, x[i] if per == 1 else x[2 * i:2 * i + 2])

    if way == "one":
        return block(0, n)
    if way == "ragged":
        e = sorted({0, 1, 4, 9, RB.R2_TILE - 1, RB.R2_TILE + 1, c.cut, 2 * RB.R2_TILE + 1, n})
        return np.concatenate([block(a, b) for a, b in zip(e[:-1], e[1:])])
    if way == "mixed":
        a, b = c.cut - 6, 2 * RB.R2_TILE      # per-call API across the loud burst's end, and behind a tile seam
        out = [block(0, a)] + [single(i) for i in range(a, c.cut)] + [block(c.cut, b)]
        out += [single(i) for i in range(b, b + 2 * c.m + 2)] + [block(b + 2 * c.m + 2, n)]
        return np.concatenate(out)
    if way in ("aligned", "off8"):
        return _r2_dev(g, c, 0 if way == "aligned" else 8)
    if way == "clear":
        g.run(mode, (np.ones(300 * per, x.dtype) * 0.4).astype(x.dtype))
        if mode == RB.FILTER:
            g.run(mode, np.ones(1, x.dtype))      # an odd count: the toggle must be cleared too
        g.clear()
        return block(0, n)
    raise ValueError(way)


R2_CASES = [(name, t) for name, _, _, ctaps in RB.R2_ROWS for t in (("cccf",) if ctaps else ("crcf", "rrrf"))]


@pytest.mark.parametrize("way", R2_WAYS)
@pytest.mark.parametrize("mode", range(5), ids=RB.MODE_NAMES)
@pytest.mark.parametrize("name,t", R2_CASES)
def test_resamp2_bound(name, t, mode, way):
    m = next(r[1] for r in RB.R2_ROWS if r[0] == name)
    want = "filter" if mode == RB.FILTER else ("tiled_b" if m <= 16 else "tiled")
    for kind in RB.KINDS:
        c = RB.case2(name, mode, kind, t)
        tile = 256 if mode == RB.FILTER else RB.R2_TILE
        assert LQ.resamp2_route(mode, m, c.x.nbytes) == (want, tile)
        y = _r2_run(c, way)
        assert len(y) == len(c.y64)
        r = c.check(y, way)
        ro = c.r_oracle
        print("r_gpu resamp2 %s %s %s %s %s %.4f r_oracle %.4f ratio %.2f"
              % (name, t, RB.MODE_NAMES[mode], kind, way, r["worst"], ro, r["worst"] / ro))
        assert r["worst"] <= MARGIN * ro


# ------------------------------------------------------------------ msresamp2, msresamp
MS_WAYS = ["one", "ragged", "aligned", "off8", "reset", "wg3"]


def _ms_dev(g, x, off_bytes, cap):
    dx = LQ.DeviceBuffer.from_array(x)
    dy = LQ.DeviceBuffer(cap * x.itemsize + 32)
    ny = g.execute_block_dev(dx.p, len(x), dy.p + off_bytes)
    g.synchronize()
    y = np.empty(ny, x.dtype)
    LQ.lib().liquid_mi355x_memcpy_d2h(LQ.ptr(y), dy.p + off_bytes, y.nbytes)
    return y


def _ms_run(c, way):
    g = LQ.MsResamp(c.rate, c.As, t=c.t)
    x, cap = c.x, len(c.y64) + 64
    if way == "one":
        return g.execute(x).copy()
    if way == "ragged":
        # 1, 3, 5; one chain input either side of the one that emits the
        # resampler tile's first output; the end of the loud burst at cut
        scale = 1 if c.typ == 0 else c.M
        tile = RB.ms_query(c.t, c.rate, c.n, c.As)[1]
        seam = int(c.idx[tile]) * scale if tile < len(c.idx) else c.n // 3
        e = sorted({0, 1, 4, 9, seam - 1, seam + 1, c.cut, c.n})
        return np.concatenate([g.execute(x[a:b]).copy() for a, b in zip(e[:-1], e[1:])])
    if way in ("aligned", "off8"):
        return _ms_dev(g, x, 0 if way == "aligned" else 8, cap)
    if way == "reset":
        g.execute((np.ones(701, x.dtype) * 0.4).astype(x.dtype))      # leaves a partial group pending when decimating
        g.reset()
        return g.execute(x).copy()
    if way == "wg3":
        LQ.set_max_workgroups(3)
        try:
            return _ms_dev(g, x, 0, cap)
        finally:
            LQ.set_max_workgroups(0)
    raise ValueError(way)


@pytest.mark.parametrize("way", MS_WAYS)
@pytest.mark.parametrize("t,rate,n,cut,hm", RB.MS_ROWS)
def test_msresamp_bound(t, rate, n, cut, hm, way):
    """The chain against the cascaded bound (T the sum of the stages', A
    through their modulus filters).  hm: the half-band stage the resampler's
    launch takes along (the fused chain), asserted through the route query."""
    route, tile, got = RB.ms_query(t, rate, n)
    assert got == hm and (tile == 256 - ((2 * hm - 1 + 3) & ~3) if hm else True)
    for kind in RB.KINDS:
        c = RB.mscase(t, rate, kind)
        y = _ms_run(c, way)
        assert len(y) == len(c.y64)
        r = c.check(y, way)
        print("r_gpu msresamp %s %g %s %s %.4f r_oracle %.4f ratio %.2f"
              % (t, rate, kind, way, r["worst"], c.r_oracle, r["worst"] / c.r_oracle))
        assert r["worst"] <= MARGIN * c.r_oracle


@pytest.mark.parametrize("way", ["one", "ragged", "wg3"])
@pytest.mark.parametrize("As,hm", RB.MS_HB_ROWS)
def test_msresamp_bound_fused_stage_lengths(As, hm, way):
    """The fused stage's semi-lengths no other test reaches (RB.MS_HB_ROWS),
    the route asserted as above, the same bound and margin."""
    route, tile, got = RB.ms_query("crcf", RB.MS_HB_RATE, RB.MS_HB_N, As)
    assert (route, got) == ("resamp4/up", hm) and tile == 256 - ((2 * hm - 1 + 3) & ~3)
    for kind in RB.KINDS:
        c = RB.mshbcase(As, kind)
        y = _ms_run(c, way)
        assert len(y) == len(c.y64)
        r = c.check(y, way)
        print("r_gpu msresamp As %g stage m %d %s %s %.4f r_oracle %.4f ratio %.2f"
              % (As, hm, kind, way, r["worst"], c.r_oracle, r["worst"] / c.r_oracle))
        assert r["worst"] <= MARGIN * c.r_oracle


MS2_WAYS = ["one", "ragged", "mixed", "aligned", "off8", "reset"]


def _ms2_run(c, way):
    g = LQ.MsResamp2(c.typ, c.ns, 0.4, 0.0, 60.0, t=c.t)
    per, n, x = (1 if c.typ == 0 else c.M), c.ncalls, c.x

    def block(a, b):
        return g.execute_block(x[a * per:b * per]).copy()

    if way == "one":
        return block(0, n)
    if way == "ragged":
        e = sorted({0, 1, 4, 9, RB.R2_TILE - 1, RB.R2_TILE + 1, c.cut, n})
        return np.concatenate([block(a, b) for a, b in zip(e[:-1], e[1:])])
    if way == "mixed":
        a = c.cut - 6
        out = [block(0, a)] + [g.execute(x[i * per:(i + 1) * per]).copy() for i in range(a, c.cut + 3)] + [block(c.cut + 3, n)]
        return np.concatenate(out)
    if way in ("aligned", "off8"):
        off = 0 if way == "aligned" else 8
        dx = LQ.DeviceBuffer.from_array(x)
        dy = LQ.DeviceBuffer(len(c.y64) * x.itemsize + 32)
        g.execute_block_dev(dx.p, n, dy.p + off)
        g.synchronize()
        y = np.empty(len(c.y64), x.dtype)
        LQ.lib().liquid_mi355x_memcpy_d2h(LQ.ptr(y), dy.p + off, y.nbytes)
        return y
    if way == "reset":
        g.execute_block((np.ones(300 * per, x.dtype) * 0.4).astype(x.dtype))
        g.reset()
        return block(0, n)
    raise ValueError(way)


@pytest.mark.parametrize("way", MS2_WAYS)
@pytest.mark.parametrize("t,typ,ns", [("crcf", 0, 1), ("crcf", 0, 4), ("rrrf", 0, 2), ("cccf", 1, 1), ("crcf", 1, 4),
                                      ("rrrf", 1, 2)])
def test_msresamp2_bound(t, typ, ns, way):
    for kind in RB.KINDS:
        c = RB.ms2case(t, typ, ns, kind)
        y = _ms2_run(c, way)
        assert len(y) == len(c.y64)
        r = c.check(y, way)
        print("r_gpu msresamp2 %s typ %d ns %d %s %s %.4f r_oracle %.4f ratio %.2f"
              % (t, typ, ns, kind, way, r["worst"], c.r_oracle, r["worst"] / c.r_oracle))
        assert r["worst"] <= MARGIN * c.r_oracle
