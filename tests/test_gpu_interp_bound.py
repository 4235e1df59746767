"""Every route of lqk_firinterp -- firinterp and firpfb's block interpolation --
against the direct form's per-output error bound (tests/interp_bound.py),
however the caller cuts the stream (`-m gpu`).

Each row first asserts the kernel its shape reaches
(liquid_mi355x_firinterp_route, the launch's own decision): k_firinterp_t<kind,
LT> for each LT class and its LDS edges, the plain k_firinterp for each of its
reasons (complex taps, L > 32, M > 64, LDS, an unaligned output pointer -- the
last through execute_block_dev only).  Then the burst and gaps streams run
  (a) as one device call,
  (b) as device calls cut at 1, 64, 65, 320 (the first calls shorter than
      L - 1: the history is composed from history),
  (c) as two calls cut at 500, the loud samples reaching the second only
      through the carried history,
  (d) through host pointers, and execute() singles interleaved with blocks in
      both small-call modes,
all against the same float64 y64; firpfb the same with the user scale and the
push / execute(i) <-> execute_block hand-over of its window.
"""
import subprocess
import sys

import numpy as np
import pytest

import interp_bound as IB
import liquidmi as LQ

pytestmark = pytest.mark.gpu

ROWS = pytest.mark.parametrize("row", IB.ROWS, ids=IB.row_id)


@pytest.fixture(params=[True, False], ids=["host-singles", "gpu-singles"])
def small_calls(request):
    old = LQ.get_small_calls()
    LQ.set_small_calls(request.param)
    try:
        yield request.param
    finally:
        LQ.set_small_calls(old)


def _assert_route(c, route, aligned=True):
    assert LQ.firinterp_route(c.t, c.M, c.L, aligned) == route, (c.t, c.M, c.hlen)


def _obj(c):
    if not c.pfb:
        return LQ.FirInterp(c.M, c.h, t=c.t)
    g = LQ.FirPfb(c.M, c.h, t=c.t)
    g.set_scale(c.s)
    return g


def _run_dev(c, cuts=(), off=0):
    """The stream through execute_block_dev, one call per piece, y `off`
    samples past a 16-byte boundary."""
    g = _obj(c)
    x, esz, n = c.x, c.x.itemsize, len(c.x)
    bx = LQ.DeviceBuffer.from_array(x)
    by = LQ.DeviceBuffer((n * c.M + off + 4) * esz)
    assert by.p % 16 == 0 and ((by.p + off * esz) % 16 == 0) == (off == 0)
    edges = [0] + list(cuts) + [n]
    for a, b in zip(edges[:-1], edges[1:]):
        g.execute_block_dev(bx.p + a * esz, b - a, by.p + (off + a * c.M) * esz)
    g.synchronize()
    return by.to_array(x.dtype, n * c.M + off)[off:]


@pytest.mark.parametrize("name", IB.ENVELOPES)
@ROWS
def test_firinterp_bound_device_calls(row, name):
    """(a) and (b)"""
    c = IB.case(row[0], row[1], row[2], name)
    _assert_route(c, row[3])
    c.check(_run_dev(c))
    c.check(_run_dev(c, IB.CUTS))


@ROWS
def test_firinterp_bound_carried_history(row):
    """(c)"""
    c = IB.case(row[0], row[1], row[2], "carried")
    _assert_route(c, row[3])
    c.check(_run_dev(c, (IB.CARRIED_CUT,)))


@pytest.mark.parametrize("name", IB.ENVELOPES + ["carried"])
@pytest.mark.parametrize("row", IB.UNALIGNED_ROWS, ids=IB.row_id)
def test_firinterp_bound_unaligned_output(row, name):
    """The plain kernel by the output pointer: y one sample (4 or 8 bytes)
    past a 16-byte boundary; every later piece then starts a M samples on,
    aligned or not as it falls."""
    c = IB.case(row[0], row[1], row[2], name)
    _assert_route(c, 0, aligned=False)
    assert LQ.firinterp_route(c.t, c.M, c.L, True) != 0
    c.check(_run_dev(c, off=1))
    c.check(_run_dev(c, IB.CUTS if name != "carried" else (IB.CARRIED_CUT,), off=1))


@pytest.mark.parametrize("name", IB.ENVELOPES)
@ROWS
def test_firinterp_bound_host_pointers(row, name):
    """(d), blocks only"""
    c = IB.case(row[0], row[1], row[2], name)
    _assert_route(c, row[3])
    c.check(LQ.FirInterp(c.M, c.h, t=c.t).execute_block(c.x))


@ROWS
def test_firinterp_bound_singles_between_blocks(row, small_calls):
    """(d): execute() for single inputs (on the host or the GPU by the mode)
    between host-pointer blocks, so the history changes hands both ways, with
    singles on the loud samples at the tile seam and at the end."""
    c = IB.case(row[0], row[1], row[2], "burst")
    _assert_route(c, row[3])
    g = LQ.FirInterp(c.M, c.h, t=c.t)
    n, out, a = len(c.x), [], 0
    for b, single in ((100, False), (103, True), (255, False), (258, True), (511, False), (513, True),
                      (n - 1, False), (n, True)):
        if single:
            out += [g.execute(v) for v in c.x[a:b]]
        else:
            out.append(g.execute_block(c.x[a:b]))
        a = b
    c.check(np.concatenate(out))


# ------------------------------------------------------------------------ firpfb
PFB = pytest.mark.parametrize("row", IB.PFB_ROWS, ids=IB.row_id)


@pytest.mark.parametrize("name", IB.ENVELOPES + ["carried"])
@PFB
def test_firpfb_bound_block_calls(row, name):
    t, M, hlen, s, route = row
    c = IB.case(t, M, hlen, name, s, True)
    _assert_route(c, route)
    cuts = (IB.CARRIED_CUT,) if name == "carried" else IB.CUTS
    c.check(_run_dev(c))
    c.check(_run_dev(c, cuts))
    c.check(_run_dev(c, cuts, off=1))   # the plain kernel, by the output pointer
    g = _obj(c)
    c.check(np.concatenate([g.execute_block(c.x[a:b]).reshape(-1) for a, b in ((0, 320), (320, len(c.x)))]))


@PFB
def test_firpfb_bound_push_execute_between_blocks(row):
    """The window's authority moves from the device copy (after a block) to
    the pinned host mirror (after push) and back: push + execute(i) for every
    bank on runs of single inputs between blocks."""
    t, M, hlen, s, route = row
    c = IB.case(t, M, hlen, "burst", s, True)
    _assert_route(c, route)
    g = _obj(c)
    n, out, a = len(c.x), [], 0
    for b, single in ((2, True), (100, False), (103, True), (255, False), (258, True), (511, False),
                      (513, True), (n - 1, False), (n, True)):
        if single:
            for v in c.x[a:b]:
                g.push(v)
                out.append(np.array([g.execute(i) for i in range(M)], c.x.dtype))
        else:
            out.append(g.execute_block(c.x[a:b]).reshape(-1))
        a = b
    c.check(np.concatenate(out))


# ------------------------------------------------------------------ long filters
def test_firinterp_longest_filter_and_limit():
    """The plain kernel holds a tile of 256 inputs and the L - 1 before them
    in LDS: the longest phase it can take (liquid_mi355x_firinterp_max_taps)
    runs and meets the bound; one tap per phase more is refused by
    firinterp_*_create and firpfb_*_create with a message and exit(1) -- the
    reference's error convention -- before any launch."""
    L = LQ.firinterp_max_taps("crcf")
    assert L >= 7936 and LQ.firinterp_route("crcf", 2, L) == 0
    c = IB.case("crcf", 2, 2 * L, "burst", n=300)
    assert c.L == L
    c.check(_run_dev(c))
    c.check(_run_dev(c, (1, 64, 65)))
    for ctor in ("LQ.FirInterp(2, np.ones(%d, np.float32))" % (2 * L + 1),
                 "LQ.FirPfb(2, np.ones(%d, np.float32))" % (2 * L + 2)):
        code = ("import sys, numpy as np; sys.path.insert(0, %r); import liquidmi as LQ; %s; print('created')"
                % (LQ.os.path.dirname(LQ.__file__), ctor))
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
        assert p.returncode == 1, (p.returncode, p.stdout, p.stderr)
        assert "exceeds the GPU kernel limit" in p.stderr
        assert "created" not in p.stdout
