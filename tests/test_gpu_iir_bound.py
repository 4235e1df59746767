"""iirfilt, iirdecim and iirinterp on the GPU (csrc/k_iirfilt.hip behind
host/iirfilt.c and host/iirdecim.c) held to the bound local to each output of
tests/iir_bound.py:

    |y[n] - y64[n]| <= 4 2^-23 A[n] + 2^-126 U[n],   exactly 0 before the first input,

and to the margin r <= 4 r_ref against the serial float32 model (iir_bound's
docstring has both, with their derivation).  Every output of every row is
checked, and every row first asserts the launch structure its call takes
(liquidmi.iirfilt_route: "apply" alone, "scan1" one scan launch, "scan3" three).

The kernels are instantiated per (KIND, MS, MODE), MS the section count
rounded up to 1, 2, 4 or 8.  Rows that cross a tile seam (k_iir_tile,
k_iir_scan and a k_iir_apply of several workgroups all run):

    MS   rrrf                        crcf                         cccf
    PLAIN  (test_plain_short; MS 1 and 8 also test_call_patterns, test_structure_edges)
    1    dc001 leak12 leak20 accum   dc01 leak12 leak20 accum     cpoles1
    2    butter4                     butter4                      cpoles2
    4    ellip8                      ellip5 ellip8 b4leaks(long)  ellip8
    8    cascade8                    cascade8                     slow8
    DECIM and INTERP  (test_rate_short, test_rate_scan_edge)
    1    leak12
    4                                ellip8 (create_prototype)
    8                                                             butter16 (create_prototype)

Scan launches: "scan1" at NS = 3 TILE + 5 and at SCAN TILE (256 tiles, 255
vectors), "scan3" at SCAN TILE + 1 and on the long stream (513 tiles in
three chunks, after a loud first call of 777 samples, so that the top scan
applies its step to a non-zero state).
"""
import functools

import numpy as np
import pytest

import iir_bound as IB
import liquidmi as LQ

pytestmark = pytest.mark.gpu

RUN, TILE, SCAN = LQ.IirFilt.RUN, LQ.IirFilt.TILE, LQ.IirFilt.SCAN
NS, CUT, TAIL = IB.NS, IB.CUT, 64
PLAIN_ROWS = [(f, k, ms, e) for f, k, ms in IB.ROWS for e in IB.envelopes(f)]
PATTERN_FILTERS = [("slow8", "cccf"), ("cascade8", "crcf"), ("leak12", "rrrf")]
EDGE_FILTERS = [("leak20", "rrrf"), ("slow8", "cccf")]


def test_geometry():
    assert (RUN, TILE, SCAN) == (IB.RUN, IB.TILE, IB.SCAN)
    assert [LQ.iirfilt_route(n) for n in (1, TILE, TILE + 1, SCAN * TILE, SCAN * TILE + 1, IB.NLONG)] == [
        "apply", "apply", "scan1", "scan1", "scan3", "scan3"]


def make(fname, kind):
    form, b, a = IB.coefs(fname, kind)
    q = LQ.IirFilt(kind, b, a) if form == "norm" else LQ.IirFilt.sos(kind, b, a)
    assert q.device_eligible          # the accumulator too: a pole on the circle qualifies
    return q


def bits(a):
    return np.ascontiguousarray(a).view(np.float32).view(np.uint32)


def hold(label, fname, kind, y, x, y64, A, U, span=slice(None)):
    """the bound and the margin over every output of the span; prints the row's figures"""
    assert len(y) == len(y64)
    ok, r, w = IB.verdict(y, x, y64, A, U, span)
    rr = IB.r_ref(fname, kind)
    print("iir_bound %-52s r_gpu %.3f at %8d  r_ref %.3f  r_gpu/r_ref %5.2f  %s"
          % (label, r, w, rr, r / rr, "ok" if ok and r <= IB.MARGIN * rr else "MISS"))
    assert ok, "%s: outside 4 2^-23 A + 2^-126 U (r = %.3g with K = 1, at %d), or not 0 before the first input" % (label, r, w)
    assert r <= IB.MARGIN * rr, "%s: r_gpu %.3g above %g x r_ref %.3g (at %d)" % (label, r, IB.MARGIN, rr, w)


def run_calls(q, x, sizes, routes=None):
    """x in calls of the given sizes (the last takes the rest); asserts each call's route if given"""
    parts, k = [], 0
    for i, c in enumerate(sizes):
        c = len(x) - k if i == len(sizes) - 1 else c
        if routes is not None:
            assert LQ.iirfilt_route(c) == routes[i], (c, routes[i])
        parts.append(q.execute_block(x[k:k + c]))
        k += c
    assert k == len(x)
    return np.concatenate(parts)


# ------------------------------------------------------------------ 1 PLAIN, the short stream
@pytest.mark.parametrize("fname,kind,ms,envelope", PLAIN_ROWS, ids=["%s_%s_%s" % (r[0], r[1], r[3]) for r in PLAIN_ROWS])
def test_plain_short(fname, kind, ms, envelope):
    assert LQ.iirfilt_route(NS) == "scan1"
    x, y64, A, U = IB.case(fname, kind, envelope)
    y = make(fname, kind).execute_block(x)
    hold("%s %s MS=%d %s" % (fname, kind, ms, envelope), fname, kind, y, x, y64, A, U)


@pytest.mark.parametrize("fname,kind", [("cascade8", "crcf"), ("slow8", "cccf"), ("butter4", "rrrf")])
def test_silence(fname, kind):
    """exact zeros in: exact zeros out, across tile seams; then zeros ahead of a stream"""
    assert LQ.iirfilt_route(2 * TILE + 3) == "scan1"
    q = make(fname, kind)
    z = np.zeros(2 * TILE + 3, IB.IM.sample_dtype(kind))
    assert not np.any(q.execute_block(z))
    x = np.concatenate([z[:TILE + 7], IB.case(fname, kind, "gaps")[0][:TILE + 100]])
    y64, A, U = IB.scale(fname, x)
    assert IB.first_input(x) >= TILE + 7
    hold("%s %s zeros, then gaps" % (fname, kind), fname, kind, q.execute_block(x), x, y64, A, U)


# ------------------------------------------------------------------ 2 call patterns
@pytest.fixture(params=["gpu", "host"])
def small_calls(request):
    LQ.set_small_calls(request.param == "host")
    yield request.param
    LQ.set_small_calls(False)


def tail_check(label, q, y, fname, kind, x, y64, A, U):
    """the state the object is left with: the next TAIL outputs against the same bound"""
    assert LQ.iirfilt_route(TAIL) == "apply"
    t = q.execute_block(x[NS:])
    hold(label + ", next %d" % TAIL, fname, kind, np.concatenate([y, t]), x, y64, A, U, slice(NS, NS + TAIL))


@pytest.mark.parametrize("pattern", ["one", "cuts", "cut"])
@pytest.mark.parametrize("fname,kind", PATTERN_FILTERS)
def test_call_patterns(fname, kind, pattern):
    x, y64, A, U = IB.case(fname, kind, "burst", NS + TAIL)
    sizes, routes = {"one": ((NS,), ("scan1",)),
                     "cuts": ((1, RUN + 1, TILE - 1, 0), ("apply", "apply", "apply", "scan1")),
                     # the run [CUT - 30, CUT) reaches the second call through the state alone
                     "cut": ((CUT, 0), ("scan1", "apply"))}[pattern]
    q = make(fname, kind)
    y = run_calls(q, x[:NS], sizes, routes)
    label = "%s %s %s" % (fname, kind, pattern)
    hold(label, fname, kind, y, x[:NS], y64[:NS], A[:NS], U[:NS])
    tail_check(label, q, y, fname, kind, x, y64, A, U)


@pytest.mark.parametrize("fname,kind", PATTERN_FILTERS)
def test_single_calls_between_blocks(fname, kind, small_calls):
    """one execute, one block, in turn; the singles on the GPU or in the host loop"""
    assert LQ.get_small_calls() == (small_calls == "host")
    x, y64, A, U = IB.case(fname, kind, "burst", NS + TAIL)
    q = make(fname, kind)
    parts, k, i, sizes = [], 0, 0, (5, RUN, 333, TILE + 3)
    while k < NS:
        parts.append(np.array([q.execute(x[k])], x.dtype))
        k += 1
        c = min(sizes[i % 4], NS - k)
        assert LQ.iirfilt_route(max(c, 1)) == ("scan1" if c > TILE else "apply")
        parts.append(q.execute_block(x[k:k + c]))
        k += c
        i += 1
    y = np.concatenate(parts)
    label = "%s %s alternating (%s singles)" % (fname, kind, small_calls)
    hold(label, fname, kind, y, x[:NS], y64[:NS], A[:NS], U[:NS])
    tail_check(label, q, y, fname, kind, x, y64, A, U)


@pytest.mark.parametrize("fname,kind", PATTERN_FILTERS)
def test_device_pointers(fname, kind):
    """aligned and one sample off 16 bytes, out of place and in place: the host-pointer result bit
    for bit (which test_call_patterns[one] holds to the bound)"""
    x = np.array(IB.case(fname, kind, "burst")[0])
    esz = x.itemsize
    host = make(fname, kind).execute_block(x)
    for off in (0, 1):
        for in_place in (False, True):
            q = make(fname, kind)
            dx = LQ.DeviceBuffer.from_array(np.concatenate([np.zeros(off, x.dtype), x]))
            dy = dx if in_place else LQ.DeviceBuffer(esz * (NS + off))
            assert ((dx.p + off * esz) % 16 == 0) == (off == 0)
            q.execute_block_dev(dx.p + off * esz, NS, dy.p + off * esz)
            q.synchronize()
            out = dy.to_array(x.dtype, NS + off)[off:]
            assert np.array_equal(bits(out), bits(host)), (off, in_place)


# ------------------------------------------------------------------ 3 structure edges
@pytest.mark.parametrize("n,route", [(TILE, "apply"), (TILE + 1, "scan1"), (SCAN * TILE, "scan1"), (SCAN * TILE + 1, "scan3")])
@pytest.mark.parametrize("fname,kind", EDGE_FILTERS)
def test_structure_edges(fname, kind, n, route):
    assert LQ.iirfilt_route(n) == route
    x, y64, A, U = IB.case(fname, kind, "burst", n)
    y = make(fname, kind).execute_block(x)
    hold("%s %s n=%d (%s)" % (fname, kind, n, route), fname, kind, y, x, y64, A, U)


@pytest.mark.parametrize("fname,kind", EDGE_FILTERS + [("b4leaks", "crcf")])
def test_long_stream_after_a_first_call(fname, kind):
    """513 tiles in three chunks, the object's state loud from a first call: the top-level scan has
    a carry to apply its step to.  Every output of both calls; the cascade with second-order
    sections too (its |g| are short enough for the whole stream's scale)."""
    x, y64, A, U = IB.long_case(fname, kind)
    q = make(fname, kind)
    y = run_calls(q, x, (IB.FIRST, 0), ("apply", "scan3"))
    hold("%s %s long stream after %d" % (fname, kind, IB.FIRST), fname, kind, y, x, y64, A, U)


# ------------------------------------------------------------------ 4 DECIM and INTERP
CLS = {"iirdecim": LQ.IirDecim, "iirinterp": LQ.IirInterp}
RATE_FILTERS = {"leak12": ("rrrf", None),
                "lib_ellip8": ("crcf", ("ellip", "lowpass", "sos", 8, 0.12, 0.0, 0.2, 50.0)),
                "lib_butter16": ("cccf", ("butter", "lowpass", "sos", 16, 0.2, 0.0, 0.1, 60.0))}
RATE_ROWS = [(o, f, M) for o in CLS for f in RATE_FILTERS for M in (3, 64)]
NBIG = SCAN * TILE + 64


@functools.lru_cache(maxsize=None)
def rate_filter(fname):
    """registers the designed filters with iir_bound: the coefficients liquid_iirdes gives, as
    create_prototype hands them to the engine (normalised per section in float32)"""
    kind, design = RATE_FILTERS[fname]
    if design is not None:
        B, A = LQ.iirdes(*design)
        b, a = B.copy(), A.copy()
        for k in range(len(B) // 3):
            b[3 * k:3 * k + 3] = B[3 * k:3 * k + 3] / A[3 * k]
            a[3 * k:3 * k + 3] = A[3 * k:3 * k + 3] / A[3 * k]
        IB.register(fname, "sos", b, a)
        if fname == "lib_ellip8":     # the design of tests/golden/iirdes.json
            assert np.allclose(b, IB.FILTERS["ellip8"][1], rtol=1e-5, atol=1e-7)
    return kind


def make_rate(obj, fname, M):
    kind, design = RATE_FILTERS[fname]
    if design is None:
        _, b, a = IB.coefs(fname, kind)
        q = CLS[obj](kind, M, b[:1], a[:2])       # create: a NORM form of two coefficients, one section
    else:
        q = CLS[obj].prototype(kind, M, *design)
    assert q.device_eligible
    return q


@functools.lru_cache(maxsize=None)
def rate_case(obj, fname, M, n, envelope="burst"):
    """(x_in, x_full, y64, A, U) over n full-rate samples, n a multiple of M.  iirdecim: the input is
    the full-rate stream.  iirinterp: every M-th sample of it, and the scale is that of the stuffed
    stream.  The stream is a prefix of one drawn per filter, and the scale is causal."""
    kind = rate_filter(fname)
    full = IB.stream(kind, NBIG, envelope, IB.seed_of(fname, kind, envelope))
    if obj == "iirdecim":
        xf = full if n > NS else full[:NS // M * M]
        y64, A, U = rate_scale(fname, None, envelope, len(xf))
        return xf[:n], xf[:n], y64[:n], A[:n], U[:n]
    xf = np.zeros(NBIG // M * M if n > NS else NS // M * M, full.dtype)
    xf[::M] = full[:len(xf):M]
    y64, A, U = rate_scale(fname, M, envelope, len(xf))
    return np.ascontiguousarray(xf[:n:M]), xf[:n], y64[:n], A[:n], U[:n]


@functools.lru_cache(maxsize=None)
def rate_scale(fname, stuffed_by, envelope, n):
    kind = rate_filter(fname)
    full = IB.stream(kind, NBIG, envelope, IB.seed_of(fname, kind, envelope))
    if stuffed_by is None:
        return IB.scale(fname, full[:n])
    xf = np.zeros(n, full.dtype)
    xf[::stuffed_by] = full[:n:stuffed_by]
    return IB.scale(fname, xf)


def hold_rate(label, obj, fname, M, y, xf, y64, A, U):
    """iirdecim: the full-rate scale at the kept samples; the zero rule by the inputs up to each"""
    kind = RATE_FILTERS[fname][0]
    if obj == "iirdecim":
        seen = (np.cumsum(xf != 0)[::M] > 0).astype(np.float32)
        hold(label, fname, kind, y, seen, y64[::M], A[::M], U[::M])
    else:
        hold(label, fname, kind, y, xf, y64, A, U)


def rate_calls(q, obj, M, x_in, cuts):
    """the input in calls cut at the full-rate positions cuts (multiples of M)"""
    parts, k = [], 0
    for c in list(cuts) + [len(x_in) * (M if obj == "iirinterp" else 1)]:
        assert c % M == 0
        c_in = c if obj == "iirdecim" else c // M
        if c_in > k:
            parts.append(q.execute_block(x_in[k:c_in]))
        k = max(k, c_in)
    return np.concatenate(parts)


@pytest.mark.parametrize("obj,fname,M", RATE_ROWS)
def test_rate_short(obj, fname, M):
    """M = 3 does not divide TILE: the first kept (or fed) sample of a tile moves from tile to tile"""
    nf = NS // M * M
    assert LQ.iirfilt_route(nf) == "scan1"
    x_in, xf, y64, A, U = rate_case(obj, fname, M, nf)
    up = lambda v: (v + M - 1) // M * M
    cuts = (up(1), up(RUN + 2), up(TILE + RUN + 1))
    for name, c in (("one call", ()), ("cuts", cuts)):
        y = rate_calls(make_rate(obj, fname, M), obj, M, x_in, c)
        hold_rate("%s %s M=%d %s" % (obj, fname, M, name), obj, fname, M, y, xf, y64, A, U)


@pytest.mark.parametrize("obj,fname,M", RATE_ROWS)
def test_rate_scan_edge(obj, fname, M):
    """the largest full-rate size with one scan launch and the smallest with three"""
    n1 = SCAN * TILE // M * M
    for n, route in ((n1, "scan1"), (n1 + M, "scan3")):
        assert LQ.iirfilt_route(n) == route and n <= NBIG
        x_in, xf, y64, A, U = rate_case(obj, fname, M, n)
        y = make_rate(obj, fname, M).execute_block(x_in)
        hold_rate("%s %s M=%d n=%d (%s)" % (obj, fname, M, n, route), obj, fname, M, y, xf, y64, A, U)
