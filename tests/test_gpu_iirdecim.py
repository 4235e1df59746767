"""iirdecim and iirinterp on the GPU (lqk_iirfilt_decim / lqk_iirfilt_interp in
csrc/k_iirfilt.hip behind host/iirdecim.c), and iirfilt objects made from
liquid_iirdes designs (the C library does not export iirfilt_*_create_prototype
or _create_lowpass; IirFilt.prototype / IirFilt.lowpass of the binding compose
them from liquid_iirdes and create_sos / create).

A rate changer by M is the full-rate filter with M - 1 of every M outputs
dropped (the first of each group kept) or M - 1 zeros fed after each input
(tests/iirdes_model.py).  The criterion is iirfilt's (tests/iirfilt_model.py):
with y64 the float64 model on the float32 coefficients and
e(y) = max|y - y64| / max|y64| over the stated span,

    e(y_gpu) <= 4 e(y_ref) + 2^-22,

y_ref the reference's float32 result: the fixture's recorded outputs where the
stream is a fixture stream, else the float32 serial model run32, which
reproduces the fixture bit for bit (gen_iirdes.py prints that).  Objects that
are not device-eligible run the library's host loop and equal run32 exactly.

Sizes: RUN samples per lane, TILE per workgroup (full-rate samples), SCAN
tiles per block of the cross-tile scan.  M = 3, 5 and 7 do not divide TILE,
so the first kept (or fed) sample of a tile moves from tile to tile.
"""
import functools

import numpy as np
import pytest

import iirdes_model as DM
import iirfilt_model as IM
import liquidmi as LQ

pytestmark = pytest.mark.gpu

RUN, TILE, SCAN = LQ.IirFilt.RUN, LQ.IirFilt.TILE, LQ.IirFilt.SCAN
TAIL = 64                  # outputs after a stream, for the state check
OBJECTS = ("iirdecim", "iirinterp")
CLS = {"iirdecim": LQ.IirDecim, "iirinterp": LQ.IirInterp}
FX = DM.load_fixture()
BUTTER4 = next(c for c in FX["designs"] if c["name"] == "butter4")      # 2 sections, fc = 0.1
CPOLES1 = next(c for c in FX["streams"] if c["kind"] == "cccf")          # 1 section, complex coefficients


def same_bits(a, b):
    a, b = np.ascontiguousarray(a).view(np.float32), np.ascontiguousarray(b).view(np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(label, y, y32, y64, span=slice(None)):
    e_gpu, e_ref, ok = IM.criterion(label, y, y32, y64, span)
    assert ok, "%s: e_gpu %.3e above 4 x %.3e + 2^-22" % (label, e_gpu, e_ref)


def make(obj, kind, M):
    """the shared filter of a kind: Butterworth 4 at 0.1 (rrrf, crcf), the complex pole pair (cccf)"""
    if kind == "cccf":
        return CLS[obj]("cccf", M, CPOLES1["raw_b"], CPOLES1["raw_a"])
    return CLS[obj].prototype(kind, M, "butter", "lowpass", "sos", 4, 0.1)


def coefs(kind):
    return ("norm", CPOLES1["b"], CPOLES1["a"]) if kind == "cccf" else ("sos", BUTTER4["b"], BUTTER4["a"])


def n_in(obj, nf, M):
    """input samples for nf full-rate samples"""
    return nf if obj == "iirdecim" else nf // M


@functools.lru_cache(maxsize=None)
def shared(obj, kind, M, nf, seed=0):
    """(x, y32, y64) for nf full-rate samples (a multiple of M), computed once: x the object's input,
    y32 / y64 its outputs by the float32 and the float64 model"""
    assert nf % M == 0
    x = IM.noise_input(kind, n_in(obj, nf, M), 7000 + 31 * M + seed)
    form, b, a = coefs(kind)
    xf = DM.full_rate(obj, x, M)
    y32, _ = IM.run32(kind, form, b, a, xf)
    return x, DM.kept(obj, y32, M), DM.kept(obj, IM.run64(kind, form, b, a, xf), M)


def n_out(obj, nf, M):
    return nf // M if obj == "iirdecim" else nf


def calls(obj, nf, M):
    """execute_block's count for nf full-rate samples"""
    return nf // M


# ------------------------------------------------------------------ 1 fixture streams
@pytest.mark.parametrize("name", [c["name"] for c in FX["streams"]])
def test_fixture_stream(name):
    c = next(c for c in FX["streams"] if c["name"] == name)
    cls, kind, M = CLS[c["obj"]], c["kind"], c["M"]
    if c["ctor"] == "default":
        q = cls.default(kind, M, c["order"])
    elif c["ctor"] == "proto":
        q = cls.prototype(kind, M, c["ftype"], c["btype"], c["format"], c["order"], c["fc"], c["f0"], c["Ap"], c["As"])
    else:
        q = cls(kind, M, c["raw_b"], c["raw_a"])
    assert q.device_eligible
    x = DM.stream_input(c)
    y = q.execute_block(x)[:DM.NOUT]
    y64 = DM.kept(c["obj"], IM.run64(kind, c["form"], c["b"], c["a"], DM.full_rate(c["obj"], x, M)), M)[:DM.NOUT]
    assert len(y) == DM.NOUT == len(c["y"])
    check(name, y, c["y"], y64)


# ------------------------------------------------------------------ 2 the constructors that design
DESIGNED = [("butter", "lowpass", "sos", 7, 0.1, 0.0), ("ellip", "bandpass", "sos", 4, 0.1, 0.25),
            ("cheby2", "highpass", "sos", 5, 0.3, 0.0), ("bessel", "bandstop", "sos", 3, 0.1, 0.2),
            ("butter", "lowpass", "sos", 16, 0.2, 0.0)]


@pytest.mark.parametrize("kind", ["rrrf", "crcf", "cccf"])
def test_create_prototype_designs_inside_the_library(kind):
    """iirdecim_*_create_prototype and iirinterp_*_create_prototype design inside the library
    (liquid_iirdes, arrays sized by the design, create_sos).  The same filter built outside, from
    liquid_iirdes's coefficients through iirfilt_*_create_sos, runs the same kernels on the same
    coefficients, so the rate changers' outputs are its outputs bit for bit: every M-th one, or those
    for the stuffed input.  Eligibility: SOS designs of up to 8 sections (an order-8 band-pass, an
    order-16 low-pass)."""
    imp = np.zeros(200, IM.sample_dtype(kind))
    imp[0], imp[7] = 1.0, -0.5
    for ft, bt, fm, order, fc, f0 in DESIGNED:
        B, A = LQ.iirdes(ft, bt, fm, order, fc, f0, 0.5, 50.0)
        assert len(B) // 3 <= 8
        y = LQ.IirFilt.sos(kind, B, A).execute_block(imp)
        d = LQ.IirDecim.prototype(kind, 2, ft, bt, fm, order, fc, f0, 0.5, 50.0)
        assert d.device_eligible
        assert same_bits(d.execute_block(imp), np.ascontiguousarray(y[::2]))
        i = LQ.IirInterp.prototype(kind, 3, ft, bt, fm, order, fc, f0, 0.5, 50.0)
        assert i.device_eligible
        ys = LQ.IirFilt.sos(kind, B, A).execute_block(DM.stuffed(imp[:60], 3))
        assert same_bits(i.execute_block(imp[:60]), ys)


def test_binding_prototype_and_lowpass():
    """IirFilt.prototype / IirFilt.lowpass of the Python binding (the C library has no
    iirfilt_*_create_prototype): the design goes to create_sos or create by its format, and the object
    filters as the models do on liquid_iirdes's coefficients"""
    B, A = LQ.iirdes("butter", "lowpass", "sos", 7, 0.1, 0.0, 0.1, 60.0)
    x = IM.noise_input("crcf", 300, 3)
    q = LQ.IirFilt.lowpass("crcf", 7, 0.1)
    assert q.device_eligible and q.get_length() == 8
    check("lowpass(7, 0.1)", q.execute_block(x), IM.run32("crcf", "sos", B, A, x)[0], IM.run64("crcf", "sos", B, A, x))
    b, a = LQ.iirdes("cheby1", "highpass", "tf", 2, 0.2, 0.0, 0.5, 60.0)
    q = LQ.IirFilt.prototype("rrrf", "cheby1", "highpass", "tf", 2, 0.2, 0.0, 0.5, 60.0)
    xr = IM.noise_input("rrrf", 300, 5)
    assert q.device_eligible and q.get_length() == 3
    check("prototype tf 2", q.execute_block(xr), IM.run32("rrrf", "norm", b, a, xr)[0], IM.run64("rrrf", "norm", b, a, xr))


def test_designs_that_take_the_host_loop():
    """a TF design of order 4 (5 coefficients, NORM form) and an order-18 cascade (9 sections)"""
    x = IM.noise_input("crcf", 300, 4)
    b, a = LQ.iirdes("butter", "lowpass", "tf", 4, 0.2)
    q = LQ.IirFilt.prototype("crcf", "butter", "lowpass", "tf", 4, 0.2)
    assert not q.device_eligible and q.get_length() == 5
    assert same_bits(q.execute_block(x), DM.run32_crcf("norm", b, a, x))
    q = LQ.IirFilt.lowpass("crcf", 18, 0.2)
    B, A = LQ.iirdes("butter", "lowpass", "sos", 18, 0.2)
    assert not q.device_eligible and q.get_length() == 18
    assert same_bits(q.execute_block(x), DM.run32_crcf("sos", B, A, x))
    # order 2 in TF form is one section: eligible
    assert LQ.IirFilt.prototype("crcf", "butter", "lowpass", "tf", 2, 0.25).device_eligible


# ------------------------------------------------------------------ 3 boundary shapes
def lengths(M):
    """full-rate lengths, multiples of M"""
    up = lambda v: (v + M - 1) // M * M   # noqa: E731
    return sorted({M, RUN * M - M, (TILE - 1) // M * M, (TILE // M + 1) * M, up(3 * TILE + 5)} - {0})


SHAPES = [(M, "crcf") for M in (2, 3, 5, 7, 64, TILE)] + [(3, "rrrf"), (3, "cccf")]


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("M,kind", SHAPES)
@pytest.mark.parametrize("obj", OBJECTS)
def test_boundary_shapes(obj, M, kind, k):
    ls = lengths(M)
    if k >= len(ls):
        assert M == TILE        # there the multiple of M below TILE is none
        k = len(ls) - 1
    nf = ls[k]
    x, y32, y64 = shared(obj, kind, M, max(ls))
    q = make(obj, kind, M)
    assert q.device_eligible
    y = q.execute_block(x[:n_in(obj, nf, M)])
    no = n_out(obj, nf, M)
    assert len(y) == no
    check("%s %s M=%d nf=%d" % (obj, kind, M, nf), y, y32[:no], y64[:no])


# ------------------------------------------------------------------ 4 two scan levels
@pytest.mark.parametrize("obj", OBJECTS)
def test_two_scan_levels(obj):
    """More than SCAN tiles, M = 3: the first multiple of 3 above SCAN * TILE full-rate samples.  The
    DC blocker (pole 0.99) as rrrf, as iirfilt's own test of this path."""
    M = 3
    nf = (SCAN * TILE // M + 1) * M
    b, a = np.array([1.0, -1.0], np.float32), np.array([1.0, -0.99], np.float32)
    x = IM.noise_input("rrrf", n_in(obj, nf, M), 79)
    xf = DM.full_rate(obj, x, M)
    y32 = DM.kept(obj, IM.run32("rrrf", "norm", b, a, xf)[0], M)
    y64 = DM.kept(obj, IM.run64("rrrf", "norm", b, a, xf), M)
    q = CLS[obj]("rrrf", M, b, a)
    assert q.device_eligible
    y = q.execute_block(x)
    no = n_out(obj, nf, M)
    assert len(y) == no
    check("%s two levels, whole stream" % obj, y, y32, y64)
    last = n_out(obj, TILE // M * M, M)
    check("%s two levels, last TILE" % obj, y, y32, y64, slice(no - last, no))
    # the state it leaves: the next TAIL outputs (the filter forgets 4 TILE samples back: the model
    # restarts there, on a multiple of M)
    back = 4 * TILE // M * M
    nt = TAIL * M if obj == "iirdecim" else (TAIL + M - 1) // M * M
    x2 = IM.noise_input("rrrf", n_in(obj, nt, M), 80)
    xx = np.concatenate([xf[nf - back:], DM.full_rate(obj, x2, M)])
    m32 = DM.kept(obj, IM.run32("rrrf", "norm", b, a, xx)[0], M)
    m64 = DM.kept(obj, IM.run64("rrrf", "norm", b, a, xx), M)
    t = q.execute_block(x2)
    assert len(t) >= TAIL
    check("%s two levels, next %d" % (obj, len(t)), t, m32[-len(t):], m64[-len(t):])


# ------------------------------------------------------------------ 5 call splitting
@pytest.fixture(params=["gpu", "host"])
def small_calls(request):
    LQ.set_small_calls(request.param == "host")
    yield request.param
    LQ.set_small_calls(False)


NS = (3 * TILE + 5 + 2) // 3 * 3      # full-rate samples of the split stream, M = 3


def run_split(q, obj, x, split, M):
    """x: the object's input for a whole number of calls; cuts counted in calls"""
    per = M if obj == "iirdecim" else 1          # input samples per call
    total = len(x) // per
    if split == "one":
        return q.execute_block(x)
    parts, k = [], 0
    if split == "cuts":
        for c in (1, RUN + 1, TILE // M - 1, total):
            c = min(c, total - k)
            parts.append(q.execute_block(x[k * per:(k + c) * per]))
            k += c
        return np.concatenate(parts)
    sizes, i = (5, RUN, 333, TILE // M + 3), 0   # alternating: one execute, one block
    while k < total:
        one = q.execute(x[k * per:(k + 1) * per]) if obj == "iirdecim" else q.execute(x[k])
        parts.append(np.atleast_1d(one))
        k += 1
        c = min(sizes[i % 4], total - k)
        parts.append(q.execute_block(x[k * per:(k + c) * per]))
        k += c
        i += 1
    return np.concatenate(parts)


@pytest.mark.parametrize("split", ["one", "cuts", "alternating"])
@pytest.mark.parametrize("obj", OBJECTS)
def test_call_splitting(obj, split, small_calls):
    assert LQ.get_small_calls() == (small_calls == "host")
    M = 3
    tail = TAIL * M if obj == "iirdecim" else (TAIL + M - 1) // M * M     # full-rate samples after the stream
    x, y32, y64 = shared(obj, "crcf", M, NS + tail, 1)
    q = make(obj, "crcf", M)
    ni, no = n_in(obj, NS, M), n_out(obj, NS, M)
    y = run_split(q, obj, x[:ni], split, M)
    assert len(y) == no
    check("%s %s (%s singles)" % (obj, split, small_calls), y, y32[:no], y64[:no])
    t = q.execute_block(x[ni:])
    assert len(t) >= TAIL
    check("%s %s, next %d" % (obj, split, len(t)), np.concatenate([y, t]), y32, y64, slice(no, no + len(t)))


@pytest.mark.parametrize("obj", OBJECTS)
def test_single_calls_only(obj, small_calls):
    """execute alone over more than RUN full-rate samples, then a block"""
    M = 3
    x, y32, y64 = shared(obj, "crcf", M, NS + (TAIL * M if obj == "iirdecim" else (TAIL + M - 1) // M * M), 1)
    q = make(obj, "crcf", M)
    per = M if obj == "iirdecim" else 1
    nc = 2 * RUN + 1
    parts = [np.atleast_1d(q.execute(x[k * per:(k + 1) * per]) if obj == "iirdecim" else q.execute(x[k]))
             for k in range(nc)]
    parts.append(q.execute_block(x[nc * per:(TILE // M) * per]))
    y = np.concatenate(parts)
    check("%s singles then block (%s)" % (obj, small_calls), y, y32[:len(y)], y64[:len(y)])


# ------------------------------------------------------------------ 6 device pointers, host aliasing
@pytest.mark.parametrize("M,kind", [(3, "crcf"), (3, "rrrf"), (64, "crcf")])
@pytest.mark.parametrize("obj", OBJECTS)
def test_device_pointers(obj, M, kind):
    nf = (3 * TILE + 5 + M - 1) // M * M
    x = shared(obj, kind, M, max(lengths(M)))[0][:n_in(obj, nf, M)]
    esz, no, nc = x.itemsize, n_out(obj, nf, M), calls(obj, nf, M)
    host = make(obj, kind, M).execute_block(x)
    q = make(obj, kind, M)
    dx, dy = LQ.DeviceBuffer.from_array(x), LQ.DeviceBuffer(esz * no)
    q.execute_block_dev(dx.p, nc, dy.p)
    q.synchronize()
    assert same_bits(dy.to_array(x.dtype, no), host)
    # pointers offset by one sample: not 16-byte aligned (the scalar path of the loads and stores)
    q2 = make(obj, kind, M)
    d2 = LQ.DeviceBuffer.from_array(np.concatenate([np.zeros(1, x.dtype), x]))
    y2 = LQ.DeviceBuffer(esz * (no + 2))
    q2.execute_block_dev(d2.p + esz, nc, y2.p + esz)
    q2.synchronize()
    assert same_bits(y2.to_array(x.dtype, no + 1)[1:], host)


def test_decimator_in_place_with_host_pointers():
    """y == x through execute_block: the library stages the input on the device"""
    M = 3
    nf = (3 * TILE + 5 + M - 1) // M * M
    x = shared("iirdecim", "crcf", M, max(lengths(M)))[0][:nf]
    host = make("iirdecim", "crcf", M).execute_block(x)
    q, xx = make("iirdecim", "crcf", M), x.copy()
    q._fn("_execute_block")(q.q, LQ.ptr(xx), nf // M, LQ.ptr(xx))
    assert same_bits(xx[:nf // M], host)
    # and in the host loop (an object that is not eligible)
    q = LQ.IirDecim.default("crcf", M, 18)
    assert not q.device_eligible
    want = q.execute_block(x[:999])
    q.reset()
    xx = x[:999].copy()
    q._fn("_execute_block")(q.q, LQ.ptr(xx), 333, LQ.ptr(xx))
    assert same_bits(xx[:333], want)


# ------------------------------------------------------------------ 7 objects that are not device-eligible
NOT_ELIGIBLE = ["M=TILE+1", "order 18", "TF order 4"]


@pytest.mark.parametrize("why", NOT_ELIGIBLE)
@pytest.mark.parametrize("obj", OBJECTS)
def test_not_eligible_objects_equal_the_float32_model(obj, why):
    cls = CLS[obj]
    if why == "M=TILE+1":
        M, (form, b, a) = TILE + 1, coefs("crcf")
        q = make(obj, "crcf", M)
        assert make(obj, "crcf", TILE).device_eligible
    elif why == "order 18":
        M, form = 3, "sos"
        b, a = LQ.iirdes("butter", "lowpass", "sos", 18, float(np.float32(0.5) / np.float32(M)))
        q = cls.default("crcf", M, 18)
    else:
        M, form = 3, "norm"
        b, a = LQ.iirdes("butter", "lowpass", "tf", 4, 0.15)
        q = cls.prototype("crcf", M, "butter", "lowpass", "tf", 4, 0.15)
    assert not q.device_eligible
    nc = 3 if M > TILE else 700
    x = IM.noise_input("crcf", n_in(obj, nc * M, M), 11)
    y32 = DM.kept(obj, DM.run32_crcf(form, b, a, DM.full_rate(obj, x, M)), M)
    per = M if obj == "iirdecim" else 1
    # a block, then single calls, then device pointers: one stream
    k1, k2 = nc // 2, nc // 2 + (1 if M > TILE else 5)   # the calls of the three parts
    parts = [q.execute_block(x[:k1 * per])]
    for k in range(k1, k2):
        parts.append(np.atleast_1d(q.execute(x[k * per:(k + 1) * per]) if obj == "iirdecim" else q.execute(x[k])))
    rest = x[k2 * per:]
    dx, dy = LQ.DeviceBuffer.from_array(rest), LQ.DeviceBuffer(x.itemsize * n_out(obj, (nc - k2) * M, M))
    q.execute_block_dev(dx.p, nc - k2, dy.p)
    q.synchronize()
    parts.append(dy.to_array(x.dtype, n_out(obj, (nc - k2) * M, M)))
    assert same_bits(np.concatenate(parts), y32)


# ------------------------------------------------------------------ 8 reset, groupdelay, argument checks
@pytest.mark.parametrize("obj", OBJECTS)
def test_reset(obj, small_calls):
    M = 3
    nf = (TILE + RUN + 1 + M - 1) // M * M
    x = shared(obj, "crcf", M, max(lengths(M)))[0][:n_in(obj, nf, M)]
    per = M if obj == "iirdecim" else 1
    q = make(obj, "crcf", M)
    first = q.execute_block(x)
    q.execute(x[:per] if obj == "iirdecim" else x[0])
    q.reset()
    assert same_bits(q.execute_block(x), first)
    q.reset()
    two = np.concatenate([q.execute_block(x[:7 * per]), q.execute_block(x[7 * per:])])
    assert same_bits(two[:7 * (1 if obj == "iirdecim" else M)], first[:7 * (1 if obj == "iirdecim" else M)])
    # the second block starts from the state the first left: the stream within the criterion
    _, y32, y64 = shared(obj, "crcf", M, max(lengths(M)))
    check("%s reset, two blocks (%s)" % (obj, small_calls), two, y32[:len(two)], y64[:len(two)])


@pytest.mark.parametrize("M", [2, 5])
def test_groupdelay(M):
    f = LQ.IirFilt.prototype("crcf", "butter", "lowpass", "sos", 4, 0.1)
    d, i = make("iirdecim", "crcf", M), make("iirinterp", "crcf", M)
    for fc in (0.01, 0.05, 0.2):
        g = np.float32(f.groupdelay(fc))
        assert np.float32(d.groupdelay(fc)) == g
        assert np.float32(i.groupdelay(fc)) == g / np.float32(M)


@pytest.mark.parametrize("obj", OBJECTS)
def test_factor_below_two_exits_like_the_reference(obj):
    import os
    import subprocess
    import sys
    for ctor, msg in (("%s_crcf_create_default(1, 4)", "error: iirinterp_crcf_create_prototype(), interp factor must "
                       "be greater than 1\n"),
                      ("%s_crcf_create(1, LQ.ptr(b), 3, LQ.ptr(b), 3)", "error: iirinterp_crcf_create(), interp factor "
                       "must be greater than 1\n")):
        code = ("import sys; sys.path.insert(0, %r); import numpy as np, liquidmi as LQ\n"
                "b = np.ones(3, np.float32); LQ.lib().%s\n" % (os.path.dirname(LQ.__file__), ctor % obj))
        res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
        assert res.returncode == 1 and res.stderr.endswith(msg), (res.returncode, res.stderr)
