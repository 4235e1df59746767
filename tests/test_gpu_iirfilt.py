"""iirfilt on the GPU (csrc/k_iirfilt.hip behind host/iirfilt.c).

Criterion (tests/iirfilt_model.py): with y64 the float64 model on the float32
coefficients and e(y) = max|y - y64| / max|y64| over the stated span,

    e(y_gpu) <= 4 e(y_ref) + 2^-22,

y_ref the reference's float32 result: the fixture's recorded outputs where the
stream is a fixture stream, else the float32 serial model (which reproduces
the fixture bit for bit, tests/test_iirfilt_model.py).  Every comparison
prints e_gpu, e_ref and their ratio.  Objects that are not device-eligible run
the library's host loop and equal the float32 model exactly.

Sizes: RUN samples per lane, TILE per workgroup, SCAN tiles per block of the
cross-tile scan.  conftest.py forces single calls onto the GPU; the host
small-call path is switched on by a fixture where it is the subject.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import iirfilt_model as IM
import liquidmi as LQ

pytestmark = pytest.mark.gpu

RUN, TILE, SCAN = LQ.IirFilt.RUN, LQ.IirFilt.TILE, LQ.IirFilt.SCAN
NS = 3 * TILE + 5          # the shared stream
TAIL = 64                  # samples after it, for the state check
FILTERS = ("dc_blocker_0.01_crcf", "butter4_rrrf", "cpoles2_cccf")


@functools.lru_cache(maxsize=None)
def fixture():
    return IM.load_fixture()


def case_names():
    return [c["name"] for c in fixture()["cases"]]


def case(name):
    return next(c for c in fixture()["cases"] if c["name"] == name)


def make(c, kind=None):
    k = kind or c["kind"]
    ctor = c["ctor"]
    if ctor == "dc_blocker":
        return LQ.IirFilt.dc_blocker(k, c["alpha"])
    if ctor == "pll":
        return LQ.IirFilt.pll(k, c["w"], c["zeta"], c["K"])
    if ctor == "integrator":
        return LQ.IirFilt.integrator(k)
    if ctor == "differentiator":
        return LQ.IirFilt.differentiator(k)
    if ctor == "create_sos":
        return LQ.IirFilt.sos(k, c["raw_b"], c["raw_a"])
    return LQ.IirFilt(k, c["raw_b"], c["raw_a"])


def bits(a):
    return np.ascontiguousarray(a).view(np.float32).view(np.uint32)


def expect_eligible(c):
    """the eligibility rule, from the float32 coefficients in float64: finite, at most 8 sections or
    3 coefficients, every pole of every section within the unit circle"""
    b, a = np.asarray(c["b"]).astype(np.complex128), np.asarray(c["a"]).astype(np.complex128)
    if not (np.all(np.isfinite(b)) and np.all(np.isfinite(a))):
        return False
    if c["form"] == "norm":
        return max(len(b), len(a)) <= 3 and (len(a) < 2 or bool(np.all(np.abs(np.roots(a)) <= 1 + 1e-9)))
    return len(a) // 3 <= 8 and all(np.all(np.abs(np.roots(a[3 * k:3 * k + 3])) <= 1 + 1e-9) for k in range(len(a) // 3))


def same_bits(a, b):
    """bit for bit; a NaN equals a NaN (its sign and payload are the platform's)"""
    a, b = np.ascontiguousarray(a).view(np.float32), np.ascontiguousarray(b).view(np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


@functools.lru_cache(maxsize=None)
def shared(name, envelope="flat"):
    """(x, y32, y64) over NS + TAIL samples for one of FILTERS, computed once"""
    c = case(name)
    n = NS + TAIL
    level = None
    if envelope == "burst":   # the middle third of the NS samples at level 1, the rest at 1e-4
        level = np.full(n, 1e-4)
        level[NS // 3:2 * NS // 3] = 1.0
    x = IM.noise_input(c["kind"], n, 9000 + FILTERS.index(name), level)
    y32, _ = IM.run32(c["kind"], c["form"], c["b"], c["a"], x)
    return x, y32, IM.run64(c["kind"], c["form"], c["b"], c["a"], x)


def check(label, y, y32, y64, span=slice(None)):
    e_gpu, e_ref, ok = IM.criterion(label, y, y32, y64, span)
    assert ok, "%s: e_gpu %.3e above 4 x %.3e + 2^-22" % (label, e_gpu, e_ref)


# ------------------------------------------------------------------ 1 fixture streams
@pytest.mark.parametrize("name", case_names())
def test_fixture_stream(name):
    c = case(name)
    x = IM.case_input(c)
    q = make(c)
    y = q.execute_block(x)
    if not expect_eligible(c):
        # a pole outside the unit circle (radius 1.01; the PLL filter's float32 coefficients put one at
        # 1.00024), or coefficients that are not finite (the reference's integrator takes the fourth
        # root of a negative gain): the host loop, the reference's arithmetic
        assert not q.device_eligible
        y32, _ = IM.run32(c["kind"], c["form"], c["b"], c["a"], x)
        assert same_bits(y, y32) and same_bits(y, c["y"])
        return
    assert q.device_eligible
    assert q.get_length() == (len(c["b"]) // 3 * 2 if c["form"] == "sos" else max(len(c["b"]), len(c["a"])))
    check(name, y, c["y"], IM.run64(c["kind"], c["form"], c["b"], c["a"], x))


@pytest.mark.parametrize("k", range(9), ids=[v["name"] for v in fixture()["vectors"]])
def test_autotest_vectors(k):
    """iirfilt_runtest.c: tolerance 0.001.  The 5- and 7-coefficient forms
    are NORM forms too long for the device: host loop, the model exactly."""
    v = fixture()["vectors"][k]
    q = LQ.IirFilt(v["kind"], v["b"], v["a"])
    y = q.execute_block(v["x"])
    assert np.max(np.abs(y - v["y"])) < v["tol"]
    y32, _ = IM.run32(v["kind"], "norm", v["bn"], v["an"], v["x"])
    if len(v["bn"]) > 3:
        assert not q.device_eligible and q.get_length() == len(v["bn"])
        assert same_bits(y, y32)
    else:
        assert q.device_eligible and q.get_length() == 3
        check(v["name"], y, y32, IM.run64(v["kind"], "norm", v["bn"], v["an"], v["x"]))
    # one sample at a time
    q.reset()
    y1 = np.array([q.execute(s) for s in v["x"]], y.dtype)
    assert np.max(np.abs(y1 - v["y"])) < v["tol"]


# ------------------------------------------------------------------ 2 boundary sizes
SIZES = [1, 2, RUN - 1, RUN, RUN + 1, 64 * RUN - 1, 64 * RUN + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", FILTERS)
def test_boundary_sizes(name, n):
    x, y32, y64 = shared(name)
    q = make(case(name))
    assert q.device_eligible
    y = q.execute_block(x[:n])
    assert len(y) == n
    check("%s n=%d" % (name, n), y, y32[:n], y64[:n])


# ------------------------------------------------------------------ 3 two scan levels
def test_two_scan_levels():
    """More than SCAN tiles: the cross-tile scan reduces chunks of SCAN tiles,
    scans the chunk totals and scans within the chunks.  The smallest such n
    is SCAN * TILE + 1 (SCAN + 1 tiles, the last of one sample)."""
    n = SCAN * TILE + 1
    c = case("dc_blocker_0.01_crcf")          # the same real coefficients, as rrrf
    x = IM.noise_input("rrrf", n, 77)
    y32, _ = IM.run32("rrrf", "norm", c["b"], c["a"], x)
    y64 = IM.run64("rrrf", "norm", c["b"], c["a"], x)
    q = make(c, "rrrf")
    assert q.device_eligible
    y = q.execute_block(x)
    check("two levels, whole stream", y, y32, y64)
    check("two levels, last TILE", y, y32, y64, slice(n - TILE, n))
    # and the state it leaves
    x2 = IM.noise_input("rrrf", TAIL, 78)
    xx = np.concatenate([x[n - 4 * TILE:], x2])
    # (a DC blocker with pole 0.99 forgets 4 TILE samples back: the model restarts there)
    m32, _ = IM.run32("rrrf", "norm", c["b"], c["a"], xx)
    m64 = IM.run64("rrrf", "norm", c["b"], c["a"], xx)
    check("two levels, next %d" % TAIL, q.execute_block(x2), m32[-TAIL:], m64[-TAIL:])


# ------------------------------------------------------------------ 4 burst
@pytest.mark.parametrize("name", ["dc_blocker_0.01_crcf", "butter4_rrrf"])
def test_burst(name):
    x, y32, y64 = shared(name, "burst")
    q = make(case(name))
    y = q.execute_block(x[:NS])
    for i, (a, b) in enumerate(((0, NS // 3), (NS // 3, 2 * NS // 3), (2 * NS // 3, NS))):
        check("%s burst, third %d" % (name, i), y, y32[:NS], y64[:NS], slice(a, b))


# ------------------------------------------------------------------ 5 call splitting
@pytest.fixture(params=["gpu", "host"])
def small_calls(request):
    LQ.set_small_calls(request.param == "host")
    yield request.param
    LQ.set_small_calls(False)


def run_split(q, x, split):
    if split == "one":
        return q.execute_block(x)
    parts, k = [], 0
    if split == "cuts":
        for c in (1, RUN + 1, TILE - 1, len(x)):
            parts.append(q.execute_block(x[k:k + c]))
            k += c
        return np.concatenate(parts)
    sizes, i = (5, RUN, 333, TILE + 3), 0     # alternating: one execute, one block
    while k < len(x):
        parts.append(np.array([q.execute(x[k])], x.dtype))
        k += 1
        parts.append(q.execute_block(x[k:k + sizes[i % 4]]))
        k += sizes[i % 4]
        i += 1
    return np.concatenate(parts)


@pytest.mark.parametrize("split", ["one", "cuts", "alternating"])
@pytest.mark.parametrize("name", FILTERS)
def test_call_splitting(name, split, small_calls):
    assert LQ.get_small_calls() == (small_calls == "host")
    x, y32, y64 = shared(name)
    q = make(case(name))
    y = run_split(q, x[:NS], split)
    assert len(y) == NS
    check("%s %s (%s singles)" % (name, split, small_calls), y, y32[:NS], y64[:NS])
    # the state the object is left with: the next TAIL outputs
    t = q.execute_block(x[NS:])
    check("%s %s, next %d" % (name, split, TAIL), np.concatenate([y, t]), y32, y64, slice(NS, NS + TAIL))


def test_single_calls_only(small_calls):
    """execute alone over more than RUN samples, then a block"""
    x, y32, y64 = shared("cpoles2_cccf")
    q = make(case("cpoles2_cccf"))
    n = 3 * RUN + 1
    y = np.array([q.execute(v) for v in x[:n]], np.complex64)
    y = np.concatenate([y, q.execute_block(x[n:TILE])])
    check("singles then block (%s)" % small_calls, y, y32[:TILE], y64[:TILE])


# ------------------------------------------------------------------ 6 in place, device pointers
@pytest.mark.parametrize("name", FILTERS)
def test_in_place_and_device_pointers(name):
    c = case(name)
    x = shared(name)[0][:NS]
    esz = x.itemsize
    host = make(c).execute_block(x)
    q = make(c)
    dx, dy = LQ.DeviceBuffer.from_array(x), LQ.DeviceBuffer(esz * NS)
    q.execute_block_dev(dx.p, NS, dy.p)
    q.synchronize()
    out = dy.to_array(x.dtype, NS)
    assert same_bits(out, host)
    q2 = make(c)
    q2.execute_block_dev(dx.p, NS, dx.p)
    q2.synchronize()
    assert same_bits(dx.to_array(x.dtype, NS), host)
    # host pointers in place
    xx = x.copy()
    q3 = make(c)
    q3._fn("_execute_block")(q3.q, LQ.ptr(xx), NS, LQ.ptr(xx))
    assert same_bits(xx, host)
    # a device pointer that is not 16-byte aligned
    q4 = make(c)
    d4 = LQ.DeviceBuffer.from_array(np.concatenate([np.zeros(1, x.dtype), x]))
    q4.execute_block_dev(d4.p + esz, NS, d4.p + esz)
    q4.synchronize()
    assert same_bits(d4.to_array(x.dtype, NS + 1)[1:], host)


def test_device_pointers_on_the_host_path():
    """not device-eligible: device pointers are copied through the host loop"""
    c = case("radius_1.01_crcf")
    x = IM.case_input(c)
    q = make(c)
    d = LQ.DeviceBuffer.from_array(x)
    q.execute_block_dev(d.p, len(x), d.p)
    q.synchronize()
    assert same_bits(d.to_array(x.dtype, len(x)), c["y"])


# ------------------------------------------------------------------ 7 reset
@pytest.mark.parametrize("name", FILTERS)
def test_reset(name, small_calls):
    x = shared(name)[0][:TILE + RUN + 1]
    q = make(case(name))
    first = q.execute_block(x)
    q.execute(x[0])
    q.reset()
    assert same_bits(q.execute_block(x), first)
    q.reset()
    assert same_bits(np.concatenate([q.execute_block(x[:7]), q.execute_block(x[7:])])[:7], first[:7])


# ------------------------------------------------------------------ 8 host-only surface
def h64(b, a, fc, form):
    """the reference's convention: sums of c[i] e^{+j 2 pi fc i}"""
    b, a = np.asarray(b).astype(np.complex128), np.asarray(a).astype(np.complex128)
    if form == "norm":
        return (np.sum(b * np.exp(2j * np.pi * fc * np.arange(len(b))))
                / np.sum(a * np.exp(2j * np.pi * fc * np.arange(len(a)))))
    e = np.exp(2j * np.pi * fc * np.arange(3))
    return np.prod([np.sum(b[3 * k:3 * k + 3] * e) / np.sum(a[3 * k:3 * k + 3] * e) for k in range(len(b) // 3)])


def gd64(b, a, fc):
    """group delay of B/A, real coefficients: Re(sum k c_k e_k / sum c_k e_k) of B minus that of A"""
    def part(c):
        c = np.asarray(c, np.float64)
        k = np.arange(len(c))
        e = np.exp(-2j * np.pi * fc * k)
        return float(np.real(np.sum(k * c * e) / np.sum(c * e)))
    return part(b) - part(a)


@pytest.mark.parametrize("name", ["butter4_rrrf", "ellip5_crcf", "cpoles2_cccf", "a0_is_2_rrrf", "dc_blocker_0.01_crcf"])
def test_freqresponse(name):
    c = case(name)
    q = make(c)
    for fc in (0.01, 0.07, 0.15, 0.3):
        want = h64(c["b"], c["a"], fc, c["form"])
        got = q.freqresponse(fc)
        assert abs(got - want) <= 1e-5 * abs(want), (name, fc, got, want)


@pytest.mark.parametrize("name", ["butter4_rrrf", "butter4_crcf", "a0_is_2_rrrf", "ellip5_crcf"])
def test_groupdelay(name):
    """(not the PLL filter: with both poles within 3e-4 of z = 1 the float32 sums of
    iir_group_delay cancel to about 3e-4 relative, in the reference as here)"""
    c = case(name)
    q = make(c)
    b, a = np.real(c["b"]), np.real(c["a"])
    for fc in (0.02, 0.05, 0.08):
        if c["form"] == "norm":
            want = gd64(b, a, fc)
        else:
            want = sum(gd64(b[3 * k:3 * k + 3], a[3 * k:3 * k + 3], fc) for k in range(len(b) // 3))
        got = q.groupdelay(fc)
        print("groupdelay %s fc=%g: %.7f (float64 %.7f)" % (name, fc, got, want))
        assert abs(got - want) <= 1e-5 * abs(want), (name, fc, got, want)


def test_get_length():
    assert make(case("dc_blocker_0.01_crcf")).get_length() == 2
    assert make(case("pll_rrrf")).get_length() == 2
    assert make(case("ellip5_crcf")).get_length() == 6
    assert make(case("differentiator_crcf")).get_length() == 8
    assert LQ.IirFilt("rrrf", [1.0], [1.0, 0.5, 0.25, 0.125]).get_length() == 4


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def test_design_helpers():
    n = 0
    for h in fixture()["helpers"]:
        if h["fn"] == "zpk":
            z = np.array(h["z"], np.float32).view(np.complex64)
            p = np.array(h["p"], np.float32).view(np.complex64)
            B, A = LQ.iirdes_dzpk2sosf(z, p, h["k"])
        else:
            fn = LQ.iirdes_pll_active_lag if h["fn"] == "lag" else LQ.iirdes_pll_active_PI
            B, A = fn(h["w"], h["zeta"], h["K"])
        assert rel(B, h["b"]) <= 1e-6 and rel(A, h["a"]) <= 1e-6, h
        n += 1
    assert n == 6
    # the constructors that design their own coefficients hold the reference's
    assert [n for n in case_names() if not expect_eligible(case(n))] == [
        "pll_rrrf", "integrator_rrrf", "integrator_crcf", "radius_1.01_crcf"]
    for name in ("pll_rrrf", "differentiator_rrrf", "differentiator_crcf", "dc_blocker_1e-3_rrrf"):
        c = case(name)
        q = make(c)
        imp = np.zeros(64, IM.sample_dtype(c["kind"]))
        imp[0] = 1.0
        want, _ = IM.run32(c["kind"], c["form"], c["b"], c["a"], imp)
        got = q.execute_block(imp)
        assert np.max(np.abs(got - want)) <= 1e-5 * np.max(np.abs(want)), name


def test_unsupported_forms_take_the_host_loop():
    """9 sections, or a NORM form of 4 coefficients: not device-eligible, the model exactly"""
    c = case("butter4_rrrf")
    B, A = np.tile(c["raw_b"][:3], 9), np.tile(c["raw_a"][:3], 9)
    q = LQ.IirFilt.sos("rrrf", B, A)
    x = IM.noise_input("rrrf", 300, 5)
    assert not q.device_eligible
    y32, _ = IM.run32("rrrf", "sos", np.tile(c["b"][:3], 9), np.tile(c["a"][:3], 9), x)
    assert same_bits(q.execute_block(x), y32)
    assert LQ.IirFilt.sos("rrrf", B[:24], A[:24]).device_eligible
    q = LQ.IirFilt("crcf", [0.1, 0.2, 0.3, 0.4], [1.0, -0.5, 0.25, -0.125])
    assert not q.device_eligible
    xc = IM.noise_input("crcf", 300, 6)
    y32, _ = IM.run32("crcf", "norm", [0.1, 0.2, 0.3, 0.4], [1.0, -0.5, 0.25, -0.125], xc)
    assert same_bits(q.execute_block(xc), y32)


# ------------------------------------------------------------------ 9 reference examples
REF_EX = os.path.join(LQ.ROOT, "build", "ref_examples_iir")
EXAMPLES = ["iirfilt_crcf_dcblocker_example", "pll_example"]


@pytest.mark.skipif(not os.path.isdir(REF_EX), reason="reference examples not built (tools/build_ref_examples_iir.sh)")
@pytest.mark.parametrize("exe", EXAMPLES)
@pytest.mark.parametrize("small", ["gpu", "host"])
def test_reference_iirfilt_examples_run(exe, small, tmp_path):
    env = dict(os.environ)
    env.pop("LQ_SMALL_CALLS", None)
    if small == "gpu":
        env["LQ_SMALL_CALLS"] = "gpu"
    res = subprocess.run([os.path.join(REF_EX, exe)], capture_output=True, text=True, timeout=120, cwd=tmp_path,
                         env=env)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0
    assert "error" not in res.stderr.lower()
