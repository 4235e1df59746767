"""autocorr on the GPU against the per-output bound of tests/fir_bound.py
(tests/autocorr_model.py): every output within (T + 8) 2^-23 A[n] of the
float64 window sum, exactly zero where A[n] = 0, finite -- for every window and
delay geometry of the kernel, however the stream is cut into calls, for the e2
output and get_energy too.

TILE (outputs per workgroup) and WMAX (the largest window the kernel takes)
come from the library; N = 3 TILE + 5 unless stated.  References are computed
once per (stream, window, delay) and shared.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import autocorr_model as AM
import liquidmi as LQ

pytestmark = pytest.mark.gpu

TILE = LQ.AutoCorr.TILE
WMAX = LQ.AutoCorr.MAX_WINDOW
N = 3 * TILE + 5
SEAMS = (TILE, 2 * TILE, 3 * TILE)
FIX = AM.load_fixture()


@functools.lru_cache(maxsize=None)
def stream(kind, env, n=N):
    x = AM.noise(kind, AM.envelope(env, n, SEAMS), 1234 + (kind == "rrrf") + 7 * (env == "gaps"))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ref(kind, env, W, d, n=N):
    r = AM.reference64(kind, W, d, stream(kind, env, n))
    for a in r:
        a.setflags(write=False)
    return r


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_calls(q, x, sizes):
    """the stream through execute_block in calls of the given sizes (the last
    takes the rest); -> outputs, get_energy after each call, call ends"""
    parts, energy, ends, k = [], [], [], 0
    sizes = list(sizes)
    while k < len(x):
        c = sizes.pop(0) if sizes else len(x) - k
        parts.append(q.execute_block(x[k:k + c]))
        k += len(parts[-1])
        energy.append(q.get_energy())
        ends.append(k)
    return np.concatenate(parts), energy, ends


# ------------------------------------------------------------------ 1 fixture streams
@pytest.mark.parametrize("c", FIX["cases"], ids=AM.case_name)
def test_fixture_stream(c):
    x = AM.case_input(c)
    y64, A, e64 = AM.reference64(c["kind"], c["W"], c["d"], x)
    q = LQ.AutoCorr(c["kind"], c["W"], c["d"])
    y = q.execute_block(x)
    rr = AM.report(c["kind"], c["W"], c["y"], y64, A)
    rg = AM.check("fixture " + AM.case_name(c), c["kind"], c["W"], y, y64, A)
    print("autocorr %s: worst ratio to the bound, GPU %.4g, reference %.4g" % (AM.case_name(c), rg["worst"], rr["worst"]))
    AM.check_e2("fixture energy " + AM.case_name(c), c["kind"], c["W"], [q.get_energy()], e64[-1:])


# ------------------------------------------------------------------ 2 geometry
GEOMETRY = [("cccf", 1, 1), ("cccf", 1, 5), ("cccf", 2, 0), ("cccf", 63, 7), ("cccf", 64, 64), ("cccf", 65, 5),
            ("cccf", 300, 1), ("cccf", 300, TILE + 3),
            ("rrrf", 1, 1), ("rrrf", 33, 7), ("rrrf", 64, 0), ("rrrf", 65, TILE + 3)]


@pytest.mark.parametrize("env", ["burst", "gaps"])
@pytest.mark.parametrize("kind,W,d", GEOMETRY)
def test_geometry(kind, W, d, env):
    x = stream(kind, env)
    y64, A, _ = ref(kind, env, W, d)
    q = LQ.AutoCorr(kind, W, d)
    assert q.device_eligible
    AM.check("geometry %s W=%d d=%d %s" % (kind, W, d, env), kind, W, q.execute_block(x), y64, A)


# ------------------------------------------------------------------ 3 short calls
@pytest.mark.parametrize("n", [1, 2, 64, 65, TILE - 1, TILE, TILE + 1])
def test_short_calls(n):
    x = stream("cccf", "burst")
    y64, A, _ = ref("cccf", "burst", 65, 5)
    y = LQ.AutoCorr("cccf", 65, 5).execute_block(x[:n])
    assert len(y) == n
    AM.check("short call n=%d" % n, "cccf", 65, y, y64[:n], A[:n])


# ------------------------------------------------------------------ 4 splitting
@functools.lru_cache(maxsize=None)
def carried():
    """1e-5 with level-1 bursts over the first two calls of the first cut and
    over the 300 samples before its last call, which is all at 1e-5"""
    env = np.full(N, 1e-5)
    env[0:8] = 1.0
    env[TILE + 9 - 300:TILE + 9] = 1.0
    x = AM.noise("cccf", env, 4321)
    x.setflags(write=False)
    return x, AM.reference64("cccf", 65, 5, x)


@pytest.mark.parametrize("cut", ["1,7,TILE+1,rest", "TILE"])
def test_splitting(cut):
    x, (y64, A, e64) = carried()
    sizes = (1, 7, TILE + 1) if cut != "TILE" else [TILE] * (N // TILE)
    y, energy, ends = run_calls(LQ.AutoCorr("cccf", 65, 5), x, sizes)
    assert ends[:3] == ([1, 8, TILE + 9] if cut != "TILE" else [TILE, 2 * TILE, 3 * TILE]) and ends[-1] == N
    AM.check("splitting " + cut, "cccf", 65, y, y64, A)
    AM.check_e2("get_energy after each call, " + cut, "cccf", 65, energy, e64[np.array(ends) - 1])


# ------------------------------------------------------------------ 5 the eligibility edge
@pytest.mark.parametrize("W,eligible", [(WMAX, True), (WMAX + 1, False)])
def test_eligibility_edge(W, eligible):
    n = TILE + 5
    x = stream("cccf", "burst", n)
    y64, A, _ = ref("cccf", "burst", W, 3, n)
    q = LQ.AutoCorr("cccf", W, 3)
    assert q.device_eligible == eligible
    AM.check("W=%d d=3 (%s)" % (W, "kernel" if eligible else "host loop"), "cccf", W, q.execute_block(x), y64, A)


# ------------------------------------------------------------------ 6 delay beyond the call
def test_delay_beyond_the_call():
    """d = 2 TILE: two calls of 100, one of TILE + 1 (every delayed sample is
    still before the stream), then 2 TILE + 7 more, whose delayed samples are
    the first calls' inputs"""
    d = 2 * TILE
    n = 200 + TILE + 1 + 2 * TILE + 7
    x = stream("cccf", "burst", n)
    y64, A, _ = ref("cccf", "burst", 64, d, n)
    y, _, ends = run_calls(LQ.AutoCorr("cccf", 64, d), x, (100, 100, TILE + 1))
    assert ends == [100, 200, TILE + 201, n]
    assert np.count_nonzero(A[TILE + 201:]) > TILE
    AM.check("delay 2 TILE", "cccf", 64, y, y64, A)


# ------------------------------------------------------------------ 7 mixed calls
@pytest.fixture(params=["gpu", "host"])
def small_calls(request):
    LQ.set_small_calls(request.param == "host")
    yield request.param
    LQ.set_small_calls(False)


@pytest.mark.parametrize("kind,W,d", [("cccf", 65, 5), ("rrrf", 33, 7)])
def test_mixed_calls(kind, W, d, small_calls):
    assert LQ.get_small_calls() == (small_calls == "host")
    n = 1000 + 70 + TILE + 1
    x = stream(kind, "burst")[:n]
    y64, A, e64 = ref(kind, "burst", W, d)
    q = LQ.AutoCorr(kind, W, d)
    parts = [q.execute_block(x[:1000])]
    singles = []
    for v in x[1000:1070]:
        q.push(v)
        singles.append(q.execute())
    again = q.execute()
    assert same_bits(np.array([again]), np.array([singles[-1]])), "execute twice without a push differs"
    AM.check_e2("mixed (%s singles) energy" % small_calls, kind, W, [q.get_energy()], e64[1069:1070])
    parts += [np.array(singles, x.dtype), q.execute_block(x[1070:])]
    AM.check("mixed %s W=%d d=%d (%s singles)" % (kind, W, d, small_calls), kind, W, np.concatenate(parts), y64[:n],
             A[:n])


# ------------------------------------------------------------------ 8 energy
@pytest.mark.parametrize("kind,W,d,env", [("cccf", 65, 5, "burst"), ("rrrf", 33, 7, "gaps")])
def test_e2_output(kind, W, d, env):
    x = stream(kind, env)
    y64, A, e64 = ref(kind, env, W, d)
    q = LQ.AutoCorr(kind, W, d)
    dx, dy, de = LQ.DeviceBuffer.from_array(x), LQ.DeviceBuffer(x.nbytes), LQ.DeviceBuffer(4 * N)
    q.execute_block_dev(dx.p, N, dy.p, de.p)
    q.synchronize()
    AM.check("with e2 %s W=%d d=%d %s" % (kind, W, d, env), kind, W, dy.to_array(x.dtype, N), y64, A)
    AM.check_e2("%s W=%d d=%d %s" % (kind, W, d, env), kind, W, de.to_array(np.float32, N), e64)


def test_energy_is_zero_after_reset_and_after_zeros(small_calls):
    x = stream("cccf", "burst")[:TILE + 5]
    q = LQ.AutoCorr("cccf", 65, 5)
    assert q.get_energy() == 0.0
    q.execute_block(x)
    assert q.get_energy() > 0.0
    q.reset()
    assert q.get_energy() == 0.0
    q.execute_block(x)
    q.execute_block(np.zeros(65, np.complex64))
    assert q.get_energy() == 0.0


# ------------------------------------------------------------------ 9 same bits
@functools.lru_cache(maxsize=None)
def caller_stream():
    """a HIP stream of the test's own, from the runtime the library runs on (a
    process that has imported torch also maps torch's own copy of the runtime,
    which is not the one that holds the library's device state)"""
    import ctypes
    LQ.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line}, key=lambda p: "/torch/" in p)
    hip = ctypes.CDLL(paths[0])
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    return s.value


@pytest.mark.parametrize("kind,W,d", [("cccf", 65, 5), ("rrrf", 300, 7)])
def test_same_bits(kind, W, d):
    x = stream(kind, "burst")
    sizes = (1, 7, TILE + 1)
    host, _, ends = run_calls(LQ.AutoCorr(kind, W, d), x, sizes)
    # device pointers on a caller's stream, the same call sizes
    s = caller_stream()
    q = LQ.AutoCorr(kind, W, d)
    q.set_stream(s)
    dx, dy = LQ.DeviceBuffer.from_array(x), LQ.DeviceBuffer(x.nbytes)
    k = 0
    for e in ends:
        q.execute_block_dev(dx.p + k * x.itemsize, e - k, dy.p + k * x.itemsize)
        k = e
    q.synchronize()
    assert same_bits(dy.to_array(x.dtype, N), host)
    q.destroy()
    # in place through host pointers
    q2 = LQ.AutoCorr(kind, W, d)
    assert same_bits(q2.execute_block(x, inplace=True), LQ.AutoCorr(kind, W, d).execute_block(x))
    # a reset object and a fresh one; two fresh ones
    q2.reset()
    a, _, _ = run_calls(q2, x, sizes)
    b, _, _ = run_calls(LQ.AutoCorr(kind, W, d), x, sizes)
    assert same_bits(a, host) and same_bits(b, host)


@pytest.mark.parametrize("kind", ["cccf", "rrrf"])
def test_unaligned_device_pointers(kind):
    """input and output one sample off 16-byte alignment"""
    W, d = (65, 5) if kind == "cccf" else (33, 7)
    x = stream(kind, "burst")
    y64, A, _ = ref(kind, "burst", W, d)
    q = LQ.AutoCorr(kind, W, d)
    dx = LQ.DeviceBuffer.from_array(np.concatenate([np.zeros(1, x.dtype), x]))
    dy = LQ.DeviceBuffer(x.nbytes + x.itemsize)
    q.execute_block_dev(dx.p + x.itemsize, N, dy.p + x.itemsize)
    q.synchronize()
    AM.check("unaligned %s" % kind, kind, W, dy.to_array(x.dtype, N + 1)[1:], y64, A)


# ------------------------------------------------------------------ 10 arguments
def test_zero_window_fails():
    code = ("import sys; sys.path.insert(0, %r); import liquidmi as LQ; LQ.lib().autocorr_cccf_create(0, 1); "
            "print('survived')" % os.path.dirname(os.path.abspath(LQ.__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert "autocorr" in r.stderr and "survived" not in r.stdout
