"""firhilbf on the GPU, at the bar of tests/firhilb_model.py: every delay
output equals the delayed input bit for bit, every dot output is within
(2m + 8) 2^-23 A of the float64 model (exactly zero where A = 0).  The model
runs with the float32 taps the object under test holds, read back through its
own impulse response.

conftest.py forces single calls onto the GPU; the host small-call path is
switched on by a fixture where it is the subject.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import firhilb_model as FM
import liquidmi as LQ

pytestmark = pytest.mark.gpu

CT = LQ.FirHilb.TILE                      # calls per workgroup of the block kernels
SWEEP_M = [2, 5, 12, 16, 17, 40]
ENVELOPES = ["flat", "burst", "gap", "two-level"]


@functools.lru_cache(maxsize=None)
def fixture():
    return FM.load_fixture()


def block_fn(q, mode):
    return {"decim": q.decim_block, "interp": q.interp_block, "r2c": q.r2c_block}[mode]


def single_fn(q, mode):
    return {"decim": q.decim, "interp": q.interp, "r2c": q.r2c}[mode]


def flat32(y):
    return np.ascontiguousarray(y).view(np.float32).reshape(-1)


def run_ops(q, ops):
    """every op as one block call; all outputs as flat float32"""
    return np.concatenate([flat32(block_fn(q, mode)(x)) for mode, x in ops])


def run_single(q, mode, x):
    """the per-call API, one call per input group"""
    x = np.ascontiguousarray(x)
    step = 2 if mode == "decim" else 1
    out = [single_fn(q, mode)(x[k:k + step] if mode == "decim" else x[k]) for k in range(0, len(x), step)]
    return flat32(np.array(out, np.float32 if mode == "interp" else np.complex64))


@functools.lru_cache(maxsize=None)
def taps(m, As):
    """the taps the object holds: unit impulse at x[0] through the decimator
    gives Im y[i] = hq[2m-1-i]"""
    imp = np.zeros(4 * m, np.float32)
    imp[0] = 1.0
    y = LQ.FirHilb(m, As).decim_block(imp)
    assert np.array_equal(y.real[1:], np.zeros(2 * m - 1, np.float32))
    hq = y.imag[::-1].copy()
    hq.setflags(write=False)
    return hq


# ------------------------------------------------------------------ taps and fixtures
@pytest.mark.parametrize("m,As", FM.CASES)
def test_taps_match_reference(m, As):
    want = next(c["hq"] for c in fixture()["cases"] if c["m"] == m)
    hq = taps(m, As)
    d = np.max(np.abs(hq.astype(np.float64) - want))
    print("m=%d: max |hq - reference| = %.3g (max |hq| %.3g)" % (m, d, np.max(np.abs(want))))
    assert d <= 1e-6 * np.max(np.abs(want))
    assert np.array_equal(hq, -hq[::-1])


@pytest.mark.parametrize("m", SWEEP_M + [130])
def test_taps_antisymmetric(m):
    hq = taps(m, 60.0)
    assert len(hq) == 2 * m and np.array_equal(hq, -hq[::-1]) and np.all(hq[:m] != 0)


@pytest.mark.parametrize("m,As", FM.CASES)
@pytest.mark.parametrize("mode", FM.MODES)
def test_fixture_stream(mode, m, As):
    ops = [(mode, FM.stream_input(m, mode))]
    FM.check(m, taps(m, As), ops, run_ops(LQ.FirHilb(m, As), ops), "gpu block " + mode)
    FM.check(m, taps(m, As), ops, run_single(LQ.FirHilb(m, As), *ops[0]), "gpu single " + mode)


@pytest.mark.parametrize("m,As", FM.CASES)
def test_fixture_mixed(m, As):
    ops = FM.mixed_ops(m)
    FM.check(m, taps(m, As), ops, run_ops(LQ.FirHilb(m, As), ops), "gpu mixed")


@pytest.mark.parametrize("mode", ["decim", "interp"])
def test_autotest_vectors(mode):
    d = fixture()
    ops, want = FM.known_answer_ops(d, mode)
    for label, y in (("block", run_ops(LQ.FirHilb(5, 60.0), ops)), ("single", run_single(LQ.FirHilb(5, 60.0), *ops[0]))):
        err = np.max(np.abs(y - want))
        print("autotest %s %s: max |y - expected| %.3g" % (mode, label, err))
        FM.check(5, taps(5, 60.0), ops, y, "autotest " + mode)
        assert err <= d["known_answers"]["tol"]


# ------------------------------------------------------------------ bound sweep
def sweep_blocks(m):
    return [1, 2 * m - 1, 2 * m, CT - 1, CT, CT + 1, 2 * CT + 3]


def sweep_envelope(name, m, nin):
    """Per call, then repeated for the call's nin input samples.  The blocks
    start at calls 0, 1, 2m, 4m, 4m+CT-1, 4m+2CT-1 and 4m+3CT; the last one
    has tile seams at its calls CT and 2CT."""
    starts = np.cumsum([0] + sweep_blocks(m))
    n, last = int(starts[-1]), int(starts[-2])
    if name == "flat":
        e = np.ones(n)
    elif name in ("burst", "gap"):
        e = np.full(n, 1e-5 if name == "burst" else 0.0)
        runs = [(0, m + 1), (3 * m, 5 * m + 3)]                                  # across the short blocks
        runs += [(int(s) - m - 2, int(s) + 3) for s in starts[4:-1]]             # across the later block starts
        runs += [(last + CT - 2 * m - 1, last + CT + 1), (last + 2 * CT - 1, last + 2 * CT + m),  # the seams
                 (last + CT + 400, last + CT + 401), (n - 5, n)]
        for a, b in runs:
            e[max(a, 0):b] = 1.0
    elif name == "two-level":   # the step falls at the last block's first tile seam
        e = np.where(np.arange(n) < last + CT, 1.0, 2.0 ** -12)
    else:
        raise ValueError(name)
    return np.repeat(e, nin)


@functools.lru_cache(maxsize=None)
def sweep_ops(mode, m, env):
    nin = FM.NIN[mode]
    e = sweep_envelope(env, m, nin)
    rng = np.random.default_rng([m, FM.MODES.index(mode), ENVELOPES.index(env)])
    flat = FM.shape(rng.uniform(-0.5, 0.5, len(e)).astype(np.float32), e)
    flat.setflags(write=False)
    ops, k = [], 0
    for c in sweep_blocks(m):
        ops.append((mode, FM.as_input(mode, flat[k:k + c * nin])))
        k += c * nin
    assert k == len(flat) <= 11500
    return ops


@pytest.mark.parametrize("env", ENVELOPES)
@pytest.mark.parametrize("m", SWEEP_M + [130])
@pytest.mark.parametrize("mode", FM.MODES)
def test_bound_sweep(mode, m, env):
    """One object per case; block calls of 1, 2m-1, 2m, CT-1, CT, CT+1 and
    2 CT + 3 calls in turn, so every block also starts from a carried state.
    (m = 130: more window than one staging pass of the workgroup covers.)"""
    ops = sweep_ops(mode, m, env)
    FM.check(m, taps(m, 60.0), ops, run_ops(LQ.FirHilb(m, 60.0), ops), "sweep %s %s" % (mode, env))


# ------------------------------------------------------------------ split invariance
def dev_run(q, mode, x):
    x = np.ascontiguousarray(x)
    n = len(x) // (2 if mode == "decim" else 1)
    dx = LQ.DeviceBuffer.from_array(x)
    dy = LQ.DeviceBuffer(8 * n)
    {"decim": q.decim_block_dev, "interp": q.interp_block_dev, "r2c": q.r2c_block_dev}[mode](dx.p, n, dy.p)
    q.synchronize()
    return dy.to_array(np.float32, 2 * n)


@pytest.mark.parametrize("m", [2, 12, 17])
@pytest.mark.parametrize("mode", FM.MODES)
def test_split_invariance(mode, m):
    n = 2 * CT + 300
    nin = FM.NIN[mode]
    rng = np.random.default_rng([7, m, FM.MODES.index(mode)])
    flat = FM.shape(rng.uniform(-0.5, 0.5, n * nin).astype(np.float32), FM.burst_envelope(n * nin))
    x = FM.as_input(mode, flat)
    per = 2 if mode == "decim" else 1                      # input elements per call
    q = LQ.FirHilb(m, 60.0)
    whole = flat32(block_fn(q, mode)(x))
    FM.check(m, taps(m, 60.0), [(mode, x)], whole, "whole " + mode)
    cuts = [1, 7, 2 * m + (1 if mode == "r2c" else 0)]     # r2c: odd cuts, the toggle carries
    cuts.append(n - sum(cuts))
    q2 = LQ.FirHilb(m, 60.0)
    parts, k = [], 0
    for c in cuts:
        parts.append(flat32(block_fn(q2, mode)(x[k * per:(k + c) * per])))
        k += c
    assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
    # the device-pointer entry points, whole and cut
    q3 = LQ.FirHilb(m, 60.0)
    assert np.array_equal(dev_run(q3, mode, x).view(np.uint32), whole.view(np.uint32))
    q3.reset()
    parts, k = [], 0
    for c in cuts:
        parts.append(dev_run(q3, mode, x[k * per:(k + c) * per]))
        k += c
    assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
    # reset, then the same stream again
    q.reset()
    assert np.array_equal(flat32(block_fn(q, mode)(x)).view(np.uint32), whole.view(np.uint32))
    # r2c after an odd number of calls, then reset: the toggle is cleared too
    if mode == "r2c":
        q.reset()
        q.r2c_block(x[:5])
        q.reset()
        assert np.array_equal(flat32(q.r2c_block(x)).view(np.uint32), whole.view(np.uint32))


def test_device_pointers_at_odd_word_offsets():
    """The real-sample sides (decim input, interp output) are only 4-byte
    aligned in general; the kernels move them as 8-byte elements."""
    m, n = 12, CT + 77
    rng = np.random.default_rng(11)
    xr = rng.uniform(-0.5, 0.5, 2 * n).astype(np.float32)
    xc = FM.as_input("interp", rng.uniform(-0.5, 0.5, 2 * n).astype(np.float32))
    want_d = flat32(LQ.FirHilb(m, 60.0).decim_block(xr))
    want_i = LQ.FirHilb(m, 60.0).interp_block(xc)
    pad = np.zeros(1, np.float32)
    q = LQ.FirHilb(m, 60.0)
    dx = LQ.DeviceBuffer.from_array(np.concatenate([pad, xr]))
    dy = LQ.DeviceBuffer(8 * n)
    q.decim_block_dev(dx.p + 4, n, dy.p)
    q.synchronize()
    assert np.array_equal(dy.to_array(np.float32, 2 * n), want_d)
    q = LQ.FirHilb(m, 60.0)
    dx = LQ.DeviceBuffer.from_array(xc)
    dy = LQ.DeviceBuffer(8 * n + 8)
    q.interp_block_dev(dx.p, n, dy.p + 4)
    q.synchronize()
    assert np.array_equal(dy.to_array(np.float32, 2 * n + 1)[1:], want_i)


# ------------------------------------------------------------------ host small-call path
@pytest.fixture
def host_small_calls():
    LQ.set_small_calls(True)
    yield
    LQ.set_small_calls(False)


@pytest.mark.parametrize("m", [2, 12, 17])
@pytest.mark.parametrize("mode", FM.MODES)
def test_host_small_calls_interleaved_with_blocks(mode, m, host_small_calls):
    """per-sample calls (host) and block calls (GPU) on one object: the
    window mirrors carry the state both ways"""
    assert LQ.get_small_calls()
    nin = FM.NIN[mode]
    plan = [("s", 3), ("b", 2 * m + 1), ("s", 2 * m + 5), ("b", CT + 9), ("s", 9), ("b", 1), ("s", 4 * m + 1)]
    n = sum(c for _, c in plan)
    rng = np.random.default_rng([3, m, FM.MODES.index(mode)])
    flat = FM.shape(rng.uniform(-0.5, 0.5, n * nin).astype(np.float32), FM.burst_envelope(n * nin))
    x = FM.as_input(mode, flat)
    per = 2 if mode == "decim" else 1
    q = LQ.FirHilb(m, 60.0)
    parts, k = [], 0
    for how, c in plan:
        seg = x[k * per:(k + c) * per]
        parts.append(run_single(q, mode, seg) if how == "s" else flat32(block_fn(q, mode)(seg)))
        k += c
    FM.check(m, taps(m, 60.0), [(mode, x)], np.concatenate(parts), "host+gpu " + mode)


def test_host_small_calls_mixed_sequence(host_small_calls):
    m, As = 5, 60.0
    ops = FM.mixed_ops(m)
    q = LQ.FirHilb(m, As)
    y = np.concatenate([run_single(q, mode, x) for mode, x in ops])
    FM.check(m, taps(m, As), ops, y, "host mixed")
    assert q.c2r(1.5 - 2.5j) == np.float32(1.5)


# ------------------------------------------------------------------ c2r, round trip, examples
def test_c2r_block_is_the_real_part():
    rng = np.random.default_rng(5)
    n = 3 * CT + 5
    x = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
    q = LQ.FirHilb(5, 60.0)
    assert np.array_equal(q.c2r_block(x).view(np.uint32), x.real.copy().view(np.uint32))
    dx, dy = LQ.DeviceBuffer.from_array(x), LQ.DeviceBuffer(4 * n)
    q.c2r_block_dev(dx.p, n, dy.p)
    q.synchronize()
    assert np.array_equal(dy.to_array(np.float32, n), x.real)
    assert q.c2r(x[3]) == x[3].real


@pytest.mark.parametrize("f", [0.123456, -0.123456])
@pytest.mark.parametrize("m,As", [(12, 60.0), (17, 80.0)])
def test_round_trip_interp_then_decim(m, As, f):
    """firhilb_example's round trip, a smooth-edged tone at the example's
    frequency: interp feeds decim.  Written out, z[i] = sum_j hq[j]
    x[i - 3m + 1 + j]: the quadrature taps applied at the complex rate, a
    Hilbert transformer whose 2m taps are centred 2m - 1/2 samples back, so
    z(i) = -j sgn(f) x(i - 2m + 1/2) up to the filter's stop-band level
    10^(-As/20).  (The semi-lengths with a transition band narrow enough for a
    tone at this frequency: m = 2 and 5 are not.)  A sign error in hq turns z
    into its negative."""
    n = 512
    N = n + 4 * m + 1

    def tone(t):
        w = np.where((t >= 0) & (t <= n - 1), 0.5 - 0.5 * np.cos(2 * np.pi * t / (n - 1)), 0.0) ** 2
        return w * np.exp(2j * np.pi * f * t)
    i = np.arange(N, dtype=np.float64)
    x = tone(i).astype(np.complex64)
    y = LQ.FirHilb(m, As).interp_block(x)
    z = LQ.FirHilb(m, As).decim_block(y)
    want = -1j * np.sign(f) * tone(i - 2 * m + 0.5)
    err = np.max(np.abs(z - want))
    print("round trip m=%d f=%g: max error %.3g (stop band %.3g)" % (m, f, err, 10 ** (-As / 20)))
    assert err < 10 ** (-As / 20)


REF_EX = os.path.join(LQ.ROOT, "build", "ref_examples_firhilb")
EXAMPLES = ["firhilb_decim_example", "firhilb_example", "firhilb_interp_example"]


@pytest.mark.skipif(not os.path.isdir(REF_EX), reason="reference examples not built (tools/build_ref_examples_firhilb.sh)")
@pytest.mark.parametrize("exe", EXAMPLES)
@pytest.mark.parametrize("small_calls", ["gpu", "host"])
def test_reference_firhilb_examples_run(exe, small_calls, tmp_path):
    env = dict(os.environ)
    env.pop("LQ_SMALL_CALLS", None)
    if small_calls == "gpu":
        env["LQ_SMALL_CALLS"] = "gpu"
    res = subprocess.run([os.path.join(REF_EX, exe)], capture_output=True, text=True, timeout=120, cwd=tmp_path,
                         env=env)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0
    assert "error" not in res.stderr.lower()
