"""The persistent kernels past their first tile (`-m gpu`).

The persistent launches cap their grid and let each workgroup walk further
tiles (t += gridDim.x), several prefetching the next tile while the current one
computes.  At the suite's sizes every workgroup does one tile, so the walk,
its prefetch guard and the barrier between tiles never run.  Here they do:

  * at a limit of 3 workgroups (liquid_mi355x_set_max_workgroups), where a
    49-segment stream or a 70 001-output decimation makes every workgroup
    walk 16 to 46 tiles in milliseconds, for every type and shape, and
  * at the real caps, with no limit, at 2 cap tiles and a ragged rest, for
    the decimator's three persistent launch shapes and the two transform
    sizes the channelizers and fftfilt lean on.

firdecim and firfilt are held to the direct form's per-output bound
(tests/fir_bound.py: (T + 8) 2^-23 A[o], exact zeros where A is 0), every
output checked; the transforms, fftfilt and the resamplers to the suite's
normwise 1e-5 -- the transforms per row, so a swapped or stale row fails by
itself.  Each firdecim case first asserts the kernel its shape reaches
(liquid_mi355x_firdecim_route): a retune that moves a shape off a kernel fails
here instead of dropping coverage.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import fir_bound as FB
import golden_io as G
import liquidmi as LQ
import oracle_lib as O
import resamp_bound as RB

pytestmark = pytest.mark.gpu

NRM = 1e-5
TYPES = {"rrrf": O.RRRF, "crcf": O.CRCF, "cccf": O.CCCF}


@pytest.fixture
def limit3():
    LQ.set_max_workgroups(3)
    try:
        yield
    finally:
        LQ.set_max_workgroups(0)


def _cx(r, n):
    return (r.uniform(-0.5, 0.5, n) + 1j * r.uniform(-0.5, 0.5, n)).astype(np.complex64)


def _sync():
    LQ.lib().liquid_mi355x_device_synchronize()


# ===================================================================== firdecim
# (type, M, taps) -> the kernel for 16-byte aligned x, the kernel otherwise.
# pf_*: k_firdecim_pf (persistent, prefetching); ph2: k_firdecim_ph2;
# ph_r1x64: k_firdecim_ph<QCT, 1, 64>; plain: k_firdecim.
DECIM_ROUTES = {
    ("rrrf", 2, 80): ("pf_r4x128", "ph2"), ("crcf", 2, 80): ("pf_r4x128", "ph2"), ("cccf", 2, 80): ("pf_r4x128", "ph2"),
    ("rrrf", 4, 37): ("pf_r4x128", "ph2"), ("crcf", 4, 37): ("pf_r4x128", "ph2"), ("cccf", 4, 37): ("pf_r4x128", "ph2"),
    ("rrrf", 8, 128): ("pf_r2x256", "ph2"), ("crcf", 8, 128): ("pf_r2x256", "ph2"),
    ("cccf", 8, 128): ("pf_r2x256", "ph2"),
    ("rrrf", 12, 96): ("pf_r2x256", "ph2"), ("crcf", 12, 96): ("ph2", "ph2"), ("cccf", 12, 96): ("ph2", "ph2"),
    ("rrrf", 16, 128): ("pf_r2x256", "ph2"), ("crcf", 16, 128): ("pf_r1x256", "ph_r1x64"),
    ("cccf", 16, 128): ("pf_r1x256", "ph_r1x64"),
    ("rrrf", 32, 256): ("pf_r1x256", "ph_r1x64"), ("crcf", 32, 256): ("ph_r1x64", "ph_r1x64"),
    ("cccf", 32, 256): ("ph_r1x64", "ph_r1x64"),
    ("rrrf", 200, 801): ("ph_r1x64", "ph_r1x64"), ("crcf", 200, 801): ("ph_r1x64", "ph_r1x64"),
    ("cccf", 200, 801): ("ph_r1x64", "ph_r1x64"),
}
assert sorted(DECIM_ROUTES) == sorted((t, M, h) for M, h in FB.DECIM_ROWS for t in TYPES)
# 70 001 + 160 outputs: 137 tiles of 512 and 17 outputs, 274 of 256 and 17
DECIM_NOUT, DECIM_CUT = 70001 + 160, 2500


def _decim_run(c, off, cuts=()):
    """The stream through execute_block_dev, one call per piece, x and y
    `off` elements past a 16-byte boundary."""
    g = LQ.FirDecim(c.M, c.h, t=c.t)
    fn = getattr(LQ.lib(), "firdecim_%s_execute_block_dev" % c.t)
    esz = c.x.itemsize
    bx = LQ.DeviceBuffer(c.x.nbytes + 16)
    LQ.lib().liquid_mi355x_memcpy_h2d(bx.p + off * esz, LQ.ptr(c.x), c.x.nbytes)
    by = LQ.DeviceBuffer((c.nout + 2) * esz)
    edges = [0] + list(cuts) + [c.nout]
    for a, b in zip(edges[:-1], edges[1:]):
        fn(g.q, bx.p + (off + a * c.M) * esz, b - a, by.p + (off + a) * esz)
    _sync()
    return by.to_array(c.x.dtype, c.nout + off)[off:]


def _decim_three_ways(c, off):
    worst = 0.0
    for cuts in ((), range(8191, c.nout, 8191), (c.cut,)):
        worst = max(worst, c.check(_decim_run(c, off, cuts))["worst"])
    return worst


@pytest.mark.parametrize("name", ["burst", "gaps"])
@pytest.mark.parametrize("f", sorted(DECIM_ROUTES), ids=lambda f: "%s-M%d-h%d" % f)
def test_firdecim_bound_at_three_workgroups(limit3, f, name):
    """(a) every row of the route table, aligned (the persistent form where
    the shape has one) and one element off (the one-shot forms), as one call,
    as calls of 8191 outputs and as two calls cut after a loud burst, all
    against the same y64.  With three workgroups a persistent launch walks 46
    tiles of 512 or 92 of 256 per workgroup; the last tile has 17 outputs."""
    t, M, hlen = f
    for aligned, route in zip((True, False), DECIM_ROUTES[f]):
        assert LQ.firdecim_route(t, M, hlen, aligned, DECIM_NOUT) == route
        if route.startswith("pf_"):   # more tiles than workgroups, ragged end
            tile = LQ.firdecim_tile(route)
            assert DECIM_NOUT > 3 * 16 * tile and DECIM_NOUT % tile == 17
    c = FB.decim_case(t, M, hlen, name, DECIM_NOUT, DECIM_CUT)
    for off in (0, 1):
        w = _decim_three_ways(c, off)
        print("firdecim %s M=%d h=%d %s off=%d: worst %.3g of the bound" % (t, M, hlen, name, off, w))


def test_firdecim_plain_kernel_bound(limit3):
    """The one shape family that reaches k_firdecim (about 6000 taps per unit
    of M and more: the phase layout pads each row by 1/32 and then needs more
    LDS than the undivided tile).  The kernel is one-shot, one workgroup per
    256 outputs, so five tiles and a ragged sixth cover it: the float64
    reference of 40 000 taps costs a pass per tap."""
    t, M, hlen = FB.DECIM_PLAIN
    nout, cut = 5 * 256 + 77 + 512, 700
    for aligned in (True, False):
        assert LQ.firdecim_route(t, M, hlen, aligned, nout) == "plain"
    for name in ("burst", "gaps"):
        c = FB.decim_case(t, M, hlen, name, nout, cut)
        for off in (0, 1):
            for cuts in ((), range(300, nout, 300), (cut,)):
                c.check(_decim_run(c, off, cuts))


def test_firdecim_refuses_what_no_tile_holds():
    """Past about M = 580 (rrrf) or 290 (complex) no kernel's tile fits the
    LDS -- 64 outputs need 64 M samples -- and the call is refused with a
    message and exit(1), the reference's error convention, where the
    reference itself would run (a stated limit)."""
    assert LQ.firdecim_route("rrrf", 1000, 8, True, 100) == "refused"
    assert LQ.firdecim_route("crcf", 200, 6500, True, 100) == "refused"
    assert LQ.firdecim_route("crcf", 200, 6000, True, 100) == "ph_r1x64"
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import liquidmi as LQ; "
            "g = LQ.FirDecim(1000, np.ones(8, np.float32), t='rrrf'); print('created', flush=True); "
            "g.execute_block(np.ones(3000, np.float32)); print('ran')") % os.path.dirname(LQ.__file__)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1, (p.returncode, p.stdout, p.stderr)
    assert "firdecim: decimation/filter length exceeds the GPU tile limit" in p.stderr
    assert "created" in p.stdout and "ran" not in p.stdout


# the three persistent launch shapes (k_firdecim.hip, decim_decide): four
# outputs per lane on 128 lanes, two on 256, one on 256
@pytest.mark.parametrize("f,route", [(("rrrf", 2, 80), "pf_r4x128"), (("crcf", 8, 128), "pf_r2x256"),
                                     (("crcf", 16, 128), "pf_r1x256")], ids=["pf_r4x128", "pf_r2x256", "pf_r1x256"])
def test_firdecim_bound_at_the_real_cap(f, route):
    """(b) no limit: nout = 2 cap TO + 3 TO + 17, cap and TO from the
    dispatch itself, so three workgroups walk three tiles, the rest two, and
    the last tile has 17 outputs."""
    t, M, hlen = f
    assert LQ.get_max_workgroups() == 0
    cap, TO = LQ.firdecim_grid_cap(t, M, hlen, route), LQ.firdecim_tile(route)
    assert cap >= 256 and TO in (256, 512)
    nout = 2 * cap * TO + 3 * TO + 17
    assert LQ.firdecim_route(t, M, hlen, True, nout) == route
    assert nout * M * (4 if t == "rrrf" else 8) <= 70 * 1024 * 1024
    t0 = time.time()
    c = FB.decim_case(t, M, hlen, "burst", nout, nout // 2 + 5)
    t1 = time.time()
    r = c.check(_decim_run(c, 0))
    print("firdecim real cap %s: cap %d x %d outputs, nout %d, worst %.3g of the bound; reference %.1f s, "
          "GPU call and check %.1f s" % (route, cap, TO, nout, r["worst"], t1 - t0, time.time() - t1))


# k_firdecim_pf's deepest prefetch class (k_firdecim.hip, lqk_firdecim_ph: NL =
# 5, 9 or 12 vectors per lane by nl <= 5, <= 9, else): the route table's rows
# give nl of at most 9
@pytest.mark.parametrize("M,hlen,route,lanes", [(4, 270, "pf_r4x128", 128), (8, 541, "pf_r2x256", 256),
                                                (16, 571, "pf_r1x256", 256)], ids=["pf_r4x128", "pf_r2x256", "pf_r1x256"])
def test_firdecim_pf_deepest_prefetch(limit3, M, hlen, route, lanes):
    """crcf, 16-byte aligned x.  A lane stages nl = ceil(((TO + QC - 1) M + 1)
    / (lanes * samples per 16 bytes)) vectors per tile, TO the route's tile,
    QC the taps per phase rounded up to four, two crcf samples per 16 bytes:
    10 at each of these shapes, so the kernel with NL = 12 runs and its last
    two vectors are past the tile.  nout = 7 TO + 17: each of the three
    workgroups walks more than one tile and the last tile is ragged."""
    TO = LQ.firdecim_tile(route)
    QC = (-(-hlen // M) + 3) // 4 * 4
    nl = -(-((TO + QC - 1) * M + 1) // (lanes * 2))
    assert 9 < nl <= 12
    nout = 7 * TO + 17
    assert LQ.firdecim_route("crcf", M, hlen, True, nout) == route
    c = FB.decim_case("crcf", M, hlen, "burst", nout, nout // 2)
    r = c.check(_decim_run(c, 0))
    print("firdecim %s M=%d h=%d nl=%d: worst %.3g of the bound" % (route, M, hlen, nl, r["worst"]))


# k_firdecim_ph's tap chunk classes (k_firdecim.hip, lqk_firdecim_ph): QC = 4,
# 8, 16 or 32 taps per phase run as one chunk, any other QC in chunks of 16 if
# 16 divides it, else of 4.  The route table's rows reach QC = 8 only.
@pytest.mark.parametrize("hlen,QC", [(100, 4), (380, 12), (500, 16), (1000, 32), (1530, 48)])
def test_firdecim_ph_chunk_classes(hlen, QC):
    """crcf M = 32 on the 64-output kernel, aligned and one element off: three
    tiles and a ragged fourth, bursts on the 64-output seams."""
    M, nout = 32, 3 * 64 + 17
    assert (-(-hlen // M) + 3) // 4 * 4 == QC
    for aligned in (True, False):
        assert LQ.firdecim_route("crcf", M, hlen, aligned, nout) == "ph_r1x64"
    c = FB.decim_case("crcf", M, hlen, "burst", nout, 100, tile=64)
    for off in (0, 1):
        r = c.check(_decim_run(c, off))
        print("firdecim ph_r1x64 M=%d h=%d QC=%d off=%d: worst %.3g of the bound" % (M, hlen, QC, off, r["worst"]))


# ========================================================== batched transforms
# transforms per workgroup (k_fft_batch.hip): launch_fftsmall 256 / (N / 16),
# launch_fftr16 16 / (N / 256), launch_fft1024 four (one per wave),
# launch_fft4096 / 8192 / 16384 one
FFT_G = {32: 128, 64: 64, 128: 32, 256: 16, 512: 8, 2048: 2, 1024: 4, 4096: 1, 8192: 1, 16384: 1}


def _fft_rows_check(n, batch, direction, off=0, slab=2048):
    """In place through the device batch entry; every row against a float64
    numpy.fft of that row, normwise."""
    r = np.random.default_rng(n * 7 + batch + off + (direction > 0))
    host = np.zeros(batch * n + 1, np.complex64)
    X = host[off:off + batch * n].reshape(batch, n)
    for a in range(0, batch, slab):
        X[a:a + slab] = _cx(r, X[a:a + slab].size).reshape(-1, n)
    dX = LQ.DeviceBuffer.from_array(host)
    L = LQ.lib()
    q = L.fft_create_plan(n, None, None, direction, 0)
    L.fft_execute_batch_dev(q, dX.p + 8 * off, dX.p + 8 * off, batch)
    _sync()
    L.fft_destroy_plan(q)
    Y = dX.to_array(np.complex64, batch * n + 1)[off:off + batch * n].reshape(batch, n)
    worst = 0.0
    for a in range(0, batch, slab):
        x64 = X[a:a + slab].astype(np.complex128)
        ref = np.fft.fft(x64, axis=1) if direction > 0 else np.fft.ifft(x64, axis=1) * n
        err = np.max(np.abs(Y[a:a + slab] - ref), axis=1) / np.max(np.abs(ref), axis=1)
        bad = np.flatnonzero(~(err < NRM))
        assert len(bad) == 0, "n=%d: rows %s of %d miss %g (worst %g)" % (n, (a + bad[:8]).tolist(), batch, NRM,
                                                                        np.max(err))
        worst = max(worst, float(np.max(err)))
    return worst


@pytest.mark.parametrize("direction", [+1, -1])
@pytest.mark.parametrize("n", sorted(FFT_G))
def test_fft_batch_rows_at_three_workgroups(limit3, n, direction):
    """(c) every size with a kernel of its own: 3 G 5 + G + 1 transforms, so
    each of three workgroups walks five or six groups of G and the last
    group holds one transform; 8192 and 16384 also one sample off (8-byte
    loads)."""
    G_ = FFT_G[n]
    batch = 3 * G_ * 5 + G_ + 1
    for off in ((0, 1) if n >= 8192 else (0,)):
        w = _fft_rows_check(n, batch, direction, off)
        print("fft n=%d dir=%+d off=%d batch=%d: worst row %.3g" % (n, direction, off, batch, w))


@pytest.mark.parametrize("n,batch", [(1024, 4096 * 4 + 4 + 1), (4096, 2048 + 3)])
def test_fft_batch_rows_at_the_real_cap(n, batch):
    """launch_fft1024's 4096 groups of four and launch_fft4096's 2048: one
    group, or three transforms, past the cap."""
    assert LQ.get_max_workgroups() == 0
    assert (batch + FFT_G[n] - 1) // FFT_G[n] > {1024: 4096, 4096: 2048}[n] and batch * n * 8 <= 135 * 1024 * 1024
    t0 = time.time()
    w = _fft_rows_check(n, batch, +1)
    print("fft real cap n=%d batch=%d: worst row %.3g, %.1f s" % (n, batch, w, time.time() - t0))


# ====================================================================== fftfilt
# k_fftfilt8k (8192-point segments, cap 768): complex I/O past 2049 taps;
# k_fftfilt_r16<true> (cap 4096): rrrf; k_fftfilt_r16<false>: crcf 512.
# lqk_fftfilt_nfft: 4096 points while hlen - 1 <= 2048, 8192 up to 4097 taps
# for complex I/O.
FFTFILT_CASES = [(t, h) for t in ("crcf", "cccf") for h in (2050, 3001, 4097)] + [("rrrf", 64), ("rrrf", 512),
                                                                                  ("crcf", 512)]


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("t,hlen", FFTFILT_CASES)
def test_fftfilt_stream_at_three_workgroups(limit3, t, hlen, off):
    """(d) 300 001 samples, 16-byte aligned and 8 bytes off, as one call and
    as four ragged calls, against the oracle's stream at 1e-5 normwise."""
    n = 300_001
    nfft = 4096 if hlen - 1 <= 2048 else 8192
    assert (nfft == 8192) == (t != "rrrf" and hlen > 2049)
    seg = nfft - (hlen - 1 if nfft == 4096 else hlen & ~1)   # new samples per segment (k_fftfilt.hip)
    assert n > 3 * 10 * seg   # more than ten segments per workgroup
    r = np.random.default_rng(hlen * 3 + off)
    h = _cx(r, hlen) if t == "cccf" else r.uniform(-0.5, 0.5, hlen).astype(np.float32)
    x = r.uniform(-0.5, 0.5, n).astype(np.float32) if t == "rrrf" else _cx(r, n)
    blk = 1 << (hlen - 2).bit_length()   # the object's block: a power of two >= hlen - 1 (the oracle's 2 blk-point
    assert hlen - 1 <= blk <= 4096       # transform is slow at 2 x 2049)
    ref = O.FftFilt(TYPES[t], h, blk).execute_stream(x)
    assert len(ref) > n - 4097
    for cuts in ((0, n), (0, 7, 70_001, 70_002, n)):
        g = LQ.FftFilt(h, blk, t=t)
        dx = LQ.DeviceBuffer(x.nbytes + 32)
        LQ.lib().liquid_mi355x_memcpy_h2d(dx.p + off, LQ.ptr(x), x.nbytes)
        dy = LQ.DeviceBuffer(x.nbytes + 32)
        for a, b in zip(cuts[:-1], cuts[1:]):
            g.execute_block_dev(dx.p + off + x.itemsize * a, b - a, dy.p + off + x.itemsize * a)
        _sync()
        yb = np.empty(x.nbytes + 32, np.uint8)
        LQ.lib().liquid_mi355x_memcpy_d2h(LQ.ptr(yb), dy.p, yb.nbytes)
        y = yb[off:off + x.nbytes].view(x.dtype)
        e = G.nrm_err(y[:len(ref)], ref)
        print("fftfilt %s h=%d off=%d calls=%d: %.3g" % (t, hlen, off, len(cuts) - 1, e))
        assert e < NRM


# ========================================================== resamp and resamp4
def _plan_env(kind):
    """LQ_RESAMP_INPUT_PLAN for the body of a test (read when a plan is built)."""
    old = os.environ.get("LQ_RESAMP_INPUT_PLAN")
    if kind == "input_plan":
        os.environ["LQ_RESAMP_INPUT_PLAN"] = "1"
    else:
        os.environ.pop("LQ_RESAMP_INPUT_PLAN", None)
    return old


def _plan_env_restore(old):
    if old is None:
        os.environ.pop("LQ_RESAMP_INPUT_PLAN", None)
    else:
        os.environ["LQ_RESAMP_INPUT_PLAN"] = old


@pytest.mark.parametrize("rate", [1.037, 0.8, 3.7])
@pytest.mark.parametrize("t,plan_kind", [("rrrf", "input_plan"), ("crcf", "output_plan"), ("crcf", "input_plan"),
                                         ("cccf", "output_plan"), ("cccf", "input_plan")])
def test_resamp_stream_at_three_workgroups(limit3, t, plan_kind, rate):
    """(e) m = 7, 64 banks (14 taps per bank: an even L <= 32, the shape of
    the suite's config 5), 200 001 inputs in one device call.
    output_plan: crcf and cccf take k_resamp4 (launch_rs4_c, k_resamp4.hip:576;
    host/resamp.c rs_want_d4: complex samples, 1/4 < r <= npfb, power-of-two
    banks, even L <= 32) -- 256-output wave tiles, four per workgroup, so three
    workgroups walk 160 to 720 tiles; rrrf has no output plan (it takes
    k_resamp3 either way).  input_plan: every type takes k_resamp3 (launch_rs,
    k_resamp.hip:595) -- wave tiles of at most 256 inputs, 65 and more per
    workgroup."""
    nx = 200_001
    assert 0.25 < rate <= 64 and nx > 3 * 4 * 256 * 10
    rate = float(np.float32(rate))
    r = np.random.default_rng(int(rate * 1000) + len(t))
    x = _cx(r, nx)
    if t == "rrrf":
        x = np.ascontiguousarray(x.real)
    ref = O.Resamp(rate, 7, 0.25, 60.0, 64).execute_block(x.astype(np.complex64))
    if t == "rrrf":
        ref = ref.real
    dx = LQ.DeviceBuffer.from_array(x)
    cap = int(np.ceil(nx * rate)) + 16
    dy = LQ.DeviceBuffer(cap * x.itemsize)
    old = _plan_env(plan_kind)
    try:
        g = LQ.Resamp(rate, 7, 0.25, 60.0, 64, t=t)
        ny = g.execute_block_dev(dx.p, nx, dy.p)
        g.synchronize()
    finally:
        _plan_env_restore(old)
    assert ny == len(ref)
    y = dy.to_array(x.dtype, ny)
    e = G.nrm_err(y, ref)
    print("resamp %s %s r=%g: %d outputs, %.3g" % (t, plan_kind, rate, ny, e))
    assert e < NRM
    # and output by output (tests/resamp_bound.py; its own streams, with level
    # edges on the tile seams, run at three workgroups in test_gpu_resamp_bound.py)
    RB.check_stream("%s %s r=%g at three workgroups" % (t, plan_kind, rate), rate, 7, 0.25, 60.0, 64, x, y)


# ============================================================= firfilt, 64 taps
@pytest.mark.parametrize("name", ["burst", "stairs"])
@pytest.mark.parametrize("t", ["crcf", "rrrf"])
def test_firfilt_mx_bound_at_three_workgroups(limit3, t, name):
    """(e) 64 taps, 300 001 samples, one device call, per-output bound.
    lqk_firfilt_mx takes the call when hc == 64, one 64-tap block, not in
    place, taps in the split's range and x, y 16-byte aligned; then crcf
    runs k_firfilt_mx16<false, 1, 4> on 2048-output chunks (launch_mx's `go`,
    k_firfilt_mx.hip:545, cap 1024) and rrrf k_firfilt_mx16_r<4> on 4096-output
    chunks (:531, cap 1024): 49 and 25 chunks per workgroup."""
    hlen, n = 64, 300_001
    c = FB.long_case(t, hlen, name, n)
    assert 33 <= hlen <= 64 and np.all((np.abs(c.h) >= 2.0 ** -50) & (np.abs(c.h) <= 2.0 ** 50))
    assert -(-n // (2048 if t == "crcf" else 4096)) > 3 * 20
    g = LQ.FirFilt(t, c.h)
    g.set_scale(c.s)
    bx = LQ.DeviceBuffer.from_array(c.x)
    by = LQ.DeviceBuffer(c.x.nbytes)
    assert bx.p % 16 == 0 and by.p % 16 == 0
    g.execute_block_dev(bx.p, n, by.p)
    g.synchronize()
    c.check(by.to_array(c.x.dtype, n))


# ================================================================ limit restored
def test_zz_limit_is_restored_and_a_high_limit_changes_nothing():
    """Last in the module: the limit is back to 0, and a limit above every
    cap leaves the grids, and so the bits, as they are."""
    assert LQ.get_max_workgroups() == 0
    t, M, hlen = "crcf", 8, 128
    c = FB.decim_case(t, M, hlen, "burst", DECIM_NOUT, DECIM_CUT)
    y0 = _decim_run(c, 0)
    try:
        LQ.set_max_workgroups(1 << 20)
        assert LQ.get_max_workgroups() == 1 << 20
        y1 = _decim_run(c, 0)
        LQ.set_max_workgroups(3)
        y3 = _decim_run(c, 0)
    finally:
        LQ.set_max_workgroups(0)
    assert LQ.get_max_workgroups() == 0
    assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32))
    # each output is formed the same way whichever workgroup walks its tile
    assert np.array_equal(y0.view(np.uint32), y3.view(np.uint32))
    c.check(y0)
