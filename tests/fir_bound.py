"""The direct form's per-output error bound for firfilt, and the cases that probe it.

The reference firfilt computes each output as one float32 dot product over
the last hlen inputs (firfilt.c:322-338), so an output's error is
proportional to the inputs that output sees -- not to the loudest sample
anywhere near it.  For a stream x with zero initial history, taps h and the
user scale s, in float64 / complex128:

    y64  = s (h * x)                       the causal convolution, whole stream
    A[n] = |s| sum_k |h[k]| |x[n-k]|       moduli for complex values
    T    = real terms per output component: hlen (rrrf, crcf), 2 hlen (cccf)

and an output y[n] passes if

    |y[n] - y64[n]| <= (T + 8) 2^-23 A[n],   or   A[n] == 0 and y[n] == 0.

Where the bound comes from (u = 2^-24): a float32 sum of T products in any
order errs by at most gamma_T A; the two components of a complex output add
a factor sqrt(2), together 0.71 T 2^-23 A.  The matrix-core kernels drop split
terms below 3 2^-24 |x||h| per tap (k_firfilt_mx.hip), about 2.1 2^-23 A more;
the scale multiply and the rounding of the result add about 1.5 2^-23 A.
(T + 8) 2^-23 covers these and an accumulator that truncates.  Every output is
checked; every output must be finite.

Shared by tests/test_fir_bound.py (the oracle meets the bound: it is
reachable, and the checker is pinned) and tests/test_gpu_fir_bound.py (every
kernel, however the caller cuts the stream).

The decimator (decim_reference, decim_case) is held to the same bound with
the same checker: firdecim forms y[o] = sum_k h[k] x[oM - k] as one float32
dot product (firdecim.c:195-204), there is no output scale, and its kernels
are plain float32 multiply-adds in some order -- no split terms -- so
gamma_T A with the sqrt(2) of a complex output is all there is, and
(T + 8) 2^-23 A[o] holds it with A[o] = sum_k |h[k]| |x[oM - k]|.  Its
envelopes put their edges on the kernels' tile seams (tests/test_gpu_persistent.py).
"""
import functools
import zlib

import numpy as np

EPS = 2.0 ** -23

# (type, taps): rrrf 45 VALU / matrix-core real; crcf 64 the 16-column
# matrix-core kernel; crcf 100 two tap blocks; crcf 129 / 200 three and four
# blocks, cccf 65 / 200 and crcf 2050 the VALU kernel -- the long complex
# filters a transform form would take (it did, and missed the bound: firfilt
# has none now, and these rows keep it so)
FILTERS = [("rrrf", 45), ("crcf", 64), ("crcf", 100), ("crcf", 129), ("crcf", 200),
           ("cccf", 65), ("cccf", 200), ("crcf", 2050)]
ENVELOPES = ["flat", "burst", "gaps", "stairs"] + ["two-level-%d" % k for k in range(1, 18, 2)]


def filter_id(f):
    return "%s%d" % f


def seg_len(hlen):
    """New samples per segment of an overlap-save transform form (4096
    points up to 2049 taps, 8192 past that): the envelopes put their bursts
    and level steps where such a form has its seams."""
    return 4096 - (hlen - 1) if hlen <= 2049 else 8192 - (hlen & ~1)


def scale_of(t):
    return (0.7 - 0.2j) if t == "cccf" else 0.7


def envelope(name, hlen):
    L = seg_len(hlen)
    n = 3 * L + 777
    if name == "flat":
        return np.ones(n)
    if name in ("burst", "gaps"):
        e = np.full(n, 1e-5 if name == "burst" else 0.0)
        for a, b in ((0, 40), (2000, 2300), (L - 50, L + 50), (2 * L + 1000, 2 * L + 1001)):
            e[a:b] = 1.0
        return e
    if name == "stairs":   # 400-sample steps 1, 1e-1, ..., 1e-5 and back up, repeating
        step = np.arange(n) // 400 % 10
        return np.array([1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5])[np.minimum(step, 10 - step)]
    if name.startswith("two-level-"):   # per run of L samples: first half at 1, second at 2^-k
        k = int(name.rsplit("-", 1)[1])
        return np.where(np.arange(n) % L < L // 2, 1.0, 2.0 ** -k)
    raise ValueError(name)


def signal(t, hlen, name, env):
    """Taps and samples of a case: uniform in [-0.5, 0.5) per component, the
    samples times the envelope; the seed is fixed per case."""
    r = np.random.default_rng(zlib.crc32(("%s %d %s" % (t, hlen, name)).encode()))
    n = len(env)
    if t == "cccf":
        h = (r.uniform(-0.5, 0.5, hlen) + 1j * r.uniform(-0.5, 0.5, hlen)).astype(np.complex64)
    else:
        h = r.uniform(-0.5, 0.5, hlen).astype(np.float32)
    if t == "rrrf":
        x = (r.uniform(-0.5, 0.5, n) * env).astype(np.float32)
    else:
        x = ((r.uniform(-0.5, 0.5, n) + 1j * r.uniform(-0.5, 0.5, n)) * env).astype(np.complex64)
    return h, x


def reference(t, h, x, s):
    """(y64, A) of the stream; s is rounded to the float32 the object holds."""
    s = complex(np.complex64(s)) if t == "cccf" else float(np.float32(s))
    wide = np.float64 if t == "rrrf" else np.complex128
    y64 = s * np.convolve(x.astype(wide), h.astype(np.complex128 if t == "cccf" else np.float64))[: len(x)]
    A = abs(s) * np.convolve(np.abs(x.astype(wide)), np.abs(h.astype(np.complex128)))[: len(x)]
    return y64, A


class Case:
    def __init__(self, t, hlen, name, h, x, s):
        self.t, self.hlen, self.name, self.h, self.x, self.s = t, hlen, name, h, x, s
        self.y64, self.A = reference(t, h, x, s)
        for a in (self.x, self.y64, self.A):   # shared among tests: left unchanged
            a.setflags(write=False)

    def check(self, y):
        check(self.t, self.hlen, y, self.y64, self.A)


@functools.lru_cache(maxsize=None)
def case(t, hlen, name):
    h, x = signal(t, hlen, name, envelope(name, hlen))
    return Case(t, hlen, name, h, x, scale_of(t))


@functools.lru_cache(maxsize=None)
def long_case(t, hlen, name, n):
    """The envelope of case() repeated to n samples (np.resize), for streams
    long enough to make a capped grid walk (tests/test_gpu_persistent.py)."""
    h, x = signal(t, hlen, "%s x%d" % (name, n), np.resize(envelope(name, hlen), n))
    return Case(t, hlen, name, h, x, scale_of(t))


def carried_split(hlen):
    """Case (c): the length of the first call, which ends inside a level-1
    burst; the second call (at least 8192 samples) is all at 1e-5."""
    return 2500, 2 * seg_len(hlen) + 777


@functools.lru_cache(maxsize=None)
def carried_case(t, hlen):
    n1, n2 = carried_split(hlen)
    assert n2 >= 8192
    env = np.full(n1 + n2, 1e-5)
    env[n1 - 300:n1] = 1.0
    h, x = signal(t, hlen, "carried", env)
    return Case(t, hlen, "carried", h, x, scale_of(t))


@functools.lru_cache(maxsize=None)
def overflow_case(small):
    """crcf, 129 equal taps of 2^13 on a constant 2^98 (direct sum 129 2^111 =
    3.3e35, finite, where a transform's intermediate sums pass 2^128); the
    mirror: taps 2^-13, input 2^-58."""
    e_h, e_x = (-13, -58) if small else (13, 98)
    h = np.full(129, 2.0 ** e_h, np.float32)
    x = np.full(9000, 2.0 ** e_x + 0j, np.complex64)
    return Case("crcf", 129, "small" if small else "overflow", h, x, 1.0)


# ------------------------------------------------------------------ firdecim
def decim_reference(t, h, x, M):
    """(y64, A) of the len(x) // M outputs of a decimator with zero initial
    history: y64[o] = sum_k h[k] x[oM - k], A[o] = sum_k |h[k]| |x[oM - k]|, in
    float64 / complex128.  One pass per tap over the input split by phase
    (x[oM - k] with k = qM + r is phase (M - r) % M, row o - q - (r > 0)), so
    every pass is a contiguous multiply-add over the outputs."""
    nout = len(x) // M
    wide = np.float64 if t == "rrrf" else np.complex128
    hw = h.astype(np.complex128 if t == "cccf" else np.float64)
    ah = np.abs(hw)
    P = np.ascontiguousarray(x[:nout * M].astype(wide).reshape(nout, M).T)   # P[r, j] = x[jM + r]
    aP = np.abs(P)
    y64, A = np.zeros(nout, wide), np.zeros(nout)
    for k in range(len(hw)):
        q, r = divmod(k, M)
        ph, d = (0, q) if r == 0 else (M - r, q + 1)
        if d < nout:
            y64[d:] += hw[k] * P[ph, :nout - d]
            A[d:] += ah[k] * aP[ph, :nout - d]
    return y64, A


def decim_envelope(name, M, nout, cut, tile=512):
    """burst (1e-5 between the bursts) or gaps (exact zeros) over nout M input
    samples, the edges of the bursts on the seams of the decimator's tiles:
    256 and 512 outputs, that is multiples of a = 256 M and b = 512 M input
    samples, and one sample either side; one burst ends with the last input
    of the first `cut` outputs, so a call that starts at output `cut` sees it
    only through the carried history; one runs to the end of the stream.
    tile = 64 puts the seams at 32 and 64 outputs instead, for streams of a
    few of the 64-output kernel's tiles."""
    assert name in ("burst", "gaps")
    n, a, b = nout * M, tile // 2 * M, tile * M
    assert nout >= 3 * tile + 1 and tile < cut < nout - tile
    e = np.full(n, 1e-5 if name == "burst" else 0.0)
    mid = max(2, nout // tile // 2) * b   # a seam of both tile sizes far from the start
    for lo, hi in ((0, 40), (a - 50, a + 1), (b - 1, b + 60), (3 * a + 1, 3 * a + 300), (2 * b - 200, 2 * b - 1),
                   (5 * a, 5 * a + 1), (mid - 1, mid + 1), (cut * M - 300, cut * M),
                   (n - 3 * M - 1, n)):
        e[max(lo, 0):min(hi, n)] = 1.0
    return e


# (M, taps): one row per kernel the decimator's dispatch reaches for 16-byte
# aligned or for unaligned input (tests/test_gpu_persistent.py names them),
# each run for rrrf, crcf and cccf; DECIM_PLAIN is the one shape family that
# reaches the undivided-taps kernel (about 6000 taps per unit of M and more)
DECIM_ROWS = [(2, 80), (4, 37), (8, 128), (12, 96), (16, 128), (32, 256), (200, 801)]
DECIM_PLAIN = ("rrrf", 2, 40000)
DECIM_SMALL = (3 * 512 + 77, 700)   # (outputs, cut) of the small versions the oracle runs


class DecimCase:
    def __init__(self, t, M, hlen, name, nout, cut, tile=512):
        self.t, self.M, self.hlen, self.name, self.nout, self.cut = t, M, hlen, name, nout, cut
        self.h, self.x = signal(t, hlen, "decim %d %s" % (M, name), decim_envelope(name, M, nout, cut, tile))
        self.y64, self.A = decim_reference(t, self.h, self.x, M)
        for a in (self.x, self.y64, self.A):
            a.setflags(write=False)

    def check(self, y):
        return check(self.t, self.hlen, y, self.y64, self.A)


def decim_case(t, M, hlen, name, nout, cut, tile=512):
    """Not cached: a large-M case is a few hundred megabytes; its one test
    runs every cut of the stream against it."""
    return DecimCase(t, M, hlen, name, nout, cut, tile)


def report(t, hlen, y, y64, A):
    """Worst ratio to the bound, its index, the number of failing outputs and
    the number of outputs that must be zero but are not."""
    y = np.asarray(y)
    assert y.shape == y64.shape
    T = 2 * hlen if t == "cccf" else hlen
    bound = (T + 8) * EPS * A
    finite = np.isfinite(y)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(y.astype(y64.dtype) - y64)
    err[~finite] = np.inf
    zero = A == 0
    ok = np.where(zero, y == 0, err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(zero, np.where(y == 0, 0.0, np.inf), err / bound)
    worst = int(np.argmax(ratio))
    return {"worst": float(ratio[worst]), "index": worst, "failing": int(np.count_nonzero(~ok)),
            "nonzero_zeros": int(np.count_nonzero(zero & (y != 0))),
            "nonfinite": int(np.count_nonzero(~finite)), "n": int(len(y))}


def check(t, hlen, y, y64, A):
    r = report(t, hlen, y, y64, A)
    print("fir_bound %s h=%d: worst %.4g of the bound at %d, %d of %d fail, %d nonzero zeros, %d non-finite"
          % (t, hlen, r["worst"], r["index"], r["failing"], r["n"], r["nonzero_zeros"], r["nonfinite"]))
    assert r["failing"] == 0 and r["nonfinite"] == 0, (
        "%s h=%d: worst error %.4g x the bound at output %d; %d of %d outputs fail; %d outputs that must be "
        "zero are not; %d non-finite" % (t, hlen, r["worst"], r["index"], r["failing"], r["n"],
                                         r["nonzero_zeros"], r["nonfinite"]))
    return r
