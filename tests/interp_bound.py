"""The direct form's per-output error bound for firinterp and firpfb's block
interpolation, and the cases that probe it.

firinterp forms each output as one float32 dot product over the last L
inputs, y[iM + p] = sum_l h'[p + lM] x[i - l] with h' the taps zero padded to
M L, L = ceil(h_len / M) (firinterp.c:187-215 via firpfb.c:325-345); firpfb's
execute_block pushes each input and evaluates every bank after it,
y[tM + i] = s sum_n h[i + nM] x[t - n], n < L = floor(h_len / M), s the
object's scale.  Both are the stream zero stuffed by M and convolved with the
taps, so with zero initial history, in float64 / complex128,

    u[iM] = x[i], 0 elsewhere
    y64   = s (h * u)             cut to len(x) M outputs  (s = 1 for firinterp)
    A     = |s| (|h| * |u|)       moduli for complex values
    T     = real terms per output component: L (rrrf, crcf), 2L (cccf)

and an output passes if |y - y64| <= (T + 8) 2^-23 A, or A == 0 and y == 0
exactly; every output must be finite.  The bound, its derivation and the
checker are tests/fir_bound.py's (report / check with hlen := L): the kernels
are plain float32 multiply-adds in some order, no split terms, so gamma_T A
with the sqrt(2) of a complex output and the scale multiply is all there is.

The stream is three tiles of the kernels' 256 inputs and a ragged, odd tail.
Its envelopes put level-1 runs on the first samples, a wave seam (64), a tile
seam (256), one single sample, the L inputs before a tile (which that tile
sees only through its staged window) and the last two samples, over a floor
of 1e-5 (burst) or exact zeros (gaps); `carried` ends a loud run at input 500
with 1e-5 after it, for a second call that sees the loud samples only through
the object's history.

Shared by tests/test_interp_bound.py (the oracle meets the bound, the routes
and the checker are pinned) and tests/test_gpu_interp_bound.py (every route of
lqk_firinterp, however the caller cuts the stream).  No GPU.
"""
import functools

import numpy as np

import fir_bound as FB

NT = 256                 # inputs per workgroup tile of both kernels
N = 3 * NT + 77
ENVELOPES = ["burst", "gaps"]
CUTS = (1, 64, 65, 320)  # the first calls shorter than L - 1: history composed from history
CARRIED_CUT = 500

# (type, M, h_len, route): route 0 is the plain k_firinterp, else the LT class
# of k_firinterp_t<kind, LT> (liquid_mi355x_firinterp_route, 16-byte aligned y)
ROWS = [
    ("rrrf", 2, 14, 8),
    ("rrrf", 2, 2, 8),       # L = 1: no history
    ("crcf", 4, 45, 12),     # ragged: L = 12, the last phase taps are padding
    ("crcf", 3, 48, 16),     # odd M
    ("rrrf", 5, 100, 20),
    ("crcf", 8, 192, 24),
    ("rrrf", 16, 512, 32),
    ("crcf", 30, 240, 8),    # the last M under the register-window kernel's 64 KB of LDS
    ("rrrf", 61, 488, 8),    # the same for real samples
    ("crcf", 31, 248, 0),    # plain: LDS
    ("rrrf", 65, 130, 0),    # plain: M > 64
    ("crcf", 4, 132, 0),     # plain: L = 33
    ("cccf", 4, 57, 0),      # plain: complex taps
]
# the unaligned-output route (plain), reached through execute_block_dev only
UNALIGNED_ROWS = [("crcf", 4, 45), ("rrrf", 5, 100)]
# firpfb (type, M, h_len, scale, route): L = floor(h_len / M)
PFB_ROWS = [
    ("rrrf", 4, 4 * 12 + 3, 1.0, 12),     # 3 taps past M L: dropped (firpfb.c:73-84)
    ("crcf", 8, 8 * 24, 0.7, 24),
    ("cccf", 4, 4 * 15, 0.7 - 0.2j, 0),
]


def row_id(r):
    return "%s-M%d-h%d" % (r[0], r[1], r[2])


def taps_per_phase(M, hlen, pfb=False):
    return hlen // M if pfb else -(-hlen // M)


def envelope(name, L, n=N):
    """Level-1 runs over a floor of 1e-5 (burst, carried) or 0 (gaps); runs
    past a short stream's end are left out."""
    e = np.full(n, 0.0 if name == "gaps" else 1e-5)
    if name == "carried":
        runs = ((0, 3), (CARRIED_CUT - max(L, 2), CARRIED_CUT))
    else:
        assert name in ENVELOPES
        runs = ((0, 3), (60, 65), (NT - 1, NT + 1), (300, 301), (2 * NT - L, 2 * NT), (n - 2, n))
    for a, b in runs:
        if 0 <= a and b <= n:
            e[a:b] = 1.0
    return e


def reference(t, h, x, M, s=1.0):
    """(y64, A) of len(x) M outputs; s is rounded to the float32 the object holds."""
    s = complex(np.complex64(s)) if t == "cccf" else float(np.float32(np.real(s)))
    wide = np.float64 if t == "rrrf" else np.complex128
    u = np.zeros(len(x) * M, wide)
    u[::M] = x
    hw = h.astype(np.complex128 if t == "cccf" else np.float64)
    y64 = s * np.convolve(u, hw)[: len(u)]
    A = abs(s) * np.convolve(np.abs(u), np.abs(hw))[: len(u)]
    return y64, A


class Case:
    def __init__(self, t, M, hlen, name, s=1.0, pfb=False, n=N):
        self.t, self.M, self.hlen, self.name, self.s, self.pfb = t, M, hlen, name, s, pfb
        self.L = taps_per_phase(M, hlen, pfb)
        self.h, self.x = FB.signal(t, hlen, "%s %d %s" % ("pfb" if pfb else "interp", M, name),
                                   envelope(name, self.L, n))
        self.y64, self.A = reference(t, self.h[: M * self.L] if pfb else self.h, self.x, M, s)
        for a in (self.h, self.x, self.y64, self.A):   # shared among tests: left unchanged
            a.setflags(write=False)

    def report(self, y):
        return FB.report(self.t, self.L, y, self.y64, self.A)

    def check(self, y):
        return FB.check(self.t, self.L, y, self.y64, self.A)


@functools.lru_cache(maxsize=None)
def case(t, M, hlen, name, s=1.0, pfb=False, n=N):
    return Case(t, M, hlen, name, s, pfb, n)
