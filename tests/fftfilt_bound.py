"""An error bound local to a window for fftfilt's transform kernels, and the
cases that probe it.

fftfilt computes y = s (h * x) by fast convolution: the reference by a
2n-point overlap-add per n-sample call (fftfilt.c:193-260), the kernels by
overlap-save over fixed nfft-point segments (csrc/k_fftfilt.hip, nfft =
lqk_fftfilt_nfft: 4096 up to 2049 taps, 8192 for complex samples up to 4097).
A transform cannot meet the direct form's per-output bound (tests/fir_bound.py):
its rounding error scales with the loudest sample of the segment, not with
the inputs an output sees.  But the error is still local -- an output can be
touched only by the inputs of the segment(s) that cover it -- and that is
what a persistent kernel that carries registers and LDS from one segment to
the next, a history job and first / last-segment special cases can break.

The bound, independent of where segments or calls fall.  With G = sum |h|,
lg = log2 nfft, eps = 2^-23, in float64 / complex128:

    y64      = s (h * x)                                   whole stream, zero initial history
    W[n]     = || x[n - (nfft-1) .. n + (nfft-1)] ||_2     clipped to the stream
    bound[n] = (8 lg + 8) eps |s| G W[n]

Derivation (u = 2^-24).  Any segment of at most nfft samples that contains
sample n lies inside the span of W[n], for overlap-save at any offset and for
the reference's overlap-add with 2n <= nfft (the block of n and the one
before it).  A power-of-two float32 FFT of N points errs normwise by at most
lg N (mu + gamma_4 (sqrt(2) + mu)) ||.||_2 (Higham, Accuracy and Stability of
Numerical Algorithms, Thm 24.2), below 4 lg N eps with float32 twiddles, as
derived in tests/pfb_bound.py.  A segment X goes through two such transforms
with a pointwise product between them: the forward error 4 lg eps ||X||_2 is
multiplied by at most max |H| <= G, the inverse adds 4 lg eps ||H X||_2 <=
4 lg eps G ||X||_2 (unitary scaling; 1/nfft is exact), together 8 lg eps G
||X||_2 to first order; the spectrum H carries its own transform error, 4 lg
eps ||h||_2 <= 4 lg eps G per bin relative to G, the product and the scale
multiply a few eps more: the + 8 covers these (and the 8 lg is itself twice
what kernels and oracle show -- see below).  One output errs by at most the
2-norm of its segment's error, and ||X||_2 <= W[n].

An output passes if |y - y64| <= bound; where the bound is exactly 0 the whole
window is zero and the output must be exactly 0 (either sign).  Every output
must be finite.

The bound is rigorous but loose: the oracle with n = nfft / 2 sits at 1e-5 to
5e-4 of it.  So a second assertion carries the tightness: the worst ratio
err / bound of the code under test must be at most MARGIN = 4 times the
oracle's worst ratio on the same case -- this project's standing margin for a
float32 computation of the same size in a different order (tests/pfb_bound.py,
tests/resamp_bound.py).

The stream: with L the new samples per segment (fir_bound.seg_len), n = 2L +
5 nfft + 777 samples, level-1 runs on [0, 40), [L - 50, L + 50) (a segment
seam), [2L - 1, 2L + 1) and the last 3 samples over a floor of 1e-5 (burst) or
exact zeros (gaps); the 8192-point rows also run one sample shorter, so the
kernel's last sample pair straddles n in one and ends on it in the other.

Filters past the transforms (rrrf over 2049 taps, any over 4097) run the
direct FIR engine and are held to fir_bound's (T + 8) 2^-23 A bound instead.

Shared by tests/test_fftfilt_bound.py (the oracle meets the bound, the
conditions on the cases hold, the checker is pinned) and
tests/test_gpu_fftfilt_bound.py (every kernel, however the stream is cut).
No GPU.
"""
import functools
import math

import numpy as np

import fir_bound as FB

EPS = 2.0 ** -23
MARGIN = 4.0
ENVELOPES = ["burst", "gaps"]

# (type, taps, kernel, mode); mode "off8": x and y 8 bytes past a 16-byte
# boundary (device calls only)
ROWS = [
    ("rrrf", 45, "k_fftfilt_r16<true>", None),
    ("rrrf", 2049, "k_fftfilt_r16<true>", None),      # the longest 4096-point filter: L = 2048
    ("crcf", 1, "k_fftfilt_r16<false>", None),        # h - 1 = 0: no history, no history job
    ("crcf", 512, "k_fftfilt_r16<false>", None),
    ("cccf", 2049, "k_fftfilt_r16<false>", None),
    ("crcf", 2050, "k_fftfilt8k<true>", None),        # odd h - 1: the discarded part hd rounds up to 2050
    ("cccf", 4097, "k_fftfilt8k<true>", None),        # the longest transform filter: L = 4096
    ("crcf", 2050, "k_fftfilt8k<false>", "off8"),     # the unpaired 8-byte loads and stores
    ("rrrf", 2050, "direct", None),                   # one tap past the real transform
    ("crcf", 4098, "direct", None),                   # one tap past the complex one
]


def row_id(r):
    return "%s-h%d%s" % (r[0], r[1], "-" + r[3] if r[3] else "")


def nfft_of(t, hlen):
    """lqk_fftfilt_nfft restated (the tests assert they agree): 0 is the direct engine."""
    if hlen - 1 <= 2048:
        return 4096
    return 8192 if t != "rrrf" and hlen - 1 <= 4096 else 0


def span_of(t, hlen):
    """Points the stream and the bound's window are sized by: the direct rows
    take the 8192 of the transform a tap shorter."""
    return nfft_of(t, hlen) or 8192


def stream_len(t, hlen, short=False):
    return 2 * FB.seg_len(hlen) + 5 * span_of(t, hlen) + 777 - (1 if short else 0)


def envelope(name, t, hlen, short=False):
    assert name in ENVELOPES
    L, n = FB.seg_len(hlen), stream_len(t, hlen, short)
    e = np.full(n, 1e-5 if name == "burst" else 0.0)
    for a, b in ((0, 40), (L - 50, L + 50), (2 * L - 1, 2 * L + 1), (n - 3, n)):
        e[a:b] = 1.0
    return e


def cuts(t, hlen):
    """A first call shorter than h - 1 for the long filters, a cut inside a
    segment, and a last call that is all quiet but for the final samples."""
    L = FB.seg_len(hlen)
    return (40, L + 7, 2 * L + 1 + span_of(t, hlen))


def window_norm(x, nfft):
    """W[n]: the 2-norm of x over [n - (nfft-1), n + (nfft-1)], clipped; exact
    zeros where the window holds none but zeros (extended-precision running sum)."""
    n = len(x)
    c = np.concatenate([[0], np.cumsum(np.abs(x.astype(np.complex128)).astype(np.longdouble) ** 2)])
    i = np.arange(n)
    lo, hi = np.maximum(i - (nfft - 1), 0), np.minimum(i + nfft, n)
    return np.sqrt(np.maximum(c[hi] - c[lo], 0)).astype(np.float64)


class Case:
    def __init__(self, t, hlen, name, short=False):
        self.t, self.hlen, self.name, self.short = t, hlen, name, short
        self.nfft = nfft_of(t, hlen)
        self.L = FB.seg_len(hlen)
        self.h, self.x = FB.signal(t, hlen, "fftfilt %s%s" % (name, " short" if short else ""),
                                   envelope(name, t, hlen, short))
        self.y1, self.A1 = FB.reference(t, self.h, self.x, 1.0)   # unit scale; A1 for the direct rows
        G = float(np.sum(np.abs(self.h.astype(np.complex128))))
        lg = math.log2(span_of(t, hlen))
        self.bound1 = (8 * lg + 8) * EPS * G * window_norm(self.x, span_of(t, hlen))
        for a in (self.h, self.x, self.y1, self.A1, self.bound1):   # shared among tests: left unchanged
            a.setflags(write=False)

    def _s(self, s):
        return complex(np.complex64(s)) if self.t == "cccf" else float(np.float32(np.real(s)))

    def report(self, y, s=1.0):
        """Worst ratio to the bound (over outputs whose bound is not 0), its
        index, the failing outputs, the must-be-zero outputs that are not."""
        s = self._s(s)
        y = np.asarray(y)
        y64, bound = s * self.y1, abs(s) * self.bound1
        assert y.shape == y64.shape
        finite = np.isfinite(y)
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(y.astype(y64.dtype) - y64)
        err[~finite] = np.inf
        zero = bound == 0
        ok = np.where(zero, y == 0, err <= bound)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(zero, np.where(y == 0, 0.0, np.inf), err / bound)
        worst = int(np.argmax(ratio))
        return {"worst": float(ratio[worst]), "index": worst, "failing": int(np.count_nonzero(~ok)),
                "nonzero_zeros": int(np.count_nonzero(zero & (y != 0))),
                "nonfinite": int(np.count_nonzero(~finite)), "n": int(len(y))}

    def check(self, y, s=1.0, oracle_worst=None, what=""):
        """Both assertions: every output within its bound (exact zeros where
        it is 0, all finite), and, given the oracle's worst ratio on this
        case, the worst ratio within MARGIN of it.  Prints both."""
        r = self.report(y, s)
        print("fftfilt_bound %s h=%d %s %s: worst %.4g of the bound at %d (oracle %s), %d of %d fail, %d nonzero "
              "zeros, %d non-finite" % (self.t, self.hlen, self.name, what, r["worst"], r["index"],
                                        "-" if oracle_worst is None else "%.4g" % oracle_worst, r["failing"],
                                        r["n"], r["nonzero_zeros"], r["nonfinite"]))
        assert r["failing"] == 0 and r["nonfinite"] == 0, (
            "%s h=%d %s: worst error %.4g x the bound at output %d; %d of %d outputs fail; %d outputs that must "
            "be zero are not; %d non-finite" % (self.t, self.hlen, what, r["worst"], r["index"], r["failing"],
                                                r["n"], r["nonzero_zeros"], r["nonfinite"]))
        if oracle_worst is not None:
            assert r["worst"] <= MARGIN * oracle_worst, (
                "%s h=%d %s: worst ratio %.4g at output %d is more than %g x the oracle's %.4g"
                % (self.t, self.hlen, what, r["worst"], r["index"], MARGIN, oracle_worst))
        return r

    def check_direct(self, y, s):
        """The direct-engine rows: fir_bound's per-output bound."""
        s = self._s(s)
        return FB.check(self.t, self.hlen, y, s * self.y1, abs(s) * self.A1)


@functools.lru_cache(maxsize=None)
def case(t, hlen, name, short=False):
    return Case(t, hlen, name, short)


def oracle_stream(O, c, n, s=1.0):
    """The oracle's fftfilt with block n over the case's stream (zero padded
    to whole blocks, cut back), at the real scale s."""
    typ = {"rrrf": O.RRRF, "crcf": O.CRCF, "cccf": O.CCCF}[c.t]
    o = O.FftFilt(typ, c.h, n)
    o.set_scale(s)
    pad = (-len(c.x)) % n
    return o.execute_stream(np.concatenate([c.x, np.zeros(pad, c.x.dtype)]))[: len(c.x)]


@functools.lru_cache(maxsize=None)
def oracle_worst(t, hlen, name, short=False):
    """The oracle's worst ratio on a case, at n = nfft / 2 (scale 0.7; the ratio
    does not depend on it but for the scale multiply's rounding)."""
    import oracle_lib as O
    c = case(t, hlen, name, short)
    r = c.check(oracle_stream(O, c, c.nfft // 2, 0.7), 0.7, what="oracle n=%d" % (c.nfft // 2))
    return r["worst"]
