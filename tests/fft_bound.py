"""Error bounds local to a row for the FFT plan API, and the batches that
probe them.

The plan API (host/fft.c over csrc/k_fft_batch.hip and csrc/k_fft.hip) runs
`batch` transforms of n points in one launch sequence.  The batch kernels put
G = 1 to 512 transforms in a workgroup and walk many groups per workgroup,
reusing registers and LDS; what that can break is the independence of the
rows, and a normwise comparison at one level cannot see it.  Every bound here
is a function of its own row alone: a row at 2^-17 between full-scale rows is
held to 2^-17 of their bound, and a row of zeros must come back as exact
zeros.  eps = 2^-23, all references float64 / complex128.

Power-of-two n (either direction, un-normalised), row b, every bin k:

    bound[b] = (4 lg n + 8) eps sqrt(n) ||x_b||_2

tests/pfb_bound.py's transform term: a float32 power-of-two FFT errs normwise
by at most lg n (mu + gamma_4 (sqrt(2) + mu)) ||X||_2 (Higham, Accuracy and
Stability of Numerical Algorithms, Thm 24.2), below 4 lg n eps ||X||_2 with
float32 twiddles, and ||X||_2 = sqrt(n) ||x||_2; one bin errs by at most the
2-norm of its row's error.  The + 8 covers the four-step's extra twiddle
product (2 eps per point, its table a product of two roundings) with room.
The bound is loose (the oracle sits at 2e-4 to 4e-2 of it), so on the inputs
without exact structure -- noise, a bin-centred tone over a 1e-5 noise floor,
a burst of n / 64 samples over that floor -- the worst ratio err / bound of
the code under test must also be at most MARGIN = 4 times the oracle's
(orc_fft) on the same batch, the project's standing margin.

Direct DFT (n = 3, 5, ... 15: k_dft_batch, float32 sums of n products with
twiddles rounded once from double):

    bound[b] = (n + 4) eps sqrt(n) ||x_b||_2

A bin is a sum of n products: each product errs by at most (sqrt(5) + 1) u
|x_j| (complex multiply, twiddle rounding; u = eps / 2), the sum by (n - 1) u
sum |x_j| to first order, together under (n + 4) u sum_j |x_j| <= (n + 4) u
sqrt(n) ||x||_2; eps = 2 u leaves a factor 2.

Bluestein (other n): with c_j = exp(-i pi dir j^2 / n), a_j = x_j c_j zero
padded to M >= 2n - 1, b the circular conj(c) and B = FFT_M(b),

    y_k = c_k IFFT_M(FFT_M(a) B)_k / M.

  forward:  ||dA||_2 <= 4 lg M eps sqrt(M) ||x||_2 (||a||_2 = ||x||_2), and the
            product carries it times at most max |B|;
  B:        computed by the same M-point transform, so each |dB_k| <= ||dB||_2
            <= 4 lg M eps ||B||_2; the product carries it as |A_k| |dB_k|,
            in 2-norm at most 4 lg M eps ||B||_2 ||A||_2, ||A||_2 = sqrt(M) ||x||_2;
  inverse:  its own error 4 lg M eps sqrt(M) ||P||_2 with ||P||_2 <= max |B|
            sqrt(M) ||x||_2, and it carries the product's error times sqrt(M);
  1 / M is exact; an output errs by at most the 2-norm of the inverse's error.
Dividing by M:

    bound[b] = eps ||x_b||_2 ((8 lg M + 8) max |B| + 4 lg M ||B||_2)

where the + 8 max |B| covers the three pointwise products (pre, B, post: 2 eps
each relative to max |B| ||x||_2) and the chirps' single rounding.  max |B|
and ||B||_2 are computed in float64 for the row's n.  The ||B||_2 term is
sqrt(M) looser than what a transform shows; it is the rigorous per-bin figure.
The oracle transforms these sizes by another algorithm, so there is no margin
assertion here: the bound is asserted and the ratio printed.

Real-to-real (k_r2r, all eight types): the kernel sums in double from exact
integer phases and rounds once, so

    bound[b][i] = 2^-24 |y64[i]| + 2^-40 2 sum_j |x_b[j]|

The first term is the one rounding to float32.  The second covers both double
sums (kernel and reference: n 2^-53 each, n <= 257) and the reference's cosine
arguments, formed in floating point (pi (2k+1)(2i+1) / 4n: 3 roundings of an
argument up to 2 pi 257, under 2e-13), times the sum's scale 2 sum |x|: 2^-40
= 9.1e-13 holds all three.

A batch of `rows` transforms: row b is all zeros for b in zero_rows (one inside
the first group of G rows, one inside the group a workgroup of three walks to
second: group 3), else full scale for b mod 4 < 2 and 2^-17 for the rest (two
rows: full scale and 2^-17; three: full scale, zeros, 2^-17).  rows = 3 G
2 + G + 1 for the kernels that loop.  Each row is asserted through
liquid_mi355x_fft_route to reach the kernels it names.

Shared by tests/test_fft_bound.py and tests/test_gpu_fft_bound.py.  No GPU.
"""
import functools
import math

import numpy as np

EPS = 2.0 ** -23
MARGIN = 4.0
QUIET = 2.0 ** -17
KINDS = ["noise", "tone", "burst"]          # the margin assertion's inputs
EXACT = ["impulse", "ones"]                 # exact structure: the bound only

# transforms per workgroup of the kernels that loop (k_fft_batch<N>, which does not, takes 1024 / N)
from test_gpu_persistent import FFT_G  # noqa: E402


def group(n):
    """Rows per workgroup of the kernel the rows of an n-point transform meet first."""
    if n & (n - 1):
        if n <= 16:
            return 1
        M = bluestein_M(n)
        return FFT_G[M] if M <= 4096 else 1
    if n <= 16:
        return 1 if n == 1 else 1024 // n
    return FFT_G.get(n, 1)


def bluestein_M(n):
    M = 1
    while M < 2 * n - 1:
        M *= 2
    return M


# (n, route with 16-byte-aligned rows, rows or None for 3 G 2 + G + 1, loops: also run at three workgroups)
POW2_ROWS = [
    (1, "dft", None, False),
    (2, "k_fft_batch<2>", None, False),
    (4, "k_fft_batch<4>", None, False),
    (8, "k_fft_batch<8>", None, False),
    (16, "k_fft_batch<16>", None, False),
    (32, "fftsmall<2>", None, True),
    (64, "fftsmall<4>", None, True),
    (128, "fftsmall<8>", None, True),
    (256, "fftr16<1>", None, True),
    (512, "fftr16<2>", None, True),
    (1024, "fft1024", None, True),
    (2048, "fftr16<8>", None, True),
    (4096, "fft4096", None, True),
    (8192, "fft8192/a16", None, True),
    (16384, "fft16384/a16", None, True),
    (32768, "four_step 256x128 cols_r<1> rows_s<8>", 5, False),
    (65536, "four_step 256x256 cols_r<1> rows_r<1>", 5, False),
    (1 << 17, "four_step 512x256 cols_r<2> rows_r<1>", 5, False),
    (1 << 21, "four_step 2048x1024 cols_r<8> rows_r<4>", 2, False),
    (1 << 23, "four_step 4096x2048 cols_r<16> rows_r<8>", 1, False),
]
# the 8-byte loads of the two largest one-pass kernels: rows one sample off a 16-byte boundary
OFF8_ROWS = [(8192, "fft8192/a8"), (16384, "fft16384/a8")]
OTHER_ROWS = [
    (3, "dft", None, False),
    (5, "dft", None, False),
    (15, "dft", None, False),
    (17, "bluestein M=64", None, True),
    (1000, "bluestein M=2048", None, True),
    (2049, "bluestein_fused M=8192 128x64 cols_s<8> rows_s<4>", 5, False),
    (12288, "bluestein_fused M=32768 256x128 cols_r<1> rows_s<8>", 5, False),
    (3 << 17, "bluestein_fused M=1048576 1024x1024 cols_r<4> rows_r<4>", 3, False),
]
ORACLE_MAX_N = 1 << 17   # orc_fft takes 2 s per row at 2^21

R2R_TYPES = [10, 11, 12, 13, 20, 21, 22, 23]
R2R_SIZES = [1, 2, 3, 255, 256, 257]
BIG_BATCH = 70000        # rows on grid.y past 65535


def row_id(r):
    return "n%d" % r[0]


def n_rows(n, rows=None):
    G = group(n)
    return rows if rows is not None else 3 * G * 2 + G + 1


def zero_rows(n, rows):
    """One zero row inside the first group, one inside group 3 (the second a
    workgroup of three walks to); short batches: row 1."""
    G = group(n)
    if rows < 4:
        return [1] if rows == 3 else []
    second = 3 * G + (1 if G > 1 else 0)
    return [1, second] if second < rows else [1]


def levels(n, rows):
    lv = np.where(np.arange(rows) % 4 < 2, 1.0, QUIET)
    if rows == 2:
        lv[1] = QUIET
    lv[zero_rows(n, rows)] = 0.0
    return lv


def _noise(r, shape):
    return r.uniform(-0.5, 0.5, shape) + 1j * r.uniform(-0.5, 0.5, shape)


def batch_input(n, kind, rows):
    """rows x n complex64; each row its level times the unit-level input."""
    r = np.random.default_rng(1000003 * (KINDS + EXACT).index(kind) + n)
    j = np.arange(n)
    if kind == "noise":
        X = _noise(r, (rows, n))
    elif kind == "tone":     # bin centred, a different bin per row, over a 1e-5 noise floor
        k0 = (n // 3 + np.arange(rows)) % n
        X = np.exp(2j * np.pi * ((k0[:, None] * j[None, :]) % n) / n) + 1e-5 * _noise(r, (rows, n))
    elif kind == "burst":    # max(n / 64, 1) level-1 samples over a 1e-5 noise floor
        L = max(n // 64, 1)
        X = 1e-5 * _noise(r, (rows, n))
        for b in range(rows):
            a = (b * 7919) % (n - L + 1)
            X[b, a:a + L] = _noise(r, L) * 2
    elif kind == "impulse":
        X = np.zeros((rows, n), np.complex128)
        X[np.arange(rows), (np.arange(rows) * 7919) % n] = 1.0
    else:
        X = np.ones((rows, n), np.complex128)
    return (X * levels(n, rows)[:, None]).astype(np.complex64)


def reference(X, direction):
    X64 = X.astype(np.complex128)
    return np.fft.fft(X64, axis=1) if direction > 0 else np.fft.ifft(X64, axis=1) * X.shape[1]


@functools.lru_cache(maxsize=None)
def chirp_spectrum(n):
    """(max |B|, ||B||_2) of Bluestein's chirp spectrum for n, in float64."""
    M = bluestein_M(n)
    j = np.arange(n, dtype=np.int64)
    c = np.exp(-1j * np.pi * ((j * j) % (2 * n)) / n)
    b = np.zeros(M, np.complex128)
    b[:n] = np.conj(c)
    b[M - n + 1:] = np.conj(c[1:][::-1])
    B = np.fft.fft(b)
    return float(np.max(np.abs(B))), float(np.linalg.norm(B))


def row_factor(n):
    """bound[b] / (eps ||x_b||_2)"""
    if n & (n - 1) == 0:
        return (4 * math.log2(n) + 8) * math.sqrt(n)
    if n <= 16:
        return (n + 4) * math.sqrt(n)
    lgM = math.log2(bluestein_M(n))
    mx, nrm = chirp_spectrum(n)
    return (8 * lgM + 8) * mx + 4 * lgM * nrm


def bound(X):
    """Per row: row_factor eps ||x_b||_2; exactly 0 for a row of zeros."""
    return row_factor(X.shape[1]) * EPS * np.sqrt(np.sum(np.abs(X.astype(np.complex128)) ** 2, axis=1))


def report(Y, Y64, bnd):
    """Per row: worst |Y - Y64| over the bins against the row's bound.  Returns
    the worst ratio (over rows whose bound is not 0), its row, the failing
    rows, the rows that must be zero and are not, the non-finite outputs."""
    Y = np.asarray(Y)
    assert Y.shape == Y64.shape and bnd.shape == (Y.shape[0],)
    finite = np.isfinite(Y.real) & np.isfinite(Y.imag) if np.iscomplexobj(Y) else np.isfinite(Y)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(Y.astype(Y64.dtype) - Y64)
    err[~finite] = np.inf
    err = np.max(err, axis=1)
    zero = bnd == 0
    nonzero_zeros = zero & np.any(Y != 0, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(zero, np.where(nonzero_zeros, np.inf, 0.0), err / np.where(zero, 1.0, bnd))
    worst = int(np.argmax(ratio))
    return {"worst": float(ratio[worst]), "row": worst, "failing": np.flatnonzero(~(ratio <= 1.0)).tolist(),
            "nonzero_zeros": int(np.count_nonzero(nonzero_zeros)), "nonfinite": int(np.count_nonzero(~finite)),
            "rows": int(Y.shape[0])}


def check(Y, Y64, bnd, oracle_worst=None, what=""):
    """Both assertions: every row within its bound (exact zeros where it is 0,
    all finite) and, given the oracle's worst ratio on the batch, the worst
    ratio within MARGIN of it.  Prints both."""
    r = report(Y, Y64, bnd)
    print("fft_bound %s: worst %.4g of the bound at row %d (oracle %s), %d of %d rows fail, %d nonzero zero rows, "
          "%d non-finite" % (what, r["worst"], r["row"], "-" if oracle_worst is None else "%.4g" % oracle_worst,
                             len(r["failing"]), r["rows"], r["nonzero_zeros"], r["nonfinite"]))
    assert not r["failing"] and r["nonfinite"] == 0, (
        "%s: worst error %.4g x the bound at row %d; rows %s of %d fail; %d rows that must be zero are not; %d "
        "non-finite" % (what, r["worst"], r["row"], r["failing"][:8], r["rows"], r["nonzero_zeros"], r["nonfinite"]))
    if oracle_worst is not None:
        assert r["worst"] <= MARGIN * oracle_worst, (
            "%s: worst ratio %.4g at row %d is more than %g x the oracle's %.4g"
            % (what, r["worst"], r["row"], MARGIN, oracle_worst))
    return r


class Case:
    """One batch: input, bound, and the float64 reference per direction."""

    def __init__(self, n, kind, rows=None):
        self.n, self.kind = n, kind
        self.rows = n_rows(n, rows)
        self.X = batch_input(n, kind, self.rows)
        self.bound = bound(self.X)
        self.X.setflags(write=False)
        self.bound.setflags(write=False)

    @functools.lru_cache(maxsize=2)
    def y64(self, direction):
        y = reference(self.X, direction)
        y.setflags(write=False)
        return y

    def check(self, Y, direction, oracle_worst=None, what=""):
        return check(Y, self.y64(direction), self.bound, oracle_worst,
                     "n=%d %s dir=%+d %s" % (self.n, self.kind, direction, what))


@functools.lru_cache(maxsize=6)
def case(n, kind, rows=None):
    return Case(n, kind, rows)


def oracle_rows(O, X, direction):
    return np.stack([O.fft(x, direction) for x in X])


@functools.lru_cache(maxsize=None)
def oracle_worst(n, kind, rows, direction):
    """The oracle's worst ratio on a batch (power-of-two n up to ORACLE_MAX_N)."""
    import oracle_lib as O
    c = case(n, kind, rows)
    return c.check(oracle_rows(O, c.X, direction), direction, what="oracle")["worst"]


# ---------------------------------------------------------------- real-to-real
def r2r_input(n, rows=3):
    """rows x n float32: full scale, 2^-17, zeros, then alternating (the large batch)."""
    r = np.random.default_rng(77 + n)
    lv = np.where(np.arange(rows) % 3 == 0, 1.0, np.where(np.arange(rows) % 3 == 1, QUIET, 0.0))
    return (r.uniform(-0.5, 0.5, (rows, n)) * lv[:, None]).astype(np.float32)


def r2r_bound(X, Y64):
    """Per output: 2^-24 |y64| + 2^-40 2 sum |x_b|."""
    return 2.0 ** -24 * np.abs(Y64) + 2.0 ** -40 * 2.0 * np.sum(np.abs(X.astype(np.float64)), axis=1)[:, None]


def r2r_report(Y, Y64, bnd):
    Y = np.asarray(Y)
    assert Y.shape == Y64.shape == bnd.shape
    finite = np.isfinite(Y)
    with np.errstate(invalid="ignore"):
        err = np.abs(Y.astype(np.float64) - Y64)
    err[~finite] = np.inf
    zero = bnd == 0
    ok = np.where(zero, Y == 0, err <= bnd)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(zero, np.where(Y == 0, 0.0, np.inf), err / np.where(zero, 1.0, bnd))
    return {"worst": float(np.max(ratio)), "at": tuple(int(v) for v in np.unravel_index(np.argmax(ratio), ratio.shape)),
            "failing": int(np.count_nonzero(~ok)), "nonfinite": int(np.count_nonzero(~finite))}


def r2r_check(Y, Y64, bnd, what=""):
    r = r2r_report(Y, Y64, bnd)
    print("fft_bound r2r %s: worst %.4g of the bound at %s, %d fail, %d non-finite"
          % (what, r["worst"], r["at"], r["failing"], r["nonfinite"]))
    assert r["failing"] == 0 and r["nonfinite"] == 0, (
        "r2r %s: worst error %.4g x the bound at %s; %d outputs fail; %d non-finite"
        % (what, r["worst"], r["at"], r["failing"], r["nonfinite"]))
    return r
