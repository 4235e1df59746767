"""The direct form's per-row error bound for dotprod_{rrrf,crcf,cccf}, and the
batches that probe it.

A dot product is one output of the direct form (tests/fir_bound.py) with
hlen = n and no scale.  For each row v of a batch, in float64 / complex128,

    y64[v] = sum_i h[i] X[v][i]
    A[v]   = sum_i |h[i]| |X[v][i]|        moduli for complex values
    T      = real terms per output component: n (rrrf, crcf), 2n (cccf)

and row v passes if

    |y[v] - y64[v]| <= (T + 8) 2^-23 A[v],   or   A[v] == 0 and y[v] == 0,

every row finite; fir_bound.report / check with hlen = n is the checker.  The
bound holds for any order of float32 multiply-adds.  The kernels use fma and
sum in a tree, so it is not tight, and for long rows it is very loose (n =
1024 cccf: about 250 times the error a kernel makes).  So every case is also
held to the oracle's own error: the worst ratio to the bound over the rows of
the case is at most MARGIN = 4 times the worst ratio of the oracle
(O.dotprod_batch, a serial float32 sum) on the same rows -- the margin of the
other bound modules.

Rows.  A batch mixes four classes by row index modulo PERIOD = 7, in the
order of PATTERN:

    full     uniform [-0.5, 0.5) per component
    quiet    the same noise times 2^-17
    zero     exact zeros: A = 0, the result must be exactly 0
    cancel   full-scale, the last sample solved in float64 as
             x[n-1] = -(sum_{i<n-1} h[i] x[i]) / h[n-1] and rounded to float32
             (|h[n-1]| >= 0.25 in every case): |y64| << A, so these rows show
             that the bound scales with A and not with |y|

A wave of the batch kernels holds 64 / G rows, G = 1 ... 16 lanes per row.
PATTERN = full quiet zero cancel full quiet zero has every one of full, quiet
and zero in any 4 consecutive rows (a window of 4 leaves out 3 consecutive
slots of the 7, and the two slots of each of these classes lie 3 apart), so
every wave of every G holds all three; 7 divides no 64 / G, so the classes
move through the lanes from wave to wave.  n = 1 has no cancelling row (there
is nothing to cancel against): its slot is a full-scale row.

Shared by tests/test_dotprod_bound.py (the oracle meets the bound, the route
table is the launch's own, the checker is pinned) and
tests/test_gpu_dotprod_bound.py (every route and grid pass of
lqk_dotprod_batch and the one-vector calls).  No GPU.
"""
import functools
import zlib

import numpy as np

import fir_bound as FB
import oracle_lib as O

TYPES = {"rrrf": O.RRRF, "crcf": O.CRCF, "cccf": O.CCCF}
KINDS = ("rrrf", "crcf", "cccf")
MARGIN = 4.0
PATTERN = ("full", "quiet", "zero", "cancel", "full", "quiet", "zero")
PERIOD = len(PATTERN)
LONG_PATTERN = ("full", "quiet", "zero")   # the one-long-row cases: 3 rows
QUIET = 2.0 ** -17
NRM = 1e-5     # the criterion the older dotprod tests use: max|d| / max|y| over a batch
NVEC = 4099    # no multiple of the 256 / G rows of a block for any G: the last block is part full
RAGGED = 37    # rows past a whole number of grid passes


def vec(t):
    """Samples per 16-byte chunk of k_dot_vec."""
    return 4 if t == "rrrf" else 2


def sample_dtype(t):
    return np.float32 if t == "rrrf" else np.complex64


# ------------------------------------------------------------------ the GPU rows
# (type, n, kernel, G): the route a 16-byte aligned batch call takes
# (liquid_mi355x_dotprod_route).  Vector kernel: work = n / VEC chunks per row
# = 1, 2, 4, 8, 64, 65, 512 walk G = 1, 2, 4, 8, 8 (the last work under gmax =
# 16), 16, 16.
LADDER_VEC = [(t, work * vec(t), "vec", G) for work, G in ((1, 1), (2, 2), (4, 4), (8, 8), (64, 8), (65, 16), (512, 16))
              for t in KINDS]
# scalar kernel: work = n.  rrrf 2, 6 and 130 are even and no multiple of 4
LADDER_SCALAR = ([(t, n, "scalar", G) for n, G in ((1, 1), (3, 2), (7, 4), (33, 8), (129, 16))
                  for t in ("crcf", "cccf")] +
                 [("rrrf", n, "scalar", G) for n, G in ((1, 1), (2, 2), (3, 2), (6, 4), (129, 16), (130, 16))])
# (type, n, bytes off 16-byte alignment, G): vector-eligible lengths that an
# unaligned input pointer sends to the scalar kernel
UNALIGNED = ([(t, n, 8, G) for n, G in ((16, 8), (130, 16)) for t in ("crcf", "cccf")] +
             [("rrrf", n, off, G) for n, G in ((16, 8), (260, 16)) for off in (4, 8, 12)])
# capped grid: each with cap 256 / G + 37 and 2 cap 256 / G + 37 rows (2 and 3 passes)
CAPPED = [("cccf", 2, "vec", 1), ("cccf", 16, "vec", 8), ("cccf", 130, "vec", 16), ("cccf", 7, "scalar", 4),
          ("rrrf", 6, "scalar", 4)]
# one long row: 2^20 + 2 (rrrf: + 4, its chunk is 4 samples) and 2^20 + 3
LONG = ([(t, (1 << 20) + vec(t), "vec", 16) for t in KINDS] + [(t, (1 << 20) + 3, "scalar", 16) for t in KINDS])
# one-vector calls: k_dot_single's 256 lanes hold under one, one, and more than one element each
SINGLE_LENGTHS = (1, 2, 255, 256, 257, 1000, 65539)
SINGLE_ROWS = 3 * PERIOD


def row_id(r):
    return "-".join(str(v) for v in r)


def capped_nvec(cap, G, passes):
    """Rows that make a grid of `cap` blocks walk `passes` times, the last
    pass RAGGED rows long."""
    return (passes - 1) * cap * 256 // G + RAGGED


# ------------------------------------------------------------------ batches
def taps(t, n, r):
    if t == "cccf":
        h = (r.uniform(-0.5, 0.5, n) + 1j * r.uniform(-0.5, 0.5, n)).astype(np.complex64)
    else:
        h = r.uniform(-0.5, 0.5, n).astype(np.float32)
    if n and abs(h[n - 1]) < 0.25:   # the divisor of the cancelling rows: its real part moved out by 0.25
        h[n - 1] += h.dtype.type(0.25 if h[n - 1].real >= 0 else -0.25)
    return h


def row_classes(n, nvec, pattern=PATTERN):
    names = ["full" if (c == "cancel" and n <= 1) else c for c in pattern]
    return np.array(names)[np.arange(nvec) % len(pattern)]


def batch(t, n, nvec, pattern=PATTERN, tag=""):
    """(h, X, classes): X of nvec rows by n samples, float32 / complex64."""
    r = np.random.default_rng(zlib.crc32(("dotprod %s %d %d %s" % (t, n, nvec, tag)).encode()))
    h = taps(t, n, r)
    c = 1 if t == "rrrf" else 2
    X = r.random((nvec, n * c), dtype=np.float32)
    X -= np.float32(0.5)
    X = X.view(sample_dtype(t)) if n else np.zeros((nvec, 0), sample_dtype(t))
    cls = row_classes(n, nvec, pattern)
    if n:
        X[cls == "quiet"] *= np.float32(QUIET)
        X[cls == "zero"] = 0
        k = np.flatnonzero(cls == "cancel")
        wide = np.float64 if t == "rrrf" else np.complex128
        hw = h.astype(np.complex128 if t == "cccf" else np.float64)
        step = max(1, (1 << 21) // n)
        for a in range(0, len(k), step):
            kk = k[a:a + step]
            X[kk, n - 1] = -(X[kk, :n - 1].astype(wide) @ hw[:n - 1]) / hw[n - 1]
    return h, X, cls


def reference(t, h, X):
    """(y64, A) of every row, a slice of rows at a time."""
    nvec, n = X.shape
    wide = np.float64 if t == "rrrf" else np.complex128
    hw = h.astype(np.complex128 if t == "cccf" else np.float64)
    ah = np.abs(hw)
    y64, A = np.zeros(nvec, wide), np.zeros(nvec)
    step = max(1, (1 << 21) // max(n, 1))
    for a in range(0, nvec, step):
        Xw = X[a:a + step].astype(wide)
        y64[a:a + step] = Xw @ hw
        A[a:a + step] = np.abs(Xw) @ ah
    return y64, A


def oracle(t, h, X):
    """The rows through the oracle's serial float32 sum."""
    nvec, n = X.shape
    if n == 0:
        return np.zeros(nvec, sample_dtype(t))
    return O.dotprod_batch(TYPES[t], h, X.reshape(-1))


def normwise(y, ref):
    """The older tests' figure: max|y - ref| / max|ref| over the batch."""
    return float(np.max(np.abs(y.astype(np.complex128) - ref)) / np.max(np.abs(ref)))


class Case:
    def __init__(self, t, n, nvec, pattern=PATTERN, tag=""):
        self.t, self.n, self.nvec, self.period = t, n, nvec, len(pattern)
        self.h, self.X, self.cls = batch(t, n, nvec, pattern, tag)
        self.y64, self.A = reference(t, self.h, self.X)
        self.ref = oracle(t, self.h, self.X)
        for a in (self.h, self.X, self.y64, self.A, self.ref):   # shared among tests: left unchanged
            a.setflags(write=False)
        self.oracle_worst = self.report(self.ref)["worst"]

    def rows(self, name):
        return np.flatnonzero(self.cls == name)

    def report(self, y):
        return FB.report(self.t, self.n, y, self.y64, self.A)

    def check_bound(self, y):
        return FB.check(self.t, self.n, y, self.y64, self.A)

    def check(self, y, what=""):
        """Every row within the bound, then the worst row within MARGIN times
        the oracle's worst."""
        r = self.check_bound(y)
        print("dotprod_bound %s n=%d nvec=%d %s: worst %.4g of the bound, the oracle's worst %.4g"
              % (self.t, self.n, self.nvec, what, r["worst"], self.oracle_worst))
        assert r["worst"] <= MARGIN * self.oracle_worst, (
            "%s n=%d %s: worst error %.4g x the bound at row %d, more than %g x the oracle's %.4g"
            % (self.t, self.n, what, r["worst"], r["index"], MARGIN, self.oracle_worst))
        return r


@functools.lru_cache(maxsize=None)
def case(t, n, nvec=NVEC, pattern=PATTERN, tag=""):
    """Cached: the ladder, alignment and one-vector batches (a few megabytes
    each).  The capped-grid and long-row batches are built by their one test."""
    return Case(t, n, nvec, pattern, tag)


# ------------------------------------------------------------------ mutations
def leak_into_quiet(c, y, gain=2.0 ** -22):
    """(a) each quiet row gains `gain` times the result of the full-scale row
    before it (PATTERN: the row just before a quiet row is full-scale)."""
    z = y.copy()
    q = c.rows("quiet")
    assert np.all(c.cls[q - 1] == "full")
    z[q] += (gain * y[q - 1]).astype(y.dtype)
    return z


def tiny_zero_rows(c, y):
    """(b) each zero row becomes 1e-30."""
    z = y.copy()
    z[c.rows("zero")] = 1e-30
    return z


def drop_quiet_of_last_pass(c, y, first):
    """(c) the quiet rows from row `first` on -- the last, ragged grid pass --
    are left 0."""
    z = y.copy()
    q = c.rows("quiet")
    z[q[q >= first]] = 0
    return z


def _trunc(p, bits):
    """float32 products cut (toward zero) to `bits` explicit mantissa bits."""
    return (np.ascontiguousarray(p, np.float32).view(np.int32) & np.int32(-(1 << (23 - bits)))).view(np.float32)


def truncated_sum(c, bits=16):
    """(d) the serial float32 sum of the oracle with every product cut to
    `bits` mantissa bits before it is added."""
    f = np.float32
    re, im = np.zeros(c.nvec, f), np.zeros(c.nvec, f)
    Xr, Xi = (c.X, None) if c.t == "rrrf" else (c.X.real, c.X.imag)
    for i in range(c.n):
        hr, hi = f(c.h[i].real), f(c.h[i].imag)
        if c.t == "cccf":   # the oracle's order: re += hr xr - hi xi, im += hr xi + hi xr
            re = re + (_trunc(hr * Xr[:, i], bits) - _trunc(hi * Xi[:, i], bits))
            im = im + (_trunc(hr * Xi[:, i], bits) + _trunc(hi * Xr[:, i], bits))
            continue
        re = re + _trunc(hr * Xr[:, i], bits)
        if c.t == "crcf":
            im = im + _trunc(hr * Xi[:, i], bits)
    return re if c.t == "rrrf" else (re + 1j * im).astype(np.complex64)
