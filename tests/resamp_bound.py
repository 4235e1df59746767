"""A per-output error bound for the resamplers, and the streams that probe it.

resamp.  The reference resampler emits, for every output k of its float32
timing schedule (b_k, mu_k, i_k) -- bank, fraction, newest input; b = -1
marks the BOUNDARY state -- the blend of two bank outputs, each one float32
dot product over 2m inputs (resamp.c:245-311).  With the banks
h_b[n] = h[b + n npfb], n < 2m, of the prototype as the object builds it
(prototype()), in float64 / complex128:

    y64[k] = (1 - mu) sum_n h_b0[n] x[i0 - n]  +  mu sum_n h_b1[n] x[i_k - n]
    (b0, b1, i0) = (b, b + 1, i_k)            INTERP
                 = (npfb - 1, 0, i_k - 1)     BOUNDARY
    A[k]      = the same expression on the moduli of every factor
    A_fold[k] = sum_n |h_b0[n]| |x[i0 - n]| + |h_b1[n]| |x[i_k - n]|    (no mu weights)
    T = 4m                                    real terms per output component

and an output y[k] passes if

    |y[k] - y64[k]| <= (T + 8) 2^-23 A[k] + fold 2^-23 A_fold[k],
    or A[k] == 0 (then A_fold[k] == 0 too) and y[k] == 0.

Where the bound comes from (u = 2^-24): the two dot products are float32
sums of 2m products each, in any order gamma_2m of their moduli; the blend
multiplies by 1 - mu (rounded) and mu and adds, three more roundings; a
complex output's two components add a factor sqrt(2): together below
0.71 (2m + 3) 2^-23 A, and (4m + 8) 2^-23 A holds it with an accumulator that
truncates.  The oracle is held to fold = 0.

The GPU kernels fold the blend into the coefficient (k_resamp3, k_resamp4:
one dot product over 2m + 1 inputs with c = h_b0 + mu (h_b1 - h_b0), the
difference d = fl(h_b1 - h_b0) taken once per tap pair, c = fma(mu, d, h_b0)
per output).  Per tap, with the exact coefficient c* = (1 - mu) h_b0 + mu h_b1:

    |d - (h_b1 - h_b0)| <= u |h_b1 - h_b0| <= u (|h_b0| + |h_b1|)
    |c - c*| <= u |c*| (1 + u) + mu u (|h_b0| + |h_b1|)

The first part, summed against |x|, is u A and is inside the (T + 8) term
(the folded form has 2m + 1 products where T counts 4m); the second is at
most mu u A_fold <= 0.5 2^-23 A_fold: fold = FOLD = 0.5, from mu <= 1, and
nothing measured.  Where every sample under both windows is zero, A and
A_fold are both exactly zero and so is any sum the kernel can form.

resamp2 (resamp2.c:273-356; oracle.c restates it with two windows w0, w1 of
2m samples and the odd taps h1).  An output that is a pure delay tap -- interp
y[0], synthesizer y[0] (the float32 sum x0 + x1, delayed), the delay half of
filter, decim and analyzer -- involves no arithmetic of the filter, so where
the output is the delay tap alone it must equal its input bit for bit.  A
dot or sum output is held to (T + 8) 2^-23 A with T = 2m real terms per
component (4m for complex taps) and A = |delay term| + sum_j |h1[j]| |w[j]|,
the 0.5 scalings included and the synthesizer's x0 +- x1 entered as
|x0| + |x1|.

Streams.  `burst` (1e-5 between full-level stretches), `gaps` (exact zeros
between them) and `stairs` (decades 1 .. 1e-5 in 400-sample steps).  The
edges of the loud stretches sit on the seams of the kernel a row takes --
wave-tile and workgroup starts (in outputs for k_resamp4, mapped to inputs
through the schedule; in inputs for k_resamp3 and k_resamp), a table entry --
on the seam and one sample either side; one burst ends on the last input
before `cut`, so a call that starts there sees it only through the carried
history; one runs to the end of the stream.

Shared by tests/test_resamp_bound.py (the oracle meets the bound, the models
and the checker are pinned by mutations) and tests/test_gpu_resamp_bound.py
(every kernel and rate class, however the caller cuts the stream).
"""
import functools
import os
import zlib

import numpy as np

import oracle_lib as O

EPS = 2.0 ** -23
FOLD = 0.5          # of 2^-23 A_fold: the folded coefficient (derivation above)
KINDS = ("burst", "gaps", "stairs")


# ------------------------------------------------------------------ resamp
def prototype(m, fc, As, npfb):
    """The taps as the object builds them (resamp.c:117-132): the Kaiser
    design scaled by npfb / sum(h), every step in float32."""
    h = O.firdes_kaiser(2 * m * npfb + 1, np.float32(fc) / np.float32(npfb), As)
    gain = np.float32(0.0)
    for v in h:
        gain = np.float32(gain + v)
    gain = np.float32(npfb) / gain
    return (h * gain).astype(np.float32)


def windows(b, idx, npfb):
    """(b0, b1, i0, i1) per output from the schedule (b = -1: BOUNDARY)."""
    bnd = b < 0
    b0 = np.where(bnd, npfb - 1, b).astype(np.int64)
    b1 = np.where(bnd, 0, b + 1).astype(np.int64)
    i1 = idx.astype(np.int64)
    i0 = np.where(bnd, i1 - 1, i1)
    return b0, b1, i0, i1


def resamp_reference(x, h, m, npfb, mu, win):
    """(y64, A, A_fold) of the outputs whose windows `win` = (b0, b1, i0, i1)
    gives; zero history before x[0].  Taken apart from the schedule so that
    a test can restate a wrong kernel (another bank, another window)."""
    L = 2 * m
    b0, b1, i0, i1 = win
    wide = np.float64 if x.dtype == np.float32 else np.complex128
    xp = np.concatenate([np.zeros(L + 1, wide), x.astype(wide)])
    ap = np.abs(xp)
    hw = h.astype(np.float64)
    mu = mu.astype(np.float64)
    y0, y1 = np.zeros(len(mu), wide), np.zeros(len(mu), wide)
    a0, a1 = np.zeros(len(mu)), np.zeros(len(mu))
    for n in range(L):
        t0, t1 = hw[b0 + n * npfb], hw[b1 + n * npfb]
        y0 += t0 * xp[i0 - n + L + 1]
        y1 += t1 * xp[i1 - n + L + 1]
        a0 += np.abs(t0) * ap[i0 - n + L + 1]
        a1 += np.abs(t1) * ap[i1 - n + L + 1]
    return (1.0 - mu) * y0 + mu * y1, (1.0 - mu) * a0 + mu * a1, a0 + a1


def report(y, y64, A, T, Af=None, fold=0.0):
    """Worst ratio to the bound, its index, the number of failing outputs,
    of outputs that must be zero and are not, and of non-finite outputs."""
    y = np.asarray(y)
    assert y.shape == y64.shape, (y.shape, y64.shape)
    bound = (T + 8) * EPS * A
    if Af is not None and fold:
        bound = bound + fold * EPS * Af
    finite = np.isfinite(y)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(y.astype(y64.dtype) - y64)
    err[~finite] = np.inf
    zero = A == 0
    ok = np.where(zero, y == 0, err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(zero, np.where(y == 0, 0.0, np.inf), err / bound)
    worst = int(np.argmax(ratio)) if len(y) else 0
    return {"worst": float(ratio[worst]) if len(y) else 0.0, "index": worst,
            "failing": int(np.count_nonzero(~ok)), "nonzero_zeros": int(np.count_nonzero(zero & (y != 0))),
            "nonfinite": int(np.count_nonzero(~finite)), "n": int(len(y))}


def excess(y, y64, A, Af, T, fold=FOLD):
    """Worst ratio to (T + 8) 2^-23 A of the error beyond the folded
    coefficient's allowance fold 2^-23 A_fold: what a kernel that folds the
    blend has to keep within a multiple of the oracle's own ratio."""
    err = np.abs(np.asarray(y).astype(y64.dtype) - y64)
    over = np.maximum(err - fold * EPS * Af, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(A == 0, 0.0, over / ((T + 8) * EPS * A))
    return float(ratio.max()) if len(ratio) else 0.0


def check(label, y, y64, A, T, Af=None, fold=0.0):
    r = report(y, y64, A, T, Af, fold)
    print("resamp_bound %s: worst %.4g of the bound at %d, %d of %d fail, %d nonzero zeros, %d non-finite"
          % (label, r["worst"], r["index"], r["failing"], r["n"], r["nonzero_zeros"], r["nonfinite"]))
    assert r["failing"] == 0 and r["nonfinite"] == 0, (
        "%s: worst error %.4g x the bound at output %d; %d of %d outputs fail; %d outputs that must be zero "
        "are not; %d non-finite" % (label, r["worst"], r["index"], r["failing"], r["n"], r["nonzero_zeros"],
                                    r["nonfinite"]))
    return r


def check_stream(label, rate, m, fc, As, npfb, x, y, fold=FOLD):
    """Any stream from a fresh object against the bound (for tests that bring
    their own input): the schedule, the model and check() in one."""
    b, mu, idx = O.resamp_schedule(rate, npfb, len(x))
    y64, A, Af = resamp_reference(x, prototype(m, fc, As, npfb), m, npfb, mu, windows(b, idx, npfb))
    return check(label, y, y64, A, 4 * m, Af, fold)


def nrm_err(y, ref):
    return float(np.linalg.norm(np.asarray(y, np.complex128) - ref) / max(np.linalg.norm(ref), 1e-300))


class Row:
    """One kernel and rate class: the shape, the route the dispatch must take
    and the stream's size.  The tile comes from the library's route query
    (liquid_mi355x_resamp_route, host only: the launch's own decision), so a
    retune that moves a seam moves the stream's edges with it, and one that
    moves the shape to another kernel fails the row's route assertion.
    seam: "out" -- tiles of `tile` outputs, four to a workgroup, a table entry
    every 4th output (k_resamp4); "in" -- tiles of `tile` inputs (k_resamp3:
    tin; k_resamp: 8 x 256; k_resamp_generic: 256)."""

    def __init__(self, name, t, rate, m, npfb, route, n=12000, cut=None, env=None, fc=0.25):
        self.name, self.t, self.rate, self.m, self.npfb = name, t, float(np.float32(rate)), m, npfb
        self.route, self.n, self.fc, self.As = route, n, fc, 60.0
        self.env = {"LQ_RESAMP_INPUT_PLAN": "0", **(env or {})}   # "1": the input plan for every type
        self.seam = "out" if route.startswith("resamp4") else "in"
        self.cut = cut if cut is not None else 5000
        self.T = 4 * m

    def __repr__(self):
        return self.name

    def environ(self):
        """Context: the row's environment switches set (read when a plan is built)."""
        return _Environ(self.env)

    def query(self, nx=None):
        """(kernel/class, tile) of a first call of nx inputs (default: the stream)."""
        import liquidmi as LQ
        with self.environ():
            return LQ.resamp_route(self.t, self.rate, self.m, self.npfb, nx or self.n)

    @functools.cached_property
    def tile(self):
        route, tile = self.query()
        assert route == self.route, (self.name, route, self.route)
        return tile


class _Environ:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# name, type, rate, m, npfb, kernel/class, inputs.  The rates are the
# shapes checked on the CPU first (1.037, 0.3, 3.7, 0.8131, 1.3, 75.5) and
# one per remaining class; streams are sized so a launch at three workgroups
# (twelve waves) still walks several tiles per wave.
ROWS = [
    # k_resamp4, its four rate classes, L = 14 at the constant-stride npfb = 64
    Row("r4-up", "crcf", 1.037, 7, 64, "resamp4/up", n=40000),
    Row("r4-up-r4", "crcf", 3.7, 7, 64, "resamp4/up_r4", n=12000),
    Row("r4-down", "crcf", 0.8131, 7, 64, "resamp4/down", n=50000),
    Row("r4-down-dn", "crcf", 0.3, 7, 64, "resamp4/down_dn", n=60000, cut=20000),
    Row("r4-cccf", "cccf", 1.037, 7, 64, "resamp4/up", n=12000),
    # L = 2, 32 and a run-time stride (npfb = 16, 32, 128)
    Row("r4-L2", "crcf", 1.3, 1, 16, "resamp4/up", n=12000),
    Row("r4-L32", "crcf", 1.3, 16, 16, "resamp4/up", n=12000),
    Row("r4-L8-down", "crcf", 0.8131, 4, 32, "resamp4/down", n=12000),
    Row("r4-npfb128", "crcf", 3.7, 4, 128, "resamp4/up_r4", n=12000),
    # k_resamp3: rrrf, a bank count that is no power of two, the input-plan switch
    Row("r3-rrrf", "rrrf", 1.037, 7, 64, "resamp3/const", n=40000),
    Row("r3-rrrf-down", "rrrf", 0.3, 7, 64, "resamp3/const", n=40000),
    Row("r3-npfb37", "crcf", 0.8131, 3, 37, "resamp3/const", n=12000),
    Row("r3-npfb100", "crcf", 1.3, 5, 100, "resamp3/stride", n=12000),
    Row("r3-env", "crcf", 1.037, 7, 64, "resamp3/const", n=40000, env={"LQ_RESAMP_INPUT_PLAN": "1"}),
    # r <= 1/4 is outside k_resamp4 whatever the type
    Row("r3-slow", "crcf", 0.2, 7, 64, "resamp3/const", n=40000),
    # high rate: tin shrinks below L + 1 = 15
    Row("r3-fast", "rrrf", 30.5, 7, 64, "resamp3/const", n=3000, cut=1000),
    # past r ~ 52 the per-input kernel; past npfb the stream stops
    Row("rs-fast", "rrrf", 57.3, 7, 64, "resamp/", n=9000, cut=3000),
    Row("rs-stops", "rrrf", 75.5, 7, 64, "resamp/", n=9000, cut=3000),
    # L > 32
    Row("generic", "crcf", 1.3, 20, 16, "generic/", n=12000),
]
# every even L the launchers instantiate (2 .. 32) that no row above reaches:
# k_resamp3 on rrrf, k_resamp4 on crcf, 3000 inputs (two tile seams and more)
ROWS += [Row("r3-L%d" % L, "rrrf", 1.3, L // 2, 16, "resamp3/const", n=3000, cut=1500)
         for L in range(2, 34, 2) if L != 14]
ROWS += [Row("r4-L%d" % L, "crcf", 1.3, L // 2, 16, "resamp4/up", n=3000, cut=1500)
         for L in range(4, 32, 2)]      # L = 14 too: the rows above run it at npfb = 64, its own instantiation
ROW = {r.name: r for r in ROWS}
# a call of at least 2^16 inputs builds the periodic plan; at r = 1.5 it
# repeats every 256 outputs, so 2^16 + 5003 inputs wrap it hundreds of times
PERIODIC = Row("r4-periodic", "crcf", 1.5, 7, 64, "resamp4/up", n=(1 << 16) + 5003, cut=0)
# r <= 1/2: a call of one loud input with no output
SILENT = Row("r4-silent-call", "crcf", 0.3, 7, 64, "resamp4/down_dn", n=3000, cut=1500)


def seam_inputs(row, idx, n):
    """Input positions of the row's kernel seams, the wider tiles first."""
    s = []
    if row.seam == "out":
        K = len(idx)
        # workgroup starts, wave-tile starts, the table entry after one, the
        # tile three workgroups (twelve waves) on: at least 512 outputs apart
        for k in (1024, 2048, 256, 1536 + 4, 2816, 3584 + 8, 4 * 3 * 1024):
            if k < K:
                s.append(int(idx[k]))
    else:
        t = row.tile * -(-130 // row.tile)      # small tiles: seams at least 130 inputs apart
        for j in (4, 8, 1, 2, 5, 3 * 4, 4 * 3 * 4):
            if j * t < n - 130:
                s.append(j * t)
    return s


def envelope(row, kind, idx):
    n, cut = row.n, row.cut
    if kind == "stairs":
        step = np.arange(n) // 400 % 10
        return np.array([1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5])[np.minimum(step, 10 - step)]
    e = np.full(n, 1e-5 if kind == "burst" else 0.0)
    s = seam_inputs(row, idx, n)
    # on the seam and one sample either side, as a start and as an end
    shapes = ((-40, 0), (0, 30), (-1, 25), (1, 50), (-30, 1), (-25, -1), (0, 1), (-60, 3), (-3, 60))
    spans = [(0, 30)] if kind == "burst" else []      # gaps: a head of exact zeros
    spans += [(p + a, p + b) for p, (a, b) in zip(s, shapes)]
    if cut:
        spans.append((cut - 60, cut))
    spans.append((n - 45, n))
    for lo, hi in spans:
        e[max(lo, 0):min(max(hi, 0), n)] = 1.0
    return e


class Case:
    def __init__(self, row, kind):
        self.row, self.kind = row, kind
        self.h = prototype(row.m, row.fc, row.As, row.npfb)
        b, mu, idx = O.resamp_schedule(row.rate, row.npfb, row.n)
        self.b, self.mu, self.idx = b, mu, idx
        r = np.random.default_rng(zlib.crc32(("resamp %s %s" % (row.name, kind)).encode()))
        env = envelope(row, kind, idx)
        self.drop = int(np.flatnonzero(env[1:] < env[:-1])[0]) + 1      # the first loud-to-quiet edge
        if row.t == "rrrf":
            self.x = (r.uniform(-0.5, 0.5, row.n) * env).astype(np.float32)
        else:
            self.x = ((r.uniform(-0.5, 0.5, row.n) + 1j * r.uniform(-0.5, 0.5, row.n)) * env).astype(np.complex64)
        self.win = windows(b, idx, row.npfb)
        self.y64, self.A, self.Af = resamp_reference(self.x, self.h, row.m, row.npfb, mu, self.win)
        for a in (self.x, self.y64, self.A, self.Af, self.b, self.mu, self.idx):
            a.setflags(write=False)

    def nout(self, nx):
        """Outputs of the first nx inputs."""
        return int(np.searchsorted(self.idx, nx, side="left"))

    def oracle(self, pieces=None):
        """The oracle's float32 outputs (crcf arithmetic; the real part for
        rrrf, whose taps are real), the stream cut at `pieces`."""
        o = O.Resamp(self.row.rate, self.row.m, self.row.fc, self.row.As, self.row.npfb)
        xs = self.x.astype(np.complex64)
        edges = [0] + list(pieces or []) + [len(xs)]
        y = np.concatenate([o.execute_block(xs[a:b]) for a, b in zip(edges[:-1], edges[1:])])
        return np.ascontiguousarray(y.real) if self.row.t == "rrrf" else y

    def check(self, y, fold=0.0, label=""):
        return check("%s %s %s" % (self.row.name, self.kind, label), y, self.y64, self.A, self.row.T, self.Af, fold)


@functools.lru_cache(maxsize=None)
def case(name, kind):
    row = {PERIODIC.name: PERIODIC, SILENT.name: SILENT}.get(name) or ROW[name]
    return Case(row, kind)


# ------------------------------------------------------------------ resamp2
FILTER, ANALYZER, SYNTHESIZER, DECIM, INTERP = range(5)
MODE_NAMES = ("filter", "analyzer", "synthesizer", "decim", "interp")
NIN = {0: 1, 1: 2, 2: 2, 3: 2, 4: 1}
NOUT = {0: 2, 1: 2, 2: 2, 3: 1, 4: 2}      # filter: (y0, y1) interleaved here


def resamp2_taps(m, f0, As, ctaps):
    """The odd taps h1, read from the oracle bit for bit: in interp mode an
    impulse's dot output is h1[j] times 1 plus exact zeros, newest first."""
    o = O.Resamp2(m, f0, As, ctaps)
    x = np.zeros(2 * m, np.complex64)
    x[0] = 1.0
    y = o.run(INTERP, x)
    return y[1::2][::-1].astype(np.complex64)        # h1[j], window oldest first


def _past(v, L):
    """W[i, j] = v[i - (L - 1) + j]: the window after push i, oldest first."""
    p = np.concatenate([np.zeros(L - 1, v.dtype), v])
    return np.lib.stride_tricks.sliding_window_view(p, L)


def halfband(mode, xw, h1, m):
    """(y64, A) of one INTERP or DECIM stage over the wide stream xw from
    cleared windows; A is formed from |xw|, so a cascade passes a stage's A in
    as xw to carry the moduli through (the modulus filter)."""
    L = 2 * m
    hw, xw = h1.astype(np.complex128), np.asarray(xw, np.complex128)
    if mode == INTERP:
        W = _past(xw, L)
        return (np.stack([W[:, m - 1], W @ hw], 1).ravel(),
                np.stack([np.abs(W[:, m - 1]), np.abs(W) @ np.abs(hw)], 1).ravel())
    assert mode == DECIM
    W, D = _past(xw[0::2], L), _past(xw[1::2], L)
    return D[:, m - 1] + W @ hw, np.abs(D[:, m - 1]) + np.abs(W) @ np.abs(hw)


def resamp2_reference(mode, x, h1, m):
    """(y64, A, exact) of n calls of one mode from cleared windows: exact[k]
    holds the float32 value an output must equal bit for bit (a pure delay
    tap), or NaN where the output is a dot product or a sum."""
    L = 2 * m
    hw = h1.astype(np.complex128)
    x = np.asarray(x, np.complex64)
    xw = x.astype(np.complex128)
    nan = np.complex64(complex(np.nan, np.nan))

    def dot(v):
        W = _past(v, L)
        return W @ hw, np.abs(W) @ np.abs(hw)

    def delay(v):
        return _past(v, L)[:, m - 1]

    if mode == INTERP:
        d, a = dot(xw)
        y64 = np.stack([delay(xw), d], 1).ravel()
        A = np.stack([np.abs(delay(xw)), a], 1).ravel()
        ex = np.stack([delay(x), np.full(len(x), nan)], 1).ravel()
    elif mode == DECIM:
        d, a = dot(xw[0::2])
        y64, A = delay(xw[1::2]) + d, np.abs(delay(xw[1::2])) + a
        ex = np.full(len(y64), nan)
    elif mode == ANALYZER:
        d, a = dot(0.5 * xw[0::2])
        y0 = delay(0.5 * xw[1::2])
        y64 = np.stack([d + y0, d - y0], 1).ravel()
        A = np.stack([a + np.abs(y0)] * 2, 1).ravel()
        ex = np.full(len(y64), nan)
    elif mode == SYNTHESIZER:
        s = (x[0::2] + x[1::2]).astype(np.complex64)                   # the float32 sum, as pushed
        d, _ = dot(xw[0::2] - xw[1::2])
        _, a = dot((np.abs(xw[0::2]) + np.abs(xw[1::2])).astype(np.complex128))
        y64 = np.stack([delay(xw[0::2] + xw[1::2]), d], 1).ravel()
        A = np.stack([delay(np.abs(xw[0::2]) + np.abs(xw[1::2])), a], 1).ravel()
        ex = np.stack([delay(s), np.full(len(s), nan)], 1).ravel()
    elif mode == FILTER:
        # calls alternate the window they push; the dot reads the other one
        n = len(x)
        ev, od = xw[0::2], xw[1::2]
        de, ae = dot(ev)      # w0 after even call 2j
        do, ao = dot(od)      # w1 after odd call 2j + 1
        yi, yq, aq = np.zeros(n, np.complex128), np.zeros(n, np.complex128), np.zeros(n)
        yi[0::2], yi[1::2] = delay(ev), delay(od)
        # even call 2j reads w1 after odd call 2j - 1; odd call 2j + 1 reads w0 after even call 2j
        yq[2::2], aq[2::2] = do[:len(yq[2::2])], ao[:len(yq[2::2])]
        yq[1::2], aq[1::2] = de[:len(od)], ae[:len(od)]
        y64 = np.stack([0.5 * (yi + yq), 0.5 * (yi - yq)], 1).ravel()
        A = np.stack([0.5 * (np.abs(yi) + aq)] * 2, 1).ravel()
        ex = np.full(len(y64), nan)
    else:
        raise ValueError(mode)
    return y64, A, ex.astype(np.complex64)


def resamp2_report(y, y64, A, ex, T):
    """report() plus the delay taps: `inexact` counts outputs that must equal
    their input bit for bit and do not."""
    r = report(y, y64, A, T)
    pure = ~np.isnan(ex.real)
    y = np.asarray(y, np.complex64)
    r["inexact"] = int(np.count_nonzero(pure & ((y.real != ex.real) | (y.imag != ex.imag))))
    return r


# (name, m, f0, complex taps): tiled_b at m <= 16, tiled past it
R2_ROWS = [("m4", 4, 0.0, False), ("m7c", 7, 0.13, True), ("m16", 16, 0.0, False), ("m20", 20, 0.0, False),
           ("m20c", 20, -0.21, True)]
R2_TILE = 1024       # calls per tile of k_resamp2_tiled / _tiled_b


class Case2:
    def __init__(self, name, mode, kind, t="crcf"):
        _, m, f0, ctaps = next(r for r in R2_ROWS if r[0] == name)
        self.name, self.mode, self.kind, self.m, self.f0, self.ctaps, self.t = name, mode, kind, m, f0, ctaps, t
        self.ncalls, self.cut = 3 * R2_TILE + 77, R2_TILE + 300
        self.h1 = resamp2_taps(m, f0, 60.0, ctaps)
        per = NIN[mode]
        n = self.ncalls * per
        if kind == "stairs":
            step = np.arange(n) // 400 % 10
            env = np.array([1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5])[np.minimum(step, 10 - step)]
        else:
            env = np.full(n, 1e-5 if kind == "burst" else 0.0)
            t1, t2 = R2_TILE * per, 2 * R2_TILE * per
            spans = [(t1 - 40, t1), (t1 + 1, t1 + 20), (t2 - 30, t2 + 1), (t2 + per * 100 - 1, t2 + per * 100 + 30),
                     (self.cut * per - 50, self.cut * per), (n - 33, n)]
            if kind == "burst":
                spans.append((0, 30))
            for lo, hi in spans:
                env[max(lo, 0):min(hi, n)] = 1.0
        r = np.random.default_rng(zlib.crc32(("resamp2 %s %d %s %s" % (name, mode, kind, t)).encode()))
        if t == "rrrf":
            self.x = (r.uniform(-0.5, 0.5, n) * env).astype(np.float32)
        else:
            self.x = ((r.uniform(-0.5, 0.5, n) + 1j * r.uniform(-0.5, 0.5, n)) * env).astype(np.complex64)
        self.T = 4 * m if ctaps else 2 * m
        self.y64, self.A, self.ex = resamp2_reference(mode, self.x, self.h1, m)
        for a in (self.x, self.y64, self.A, self.ex):
            a.setflags(write=False)

    def oracle(self):
        y = O.Resamp2(self.m, self.f0, 60.0, self.ctaps).run(self.mode, self.x.astype(np.complex64))
        if self.mode == FILTER:
            y = np.stack(y, 1).ravel()
        return y

    @functools.cached_property
    def r_oracle(self):
        """The oracle's worst ratio to the bound (its real part for rrrf)."""
        y = self.oracle()
        return self.report(np.ascontiguousarray(y.real) if self.t == "rrrf" else y)["worst"]

    def report(self, y):
        """y: the outputs, filter mode's (y0, y1) interleaved."""
        return resamp2_report(y, self.y64, self.A, self.ex, self.T)

    def check(self, y, label=""):
        r = self.report(y)
        tag = "resamp2 %s %s %s %s %s" % (self.name, MODE_NAMES[self.mode], self.t, self.kind, label)
        print("resamp_bound %s: worst %.4g of the bound at %d, %d of %d fail, %d nonzero zeros, %d delay taps "
              "inexact" % (tag, r["worst"], r["index"], r["failing"], r["n"], r["nonzero_zeros"], r["inexact"]))
        assert r["failing"] == 0 and r["nonfinite"] == 0 and r["inexact"] == 0, (tag, r)
        return r


@functools.lru_cache(maxsize=None)
def case2(name, mode, kind, t="crcf"):
    return Case2(name, mode, kind, t)


# ------------------------------------------------------------------ msresamp2, msresamp
# The same float64 stages cascaded.  A stage's error is its own rounding,
# (T_s + 8) 2^-23 of its own A, plus the error of its input passed through
# its modulus filter; to first order the sum is (sum_s T_s + 8) 2^-23 of the
# A carried through every stage's modulus filter.  The bound is first order
# (eight roundings of slack are counted once, not per stage), so it is held
# by measurement: the oracle must stay under it (test_resamp_bound.py) -- if
# it does not, the model is wrong, not the constant.
def stage_m(fc, As):
    """msresamp2.c:137-150 in float32: the stage's semi-length from the Kaiser
    length estimate, as the oracle and the library design it."""
    ft = np.float32((np.float32(0.5) - np.float32(fc)) / np.float32(2.0))
    hl = int(np.float32(np.float32(As) - np.float32(7.95)) / np.float32(np.float32(14.26) * ft))
    return max(3, int(np.ceil(np.float32(hl - 1) / np.float32(4.0))))


def ms2_stages(ns, fc, As):
    """[(m, h1)] for stages 0 .. ns - 1 (real taps, f0 = 0)."""
    out, fc = [], np.float32(min(fc, 0.45))
    for _ in range(ns):
        fc = np.float32(0.5) * fc
        m = stage_m(fc, As)
        out.append((m, resamp2_taps(m, 0.0, As, False)))
    return out


def ms2_reference(typ, stages, xw, aw):
    """(y64, A, T) of the half-band cascade over the wide stream xw with
    moduli aw: interpolating (typ 0) applies stage ns - 1 first, decimating
    stage 0 first and scales by 1 / 2^ns."""
    T = 0
    order = stages[::-1] if typ == 0 else stages
    for m, h1 in order:
        mode = INTERP if typ == 0 else DECIM
        if mode == DECIM:
            xw, aw = xw[:len(xw) // 2 * 2], aw[:len(aw) // 2 * 2]
        xw, _ = halfband(mode, xw, h1, m)
        _, aw = halfband(mode, aw, h1, m)
        T += 2 * m
    if typ == 1:
        z = 1.0 / (1 << len(stages))
        xw, aw = xw * z, aw * z
    return xw, aw, T


def ms_split(rate):
    """msresamp.c:68-110 in float32: (type, stages, arbitrary rate)."""
    ra, ns = np.float32(rate), 0
    typ = 0 if ra > 1 else 1
    while (ra > 2) if typ == 0 else (ra < 0.5):
        ns += 1
        ra = ra * np.float32(0.5 if typ == 0 else 2.0)
    return typ, ns, float(ra)


class MsCase:
    """msresamp at `rate`, As = 60 unless given: resamp (m = 7, fc = 0.4, 64
    banks) then the interpolating half-bands, or the decimating half-bands
    then resamp."""

    def __init__(self, t, rate, kind, n, cut, seam_out=None, As=60.0):
        self.t, self.rate, self.kind, self.n, self.cut, self.As = t, float(np.float32(rate)), kind, n, cut, As
        self.typ, self.ns, self.ra = ms_split(self.rate)
        self.M = 1 << self.ns
        self.stages = ms2_stages(self.ns, 0.4, self.As)
        nrs = n if self.typ == 0 else n // self.M           # inputs of the arbitrary resampler
        b, mu, idx = O.resamp_schedule(self.ra, 64, nrs)
        self.idx = idx
        if kind == "stairs":
            step = np.arange(n) // 400 % 10
            env = np.array([1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5])[np.minimum(step, 10 - step)]
        else:
            env = np.full(n, 1e-5 if kind == "burst" else 0.0)
            # seams: the resampler's tiles, seam_out resampler outputs each (the
            # fused launch: 256 less the stage's halo), mapped to chain inputs
            so = seam_out or 256
            pos = [int(idx[k]) * (1 if self.typ == 0 else self.M) for k in (so, 4 * so, 8 * so, 13 * so) if k < len(idx)]
            spans = [(p + a, p + c) for p, (a, c) in zip(pos, ((-40, 0), (0, 30), (-1, 25), (1, 50)))]
            spans += [(cut - 60, cut), (n - 45, n)] + ([(0, 30)] if kind == "burst" else [])
            for lo, hi in spans:
                env[max(lo, 0):min(max(hi, 0), n)] = 1.0
        seed = "msresamp %s %g %s" % (t, rate, kind) + ("" if As == 60.0 else " %g" % As)
        r = np.random.default_rng(zlib.crc32(seed.encode()))
        if t == "rrrf":
            self.x = (r.uniform(-0.5, 0.5, n) * env).astype(np.float32)
        else:
            self.x = ((r.uniform(-0.5, 0.5, n) + 1j * r.uniform(-0.5, 0.5, n)) * env).astype(np.complex64)
        h = prototype(7, 0.4, self.As, 64)
        win = windows(b, idx, 64)
        xw, aw = self.x.astype(np.complex128), np.abs(self.x.astype(np.complex128)).astype(np.complex128)
        if self.typ == 0:
            y, _, _ = resamp_reference(xw, h, 7, 64, mu, win)
            a = _abs_taps_resamp(aw, h, mu, win)
            self.y64, A, T2 = ms2_reference(0, self.stages, y, a.astype(np.complex128))
        else:
            u, ua, T2 = ms2_reference(1, self.stages, xw[:nrs * self.M], aw[:nrs * self.M])
            self.y64, _, _ = resamp_reference(u, h, 7, 64, mu, win)
            A = _abs_taps_resamp(ua, h, mu, win)
        self.A = np.abs(A)
        self.T = 4 * 7 + T2
        for arr in (self.x, self.y64, self.A):
            arr.setflags(write=False)

    def oracle(self, pieces=None):
        o = O.MsResamp(self.rate, self.As)
        xs = self.x.astype(np.complex64)
        edges = [0] + list(pieces or []) + [len(xs)]
        y = np.concatenate([o.execute(xs[a:b]) for a, b in zip(edges[:-1], edges[1:])])
        return np.ascontiguousarray(y.real) if self.t == "rrrf" else y

    def report(self, y):
        y = np.asarray(y)
        return report(y.astype(np.complex64), self.y64, self.A, self.T)

    def check(self, y, label=""):
        return check("msresamp %s r=%g %s %s" % (self.t, self.rate, self.kind, label), np.asarray(y).astype(np.complex64),
                     self.y64, self.A, self.T)

    @functools.cached_property
    def r_oracle(self):
        return self.report(self.oracle())["worst"]


def _abs_taps_resamp(aw, h, mu, win):
    """The resampler's A for an input of moduli aw: the blend of the two
    banks' sums of |h| |x|."""
    return resamp_reference(np.abs(aw).astype(np.complex128), np.abs(h), 7, 64, mu, win)[1]


# (type, rate, inputs, cut, fused stage m): the fused chain (1 < r_a < 2, one
# half-band stage, crcf); the same rate unfused (rrrf); two and three stages
# (the first fused, the later ones on their own); no stage at all; the
# decimating chain, its cuts off the groups of M so a partial group is pending
# between calls
MS_ROWS = [("crcf", 2.6, 12000, 5000, 6), ("rrrf", 2.6, 12000, 5000, 0), ("cccf", 5.3, 8000, 3000, 5),
           ("crcf", 10.4, 6000, 2500, 4), ("crcf", 1.3, 12000, 5000, 0), ("crcf", 0.19, 40001, 15003, 0),
           ("rrrf", 0.09, 40003, 15001, 0)]


# (As, fused stage m): the semi-lengths of the fused stage (3 .. 12) that
# neither MS_ROWS (4, 5, 6) nor test_gpu_parity.py's interpolating chain (3, 4,
# 6, 8) reaches, each by its stop-band attenuation at r = 2.6 (one stage,
# fc = 0.2); crcf, 3000 inputs: 3900 resampler outputs, 16 tiles and more
MS_HB_ROWS = [(68.0, 7), (85.0, 9), (94.0, 10), (102.0, 11), (110.0, 12)]
MS_HB_RATE, MS_HB_N, MS_HB_CUT = 2.6, 3000, 1500


def ms_query(t, rate, n, As=60.0):
    import liquidmi as LQ
    with _Environ({"LQ_RESAMP_INPUT_PLAN": "0"}):
        return LQ.msresamp_route(t, float(np.float32(rate)), As, n)


@functools.lru_cache(maxsize=None)
def mscase(t, rate, kind):
    """The row's case, its seams every `tile` resampler outputs or inputs as
    the library's route query gives them."""
    _, _, n, cut, _ = next(r for r in MS_ROWS if r[:2] == (t, rate))
    route, tile, hm = ms_query(t, rate, n)
    return MsCase(t, rate, kind, n, cut, tile if route.startswith("resamp4") else None)


@functools.lru_cache(maxsize=None)
def mshbcase(As, kind):
    """The MS_HB_ROWS case at stop-band attenuation As."""
    route, tile, hm = ms_query("crcf", MS_HB_RATE, MS_HB_N, As)
    return MsCase("crcf", MS_HB_RATE, kind, MS_HB_N, MS_HB_CUT, tile, As)


class Ms2Case:
    """msresamp2 alone: ns half-band stages, fc = 0.4, As = 60; n calls."""

    def __init__(self, t, typ, ns, kind, ncalls=2 * R2_TILE + 77, cut=R2_TILE + 300):
        self.t, self.typ, self.ns, self.kind, self.ncalls, self.cut, self.M = t, typ, ns, kind, ncalls, cut, 1 << ns
        self.stages = ms2_stages(ns, 0.4, 60.0)
        per = 1 if typ == 0 else self.M
        n = ncalls * per
        if kind == "stairs":
            step = np.arange(n) // 400 % 10
            env = np.array([1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5])[np.minimum(step, 10 - step)]
        else:
            env = np.full(n, 1e-5 if kind == "burst" else 0.0)
            t1 = R2_TILE * per          # the last stage's tile of 1024 calls, in chain inputs
            for lo, hi in ((t1 - 40, t1), (t1 + 1, t1 + 20), (t1 // 2 - 30, t1 // 2 + 1), (cut * per - 50, cut * per),
                           (n - 33, n)) + (((0, 30),) if kind == "burst" else ()):
                env[max(lo, 0):min(hi, n)] = 1.0
        r = np.random.default_rng(zlib.crc32(("msresamp2 %s %d %d %s" % (t, typ, ns, kind)).encode()))
        if t == "rrrf":
            self.x = (r.uniform(-0.5, 0.5, n) * env).astype(np.float32)
        else:
            self.x = ((r.uniform(-0.5, 0.5, n) + 1j * r.uniform(-0.5, 0.5, n)) * env).astype(np.complex64)
        xw = self.x.astype(np.complex128)
        self.y64, A, self.T = ms2_reference(typ, self.stages, xw, np.abs(xw).astype(np.complex128))
        self.A = np.abs(A)
        for arr in (self.x, self.y64, self.A):
            arr.setflags(write=False)

    def oracle(self):
        y = O.MsResamp2(self.typ, self.ns, 0.4, 0.0, 60.0).execute_block(self.x.astype(np.complex64))
        return np.ascontiguousarray(y.real) if self.t == "rrrf" else y

    def report(self, y):
        return report(np.asarray(y).astype(np.complex64), self.y64, self.A, self.T)

    def check(self, y, label=""):
        return check("msresamp2 %s typ %d ns %d %s %s" % (self.t, self.typ, self.ns, self.kind, label),
                     np.asarray(y).astype(np.complex64), self.y64, self.A, self.T)

    @functools.cached_property
    def r_oracle(self):
        return self.report(self.oracle())["worst"]


@functools.lru_cache(maxsize=None)
def ms2case(t, typ, ns, kind):
    return Ms2Case(t, typ, ns, kind)
