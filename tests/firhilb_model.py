"""The bar for firhilbf, the float64 model behind it, and the fixture's inputs.

firhilbf (src/filter/src/firhilb.c) keeps two windows w0, w1 of 2m real
samples (zero at create and reset), 2m quadrature taps hq and a toggle:

    decim  call i: w1 <- x[2i], yq = dot(w1); w0 <- x[2i+1], yi = delay(w0); y[i] = yi + j yq
    interp call i: w0 <- Im x[i], y[2i] = delay(w0); w1 <- Re x[i], y[2i+1] = dot(w1)
    r2c    call  : p = toggle; w_p <- x; yi = delay(w_p); yq = dot(w_{1-p}); toggle ^= 1

with delay(w) the sample pushed m pushes before the newest one and
dot(w) = sum_j hq[j] w[j], w oldest first.  All modes share the windows.

The bar, for every output:
  * a delay output equals the delayed input sample bit for bit;
  * a dot output yq meets the direct form's per-output bound (as firfilt's,
    tests/fir_bound.py) with T = 2m real terms:
        |yq - yq64| <= (2m + 8) 2^-23 A,   A = sum_k |hq[k]| |sample under tap k|,
    yq64 from the float64 model below; where A = 0 the output is exactly 0.
A float32 sum of T products in any order errs by at most about T 2^-24 A; the
rounding of the result adds 2^-24 A; (T + 8) 2^-23 covers both with room for
an accumulator that truncates.  The reference alone uses under a tenth of it.

Shared by tests/test_firhilb_model.py (the model reproduces the reference's
recorded outputs: the checker is pinned), tests/test_gpu_firhilb.py (the
kernels) and tests/golden/gen_firhilb.py (which records the fixture).
"""
import json
import os

import numpy as np

EPS = 2.0 ** -23
MODES = ("decim", "interp", "r2c")
CASES = [(2, 60.0), (5, 60.0), (12, 60.0), (17, 80.0)]   # (m, As) of the fixture
CALLS = 300                                               # calls per fixture stream
NIN = {"decim": 2, "interp": 2, "r2c": 1}                 # input floats per call (interp: re, im)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "firhilb.json")


# ------------------------------------------------------------------ inputs
def lcg_uniform(n, seed):
    """n float32 samples uniform in [-0.5, 0.5) on a 2^-16 grid, from integer
    arithmetic alone (x <- 1664525 x + 1013904223 mod 2^32, bits 8..23)."""
    out = np.empty(n, np.float32)
    s = seed & 0xFFFFFFFF
    for k in range(n):
        s = (1664525 * s + 1013904223) & 0xFFFFFFFF
        out[k] = (((s >> 8) & 0xFFFF) - 32768) / 65536.0
    return out


def burst_envelope(n):
    """Level 1 in a few runs, 1e-5 elsewhere, and a stretch of exact zeros;
    positions as fractions of n, so every length has all three."""
    e = np.full(n, 1e-5)
    for a, b in ((0.0, 0.07), (0.22, 0.3), (0.55, 0.552), (0.8, 0.93)):
        e[int(a * n):max(int(b * n), int(a * n) + 1)] = 1.0
    e[int(0.36 * n):int(0.5 * n)] = 0.0
    return e


def shape(u, env):
    """uniform samples times an envelope, rounded once to float32; zeros are
    +0 (the reference's decimator forms yi + j yq in complex arithmetic, which
    turns a delayed -0 into +0: with +0 alone, "bit for bit" holds for it too)"""
    return (u.astype(np.float64) * env + 0.0).astype(np.float32)


def as_input(mode, flat):
    """the flat float32 samples as the mode's input array"""
    return flat.view(np.complex64) if mode == "interp" else flat


def stream_input(m, mode):
    n = CALLS * NIN[mode]
    flat = shape(lcg_uniform(n, 1000 * m + MODES.index(mode)), burst_envelope(n))
    return as_input(mode, flat)


def mixed_ops(m):
    """One object: decim, an odd number of r2c calls, interp, r2c again."""
    plan = (("decim", 40), ("r2c", 2 * m + 3), ("interp", 30), ("r2c", 2 * m + 6))
    n = sum(c * NIN[md] for md, c in plan)
    flat = shape(lcg_uniform(n, 77 * m + 5), burst_envelope(n))
    ops, k = [], 0
    for md, c in plan:
        ops.append((md, as_input(md, flat[k:k + c * NIN[md]])))
        k += c * NIN[md]
    return ops


# ------------------------------------------------------------------ model
class Model:
    """float64 two-window simulator; run() returns per output component
    (value, A, is_dot): value is the delayed sample (delay outputs) or the
    float64 dot product."""

    def __init__(self, m, hq):
        self.m = m
        self.hq = np.asarray(hq, np.float64)
        self.ah = np.abs(self.hq)
        assert len(self.hq) == 2 * m
        self.reset()

    def reset(self):
        self.w = [np.zeros(2 * self.m), np.zeros(2 * self.m)]
        self.toggle = 0

    def _push(self, p, v):
        w = self.w[p]
        w[:-1] = w[1:]
        w[-1] = v

    def _delay(self, p):
        return self.w[p][self.m - 1]

    def _dot(self, p):
        return float(np.dot(self.hq, self.w[p])), float(np.dot(self.ah, np.abs(self.w[p])))

    def run(self, mode, x):
        flat = np.ascontiguousarray(x).view(np.float32).astype(np.float64)
        n = len(flat) // NIN[mode]
        val, A = np.zeros(2 * n), np.zeros(2 * n)
        dot = np.zeros(2 * n, bool)
        for i in range(n):
            if mode == "decim":
                self._push(1, flat[2 * i])
                val[2 * i + 1], A[2 * i + 1] = self._dot(1)
                self._push(0, flat[2 * i + 1])
                val[2 * i] = self._delay(0)
            elif mode == "interp":   # flat: (re, im) pairs
                self._push(0, flat[2 * i + 1])
                val[2 * i] = self._delay(0)
                self._push(1, flat[2 * i])
                val[2 * i + 1], A[2 * i + 1] = self._dot(1)
            else:
                p = self.toggle
                self._push(p, flat[i])
                val[2 * i] = self._delay(p)
                val[2 * i + 1], A[2 * i + 1] = self._dot(1 - p)
                self.toggle ^= 1
            dot[2 * i + 1] = True
        return val, A, dot

    def run_ops(self, ops):
        parts = [self.run(mode, x) for mode, x in ops]
        return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def report(m, hq, ops, y):
    """y: every output of the ops in order, as flat float32 (complex outputs
    as re, im).  Worst dot error as a ratio to the bound and the counts of
    failing outputs."""
    y = np.ascontiguousarray(y).view(np.float32)
    val, A, dot = Model(m, hq).run_ops(ops)
    assert y.shape == val.shape, (y.shape, val.shape)
    delay_bad = ~dot & (y.view(np.uint32) != val.astype(np.float32).view(np.uint32))
    bound = (2 * m + 8) * EPS * A
    finite = np.isfinite(y)
    err = np.abs(np.where(finite, y, 0).astype(np.float64) - val)
    zero = dot & (A == 0)
    dot_bad = dot & np.where(zero, y != 0, ~finite | (err > bound))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(dot & ~zero, err / bound, 0.0)
    worst = int(np.argmax(ratio))
    return {"worst": float(ratio[worst]), "index": worst, "n": int(len(y)),
            "delay_bad": int(np.count_nonzero(delay_bad)), "dot_bad": int(np.count_nonzero(dot_bad)),
            "nonzero_zeros": int(np.count_nonzero(zero & (y != 0))),
            "first_bad": int(np.argmax(delay_bad | dot_bad)) if (delay_bad | dot_bad).any() else -1}


def check(m, hq, ops, y, label=""):
    r = report(m, hq, ops, y)
    print("firhilb %s m=%d: worst dot error %.4g of the bound at output %d; of %d outputs %d delay outputs differ, "
          "%d dot outputs fail (%d must be zero and are not)"
          % (label, m, r["worst"], r["index"], r["n"], r["delay_bad"], r["dot_bad"], r["nonzero_zeros"]))
    assert r["delay_bad"] == 0 and r["dot_bad"] == 0, (
        "%s m=%d: %d delay outputs are not the delayed input bit for bit, %d dot outputs miss the bound (worst %.4g "
        "x the bound at output %d, %d must be zero and are not); first failing output %d"
        % (label, m, r["delay_bad"], r["dot_bad"], r["worst"], r["index"], r["nonzero_zeros"], r["first_bad"]))
    return r


# ------------------------------------------------------------------ fixture
def load_fixture():
    with open(FIXTURE) as f:
        d = json.load(f)
    for c in d["cases"]:
        for k in ("hq",) + MODES + ("mixed",):
            c[k] = np.array(c[k], np.float32)
    return d


def known_answer_ops(d, mode):
    """(ops, expected flat outputs) of one of the reference autotest's vectors"""
    ka = d["known_answers"][mode]
    x = np.array(ka["x"], np.float32)
    return [(mode, as_input(mode, x))], np.array(ka["y"], np.float32)
