"""Models, inputs and the criterion for autocorr (src/filter/src/autocorr.c).

With samples counted from the last reset and zero before it, a window W and a
delay d:

    p[k]   = x[k] conj(x[k-d])           (rrrf: x[k] x[k-d])
    rxx[n] = sum_{k=n-W+1..n} p[k]
    e2[n]  = sum_{k=n-W+1..n} |x[k]|^2

The criterion is the per-output bound of tests/fir_bound.py with W in place of
the tap count: in float64 from the float32 input,

    y64[n] = rxx[n],   A[n] = sum_{k=n-W+1..n} |x[k]| |x[k-d]|,
    T = W (rrrf) or 2 W (cccf),

and an output passes if |rxx[n] - y64[n]| <= (T + 8) 2^-23 A[n], or A[n] == 0
and rxx[n] == 0; every output is finite.  For e2 (and get_energy) A = e2 in
float64.  fir_bound.report does the checking; nothing of it is copied here.

reference64 sums every window directly (sliding_window_view): a difference of
float64 cumulative sums is itself too inaccurate at quiet outputs next to a
burst.  Inputs have components on [-0.5, 0.5) times a level of exactly 0 or at
least 1e-5, so no product underflows.

Three float32 forms of the sum, for tests/test_autocorr_model.py:
  direct32     one serial float32 dot product per output (the reference's order)
  segmented32  prefix and suffix sums inside segments of W products; an output
               is S[n-W+1] + P[n], or P[n] alone when its window is one whole
               segment (the kernel's form, csrc/k_autocorr.hip)
  running32    add the newest product, subtract the oldest: misses the bound
               after the first loud stretch, which pins the checker

The fixture (tests/golden/autocorr.json, written by tests/golden/gen_autocorr.py)
holds the reference's outputs; its inputs are regenerated here from integers
(stream_input), as iirfilt_model does.
"""
import json
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import fir_bound as FB
import firhilb_model as FM

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "autocorr.json")
NOUT = 512   # outputs per fixture stream

# the fixture's streams: (kind, W, d, how the reference was driven)
CASES = [("cccf", 1, 0, "block"), ("cccf", 16, 1, "block"), ("cccf", 64, 32, "block"), ("cccf", 65, 5, "block"),
         ("cccf", 64, 100, "block"), ("cccf", 16, 5, "push"),
         ("rrrf", 1, 1, "block"), ("rrrf", 16, 0, "block"), ("rrrf", 64, 5, "block"), ("rrrf", 65, 100, "block"),
         ("rrrf", 65, 32, "block")]


def is_complex(kind):
    return kind == "cccf"


def sample_dtype(kind):
    return np.complex64 if is_complex(kind) else np.float32


def case_seed(idx):
    return 9000 + 31 * idx


# ------------------------------------------------------------------ inputs
def stream_input(kind, n, seed):
    """n samples: uniform on a 2^-16 grid times the burst envelope (level 1 in
    a few runs, 1e-5 elsewhere, a stretch of exact zeros)"""
    nf = 2 * n if is_complex(kind) else n
    flat = FM.shape(FM.lcg_uniform(nf, seed), FM.burst_envelope(nf))
    return flat.view(np.complex64) if is_complex(kind) else flat


def noise(kind, env, seed):
    """len(env) samples, components uniform in [-0.5, 0.5) times the envelope"""
    r = np.random.default_rng(seed)
    n = len(env)
    if is_complex(kind):
        return ((r.uniform(-0.5, 0.5, n) + 1j * r.uniform(-0.5, 0.5, n)) * env).astype(np.complex64)
    return (r.uniform(-0.5, 0.5, n) * env).astype(np.float32)


def envelope(name, n, seams=()):
    """"burst": 1e-5 with short runs at 1; "gaps": exact zeros with the same
    runs.  Every seam (a tile boundary of the kernel) gets a level change on
    it: a run that ends exactly there, and one that starts 3 samples after the
    next."""
    e = np.full(n, 1e-5 if name == "burst" else 0.0)
    for a, b in ((0, 40), (n // 3, n // 3 + 300), (n - 200, n - 199)):
        e[max(a, 0):max(b, 0)] = 1.0
    for i, s in enumerate(seams):
        if i % 2 == 0:
            e[max(s - 37, 0):s] = 1.0
        else:
            e[s + 3:s + 50] = 1.0
    return e


# ------------------------------------------------------------------ float64 model
def _windows(a, W):
    """rows n: a[n-W+1 .. n], zeros before the start"""
    return sliding_window_view(np.concatenate([np.zeros(W - 1, a.dtype), a]), W)


def reference64(kind, W, d, x):
    """(y64, A, e64): every window summed directly in float64"""
    x = np.ascontiguousarray(x, sample_dtype(kind))
    wide = x.astype(np.complex128 if is_complex(kind) else np.float64)
    xd = np.concatenate([np.zeros(d, wide.dtype), wide])[:len(wide)]
    p = wide * np.conj(xd)
    y64 = _windows(p, W).sum(axis=1)
    A = _windows(np.abs(wide) * np.abs(xd), W).sum(axis=1)
    e64 = _windows(np.abs(wide) ** 2, W).sum(axis=1)
    return y64, A, e64


def report(kind, W, y, y64, A):
    return FB.report(kind, W, np.asarray(y), y64, A)


def report_e2(kind, W, e2, e64):
    """e2 against its own bound: A = e2 in float64 (e2 is real: the complex
    kind's 2 W real terms still set T)"""
    return FB.report(kind, W, np.asarray(e2, np.float32), e64, e64)


def check(label, kind, W, y, y64, A):
    r = report(kind, W, y, y64, A)
    print("autocorr %-40s worst %.4g of the bound at %d, %d of %d fail, %d nonzero zeros, %d non-finite"
          % (label, r["worst"], r["index"], r["failing"], r["n"], r["nonzero_zeros"], r["nonfinite"]))
    assert r["failing"] == 0 and r["nonfinite"] == 0, (
        "%s: worst error %.4g x the bound at output %d; %d of %d outputs fail; %d outputs that must be zero are "
        "not; %d non-finite" % (label, r["worst"], r["index"], r["failing"], r["n"], r["nonzero_zeros"],
                                r["nonfinite"]))
    return r


def check_e2(label, kind, W, e2, e64):
    return check(label + " e2", kind, W, np.asarray(e2, np.float32), e64, e64)


# ------------------------------------------------------------------ float32 forms
def products32(kind, d, x):
    """p[k] in float32, one rounding per operation; complex as (re, im) columns"""
    x = np.ascontiguousarray(x, sample_dtype(kind))
    xd = np.concatenate([np.zeros(d, x.dtype), x])[:len(x)]
    if not is_complex(kind):
        return (x * xd).astype(np.float32)[:, None]
    xr, xi, dr, di = x.real, x.imag, xd.real, xd.imag
    return np.stack([xr * dr + xi * di, xi * dr - xr * di], axis=1).astype(np.float32)


def _pack(kind, s):
    return (s[:, 0] + 1j * s[:, 1]).astype(np.complex64) if is_complex(kind) else s[:, 0].astype(np.float32)


def direct32(kind, W, d, x):
    p = products32(kind, d, x)
    pad = np.concatenate([np.zeros((W - 1, p.shape[1]), np.float32), p])
    acc = np.zeros((len(p), p.shape[1]), np.float32)
    for i in range(W):   # term i of every window, in window order
        acc = (acc + pad[i:i + len(p)]).astype(np.float32)
    return _pack(kind, acc)


def segmented32(kind, W, d, x):
    """segments of W products from W-1 zeros before the stream; float32
    running sums inside each segment from the left (P) and from the right (S)"""
    p = products32(kind, d, x)
    n, nc = p.shape
    nseg = (W - 1 + n + W - 1) // W
    pad = np.zeros((nseg * W, nc), np.float32)
    pad[W - 1:W - 1 + n] = p
    seg = pad.reshape(nseg, W, nc)
    P = np.cumsum(seg, axis=1, dtype=np.float32).reshape(-1, nc)
    S = np.cumsum(seg[:, ::-1], axis=1, dtype=np.float32)[:, ::-1].reshape(-1, nc)
    u = np.arange(n) + W - 1                       # element of output n; its window starts at u - W + 1
    whole = (u + 1) % W == 0
    out = np.where(whole[:, None], P[u], (S[u - W + 1] + P[u]).astype(np.float32))
    return _pack(kind, out)


def running32(kind, W, d, x):
    p = products32(kind, d, x)
    out = np.zeros_like(p)
    acc = np.zeros(p.shape[1], np.float32)
    for k in range(len(p)):
        acc = (acc + p[k]).astype(np.float32)
        if k >= W:
            acc = (acc - p[k - W]).astype(np.float32)
        out[k] = acc
    return _pack(kind, out)


# ------------------------------------------------------------------ fixture
def load_fixture():
    """cases: kind, W, d, drive ("block" / "push"), n, seed, y (the reference's
    outputs), energy (its get_energy after the last sample)"""
    with open(FIXTURE) as f:
        d = json.load(f)
    for c in d["cases"]:
        y = np.array(c["y"], np.float32)
        c["y"] = y.view(np.complex64) if is_complex(c["kind"]) else y
        c["energy"] = np.float32(c["energy"])
    return d


def case_input(c):
    return stream_input(c["kind"], c["n"], c["seed"])


def case_name(c):
    return "%s_W%d_d%d_%s" % (c["kind"], c["W"], c["d"], c["drive"])
