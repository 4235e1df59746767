"""Models and inputs for iirfilt (src/filter/src/iirfilt.c, iirfiltsos.c).

A filter is (kind, form, b, a) with normalised coefficients (a[0] = 1 done):
  form "norm"  direct form II over n = max(nb, na) states,
                 v[i] <- v[i-1];  v[0] = x - sum_{i>=1} a[i] v[i];  y = sum_i b[i] v[i]
  form "sos"   a cascade of sections, 3 coefficients each in b and a,
                 v2 <- v1 <- v0;  v0 = x - a1 v1 - a2 v2;  y = b0 v0 + b1 v1 + b2 v2
kind "rrrf" (real samples, real coefficients), "crcf" (complex, real) or
"cccf" (complex, complex).

run32   the reference's arithmetic: float32, its statement order, one rounding
        per operation (numpy float32 scalars; complex values as separate real
        and imaginary parts, a complex product as (ac - bd, ad + bc)).
run64   scipy.signal.lfilter per section in float64 on the same float32
        coefficients: what the outputs are compared against.

The criterion of tests/test_gpu_iirfilt.py: with e(y) = max|y - y64| / max|y64|
over a span, a GPU result passes when e(y_gpu) <= 4 e(y_ref) + 2^-22, y_ref
the reference's float32 result (the fixture's where the stream is a fixture
stream, else run32's).

Inputs are not stored in the fixture (tests/golden/iirfilt.json, written by
tests/golden/gen_iirfilt.py): stream_input regenerates them from the integer
arithmetic of firhilb_model.
"""
import json
import os

import numpy as np

import firhilb_model as FM

F = np.float32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iirfilt.json")
FACTOR, FLOOR = 4.0, 2.0 ** -22
NOUT = 512   # outputs per fixture stream


def is_complex(kind):
    return kind != "rrrf"


def sample_dtype(kind):
    return np.complex64 if is_complex(kind) else np.float32


def coef_dtype(kind):
    return np.complex64 if kind == "cccf" else np.float32


# ------------------------------------------------------------------ inputs
def stream_input(kind, n, seed):
    """n samples of the kind: uniform on a 2^-16 grid times the burst envelope"""
    nf = 2 * n if is_complex(kind) else n
    flat = FM.shape(FM.lcg_uniform(nf, seed), FM.burst_envelope(nf))
    return flat.view(np.complex64) if is_complex(kind) else flat


def noise_input(kind, n, seed, level=None):
    """as stream_input without the envelope (level: per-sample scale), from a
    vectorised form of the same generator"""
    nf = 2 * n if is_complex(kind) else n
    # s_k of x <- a x + c mod 2^32 by blocks: s_{k+B} = A_B s_k + C_B
    a, c, m = 1664525, 1013904223, 1 << 32
    B = 1 << 12
    blk = np.empty(B, np.uint64)
    s = seed & 0xFFFFFFFF
    for k in range(B):
        s = (a * s + c) % m
        blk[k] = s
    AB, CB = pow(a, B, m), 0
    for _ in range(B):
        CB = (a * CB + c) % m
    out = np.empty(((nf + B - 1) // B) * B, np.uint64)
    cur = blk
    for j in range(0, len(out), B):
        out[j:j + B] = cur
        cur = (cur * np.uint64(AB) + np.uint64(CB)) % np.uint64(m)
    u = (((out[:nf] >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.float64) - 32768.0) / 65536.0
    env = np.ones(nf) if level is None else (np.repeat(level, 2) if is_complex(kind) else np.asarray(level))
    flat = FM.shape(u.astype(np.float32), env)
    return flat.view(np.complex64) if is_complex(kind) else flat


# ------------------------------------------------------------------ float32 model
def _parts(a):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return [F(v) for v in a.real], [F(v) for v in a.imag]
    return [F(v) for v in a], None


def run32(kind, form, b, a, x, state=None):
    """-> (y, state).  state: the reference's v arrays ([n] values for norm,
    [v0, v1, v2] per section for sos), as (re, im) lists; None = zero."""
    x = np.ascontiguousarray(x, sample_dtype(kind))
    cx = is_complex(kind)
    cc = kind == "cccf"
    br, bi = _parts(np.asarray(b, coef_dtype(kind)))
    ar, ai = _parts(np.asarray(a, coef_dtype(kind)))
    xr = [F(v) for v in (x.real if cx else x)]
    xi = [F(v) for v in x.imag] if cx else None
    Z = F(0)
    yr, yi = [Z] * len(x), [Z] * len(x)
    if form == "norm":
        nb, na = len(br), len(ar)
        n = max(nb, na)
        vr, vi = state if state is not None else ([Z] * n, [Z] * n)
        vr, vi = list(vr), list(vi)
        for t in range(len(x)):
            vr[1:] = vr[:-1]
            v0r = xr[t]
            if not cx:
                for i in range(1, na):
                    v0r = v0r - ar[i] * vr[i]
                vr[0] = v0r
                y0 = Z
                for i in range(nb):
                    y0 = y0 + br[i] * vr[i]
                yr[t] = y0
                continue
            vi[1:] = vi[:-1]
            v0i = xi[t]
            for i in range(1, na):
                if cc:
                    v0r, v0i = v0r - (ar[i] * vr[i] - ai[i] * vi[i]), v0i - (ar[i] * vi[i] + ai[i] * vr[i])
                else:
                    v0r, v0i = v0r - ar[i] * vr[i], v0i - ar[i] * vi[i]
            vr[0], vi[0] = v0r, v0i
            y0r = y0i = Z
            for i in range(nb):
                if cc:
                    y0r, y0i = y0r + (br[i] * vr[i] - bi[i] * vi[i]), y0i + (br[i] * vi[i] + bi[i] * vr[i])
                else:
                    y0r, y0i = y0r + br[i] * vr[i], y0i + br[i] * vi[i]
            yr[t], yi[t] = y0r, y0i
        st = (vr, vi)
    else:
        ns = len(br) // 3
        vr, vi = state if state is not None else ([Z] * (3 * ns), [Z] * (3 * ns))
        vr, vi = list(vr), list(vi)
        for t in range(len(x)):
            tr = xr[t]
            ti = xi[t] if cx else Z
            for k in range(ns):
                o = 3 * k
                vr[o + 2], vr[o + 1] = vr[o + 1], vr[o]
                if not cx:
                    vr[o] = tr - ar[o + 1] * vr[o + 1] - ar[o + 2] * vr[o + 2]
                    tr = br[o] * vr[o] + br[o + 1] * vr[o + 1] + br[o + 2] * vr[o + 2]
                    continue
                vi[o + 2], vi[o + 1] = vi[o + 1], vi[o]
                if cc:
                    def mul(kr, ki, sr, si):
                        return kr * sr - ki * si, kr * si + ki * sr
                    p1r, p1i = mul(ar[o + 1], ai[o + 1], vr[o + 1], vi[o + 1])
                    p2r, p2i = mul(ar[o + 2], ai[o + 2], vr[o + 2], vi[o + 2])
                    vr[o], vi[o] = tr - p1r - p2r, ti - p1i - p2i
                    q0r, q0i = mul(br[o], bi[o], vr[o], vi[o])
                    q1r, q1i = mul(br[o + 1], bi[o + 1], vr[o + 1], vi[o + 1])
                    q2r, q2i = mul(br[o + 2], bi[o + 2], vr[o + 2], vi[o + 2])
                    tr, ti = q0r + q1r + q2r, q0i + q1i + q2i
                else:
                    vr[o] = tr - ar[o + 1] * vr[o + 1] - ar[o + 2] * vr[o + 2]
                    vi[o] = ti - ar[o + 1] * vi[o + 1] - ar[o + 2] * vi[o + 2]
                    tr = br[o] * vr[o] + br[o + 1] * vr[o + 1] + br[o + 2] * vr[o + 2]
                    ti = br[o] * vi[o] + br[o + 1] * vi[o + 1] + br[o + 2] * vi[o + 2]
            yr[t], yi[t] = tr, ti
        st = (vr, vi)
    with np.errstate(all="ignore"):
        y = np.array(yr, np.float32)
        if cx:
            y = (y + 1j * np.array(yi, np.float32)).astype(np.complex64)
    return y, st


# ------------------------------------------------------------------ float64 model
def run64(kind, form, b, a, x):
    from scipy.signal import lfilter
    wide = np.complex128 if is_complex(kind) else np.float64
    b = np.asarray(b, coef_dtype(kind)).astype(np.complex128 if kind == "cccf" else np.float64)
    a = np.asarray(a, coef_dtype(kind)).astype(b.dtype)
    y = np.ascontiguousarray(x, sample_dtype(kind)).astype(wide)
    if form == "norm":
        return lfilter(b, a, y)
    for k in range(len(b) // 3):
        y = lfilter(b[3 * k:3 * k + 3], a[3 * k:3 * k + 3], y)
    return y


# ------------------------------------------------------------------ criterion
def err(y, y64, span=slice(None)):
    d = np.max(np.abs(np.asarray(y)[span].astype(y64.dtype) - y64[span]))
    s = np.max(np.abs(y64[span]))
    return float(d / s) if s > 0 else (0.0 if d == 0 else float("inf"))


def criterion(label, y_gpu, y_ref, y64, span=slice(None)):
    """prints the figures, returns (e_gpu, e_ref, ok)"""
    e_gpu, e_ref = err(y_gpu, y64, span), err(y_ref, y64, span)
    ok = bool(np.all(np.isfinite(np.asarray(y_gpu)[span]))) and e_gpu <= FACTOR * e_ref + FLOOR
    print("iirfilt %-44s e_gpu %.3e  e_ref %.3e  e_gpu/e_ref %6.2f  bound %.3e  %s"
          % (label, e_gpu, e_ref, e_gpu / e_ref if e_ref > 0 else float("inf") if e_gpu > 0 else 0.0,
             FACTOR * e_ref + FLOOR, "ok" if ok else "MISS"))
    return e_gpu, e_ref, ok


# ------------------------------------------------------------------ fixture
def _coefs(c, kind):
    c = np.array(c, np.float32)
    return c.view(np.complex64) if kind == "cccf" else c


def _samples(c, kind):
    c = np.array(c, np.float32)
    return c.view(np.complex64) if is_complex(kind) else c


def load_fixture():
    """cases: name, kind, form, ctor (constructor name), args (its arguments;
    coefficient arrays as raw_b / raw_a), b / a (normalised, for the models),
    n, seed, y.  vectors: the reference's autotest vectors (name, kind, b, a
    as given, bn / an normalised, x, y, tol).  helpers: recorded results of
    the design helpers."""
    with open(FIXTURE) as f:
        d = json.load(f)
    for c in d["cases"]:
        k = c["kind"]
        for key in ("b", "a", "raw_b", "raw_a"):
            if key in c:
                c[key] = _coefs(c[key], k)
        c["y"] = _samples(c["y"], k)
    for v in d["vectors"]:
        k = v["kind"]
        for key in ("b", "a", "bn", "an"):
            v[key] = _coefs(v[key], k)
        for key in ("x", "y"):
            v[key] = _samples(v[key], k)
    return d


def case_input(c):
    return stream_input(c["kind"], c["n"], c["seed"])
