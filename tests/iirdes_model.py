"""The fixture of the recursive filter designs and of iirdecim / iirinterp
(tests/golden/iirdes.json, written by tests/golden/gen_iirdes.py), and the
models the tests compare against.

A rate changer by M is the full-rate filter of iirfilt_model:
  iirdecim   run(x)[::M]           (the output for the first of each M inputs)
  iirinterp  run(stuffed(x, M))    (x[i] followed by M - 1 zeros; no gain)
"""
import functools
import json
import os

import numpy as np

import iirfilt_model as IM

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iirdes.json")
NOUT = IM.NOUT


def cplx(v):
    return np.array(v, np.float32).view(np.complex64)


@functools.lru_cache(maxsize=None)
def load_fixture():
    """designs: name, ftype, btype, format, order, fc, f0, Ap, As, b, a.
    azpk: fn, n, par, z, p, k.  bilinear: za, pa, ka, m, zd, pd, kd.
    stable: name, b, a, stable.  cplxpair: n, tol, pair_tol, z, p.
    streams: name, obj, kind, ctor, M, the constructor's arguments, form,
    b / a (the filter inside, normalised), n (execute_block's count), seed,
    y (the first NOUT outputs)."""
    with open(FIXTURE) as f:
        d = json.load(f)
    for c in d["designs"]:
        c["b"], c["a"] = np.array(c["b"], np.float32), np.array(c["a"], np.float32)
    for c in d["azpk"]:
        c["z"], c["p"], c["k"] = cplx(c["z"]), cplx(c["p"]), complex(cplx(c["k"])[0])
    bl = d["bilinear"]
    for key in ("za", "pa", "zd", "pd"):
        bl[key] = cplx(bl[key])
    bl["ka"], bl["kd"] = complex(cplx(bl["ka"])[0]), complex(cplx(bl["kd"])[0])
    for c in d["stable"]:
        c["b"], c["a"] = np.array(c["b"], np.float32), np.array(c["a"], np.float32)
    for c in d["cplxpair"]:
        c["z"], c["p"] = cplx(c["z"]), cplx(c["p"])
    for c in d["streams"]:
        k = c["kind"]
        for key in ("b", "a", "raw_b", "raw_a"):
            if key in c:
                c[key] = IM._coefs(c[key], k)
        c["y"] = IM._samples(c["y"], k)
    return d


def stream_input(c):
    return IM.stream_input(c["kind"], c["n"] * c["M"] if c["obj"] == "iirdecim" else c["n"], c["seed"])


def stuffed(x, M):
    z = np.zeros(len(x) * M, x.dtype)
    z[::M] = x
    return z


def full_rate(obj, x, M):
    """the full-rate filter's input for the object's input x"""
    return x if obj == "iirdecim" else stuffed(x, M)


def kept(obj, yfull, M):
    """the object's output from the full-rate filter's"""
    return np.ascontiguousarray(yfull[::M]) if obj == "iirdecim" else yfull


def run32_crcf(form, b, a, x):
    """iirfilt_model.run32 for kind crcf with the sign of every zero kept.  run32 puts its result
    together as yr + 1j * yi, which turns an imaginary part of -0 into +0 (0 * 0 + 1 * -0); a stuffed
    stream decays to signed zeros between inputs when M is large, and a comparison bit for bit
    sees that.  With real coefficients the two components never mix and each is the rrrf
    arithmetic, so they are run apart and stored side by side."""
    x = np.ascontiguousarray(x, np.complex64)
    y = np.empty(len(x), np.complex64)
    y.real = IM.run32("rrrf", form, b, a, np.ascontiguousarray(x.real))[0]
    y.imag = IM.run32("rrrf", form, b, a, np.ascontiguousarray(x.imag))[0]
    return y


def response(b, a, form, f):
    """H(e^{j 2 pi f}) in float64, the usual sign: sums of c[i] e^{-j 2 pi f i}"""
    b, a = np.asarray(b, np.float64), np.asarray(a, np.float64)
    f = np.asarray(f, np.float64)

    def poly(c):
        return np.sum(c[None, :] * np.exp(-2j * np.pi * f[:, None] * np.arange(len(c))[None, :]), axis=1)
    if form == "tf":
        return poly(b) / poly(a)
    h = np.ones(len(f), np.complex128)
    for k in range(len(b) // 3):
        h *= poly(b[3 * k:3 * k + 3]) / poly(a[3 * k:3 * k + 3])
    return h
