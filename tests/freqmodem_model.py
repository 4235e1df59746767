"""numpy model of freqmod and freqdem (src/modem/src/freqmod.c, freqdem.c), the
inputs of tests/golden/freqmodem.json and the bound the demodulator is held to.

freqmod.  ref = float32(kf) * 65536 in float32.  Per sample the float32 product
p = ref * m is rounded half away from zero -- in float64 as
sign(p) floor(|p| + 0.5), which is exact there (np.round rounds halves to even
and is not used) -- converted to a 32-bit integer and reduced modulo 2^16; a
product that is not finite or reaches 2^31 in magnitude adds 0 (the low 16 bits
of the 0x80000000 the x86 conversion yields).  The accumulator is a sum modulo
2^16; the output is table[((phase + 0x20) >> 6) & 0x3ff].  Model.step is the
per-sample loop, Model.block the prefix sum: the tests hold them equal.

freqdem.  ref = float32(1 / (2 pi kf)) with the quotient in float64.  The
float32 product of the conjugated sample M back with the sample is
z32 = (a c + b d, a d - b c), four rounded products; phi = atan2 of z32 in
float64, signed zeros kept; an output m meets the bound when
    |m - ref phi| <= E 2^-23 |ref phi|
and is exactly zero in value where phi is zero.

E.  The reference evaluates atan2f(z32) * ref in float32: atan2f's own error and
two roundings.  Worst ratio against the bound with E = 1:
    the fixture's recorded freqdem outputs (the reference itself)      1.33
    numpy's float32 arctan2 and one float32 multiply, the same inputs  1.71
    the same evaluation on the GPU tests' inputs (dem_input, 2^20
    samples per kf of KFS and M of 1, 2, 3, 64, 127, 128, 1024)         2.26
E = 5 is twice the worst of these, rounded up.  The library's block calls take
the argument in float64 and round it once before the multiply (at most one
unit of the E = 1 bound); tests/test_gpu_freqmodem.py prints their worst ratio
on the MI355X and DESIGN.md records it.
"""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "freqmodem.json")
f32, f64 = np.float32, np.float64

E = 5.0
U23 = 2.0 ** -23
KFS = [0.02, 0.04, 0.08, 0.5, 1.0]
TABLE_LEN = 1024


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def load_fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


# ------------------------------------------------------------------ inputs (integer arithmetic)
def hash32(i, seed):
    """a 32-bit integer mix of the index and the seed, vectorised"""
    M = np.uint64(0xffffffff)
    x = (np.asarray(i, np.uint64) * np.uint64(0x9E3779B1) + np.uint64(seed) * np.uint64(0x85EBCA77)) & M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M
    x ^= x >> np.uint64(16)
    return x


def message(n, seed, scale=1.0):
    """n float32 messages k / 2^23 * scale, k a 24-bit signed integer: [-scale, scale)"""
    k = (hash32(np.arange(n), seed) >> np.uint64(8)).astype(np.int64) - (1 << 23)
    return (k.astype(f64) / 2.0 ** 23 * scale).astype(f32)


def dem_input(n, seed):
    """n complex64 samples: components (v - 32768) / 65536, v 16-bit, times a power of two from
    2^-14 .. 2^14 that changes every 29 samples; every 11th sample is exactly zero, every 13th has
    a zero imaginary part, every 17th a zero real part.  Non-zero magnitudes lie in [2^-30, 2^14]."""
    k = np.arange(n)
    h = hash32(k, seed)
    re = ((h >> np.uint64(16)).astype(np.int64) - 32768).astype(f64) / 65536.0
    im = ((h & np.uint64(0xffff)).astype(np.int64) - 32768).astype(f64) / 65536.0
    scale = np.ldexp(1.0, ((k // 29) * 5) % 29 - 14)
    x = ((re * scale).astype(f32) + 1j * (im * scale).astype(f32)).astype(np.complex64)
    x[k % 11 == 0] = 0
    x.imag[k % 13 == 0] = 0
    x.real[k % 17 == 0] = 0
    return x


def cosines(n):
    """the round-trip message of the reference's autotest: three cosines"""
    i = np.arange(n, dtype=f64)
    return (0.3 * np.cos(2 * math.pi * 0.013 * i) + 0.2 * np.cos(2 * math.pi * 0.021 * i + 0.4)
            + 0.4 * np.cos(2 * math.pi * 0.037 * i + 1.7)).astype(f32)


def halfway_messages():
    """kf = 0.5 (ref = 32768): products exactly k + 0.5, both signs, even and odd k, and 32767.5
    (an increment of 2^15); then runs of 70 equal products whose wrong roundings add up past a
    table entry (64): 0.5 (rintf adds 0), 0.49999997 (x + 0.5f is 1 in float32) and 2^23 + 1
    (x + 0.5f rounds to 2^23 + 2)"""
    k = np.array([0, 1, 2, 3, 4, 7, 100, 101, 32766, 32767, 12344, 12345], f64)
    p = np.concatenate([k + 0.5, -(k + 0.5), [2.0 ** 23 + 3, -(2.0 ** 23 + 1), 0.0, -0.0], np.full(70, 0.5),
                        np.full(70, float(f32(0.49999997))), np.full(70, 2.0 ** 23 + 1)])
    m = (p / 32768.0).astype(f32)
    assert np.array_equal(m.astype(f64) * 32768.0, p) and len(m) <= 256
    return m


def range_messages():
    """kf = 1 (ref = 65536): products at and beyond +-2^31, infinities, a NaN, between in-range ones"""
    return np.array([0.25, 32768.0, 0.125, -32768.0, 1e-3, 40000.0, -40000.0, 0.5, np.inf, -0.3, -np.inf, 0.7,
                     np.nan, 32767.99, -32767.99, 0.1, 3e38, -3e38, 0.0], f32)


def quadrant_samples():
    return np.array([0.75 + 0.5j, -0.75 + 0.5j, -0.75 - 0.5j, 0.75 - 0.5j], np.complex64)


def zero_samples():
    """samples next to exact zeros of either sign, and on the axes"""
    v = [(1, 1), (0, 0), (-1, -1), (0, 0), (-1, 1), (0, -0.0), (1, -1), (-0.0, 0), (-1, 0), (-0.0, -0.0), (0, -1),
         (-1, -0.0), (1, 0), (1, -0.0), (2, 0), (-3, 0), (-3, -0.0), (0, 2), (0, -2), (0, 0), (0, 0), (-0.5, -0.25),
         (-0.0, 0), (-2, -1), (0, -0.0), (-2, 1), (-0.0, -0.0), (2, -1)]
    a = np.zeros(len(v), np.complex64)
    a.real[:] = np.array([z[0] for z in v], f32)   # the parts are stored, not added: signs of zeros kept
    a.imag[:] = np.array([z[1] for z in v], f32)
    return a


def case_list():
    """(name, kind "mod" / "dem", kf, ops): ops are ("b", input) a block call, ("s", input)
    per-sample calls, ("r", None) reset"""
    out = []
    for k, kf in enumerate(KFS):
        m = message(256, 100 + k, 1.0 if kf < 0.5 else 4.0)
        out.append(("mod_kf%g" % kf, "mod", kf, [("b", m[:100]), ("s", m[100:130]), ("b", m[130:])]))
        x = dem_input(256, 200 + k)
        out.append(("dem_kf%g" % kf, "dem", kf, [("b", x[:100]), ("s", x[100:130]), ("b", x[130:])]))
    for kf in (0.02, 0.04, 0.08):
        out.append(("roundtrip_mod_kf%g" % kf, "mod", kf, [("b", cosines(256))]))
    out.append(("halfway", "mod", 0.5, [("b", halfway_messages())]))
    out.append(("range", "mod", 1.0, [("b", range_messages())]))
    q = quadrant_samples()
    out.append(("quadrants", "dem", 0.04, [op for z in q for op in (("r", None), ("s", np.array([z], np.complex64)))]))
    out.append(("zeros", "dem", 0.08, [("b", zero_samples())]))
    return out


def case_inputs(ops):
    xs = [x for _, x in ops if x is not None]
    return np.concatenate(xs) if xs else np.zeros(0, f32)


# ------------------------------------------------------------------ freqmod
def mod_ref(kf):
    return f32(kf) * f32(65536.0)


def table_angles():
    return (2 * math.pi * np.arange(TABLE_LEN, dtype=f64) / TABLE_LEN).astype(f32)


def table64():
    """cos + j sin of the float32 angles, rounded from float64: within a unit of the reference's cexpf"""
    a = table_angles().astype(f64)
    return (np.cos(a).astype(f32) + 1j * np.sin(a).astype(f32)).astype(np.complex64)


def increments(ref, m):
    with np.errstate(over="ignore", invalid="ignore"):
        p = (np.asarray(m, f32) * f32(ref)).astype(f64)
        r = np.where(p < 0, -1.0, 1.0) * np.floor(np.abs(p) + 0.5)
        ok = np.isfinite(r) & (np.abs(r) < 2.0 ** 31)
    return np.where(ok, r, 0.0).astype(np.int64) & 0xffff


def increments_rint(ref, m):
    """a wrong model: halves to even"""
    p = (np.asarray(m, f32) * f32(ref)).astype(f64)
    return np.rint(p).astype(np.int64) & 0xffff


def increments_add_half(ref, m):
    """a wrong model: floorf(x + 0.5f) in float32"""
    p = np.asarray(m, f32) * f32(ref)
    r = np.where(p < 0, -np.floor(-p + f32(0.5)), np.floor(p + f32(0.5)))
    return r.astype(np.int64) & 0xffff


def table_index(phase):
    return ((np.asarray(phase, np.int64) + 0x20) >> 6) & 0x3ff


class ModModel:
    def __init__(self, kf, table, inc=increments):
        self.ref, self.table, self.phase, self.inc = mod_ref(kf), np.asarray(table, np.complex64), 0, inc

    def reset(self):
        self.phase = 0

    def step(self, m):
        """the per-sample loop"""
        out = np.empty(len(m), np.complex64)
        for i, v in enumerate(np.asarray(m, f32)):
            self.phase = (self.phase + int(self.inc(self.ref, np.array([v], f32))[0])) & 0xffff
            out[i] = self.table[int(table_index(self.phase))]
        return out

    def block(self, m):
        """the prefix sum"""
        if len(m) == 0:
            return np.zeros(0, np.complex64)
        ph = (self.phase + np.cumsum(self.inc(self.ref, m))) & 0xffff
        self.phase = int(ph[-1])
        return self.table[table_index(ph)]


def phase_from_probe(table, last, probe):
    """the accumulator from what the interface shows: `last` the output of the sample that left
    the accumulator at P, `probe` the outputs of 64 further samples that each add 1.  The index
    first changes at the c-th of them, so (P + c + 0x20) % 64 == 0."""
    lut = {(int(bits(table.real)[i]), int(bits(table.imag)[i])): i for i in range(TABLE_LEN)}
    idx = lambda z: lut[(int(bits(np.array([z.real], f32))[0]), int(bits(np.array([z.imag], f32))[0]))]  # noqa: E731
    i0 = idx(last)
    c = next(k + 1 for k, z in enumerate(probe) if idx(z) != i0)
    return (((i0 << 6) | ((64 - c) & 0x3f)) - 0x20) & 0xffff


def probe_message(kf):
    """a message whose increment is 1"""
    m = f32(1.0) / mod_ref(kf)
    assert int(increments(mod_ref(kf), np.array([m], f32))[0]) == 1
    return np.full(64, m, f32)


# ------------------------------------------------------------------ freqdem
def dem_ref(kf):
    return f32(1.0 / (2 * math.pi * float(f32(kf))))


def product32(p, r):
    """conj(p) r in float32: four rounded products, a rounded sum and difference"""
    p, r = np.asarray(p, np.complex64), np.asarray(r, np.complex64)
    a, b, c, d = p.real, p.imag, r.real, r.imag
    with np.errstate(all="ignore"):
        return a * c + b * d, a * d - b * c


class DemModel:
    def __init__(self, kf, M=1):
        self.ref, self.M, self.state = dem_ref(kf), M, np.zeros(M, np.complex64)

    def reset(self):
        self.state = np.zeros(self.M, np.complex64)

    def block(self, r):
        """(re, im) of the float32 products for the samples r; the state moves on"""
        r = np.asarray(r, np.complex64)
        ext = np.concatenate([self.state, r])
        self.state = ext[len(ext) - self.M:].copy()
        return product32(ext[:len(r)], r)


def phi64(re, im):
    return np.arctan2(np.asarray(im, f32).astype(f64), np.asarray(re, f32).astype(f64))


def reference32(re, im, ref):
    """the reference's evaluation: float32 atan2, one float32 multiply"""
    return np.arctan2(np.asarray(im, f32), np.asarray(re, f32)).astype(f32) * f32(ref)


def report(m, re, im, ref, e=E):
    """worst |m - ref phi| / (e 2^-23 |ref phi|); inf if an output is not zero where phi is"""
    m = np.asarray(m, f32).astype(f64)
    want = float(ref) * phi64(re, im)
    if not np.all(np.isfinite(m)):
        return math.inf
    z = want == 0
    if np.any(m[z] != 0):
        return math.inf
    return float(np.max(np.abs(m[~z] - want[~z]) / (e * U23 * np.abs(want[~z])))) if (~z).any() else 0.0


def check(what, m, re, im, ref):
    r = report(m, re, im, ref)
    print("freqdem %s: worst %.4g of the bound (%d outputs)" % (what, r, len(np.atleast_1d(m))))
    assert r <= 1.0, "%s: %.4g x the bound" % (what, r)
    return r


# ------------------------------------------------------------------ driving the library
def drive_library(q, kind, ops, blocks=True):
    """the ops of a case on a liquidmi.FreqMod / FreqDem; blocks=False: block ops as per-sample
    loops (the reference's own definition of them), which touch no device"""
    out = []
    for op, x in ops:
        if op == "r":
            q.reset()
        elif op == "b" and blocks:
            out.append(q.modulate_block(x) if kind == "mod" else q.demodulate_block(x))
        elif kind == "mod":
            out.append(np.array([q.modulate(v) for v in x], np.complex64))
        else:
            out.append(np.array([q.demodulate(v) for v in x], f32))
    return np.concatenate(out)


def dem_case_products(kf, ops, M=1):
    """(re, im, ref) of the float32 products over the sample ops of a freqdem case"""
    m, parts = DemModel(kf, M), []
    for op, x in ops:
        if op == "r":
            m.reset()
        else:
            parts.append(m.block(x))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), m.ref
