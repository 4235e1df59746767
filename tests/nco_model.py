"""nco_crcf in numpy: the reference's float32 phase walk and table index with
every rounding explicit, the float32 mixing arithmetic, the float64 reference
output and the per-output bound (tests/test_nco_model.py, tests/test_gpu_nco.py,
tests/golden/gen_nco.py).

Arithmetic restated from src/nco/src/nco.c:
  step    theta = f32(theta + d_theta); then ONE wrap: compared against the
          double pi, theta = f32(double(theta) -+ 2 pi)
  index   ((unsigned)(f32(f32(f32(theta * 40.743665f) + 512) + 0.5))) & 0xff
  table   tab[i] = sinf(a_i), a_i = f32(2 pi i / 256); cosine = tab[(i + 64) & 0xff]
  mix     y = x (c +- j s): two rounded products and a rounded sum per component

An op sequence drives an object.  Ops are (name, argument) pairs; float
arguments travel as uint32 bit patterns:
  F set_frequency   f adjust_frequency   P set_phase   p adjust_phase
  B pll_set_bandwidth   L pll_step   R reset   S step (count)
  U / D  mix_block_up / _down of (count) samples
  u / d  (count) times mix_up / mix_down of one sample, then step
  m      one mix_up, no step        c  cexpf        g  get_phase, get_frequency
Every U, D, u, d, m output is two recorded floats per sample, c and g two floats.
The samples come from stream_input (integer arithmetic only), consumed in order.
"""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "nco.json")
NCO, VCO = 0, 1
f32 = np.float32
E = 5.0                      # the bound: E 2^-24 (|Re x| + |Im x|) per output component
U24 = 2.0 ** -24
PI = math.pi
KIDX, C512, CHALF = f32(40.743665), f32(512.0), f32(0.5)
LONG_D = [0.1, -0.7, 3.0, 1e-3, 2.5]
LONG_STEPS = 200000


def bits(v):
    return int(np.array(v, f32).view(np.uint32))


def unbits(b):
    return np.array(b, np.uint32).view(f32)[()]


def load_fixture():
    return json.load(open(FIXTURE))


# ------------------------------------------------------------------ phase
def constrain(th):
    if float(th) > PI:
        return f32(float(th) - 2 * PI)
    if float(th) < -PI:
        return f32(float(th) + 2 * PI)
    return th


def step(th, d):
    return constrain(f32(th + d))


def walk(theta0, d, n):
    """the phases before samples 0 .. n-1, and the phase after them"""
    th, d = f32(theta0), f32(d)
    out = np.empty(n, f32)
    for i in range(n):
        out[i] = th
        th = step(th, d)
    return out, th


def walk64(theta0, d, n):
    """the same walk with a float64 accumulator wrapped the same way (a wrong model)"""
    th, d = float(f32(theta0)), float(f32(d))
    out = np.empty(n, np.float64)
    for i in range(n):
        out[i] = th
        th += d
        if th > PI:
            th -= 2 * PI
        elif th < -PI:
            th += 2 * PI
    return out


def cycle(theta0, d, limit=1 << 24):
    """(pre-period, period) of the walk from theta0, by Brent's algorithm on the bit patterns"""
    th0, d = f32(theta0), f32(d)
    power = lam = 1
    tort, hare = th0, step(th0, d)
    n = 0
    while bits(tort) != bits(hare):
        if power == lam:
            tort, power, lam = hare, power * 2, 0
        hare = step(hare, d)
        lam += 1
        n += 1
        assert n < limit
    lead = th0
    for _ in range(lam):
        lead = step(lead, d)
    tail, mu = th0, 0
    while bits(tail) != bits(lead):
        tail, lead, mu = step(tail, d), step(lead, d), mu + 1
    return mu, lam


def index(th):
    """the table index of float32 phases (array or scalar), three rounded operations"""
    th = np.asarray(th, f32)
    t = ((th * KIDX).astype(f32) + C512).astype(f32)
    return ((t + CHALF).astype(f32)).astype(np.int64) & 0xff


def index_contracted(th):
    """theta * K + 512 as one fused operation (what a compiler's contraction makes of it)"""
    th = np.asarray(th, f32)
    t = (th.astype(np.float64) * float(KIDX) + 512.0).astype(f32)   # the product is exact in float64
    return ((t + CHALF).astype(f32)).astype(np.int64) & 0xff


def table_angles():
    return np.array([2.0 * PI * i / 256.0 for i in range(256)]).astype(f32)


def table_phases():
    """phases whose table index is i, i = 0 .. 255 (reading the table through set_phase / sin)"""
    return np.array([2.0 * PI * (i if i <= 128 else i - 256) / 256.0 for i in range(256)]).astype(f32)


# ------------------------------------------------------------------ rotator and mixing
def rotator32(typ, th, table):
    th = np.asarray(th, f32)
    if typ == NCO:
        k = index(th)
        return np.asarray(table, f32)[(k + 64) & 0xff], np.asarray(table, f32)[k]
    return np.cos(th.astype(np.float64)).astype(f32), np.sin(th.astype(np.float64)).astype(f32)


def rotator64(typ, th, idx=None):
    """float64 (cos, sin): of the float32 phase itself (VCO), of the table's float32 angle (NCO)"""
    th = np.asarray(th, f32)
    if typ == NCO:
        k = index(th) if idx is None else np.asarray(idx)
        a = table_angles().astype(np.float64)
        return np.sin(a[(k + 64) & 0xff]), np.sin(a[k])
    return np.cos(th.astype(np.float64)), np.sin(th.astype(np.float64))


def mix32(x, c, s, down):
    x = np.asarray(x, np.complex64)
    a, b = x.real.astype(f32), x.imag.astype(f32)
    c, s = np.asarray(c, f32), np.asarray(s, f32)
    s = -s if down else s
    y = np.empty(x.shape, np.complex64)
    y.real = ((a * c).astype(f32) - (b * s).astype(f32)).astype(f32)
    y.imag = ((a * s).astype(f32) + (b * c).astype(f32)).astype(f32)
    return y


def mix64(x, c64, s64, down):
    return np.asarray(x, np.complex64).astype(np.complex128) * (c64 + (-1j if down else 1j) * s64)


def report(y, y64, x):
    """worst |error| / bound over the components (inf if a zero-bound output is not zero)"""
    y, x = np.asarray(y, np.complex64).astype(np.complex128), np.asarray(x, np.complex64)
    A = np.abs(x.real.astype(np.float64)) + np.abs(x.imag.astype(np.float64))
    err = np.maximum(np.abs(y.real - y64.real), np.abs(y.imag - y64.imag))
    if not np.all(np.isfinite(err)):
        return math.inf
    if np.any(err[A == 0] != 0):
        return math.inf
    nz = A > 0
    return float(np.max(err[nz] / (E * U24 * A[nz]))) if nz.any() else 0.0


def check(what, y, y64, x):
    r = report(y, y64, x)
    print("nco %s: worst %.4g of the bound (%d outputs)" % (what, r, len(np.atleast_1d(x))))
    assert r <= 1.0, "%s: %.4g x the bound" % (what, r)
    return r


# ------------------------------------------------------------------ inputs
def stream_input(n, seed):
    """n complex samples from a 32-bit LCG: 16-bit values v, float32((v - 32768) / 65536) per
    component, times a power of two from 2^-20 .. 2^20 that changes every 37 samples; every 11th
    sample is exactly zero, every 13th has a zero imaginary part"""
    s = int(seed)
    v = np.empty(2 * n, np.int64)
    for i in range(2 * n):
        s = (s * 1664525 + 1013904223) & 0xffffffff
        v[i] = s >> 16
    u = ((v - 32768).astype(np.float64) / 65536.0).astype(f32)
    k = np.arange(n)
    scale = np.ldexp(1.0, ((k // 37) * 7) % 41 - 20).astype(f32)
    x = (u[0::2] * scale + 1j * (u[1::2] * scale)).astype(np.complex64)
    x[k % 11 == 0] = 0
    x.imag[k % 13 == 0] = 0
    return x


def unwrap_input(n=48):
    """a wrapped ramp with a bend: integer arithmetic, then float32"""
    k = np.arange(n)
    ph = (k * 37 + (k * k * 5) // 7) % 200
    return ((ph.astype(np.float64) - 100.0) * (PI / 100.0)).astype(f32)


# ------------------------------------------------------------------ the object
class Model:
    def __init__(self, typ, table):
        self.typ, self.table = typ, np.asarray(table, f32)
        self.alpha = f32(0.1)
        self.beta = np.sqrt(self.alpha)
        self.theta = self.d = f32(0)

    def sincos(self):
        c, s = rotator32(self.typ, self.theta, self.table)
        return s[()], c[()]

    def pll_step(self, dphi):
        self.d = f32(self.d + f32(f32(dphi) * self.alpha))
        self.theta = constrain(f32(self.theta + f32(f32(dphi) * self.beta)))

    def run(self, ops, x):
        """returns (recorded float32 values, mix records): a record is (first sample, count,
        phases, down) of one block or per-sample op, for the float64 reference"""
        out, recs, k = [], [], 0
        for name, arg in ops:
            if name in "FfPpBL":
                v = unbits(arg)
            if name == "F":
                self.d = v
            elif name == "f":
                self.d = f32(self.d + v)
            elif name == "P":
                self.theta = constrain(v)
            elif name == "p":
                self.theta = constrain(f32(self.theta + v))
            elif name == "B":
                self.alpha, self.beta = v, np.sqrt(v)
            elif name == "L":
                self.pll_step(v)
            elif name == "R":
                self.theta = self.d = f32(0)
            elif name == "S":
                self.theta = walk(self.theta, self.d, arg)[1]
            elif name in "UDud":
                th, self.theta = walk(self.theta, self.d, arg)
                c, s = rotator32(self.typ, th, self.table)
                y = mix32(x[k:k + arg], c, s, name in "Dd")
                out.append(y.view(f32))
                recs.append((k, arg, th, name in "Dd"))
                k += arg
            elif name == "m":
                c, s = rotator32(self.typ, self.theta, self.table)
                out.append(mix32(x[k:k + 1], c, s, False).view(f32))
                recs.append((k, 1, np.array([self.theta], f32), False))
                k += 1
            elif name == "c":
                s, c = self.sincos()
                out.append(np.array([c, s], f32))
            elif name == "g":
                out.append(np.array([self.theta, self.d], f32))
            else:
                raise ValueError(name)
        return (np.concatenate(out) if out else np.zeros(0, f32)), recs


def drive_library(q, ops, x, blocks=True):
    """the op sequence on a liquidmi.NCO; blocks=False: U / D as per-sample loops (no GPU).
    Returns the recorded float32 values."""
    out, k = [], 0
    for name, arg in ops:
        v = unbits(arg) if name in "FfPpBL" else None
        if name == "F":
            q.set_frequency(v)
        elif name == "f":
            q.adjust_frequency(v)
        elif name == "P":
            q.set_phase(v)
        elif name == "p":
            q.adjust_phase(v)
        elif name == "B":
            q.pll_set_bandwidth(v)
        elif name == "L":
            q.pll_step(v)
        elif name == "R":
            q.reset()
        elif name == "S":
            for _ in range(arg):
                q.step()
        elif name in "UD" and blocks:
            y = (q.mix_block_down if name == "D" else q.mix_block_up)(x[k:k + arg])
            out.append(y.view(f32))
            k += arg
        elif name in "UDud":
            y = np.empty(arg, np.complex64)
            for j in range(arg):
                y[j] = (q.mix_down if name in "Dd" else q.mix_up)(x[k + j])
                q.step()
            out.append(y.view(f32))
            k += arg
        elif name == "m":
            out.append(np.array([q.mix_up(x[k])], np.complex64).view(f32))
            k += 1
        elif name == "c":
            out.append(np.array([q.cexpf()], np.complex64).view(f32))
        elif name == "g":
            out.append(np.array([q.get_phase(), q.get_frequency()], f32))
        else:
            raise ValueError(name)
    return np.concatenate(out) if out else np.zeros(0, f32)


def state_values(ops, vals):
    """the g values (phase, frequency pairs) among the recorded values"""
    out, k = [], 0
    for name, arg in ops:
        n = 2 * arg if name in "UDud" else 2 if name in "mcg" else 0
        if name == "g":
            out.append(np.asarray(vals[k:k + 2], f32))
        k += n
    return np.concatenate(out) if out else np.zeros(0, f32)


def samples_of(ops):
    return sum(a if n in "UDud" else 1 for n, a in ops if n in "UDudm")


def reference64(typ, recs, x):
    """float64 outputs of the mix records, concatenated, with the matching inputs"""
    ys, xs = [], []
    for k, n, th, down in recs:
        c64, s64 = rotator64(typ, th)
        ys.append(mix64(x[k:k + n], c64, s64, down))
        xs.append(x[k:k + n])
    return np.concatenate(ys), np.concatenate(xs)


def mix_outputs(ops, vals):
    """the complex mix outputs among the recorded values of an op sequence"""
    ys, k = [], 0
    for name, arg in ops:
        if name in "UDud":
            ys.append(np.asarray(vals[k:k + 2 * arg], f32).view(np.complex64))
            k += 2 * arg
        elif name == "m":
            ys.append(np.asarray(vals[k:k + 2], f32).view(np.complex64))
            k += 2
        elif name in "cg":
            k += 2
    return np.concatenate(ys) if ys else np.zeros(0, np.complex64)


# ------------------------------------------------------------------ the recorded cases
def _b(v):
    return bits(f32(v))


PI32 = f32(PI)


def pll_ops(typ, table, n=200):
    """the reference's pll autotest as an op sequence: an oscillator chases a fixed tone; the
    phase errors are computed here once (any sequence of them is a valid scenario) and fed as L ops"""
    tx = Model(typ, table)
    rx = Model(typ, table)
    tx.theta, tx.d = f32(0.8), f32(0.2)
    ops = [("B", _b(0.05)), ("P", _b(0.0)), ("F", _b(0.19))]
    rx.alpha, rx.beta = f32(0.05), np.sqrt(f32(0.05))
    rx.d = f32(0.19)
    for _ in range(n):
        st, ct = tx.sincos()
        sr, cr = rx.sincos()
        dphi = f32(np.angle(complex(ct, st) * complex(cr, -sr)))
        ops += [("L", _b(dphi)), ("S", 1), ("g", 0)]
        rx.pll_step(dphi)
        rx.theta = step(rx.theta, rx.d)
        tx.theta = step(tx.theta, tx.d)
    return ops


def case_ops(table):
    """[(name, type, ops)]: every case has at most 4096 samples"""
    changes = [("P", _b(0.3)), ("F", _b(-0.7)), ("U", 333), ("F", _b(3.0)), ("D", 100), ("p", _b(1.0)), ("U", 64),
               ("L", _b(0.2)), ("U", 65), ("S", 3), ("u", 1), ("m", 0), ("R", 0), ("F", _b(1e-3)), ("U", 130),
               ("f", _b(0.25)), ("D", 63), ("g", 0)]
    edges = [("P", _b(0.3)), ("F", bits(PI32)), ("U", 100), ("F", bits(-PI32)), ("D", 100), ("F", _b(0.0)), ("U", 20),
             ("P", bits(PI32)), ("F", _b(2.5)), ("U", 50), ("g", 0)]
    single = [("F", _b(0.25)), ("P", _b(-2.0)), ("u", 80), ("c", 0), ("d", 80), ("c", 0), ("g", 0)]
    phase = [op for phi in np.linspace(-6.2, 6.2, 63) for op in (("P", _b(phi)), ("c", 0), ("g", 0))]
    freq = [("F", _b(0.37)), ("P", _b(0.1))] + [op for _ in range(64) for op in (("c", 0), ("S", 1))] + [("g", 0)]
    cases = []
    for typ, tn in ((NCO, "nco"), (VCO, "vco")):
        cases += [("tone-" + tn, typ, [("F", _b(0.1)), ("U", 300), ("D", 200), ("g", 0)]),
                  ("changes-" + tn, typ, changes), ("edges-" + tn, typ, edges), ("single-" + tn, typ, single),
                  ("phase-" + tn, typ, phase), ("frequency-" + tn, typ, freq), ("pll-" + tn, typ, pll_ops(typ, table))]
    return cases


def case_seed(idx):
    return 1234 + 97 * idx
