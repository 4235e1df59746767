"""Models, inputs and the criterion for detector_cccf
(src/framing/src/detector_cccf.c).

A sequence s of n samples, a threshold and dphi_max give a bank of
m = max(2, ceil(|dphi_max / step|)) templates, step = 0.8 pi / n,
dphi[k] = (k - (m-1)/2) step, p_k[i] = conj(s[i]) exp(-j dphi[k] i).  With
samples counted from the last reset and zero before it, w_t = x[t-n+1 .. t]:

    c_k[t] = sum_i p_k[i] w_t[i]      E[t] = sum_i |w_t[i]|^2
    r_k[t] = |c_k[t]| / sqrt(n E[t])  (0 where E[t] = 0)

and the state machine of detector_cccf_correlate runs over the rows r[t]
(StateMachine below, line for line).

The criterion, per output, in float64 from the float32 input and the float64
templates (T = 2n as tests/fir_bound.py takes for cccf):

    |r - r64| <= 2^-23 (2n + 12) A_k[t] / sqrt(n E[t]) + 2^-23 (n/2 + 8) r64
    A_k[t] = sum_i |p_k[i]| |w_t[i]|

The first term is fir_bound's bound on c_k (its constant 8, plus 4 for the
float32 templates: each differs from the float64 formula by at most 2 ulp per
component) divided by the normaliser; the second covers the normaliser: E is a
sum of 2n squares (relative error (2n + 2) 2^-24 at most, halved by the square
root), the product with n, two square roots, the magnitude and the division.
By Cauchy-Schwarz A_k / sqrt(n E) <= |s|_2 / sqrt(n) whatever the signal level,
so the bound does not grow at quiet samples.  Where E[t] = 0 the output is
exactly 0; every output is finite.  Nonzero samples of every stream made here
are no quieter than 2^-17, so squares stay normal and the bound carries no
underflow term.

Estimates.  tau_hat = N / (2 D), N = rp - rm, D = rp + rm - 2 r0, and dphi_hat
= dphi[d] - step N' / (2 D') likewise in the frequency direction, are held to
the first-order propagation sum |d/dr| delta_r of the row bound from the
float64 rows.
gamma_hat = sqrt(E / n) is held to (n/2 + 8) 2^-24 relative.

Decision margin: a condition on the inputs.  Every comparison the state
machine makes on a stream handed out here -- r[imax] against the threshold in
SEEK, against the previous maximum in FINDMAX -- is decided in float64 by at
least max(5e-3, 64 x the bound of the values compared).  Then the reference,
the host path and the kernel cannot disagree about an index.  check_margin
asserts it; the fixture generator refuses a case that fails it.

Marked samples (the records the kernel hands to the host pass,
csrc/k_detector.hip): those whose row maximum exceeds the threshold, their
neighbours, and the first and last sample of every call.  marked() computes the set; StateMachine.run with
poison= replaces every other row by NaN, and the detections must not change:
an unmarked row decides nothing and is read by no estimate.

Inputs come from integer arithmetic alone: an LFSR gives the +-1 sequence at
two samples per symbol (as the reference's autotest builds its sequence), a
32-bit LCG gives the noise on a 12-bit grid offset by half a step, so that no
component is zero.

The fixture (tests/golden/detector.json, written by tests/golden/gen_detector.py)
holds the reference's detections; the inputs are regenerated here.
"""
import json
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detector.json")
EPS = 2.0 ** -23
QUIET = 2.0 ** -17
MARGIN_MIN = 5e-3
MARGIN_BOUNDS = 64

# the reference autotest's lengths (threshold 0.3, carrier 0.01, dphi_max 0.02 there)
AUTOTEST_N = (64, 83, 128, 167, 256, 335, 512, 671, 1024, 1341)


def threshold_for(n):
    """thresholds of the shapes the margin figures were taken at"""
    return 0.5 if n <= 65 else (0.4 if n < 256 else 0.3)


# ------------------------------------------------------------------ inputs
_LFSR_TAPS = {2: (2, 1), 3: (3, 2), 4: (4, 3), 5: (5, 3), 6: (6, 5), 7: (7, 6), 8: (8, 6, 5, 4), 9: (9, 5),
              10: (10, 7), 11: (11, 9)}


def lfsr_bits(nbits, count):
    st = [1] * nbits
    out = []
    for _ in range(count):
        b = 0
        for t in _LFSR_TAPS[nbits]:
            b ^= st[t - 1]
        out.append(st[-1])
        st = [b] + st[:-1]
    return np.array(out, np.int64)


def sequence(n):
    """n samples of an LFSR +-1 sequence at two samples per symbol"""
    n2 = max((n + 1) // 2, 1)
    nbits = min(max(int(np.ceil(np.log2(n2 + 1))), 2), 11)
    bits = lfsr_bits(nbits, n2)
    return np.repeat(2.0 * bits - 1.0, 2)[:n].astype(np.complex64)


def lcg_words(count, seed):
    out = np.empty(count, np.int64)
    s = seed & 0xFFFFFFFF
    for k in range(count):
        s = (1664525 * s + 1013904223) & 0xFFFFFFFF
        out[k] = s
    return out


def noise(N, seed, scale=0.25):
    """N complex samples, components uniform on a 12-bit grid offset by half a
    step (never zero: |component| >= scale 2^-13), standard deviation
    scale / sqrt(6) per sample (0.102 at the default)"""
    w = lcg_words(2 * N, seed)
    v = (((w >> 12) & 0xFFF) - 2047.5) / 4096.0 * scale
    return (v[0::2] + 1j * v[1::2]).astype(np.complex64)


def unit_noise(N, seed):
    """N complex samples with both components in +-[0.75, 1.25): for the
    envelope streams, whose level then bounds every sample from below"""
    w = lcg_words(2 * N, seed)
    mag = 0.75 + ((w >> 12) & 0xFFF) / 8192.0
    v = np.where((w >> 30) & 1, -mag, mag)
    return (v[0::2] + 1j * v[1::2]).astype(np.complex64)


def stream(s, N, positions, seed, amp=1.0, dphi=0.01, sigma_scale=0.25):
    """noise plus the sequence at each position, with a carrier offset"""
    n = len(s)
    x = noise(N, seed, sigma_scale).astype(np.complex128)
    rot = np.exp(1j * dphi * np.arange(n))
    for p in positions:
        x[p:p + n] += (amp * s.astype(np.complex128) * rot)[:max(min(n, N - p), 0)]
    x = x.astype(np.complex64)
    assert_not_quiet(x)
    return x


def assert_not_quiet(x):
    a = np.abs(np.asarray(x).astype(np.complex128))
    assert np.all((a == 0) | (a >= QUIET)), "a nonzero sample quieter than 2^-17"


def envelope_stream(name, N, seed, seams, n):
    """"burst": level 1 on each seam over 2^-17 elsewhere; "gaps": the same
    bursts over exact zeros, every zero stretch at least n long, a loud
    stretch immediately before a gap"""
    e = np.full(N, QUIET if name == "burst" else 0.0)
    for sm in seams:
        e[max(sm - 19, 0):sm + 23] = 1.0
    e[:7] = 1.0
    if name == "gaps":
        # bursts closer than n would leave a zero stretch shorter than n: join them
        idx = np.flatnonzero(e)
        for a, b in zip(idx[:-1], idx[1:]):
            if 1 < b - a <= n:
                e[a:b] = 1.0
    x = (unit_noise(N, seed).astype(np.complex128) * e).astype(np.complex64)
    assert_not_quiet(x)
    return x


# ------------------------------------------------------------------ the bank
class Bank:
    """m, dphi (float32, as the library forms them) and the float64 templates"""

    def __init__(self, s, dphi_max):
        self.s = np.ascontiguousarray(s, np.complex64)
        n = self.n = len(self.s)
        self.step = step_of(n)
        self.m = num_correlators(n, dphi_max)
        k = np.arange(self.m, dtype=np.float32)
        self.dphi = ((k - np.float32(self.m - 1) / np.float32(2)) * self.step).astype(np.float32)
        # the reference forms the phase dphi[k] * i in float32
        ph = (self.dphi[:, None] * np.arange(n, dtype=np.float32)[None, :]).astype(np.float32).astype(np.float64)
        self.P = np.conj(self.s.astype(np.complex128))[None, :] * np.exp(-1j * ph)


def step_of(n):
    """0.8f * M_PI / (float)n as C evaluates it: the float32 constant 0.8f in
    double arithmetic, rounded once"""
    return np.float32(float(np.float32(0.8)) * np.pi / n)


def num_correlators(n, dphi_max):
    step = step_of(n)
    m = int(np.ceil(np.abs(np.float32(dphi_max) / step)))
    return max(m, 2)


# ------------------------------------------------------------------ float64 rows and the bound
def _padded(x, n, dtype):
    return np.concatenate([np.zeros(n - 1, dtype), np.asarray(x).astype(dtype)])


def rows64(bank, x, chunk=1024):
    """(r64, E64, bound): N x m, N, N x m"""
    n, m = bank.n, bank.m
    xp = _padded(x, n, np.complex128)
    N = len(x)
    r = np.zeros((N, m))
    bound = np.zeros((N, m))
    E = np.zeros(N)
    PT, AP = bank.P.T.copy(), np.abs(bank.P).T.copy()
    for a in range(0, N, chunk):
        b = min(a + chunk, N)
        W = sliding_window_view(xp[a:b + n - 1], n)
        c = W @ PT
        aw = np.abs(W)
        A = aw @ AP
        e = (aw * aw).sum(axis=1)
        E[a:b] = e
        den = np.sqrt(n * e)
        ok = e > 0
        r[a:b][ok] = np.abs(c[ok]) / den[ok, None]
        bound[a:b][ok] = EPS * (2 * n + 12) * A[ok] / den[ok, None] + EPS * (n / 2 + 8) * r[a:b][ok]
    return r, E, bound


def report(r, r64, E64, bound):
    r = np.asarray(r, np.float64)
    err = np.abs(r - r64)
    zero = (E64 == 0)[:, None] & np.ones_like(r64, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, 0.0)
    ratio[~np.isfinite(r)] = np.inf
    return {"worst": float(ratio.max()) if ratio.size else 0.0, "failing": int((ratio > 1).sum()),
            "nonzero_zeros": int((zero & (r != 0)).sum()), "nonfinite": int((~np.isfinite(r)).sum()), "n": r.size}


def check_rows(label, r, r64, E64, bound, serial_worst=None):
    rp = report(r, r64, E64, bound)
    print("detector %-44s worst %.4g of the bound, %d of %d fail, %d nonzero zeros, %d non-finite%s"
          % (label, rp["worst"], rp["failing"], rp["n"], rp["nonzero_zeros"], rp["nonfinite"],
             "" if serial_worst is None else ", serial model %.4g" % serial_worst))
    assert rp["failing"] == 0 and rp["nonzero_zeros"] == 0 and rp["nonfinite"] == 0, (label, rp)
    if serial_worst is not None:
        assert rp["worst"] <= 4 * serial_worst, "%s: %.4g of the bound, more than 4 x the serial model's %.4g" % (
            label, rp["worst"], serial_worst)
    return rp


# ------------------------------------------------------------------ float32 forms
def _f32(a):
    return np.asarray(a, np.float32)


def serial32(bank, x, energy="window"):
    """One float32 accumulator per output and correlator, taps in order, one
    rounding per operation.  energy "window": the sum of each window's own
    squares (the library); "running": the reference's accumulator (add the
    newest, subtract the oldest, :337-352) and its cabsf n_inv / sqrtf form."""
    n, m = bank.n, bank.m
    N = len(x)
    P = bank.P.astype(np.complex64)
    pr, pi = P.real.copy(), P.imag.copy()
    xp = _padded(x, n, np.complex64)
    xr, xi = xp.real.copy(), xp.imag.copy()
    cr = np.zeros((N, m), np.float32)
    ci = np.zeros((N, m), np.float32)
    E = np.zeros(N, np.float32)
    for i in range(n):
        wr, wi = xr[i:i + N, None], xi[i:i + N, None]
        cr = (cr + (pr[None, :, i] * wr - pi[None, :, i] * wi)).astype(np.float32)
        ci = (ci + (pr[None, :, i] * wi + pi[None, :, i] * wr)).astype(np.float32)
        if energy == "window":
            E = (E + (wr[:, 0] * wr[:, 0] + wi[:, 0] * wi[:, 0])).astype(np.float32)
    mag = np.sqrt((cr * cr + ci * ci).astype(np.float32)).astype(np.float32)
    if energy == "window":
        den = np.sqrt(np.float32(n) * E).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(E[:, None] > 0, mag / den[:, None], np.float32(0)).astype(np.float32)
        return r, E
    x2 = (x.real.astype(np.float32) ** 2 + x.imag.astype(np.float32) ** 2).astype(np.float32)
    n_inv = np.float32(1.0) / np.float32(n)
    acc = np.float32(0)
    hat = np.zeros(N, np.float32)
    for t in range(N):
        acc = np.float32(np.float32(acc + x2[t]) - (x2[t - n] if t >= n else np.float32(0)))
        hat[t] = acc * n_inv
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (mag * n_inv / np.sqrt(hat).astype(np.float32)[:, None]).astype(np.float32)
    return r, (hat * np.float32(n)).astype(np.float32)


# ------------------------------------------------------------------ the state machine
SEEK, FINDMAX = 0, 1


class StateMachine:
    """detector_cccf_correlate (:247-330) over given rows.  dtype float32
    evaluates the estimates as the C code does, float64 exactly.
    mutate: None, "timer+1" (n/4 + 1 after a detection), "shift_in_timer"
    (rows shift while the timer runs), "ge" (>= for > in FINDMAX)."""

    def __init__(self, bank, threshold, dtype=np.float64, mutate=None):
        self.b, self.thr, self.dt, self.mutate = bank, dtype(np.float32(threshold)), dtype, mutate
        self.reset()

    def reset(self):
        m = self.b.m
        self.timer, self.state, self.imax, self.idetect = self.b.n, SEEK, 0, 0
        self.r0 = np.zeros(m, self.dt)   # rxy0
        self.r1 = np.zeros(m, self.dt)   # rxy1
        self.rr = np.zeros(m, self.dt)   # rxy
        self.src = [None, None, None]    # the samples the three rows came from
        self.t = 0

    def estimates(self):
        dt, d, m = self.dt, self.idetect, self.b.m
        rm0 = self.r0[d]
        r0m = self.r1[d + 1] if d == 0 else self.r1[d - 1]
        r00 = self.r1[d]
        r0p = self.r1[d - 1] if d == m - 1 else self.r1[d + 1]
        rp0 = self.rr[d]
        with np.errstate(divide="ignore", invalid="ignore"):
            dphi = dt(self.b.dphi[d]) - dt(self.b.step) * dt(0.5) * (r0p - r0m) / (r0p + r0m - dt(2) * r00)
            tau = dt(0.5) * (rp0 - rm0) / (rp0 + rm0 - dt(2) * r00)
        tau = min(max(tau, dt(-0.499)), dt(0.499))
        return tau, dphi

    def step(self, row, E, log=None):
        """one sample; returns None or a detection dict"""
        t = self.t
        self.t += 1
        if self.timer:
            self.timer -= 1
            if self.mutate == "shift_in_timer":
                self.r0, self.r1, self.rr = self.r1, self.rr, np.asarray(row, self.dt)
            return None
        self.r0, self.r1, self.rr = self.r1, self.rr, np.asarray(row, self.dt)
        self.src = [self.src[1], self.src[2], t]
        if np.any(self.rr > 0):
            self.imax = int(np.argmax(self.rr))
        v = self.rr[self.imax]
        if self.state == SEEK:
            if log is not None:
                log.append((t, "seek", self.imax, None))
            if v > self.thr:
                self.idetect, self.state = self.imax, FINDMAX
            return None
        if log is not None:
            log.append((t, "findmax", self.imax, (self.src[1], self.idetect)))
        if (v >= self.r1[self.idetect]) if self.mutate == "ge" else (v > self.r1[self.idetect]):
            self.idetect = self.imax
            return None
        tau, dphi = self.estimates()
        n = self.b.n
        det = {"index": t, "idetect": self.idetect, "tau": tau, "dphi": dphi, "gamma": np.sqrt(self.dt(E) / self.dt(n)),
               "src": tuple(self.src)}
        self.state = SEEK
        self.timer = n // 4 + (1 if self.mutate == "timer+1" else 0)
        return det

    def run(self, rows, E, log=None, poison=None):
        """every sample of rows; poison: a boolean mask of samples whose rows
        are replaced by NaN (the unmarked ones)"""
        out = []
        for t in range(len(rows)):
            row = rows[t]
            if poison is not None and poison[t]:
                row = np.full_like(row, np.nan)
            d = self.step(row, E[t], log)
            if d:
                out.append(d)
        return out


def marked(rows, threshold, calls=None):
    """the samples whose records reach the host pass: a row maximum above the
    threshold, a neighbour of one, the first and last sample of every call (a
    piece of a call that is cut for the list's capacity counts as a call)"""
    N = len(rows)
    hot = np.asarray(rows).max(axis=1) > np.float32(threshold)
    mk = hot.copy()
    mk[1:] |= hot[:-1]
    mk[:-1] |= hot[1:]
    a = 0
    for c in (calls or [N]):
        mk[a] = mk[a + c - 1] = True
        a += c
    assert a == N
    return mk


def margins(bank, threshold, r64, bound, E64):
    """the least margin/requirement ratio over every comparison of the float64
    state machine, the least margin, and the detections"""
    sm = StateMachine(bank, threshold)
    log = []
    dets = sm.run(r64, E64, log)
    worst_ratio, least = np.inf, np.inf
    thr = float(np.float32(threshold))
    for t, kind, imax, prev in log:
        v, bv = r64[t, imax], bound[t, imax]
        if kind == "seek":
            mg, need = abs(v - thr), max(MARGIN_MIN, MARGIN_BOUNDS * bv)
        else:
            tp, d = prev
            mg, need = abs(v - r64[tp, d]), max(MARGIN_MIN, MARGIN_BOUNDS * max(bv, bound[tp, d]))
        least = min(least, mg)
        worst_ratio = min(worst_ratio, mg / need)
    return worst_ratio, least, dets


def check_margin(label, bank, threshold, r64, bound, E64):
    ratio, least, dets = margins(bank, threshold, r64, bound, E64)
    print("detector %-44s least decision margin %.3g, %.3g x what is required, %d detections"
          % (label, least, ratio, len(dets)))
    assert ratio >= 1, "%s: a comparison is decided by %.3g x the required margin only" % (label, ratio)
    return dets


# ------------------------------------------------------------------ estimate bounds
def estimate_bounds(bank, det, r64, bound):
    """(tau bound, dphi bound) at a float64 detection: sum |d/dr| delta_r over
    the values the formulas read, delta_r = the row bound"""
    s0, s1, s2 = det["src"]
    d, m = det["idetect"], bank.m
    lo = d + 1 if d == 0 else d - 1
    hi = d - 1 if d == m - 1 else d + 1

    def val(src, k):
        if src is None:
            return 0.0, 0.0
        return r64[src, k], bound[src, k]

    (rm0, dm), (r00, d0), (rp0, dp) = val(s0, d), val(s1, d), val(s2, d)
    (r0m, dlo), (r0p, dhi) = val(s1, lo), val(s1, hi)

    def prop(a, da, b, db, c, dc):
        # f = (b - a) / (2 (a + b - 2 c))
        N, D = b - a, a + b - 2 * c
        return abs((-D - N) / (2 * D * D)) * da + abs((D - N) / (2 * D * D)) * db + abs(N / (D * D)) * dc

    return prop(rm0, dm, rp0, dp, r00, d0), float(bank.step) * prop(r0m, dlo, r0p, dhi, r00, d0)


def check_detections(label, got, bank, r64, E64, bound, threshold, want64=None):
    """got: [(index, tau, dphi, gamma)] against the float64 state machine's:
    indices exactly, estimates within the propagated bounds; prints the worst
    ratio.  Returns it."""
    want = StateMachine(bank, threshold).run(r64, E64) if want64 is None else want64
    gi, wi = [int(g[0]) for g in got], [w["index"] for w in want]
    assert gi == wi, "%s: detections at %s, the model's at %s" % (label, gi, wi)
    worst = 0.0
    n = bank.n
    for g, w in zip(got, want):
        tb, pb = estimate_bounds(bank, w, r64, bound)
        gb = (n / 2 + 8) * 2.0 ** -24 * w["gamma"]
        clamped = abs(w["tau"]) >= 0.499
        for name, a, b, bd in (("tau_hat", g[1], w["tau"], tb), ("dphi_hat", g[2], w["dphi"], pb),
                               ("gamma_hat", g[3], w["gamma"], gb)):
            assert np.isfinite(a), "%s: %s at %d is not finite" % (label, name, w["index"])
            if name == "tau_hat" and clamped and abs(float(a)) >= 0.499 - 1e-6 and float(a) * w["tau"] > 0:
                continue   # both at the same clamp
            ratio = abs(float(a) - float(b)) / bd
            worst = max(worst, ratio)
            assert ratio <= 1, "%s: %s at %d is %.9g, the model's %.9g: %.3g x the bound %.3g" % (
                label, name, w["index"], a, b, ratio, bd)
    where = str(gi) if len(gi) <= 8 else "%s ... %d" % (str(gi[:6])[:-1], gi[-1])
    print("detector %-44s %d detections at %s, estimates within %.3g of their bounds" % (label, len(got), where, worst))
    return worst


# ------------------------------------------------------------------ pin streams
def plateau_case():
    """A stream with two consecutive rows that are equal bit for bit (a
    constant stretch longer than the window): FINDMAX ends at the second with
    > and goes on with >=.  It has no decision margin by construction and
    serves only to pin the checker."""
    n = 32
    s = np.ones(n, np.complex64)
    x = np.concatenate([noise(40, 5, 0.25), np.ones(n + 9, np.complex64), noise(60, 6, 0.25)]).astype(np.complex64)
    return s, 0.5, 0.02, x


# ------------------------------------------------------------------ fixture
# (name, n, threshold, dphi_max, carrier, stream length, positions); seeds in SEEDS.  One preamble for the ten
# autotest lengths; "missed": a second preamble that ends inside the n/4 timer of the first detection and is
# not reported; "stale": a second one that ends exactly on the first sample after that timer, so the detection
# at the next sample reads its rxy0 across the timer gap.
def _cases():
    out = []
    for n in AUTOTEST_N:
        out.append(("n%d" % n, n, threshold_for(n), 0.02, 0.01, 2 * n + 160, (n + 37,)))
    n = 128
    p0 = n + 21
    out.append(("missed", n, 0.4, 0.02, 0.01, 4 * n + 200, (p0, p0 + n // 8 + 5)))
    # first detection at p0 + n; the timer covers the next n/4 samples; the first computed sample is
    # p0 + n + n/4 + 1, where the second preamble ends
    out.append(("stale", n, 0.4, 0.02, 0.01, 4 * n + 200, (p0, p0 + n // 4 + 2)))
    return out


CASES = _cases()
SEEDS = {"n64": 1, "n83": 1, "n128": 1, "n167": 1, "n256": 1, "n335": 1, "n512": 1, "n671": 1, "n1024": 1,
         "n1341": 1, "missed": 1, "stale": 1}


def case_by_name(name):
    return [c for c in CASES if c[0] == name][0]


def case_stream(case, seed=None):
    name, n, thr, dphi_max, carrier, N, pos = case
    s = sequence(n)
    x = stream(s, N, pos, 7000 + 13 * (SEEDS[name] if seed is None else seed) + n, dphi=carrier)
    return s, x


_CACHE = {}


def case_model(case):
    """(bank, s, x, r64, E64, bound, float64 detections), computed once per
    case and shared; the margin is asserted"""
    name = case[0]
    if name not in _CACHE:
        s, x = case_stream(case)
        bank = Bank(s, case[3])
        r64, E64, bound = rows64(bank, x)
        dets = check_margin(name, bank, case[2], r64, bound, E64)
        _CACHE[name] = (bank, s, x, r64, E64, bound, dets)
    return _CACHE[name]


def load_fixture():
    with open(FIXTURE) as f:
        d = json.load(f)
    for c in d["cases"]:
        c["detections"] = [(int(i), np.float32(t), np.float32(p), np.float32(g)) for i, t, p, g in c["detections"]]
    return d
