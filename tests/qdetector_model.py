"""Float64 model of qdetector_cccf (src/framing/src/qdetector_cccf.c) and the
bar its implementations are held to.  Like detector_model.py:

  inputs    regenerated from integer arithmetic (a 32-bit LCG), never stored:
            QPSK symbols, the autotest's interpolated burst (k = 2, m = 7,
            beta = 0.3, tau = -0.3, phi = 0.5, gamma = 1), chip templates over a
            quiet floor 100 dB under the bursts;
  records   window_record64: peak, index, offset, energy of one window in
            float64, with the best value at any other (offset, lag);
  machine   walk64: SEEK / ALIGN over the window grid, which restarts half a
            buffer into every aligned frame; the float64 estimates with bounds;
  serial32  the reference's loop restated in float32 (numpy's float32 FFT, the
            running energy sums in arrival order);
  margin    check_margin refuses a case unless every decision (peak against
            the threshold, the top against any other (offset, lag) where the
            window's index decides, the align stage's arg-max bin) is more
            than twice the bound away from flipping.

Bound on a scaled row value rxy (the issue's B):
  B = (8 log2 nfft + 8) 2^-23 sqrt(nfft / s_len) + 2^-23 (nfft / 4 + 8) |rxy|
the transform bound of fftfilt_bound.py carried through g (g nfft |x_w|_2 |s|_2
= sqrt(nfft / s_len) at any signal level) plus the energy sum's.  An
implementation is also held to 4x the serial model's own worst ratio to B.
The align stage's unscaled values carry the same transform term times 1 / g:
  eR = c nfft |x|_2 |s|_2,   eV = c sqrt(nfft) |x conj s|_2,   c = (8 log2 nfft + 8) 2^-23
and the estimates' bounds are those errors pushed through the fit formulas
(every corner of the three magnitudes) plus the float32 formulas' own rounding.
"""
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qdetector.json")
EPS = 2.0 ** -23
AUTOTEST_LEN = (64, 83, 128, 167, 256, 335, 512, 671, 1024, 1341)
AUTOTEST_TOL = {"tau": 0.05, "gamma": 0.05, "dphi": 0.01, "phi": 0.1}
K, M, BETA, TAU, PHI = 2, 7, 0.3, -0.3, 0.5
FLOOR = 1e-5        # 100 dB under a full-scale burst
THRESHOLD = 0.5
EST = ("tau", "gamma", "dphi", "phi")


def lcg_words(count, seed):
    out = np.empty(count, np.int64)
    s = seed & 0xFFFFFFFF
    for k in range(count):
        s = (1664525 * s + 1013904223) & 0xFFFFFFFF
        out[k] = s
    return out


def qpsk(n, seed):
    w = lcg_words(n, seed)
    re = np.where((w >> 20) & 1, 1.0, -1.0)
    im = np.where((w >> 21) & 1, 1.0, -1.0)
    return ((re + 1j * im) * np.sqrt(0.5)).astype(np.complex64)


def floor_noise(N, seed, level=FLOOR):
    w = lcg_words(2 * N, seed)
    v = (((w >> 12) & 0xFFF) - 2047.5) / 2048.0 * level
    return v[0::2] + 1j * v[1::2]


def nfft_of(s_len):
    return 1 << int(np.ceil(np.log2(2 * s_len)))


def range_of(dphi_max, nfft):
    """qdetector_cccf_set_range: float product, double division, truncation"""
    return max(int(float(np.float32(dphi_max) * np.float32(nfft)) / (2 * np.pi)), 0)


def prototype(dt):
    """the arkaiser prototype the autotest uses (the library's host design code)"""
    import liquidmi as LQ
    return LQ.firdes_prototype("arkaiser", K, M, BETA, dt).astype(np.float64)


def interpolate(sym, h, k=K):
    """firinterp: y[k i + p] = sum_l h[p + l k] sym[i - l]"""
    y = np.zeros(k * len(sym), np.complex128)
    hp = np.concatenate([h, np.zeros((-len(h)) % k)])
    for p in range(k):
        y[p::k] = np.convolve(sym, hp[p::k])[:len(sym)]
    return y


def linear_template(seq):
    sym = np.concatenate([seq.astype(np.complex128), np.zeros(2 * M)])
    return interpolate(sym, prototype(0.0)).astype(np.complex64)


def linear_stream(seq, seed):
    """the autotest's received signal: the sequence, then symbols drawn from it"""
    L = len(seq)
    nsym = 8 * L + 2 * M
    pick = (lcg_words(nsym - L, seed + 77) >> 8) % L
    sym = np.concatenate([seq, seq[pick]]).astype(np.complex128)
    return (interpolate(sym, prototype(-TAU)) * np.exp(1j * PHI)).astype(np.complex64)


class Template:
    def __init__(self, s):
        self.s = np.asarray(s, np.complex64)
        self.s_len = len(self.s)
        self.nfft = nfft_of(self.s_len)
        pad = np.zeros(self.nfft, np.complex128)
        pad[:self.s_len] = self.s
        self.pad = pad
        self.S = np.fft.fft(pad)
        self.s2 = float(np.sum(np.abs(self.s.astype(np.complex128)) ** 2))
        self.c = (8 * np.log2(self.nfft) + 8) * EPS

    def bound(self, rxy):
        return self.c * np.sqrt(self.nfft / self.s_len) + EPS * (self.nfft / 4 + 8) * np.abs(rxy)


def _shifted(S, nfft, offs):
    i = np.arange(nfft)
    return np.conj(S)[(i[None, :] - np.asarray(offs)[:, None]) % nfft]


def window_record64(T, xw, rng):
    """(peak, index, offset, energy, second): the first maximum in (offset, lag)
    order and the best value anywhere else, float64"""
    xw = np.asarray(xw).astype(np.complex128)
    E = float(np.sum(np.abs(xw) ** 2))
    if E == 0.0:
        return 0.0, 0, 0, 0.0, 0.0
    n = T.nfft
    g = 1.0 / (n * np.sqrt(E) * np.sqrt(T.s_len / n) * np.sqrt(T.s2))
    X = np.fft.fft(xw)
    top, key, second = -1.0, 0, 0.0
    offs = np.arange(-rng, rng + 1)
    for b in range(0, len(offs), 32):
        r = np.abs(np.fft.ifft(X[None, :] * _shifted(T.S, n, offs[b:b + 32]), axis=1)).ravel() * (n * g)
        k = int(np.argmax(r))
        v = float(r[k])
        r[k] = -1.0
        rest = float(np.max(r)) if len(r) > 1 else 0.0
        if v > top:
            second = max(second, top, rest)
            top, key = v, b * n + k
        else:
            second = max(second, v)
    return top, key % n, key // n - rng, E, max(second, 0.0)


def align64(T, frame, offset):
    """the align stage in float64: estimates, the values they are made of and their error scales"""
    n = T.nfft
    x = np.asarray(frame).astype(np.complex128)
    R = np.fft.ifft(np.fft.fft(x) * _shifted(T.S, n, [offset])[0]) * n
    a = np.abs(R[[n - 1, 0, 1 % n]])
    v = x * np.conj(T.pad)
    V = np.fft.fft(v)
    av = np.abs(V)
    i0 = int(np.argmax(av))
    vv = av[[(i0 - 1) % n, i0, (i0 + 1) % n]]
    rest = av.copy()
    rest[i0] = 0
    xn, sn = np.sqrt(np.sum(np.abs(x) ** 2)), np.sqrt(T.s2)
    return {"a": a, "i0": i0, "v": vv, "v_second": float(np.max(rest)), "vt": v[:T.s_len],
            "eR": T.c * n * xn * sn, "eV": T.c * np.sqrt(n) * np.sqrt(np.sum(np.abs(v) ** 2))}


def fit_tau_gamma(a, nfft, s2):
    y = np.sqrt(a)
    qa = 0.5 * (y[2] + y[0]) - y[1]
    qb = 0.5 * (y[2] - y[0])
    tau = -qb / (2 * qa)
    g = qa * tau * tau + qb * tau + y[1]
    return tau, g * g / (nfft * s2)


def fit_dphi(i0, v, nfft):
    qa = 0.5 * (v[2] + v[0]) - v[1]
    qb = 0.5 * (v[2] - v[0])
    index = i0 - qb / (2 * qa)
    return (index - nfft if i0 > nfft / 2 else index) * 2 * np.pi / nfft


def _corners(e):
    return [np.array([sa, sb, sc]) * e for sa in (-1, 1) for sb in (-1, 1) for sc in (-1, 1)]


def estimates64(T, al):
    """(estimates, bounds): the float64 values and what an implementation may differ by"""
    n = T.nfft
    tau, gamma = fit_tau_gamma(al["a"], n, T.s2)
    dphi = fit_dphi(al["i0"], al["v"], n)
    idx = np.arange(T.s_len)
    metric = np.sum(al["vt"] * np.exp(-1j * dphi * idx))
    phi = float(np.angle(metric))
    bt = bg = bd = 0.0
    for d in _corners(al["eR"]):
        t, g = fit_tau_gamma(np.maximum(al["a"] + d, 0), n, T.s2)
        bt, bg = max(bt, abs(t - tau)), max(bg, abs(g - gamma))
    for d in _corners(al["eV"]):
        bd = max(bd, abs(fit_dphi(al["i0"], al["v"] + d, n) - dphi))
    # the float32 formulas' own rounding: a few operations on values of size <= 1 / |gamma| / pi
    bt += 16 * EPS * max(1.0, abs(tau))
    bg += 16 * EPS * abs(gamma)
    bd += 16 * EPS * np.pi
    sv = float(np.sum(np.abs(al["vt"])))
    eM = sv * (EPS * (4 + abs(dphi) * T.s_len) + T.s_len * EPS / 2)
    bp = bd * (T.s_len - 1) + 2 * eM / abs(metric) + 8 * EPS * np.pi
    return ({"tau": float(tau), "gamma": float(gamma), "dphi": float(dphi), "phi": phi},
            {"tau": bt, "gamma": bg, "dphi": bd, "phi": bp})


def detects(T, rec, thr):
    return rec[0] > thr and rec[1] < T.nfft - T.s_len


def walk64(T, x, rng, thr=THRESHOLD, grid_shift=0):
    """The float64 state machine over the stream x (preceded by the nfft/2 zeros
    of a fresh object).  Returns (windows, detections): windows = [(ext
    position, record)] of every seek window completed, detections = [(index of
    the completing sample, estimates, bounds, align values)].  grid_shift: a
    deliberately wrong restart of the grid after a frame (for the mutation tests)."""
    n, h = T.nfft, T.nfft // 2
    ext = np.concatenate([np.zeros(h, np.complex64), np.asarray(x, np.complex64)])
    base, wins, dets = 0, [], []
    while base + n <= len(ext):
        rec = window_record64(T, ext[base:base + n], rng)
        wins.append((base, rec))
        if not detects(T, rec, thr):
            base += h
            continue
        a = base + rec[1]
        if a + n > len(ext):
            break
        al = align64(T, ext[a:a + n], rec[2])
        est, bnd = estimates64(T, al)
        dets.append((a + n - 1 - h, est, bnd, al))
        base = a + h + grid_shift
    return wins, dets


def margins(T, wins, dets, thr=THRESHOLD):
    """the smallest margin-to-bound ratio over every decision of a walk"""
    worst = np.inf
    for _, rec in wins:
        peak, index, _, E, second = rec
        if E == 0.0:
            continue
        B = T.bound(peak)
        worst = min(worst, abs(peak - thr) / B)
        if peak > thr:   # the index decides (and, on a hit, where the frame starts)
            worst = min(worst, (peak - second) / B)
    for _, _, _, al in dets:
        worst = min(worst, (al["v"][1] - al["v_second"]) / al["eV"])
    return worst


def check_margin(label, T, wins, dets, thr=THRESHOLD):
    m = margins(T, wins, dets, thr)
    assert m > 2.0, "%s: a decision is only %.3g bounds from flipping; the case is refused" % (label, m)
    return m


def _f32sum(a):
    """float32 sum in arrival order"""
    return np.cumsum(np.asarray(a, np.float32), dtype=np.float32)[-1] if len(a) else np.float32(0)


def serial32(T, x, rng, thr=THRESHOLD):
    """The reference's loop restated in float32: windows = [(ext position, (peak,
    index, offset, energy))], detections = [(index, estimates)]"""
    f = np.float32
    n, h = T.nfft, T.nfft // 2
    S = np.fft.fft(T.pad.astype(np.complex64))
    assert S.dtype == np.complex64
    ext = np.concatenate([np.zeros(h, np.complex64), np.asarray(x, np.complex64)])
    s2 = _f32sum(T.s.real ** 2 + T.s.imag ** 2)
    base, wins, dets = 0, [], []
    i = np.arange(n)
    while base + n <= len(ext):
        xw = ext[base:base + n]
        p2 = xw.real * xw.real + xw.imag * xw.imag
        E = f(_f32sum(p2[:h]) + _f32sum(p2[h:]))
        peak, index, offset = f(0), 0, 0
        if E > 0:
            g0 = f(np.sqrt(E)) * f(np.sqrt(f(T.s_len) / f(n)))
            g = f(1) / (f(n) * g0 * f(np.sqrt(s2)))
            X = np.fft.fft(xw)
            for off in range(-rng, rng + 1):
                r = np.fft.ifft(X * np.conj(S[(i - off) % n])) * f(n)
                a = np.abs((r * g).astype(np.complex64))
                k = int(np.argmax(a))
                if a[k] > peak:
                    peak, index, offset = a[k], k, off
        wins.append((base, (float(peak), index, offset, float(E))))
        if not (peak > f(thr) and index < n - T.s_len):
            base += h
            continue
        a0 = base + index
        if a0 + n > len(ext):
            break
        fr = ext[a0:a0 + n]
        R = np.fft.ifft(np.fft.fft(fr) * np.conj(S[(i - offset) % n])) * f(n)
        y = np.sqrt(np.abs(R[[n - 1, 0, 1 % n]]).astype(np.float32))
        qa = f(0.5) * (y[2] + y[0]) - y[1]
        qb = f(0.5) * (y[2] - y[0])
        tau = -qb / (f(2) * qa)
        gh = qa * tau * tau + qb * tau + y[1]
        gamma = gh * gh / (f(n) * s2)
        v = (fr * np.conj(T.pad.astype(np.complex64))).astype(np.complex64)
        av = np.abs(np.fft.fft(v)).astype(np.float32)
        i0 = int(np.argmax(av))
        vn, v0, vp = av[(i0 - 1) % n], av[i0], av[(i0 + 1) % n]
        qa = f(0.5) * (vp + vn) - v0
        qb = f(0.5) * (vp - vn)
        index_f = f(i0) + (-qb / (f(2) * qa))
        dphi = f(float((index_f - f(n)) if i0 > n // 2 else index_f) * 2 * np.pi / float(n))
        ang = (dphi * np.arange(T.s_len, dtype=np.float32)).astype(np.float32)
        metric = np.sum((v[:T.s_len] * np.exp(-1j * ang).astype(np.complex64)).astype(np.complex64))
        dets.append((a0 + n - 1 - h, {"tau": float(tau), "gamma": float(gamma), "dphi": float(dphi),
                                      "phi": float(np.angle(metric))}))
        base = a0 + h
    return wins, dets


# ------------------------------------------------------------------ checks

def record_ratio(T, got, want):
    """|peak - peak64| / B of one record"""
    return abs(float(got[0]) - want[0]) / T.bound(want[0])


def check_records(label, T, got, wins, serial_worst=None, thr=THRESHOLD):
    """got: records (peak, index, offset, energy) of the windows of a float64
    walk, in order.  Peaks within B (and within 4x the serial model's worst
    ratio); a window whose index decides carries the model's (index, offset);
    energies to the sum's bound; zero windows exactly (0, 0, 0).  Returns the worst ratio."""
    assert len(got) == len(wins), "%s: %d records, the model has %d windows" % (label, len(got), len(wins))
    worst = 0.0
    for k, (g, (pos, w)) in enumerate(zip(got, wins)):
        if w[3] == 0.0:
            assert (float(g[0]), int(g[1]), int(g[2]), float(g[3])) == (0.0, 0, 0, 0.0), \
                "%s: window %d is all zero, got %r" % (label, k, tuple(g))
            continue
        r = record_ratio(T, g, w)
        assert r <= 1.0, "%s: window %d at %d: peak %.9g, model %.9g, %.3g bounds" % (label, k, pos, g[0], w[0], r)
        worst = max(worst, r)
        assert abs(float(g[3]) - w[3]) <= EPS * (T.nfft / 4 + 8) * w[3], \
            "%s: window %d: energy %.9g, model %.9g" % (label, k, g[3], w[3])
        if w[0] > thr:
            assert (int(g[1]), int(g[2])) == (w[1], w[2]), \
                "%s: window %d at %d: (index, offset) %r, model %r" % (label, k, pos, (int(g[1]), int(g[2])), w[1:3])
    if serial_worst is not None:
        assert worst <= 4 * serial_worst, "%s: %.3g bounds, the serial model stays within %.3g" % (
            label, worst, serial_worst)
    return worst


def check_detections(label, got, dets, autotest=None):
    """got: [(index, {tau, gamma, dphi, phi})] against a float64 walk's detections"""
    assert [int(g[0]) for g in got] == [d[0] for d in dets], "%s: detections at %r, model %r" % (
        label, [int(g[0]) for g in got], [d[0] for d in dets])
    for g, d in zip(got, dets):
        for name in EST:
            diff = abs(float(g[1][name]) - d[1][name])
            if name == "phi":
                diff = min(diff, 2 * np.pi - diff)
            assert diff <= d[2][name], "%s: %s_hat %.9g, model %.9g, bound %.3g" % (
                label, name, g[1][name], d[1][name], d[2][name])
    if autotest is not None:
        assert len(got) >= 1, label + ": no frame"
        for name in EST:
            assert abs(float(got[0][1][name]) - autotest[name]) <= AUTOTEST_TOL[name], "%s: autotest %s_hat %r" % (
                label, name, got[0][1][name])


# ------------------------------------------------------------------ cases

def chips(n, seed):
    return qpsk(n, seed)


def burst_stream(s, N, positions, seed, bin_=0, nfft=None, phase=0.3):
    """s at the given positions over the floor, on carrier bin `bin_` of nfft"""
    x = floor_noise(N, seed)
    nfft = nfft or nfft_of(len(s))
    for p in positions:
        t = np.arange(len(s))
        x[p:p + len(s)] += s.astype(np.complex128) * np.exp(1j * (2 * np.pi * bin_ / nfft * t + phase))
    return x.astype(np.complex64)


# name -> (kind, parameters); the fixture holds what the reference did with each
LINEAR = ["linear_n%d" % L for L in AUTOTEST_LEN]
PLAIN = {
    # name: (s_len, seed, N, positions, bin, dphi_max for set_range or None)
    "bin3": (100, 11, 1536, (700,), 3, 0.2),
    "two_frames": (100, 12, 2560, (500, 1500), 0, None),
    "straddle": (100, 13, 1024, (298,), 0, None),
}
CASE_NAMES = LINEAR + list(PLAIN)
_CACHE = {}


def case_inputs(name):
    """(kind, symbols or template, stream, dphi_max or None)"""
    if name.startswith("linear_n"):
        L = int(name[len("linear_n"):])
        seq = qpsk(L, 1000 + L)
        return "linear", seq, linear_stream(seq, 1000 + L), None
    s_len, seed, N, pos, b, dmax = PLAIN[name]
    s = chips(s_len, seed)
    return "plain", s, burst_stream(s, N, pos, seed + 100, b), dmax


def case_model(name):
    """(T, x, rng, windows, detections) with the margin asserted; cached, shared, not to be changed"""
    if name not in _CACHE:
        kind, a, x, dmax = case_inputs(name)
        T = Template(linear_template(a) if kind == "linear" else a)
        rng = range_of(0.3 if dmax is None else dmax, T.nfft)
        wins, dets = walk64(T, x, rng)
        check_margin(name, T, wins, dets)
        _CACHE[name] = (T, x, rng, wins, dets)
    return _CACHE[name]


def load_fixture():
    with open(FIXTURE) as fh:
        fx = json.load(fh)
    out = {}
    for c in fx["cases"]:
        dets = []
        for d in c["detections"]:
            est = np.array(d[1:], np.uint32).view(np.float32)
            dets.append((d[0], dict(zip(EST, (float(v) for v in est)))))
        out[c["name"]] = {"s_len": c["s_len"], "nfft": c["nfft"], "detections": dets}
    return out
