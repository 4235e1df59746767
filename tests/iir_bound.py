"""An error bound local to each output for the recursive filters (iirfilt,
iirdecim, iirinterp: csrc/k_iirfilt.hip behind host/iirfilt.c and
host/iirdecim.c), the filters and the streams that probe it.

The filter as the object holds it: float32 coefficients, normalised by a[0],
as sections (b0 b1 b2 / 1 a1 a2); a NORM form of n <= 3 is one section.  For a
full-rate input x, in float64 / complex128, per section k with t_0 = x:

    v_k      = t_k filtered by 1/A_k                    the direct-form-II state
    t_k+1[n] = b_k0 v_k[n] + b_k1 v_k[n-1] + b_k2 v_k[n-2]
    R_k[n]   = |t_k[n]| + |a_k1| |v_k[n-1]| + |a_k2| |v_k[n-2]|   local scale of the v update
    S_k[n]   = sum_i |b_ki| |v_k[n-i]|                            local scale of the output sum
    Ev_k     = |g_k| (*) (R_k + E_k)     g_k the impulse response of 1/A_k, E_0 = 0
    E_k+1[n] = sum_i |b_ki| Ev_k[n-i] + S_k[n]
    A = E_nsec,   U = the same recursion with R_k = S_k = 1,   y64 = t_nsec

An output passes if it is finite and

    |y[n] - y64[n]| <= K 2^-23 A[n] + 2^-126 U[n],      K = 4,

and it must be exactly 0 (either sign) where no non-zero input has yet arrived.

Derivation (u = 2^-24, first order).  The v update x - a1 v1 - a2 v2 is two
products and two subtractions: each product errs by u |a v|, each difference
by u times its own result, which is at most R; together at most 3u R.  The
output sum of three products and two additions errs likewise by at most 3u S.
A complex sample is two such components: the modulus of the error takes a
factor of at most sqrt(2): 4.25 u.  A complex-by-complex product errs by
sqrt(5) u |a||v| in place of u |a||v| (Brent, Percival and Zimmermann 2007):
(sqrt(5) + 2) u = 4.24 u for the update, (sqrt(5) + 2) u for the sum.  K = 4,
that is 8u = K 2^-23, covers all three kinds to first order.
An error made in v_k[m] is an extra input to 1/A_k: it reaches v_k[n] through
g_k[n-m], then the output through b_k and the sections after it, whose own
input errors E_k+1 are treated the same way.  That is the recursion above,
with moduli throughout, so it holds for any order of the float32 operations
that forms each v and each sum from the same operands -- but not for a
computation that carries a state between spans in another form: that is what
the second assertion is for.  U propagates one unit per operation the same
way: 2^-126 U covers a gradual underflow (each operation off by at most
2^-150) and a flush to zero (at most 2^-126) alike.  Without that floor no
float32 implementation passes a stream with exact zeros after a burst: A
decays geometrically for ever, float32 stops at 2^-149.

The bound is rigorous and loose (|g| (*) . forgets every cancellation), and
looser the longer the cascade.  So a second assertion carries the tightness,
with the project's standing margin between two float32 orderings of one
computation (MARGIN = 4, as in fftfilt_bound.py): with

    r(y) = max_n |y[n] - y64[n]| / (2^-23 A[n] + 2^-126 U[n])        (K = 1)

the code under test must have r <= MARGIN r_ref on every row, r_ref the
largest r that the serial float32 model (iirfilt_model.run32, the reference's
statement order) reaches over that filter's streams of NS samples.  The
maximum over the streams, since one stream's worst is an extreme value; the
longer streams reuse it (r does not grow with the length: A does).

Cost.  A first-order section (a2 = 0) has |g| (*) r = lfilter([1], [1, -|a1|],
r), exact and O(n).  A second-order section convolves directly (np.convolve:
a transform convolution would smear the exact zeros) with |g| cut at the
length L where the geometric majorant of the dropped tail, sum_{j>=L} (j + 1)
rho^j (rho the larger pole modulus; g[j] = sum_i p1^i p2^(j-i)), times the
peak of what it multiplies is below 2^-24 of the floor's smallest value.
Streams of more than 2^16 samples take |g| exactly up to the lag J where that
majorant sums to 2^-40 and through the majorant beyond it (_absg_conv): an
upper bound of the exact scale, O(n) past J.

Filters (FILTERS: form, b, a in float32 / complex64, normalised) and the
kinds they run as (ROWS, with the kernels' section count MS):
    dc01, dc001     the DC blockers with pole 0.99 and 0.999           1 section
    cpoles1         one complex section of tests/golden/iirfilt.json   1
    butter4, cpoles2                                                    2
    ellip5 (3 sections), ellip8 (4)                                     MS = 4
    cascade8        ellip8 followed by butter7, real                    8
    slow8           eight first-order complex sections b = (2^-k, 0, 0),
                    a = (1, -(1 - 2^-k) e^{j theta_k}, 0), k = 6, 8 .. 20          8
                    theta_k = 0.7 + (k - 13) 2^-23: distinct, and all inside the
                    narrowest section's passband.  (With the angles spread out
                    the eight passbands do not meet: the output is 1e-31 of the
                    input, below any bound, and no state error can be seen.)
    leak12, leak20  b = (2^-k, 0, 0), a = (1, -(1 - 2^-k), 0)          1
    accum           b = (1, 0, 0), a = (1, -1, 0): a pole on the circle 1
    b4leaks         butter4, leak12, leak20: the long cascade row       MS = 4
The leaks, the accumulator and slow8 have |G| between 0.02 and 1 at every
level of the kernels' ladder of powers up to the top, so every lag of every
scan carries weight.  The design coefficients are those of
tests/golden/iirdes.json and tests/golden/iirfilt.json.

Streams (stream): uniform noise on a 2^-16 grid times an envelope.  "flat" is
level 1; "burst" has level-1 runs over 1e-5 and "gaps" the same runs over
exact zeros; "stairs" (the accumulator's flat: sums of level-1 grid values
are exact in float32, which would make r_ref zero) steps through levels that
are not powers of two.  The runs of the short stream, NS = 3 TILE + 5:
[0, 40); mid-tile [1000, 1300), 2800 samples before the next seam; a lane
seam and a wave seam of tile 1, two samples each; the tile seams [TILE - 50,
TILE + 1) and [2 TILE - 1, 2 TILE + 60); one sample at 2 TILE + 1000; a run
that ends on the last sample before CUT (a call cut there hands the burst to
the next call through the state alone); the last 5 samples.  Longer streams
repeat that pattern every 3 TILE samples and keep the last 5.

Shared by tests/test_iir_bound.py (run32 meets the bound, the checker is
pinned by mutations) and tests/test_gpu_iir_bound.py.  No GPU.
"""
import functools
import json
import os
import zlib

import numpy as np
from scipy.signal import lfilter

import iirfilt_model as IM

K = 4.0
MARGIN = 4.0
EPS = 2.0 ** -23
TINY = 2.0 ** -126
RUN, TILE, SCAN = 16, 4096, 256      # the kernels' geometry (the GPU module asserts it)
NS = 3 * TILE + 5
CUT = 2 * TILE + 1777
NLONG = 2 * SCAN * TILE + TILE + 5
FIRST = 777                          # the loud first call before a long stream
ENVELOPES = ("flat", "burst", "gaps")

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _design(name):
    with open(os.path.join(_GOLD, "iirdes.json")) as f:
        d = next(c for c in json.load(f)["designs"] if c["name"] == name)
    b, a = np.array(d["b"], np.float32), np.array(d["a"], np.float32)
    assert np.all(a[0::3] == 1.0)
    return b, a


def _case(name):
    c = next(c for c in IM.load_fixture()["cases"] if c["name"] == name)
    return np.asarray(c["b"]), np.asarray(c["a"])


def _first_order(ks, thetas=None):
    b = np.zeros(3 * len(ks), np.complex64 if thetas else np.float32)
    a = np.zeros_like(b)
    for i, k in enumerate(ks):
        b[3 * i], a[3 * i] = 2.0 ** -k, 1.0
        a[3 * i + 1] = -(1.0 - 2.0 ** -k) * (np.exp(1j * thetas[i]) if thetas else 1.0)
    return b, a


def _filters():
    f = {}
    f["dc01"] = ("norm",) + _case("dc_blocker_0.01_crcf")
    f["dc001"] = ("norm",) + _case("dc_blocker_1e-3_rrrf")
    f["cpoles1"] = ("sos",) + _case("cpoles1_cccf")
    f["butter4"] = ("sos",) + _case("butter4_rrrf")
    f["cpoles2"] = ("sos",) + _case("cpoles2_cccf")
    f["ellip5"] = ("sos",) + _case("ellip5_crcf")
    e8, b7 = _design("ellip8"), _design("butter7")
    f["ellip8"] = ("sos",) + e8
    f["cascade8"] = ("sos", np.concatenate([e8[0], b7[0]]), np.concatenate([e8[1], b7[1]]))
    ks = (6, 8, 10, 12, 14, 16, 18, 20)
    f["slow8"] = ("sos",) + _first_order(ks, [0.7 + (k - 13) * 2.0 ** -23 for k in ks])
    f["leak12"] = ("sos",) + _first_order([12])
    f["leak20"] = ("sos",) + _first_order([20])
    f["accum"] = ("sos", np.array([1, 0, 0], np.float32), np.array([1, -1, 0], np.float32))
    l2 = _first_order([12, 20])
    f["b4leaks"] = ("sos", np.concatenate([f["butter4"][1], l2[0]]), np.concatenate([f["butter4"][2], l2[1]]))
    return f


FILTERS = _filters()

# (filter, kind) -> MS, the kernels' section count: every (KIND, MS) appears
ROWS = [("dc01", "crcf", 1), ("dc001", "rrrf", 1), ("leak12", "rrrf", 1), ("leak12", "crcf", 1),
        ("leak20", "rrrf", 1), ("leak20", "crcf", 1), ("accum", "rrrf", 1), ("accum", "crcf", 1),
        ("cpoles1", "cccf", 1),
        ("butter4", "rrrf", 2), ("butter4", "crcf", 2), ("cpoles2", "cccf", 2),
        ("ellip5", "crcf", 4), ("ellip8", "rrrf", 4), ("ellip8", "crcf", 4), ("ellip8", "cccf", 4),
        ("cascade8", "rrrf", 8), ("cascade8", "crcf", 8), ("slow8", "cccf", 8)]


def register(fname, form, b, a):
    """a filter designed by the library under test (the GPU module's rate changers): float32, normalised"""
    FILTERS[fname] = (form, np.asarray(b), np.asarray(a))


def envelopes(fname):
    """the three streams of a filter: the accumulator takes stairs for flat and has no gaps row"""
    return ("stairs", "burst") if fname == "accum" else ENVELOPES


def nsec(fname):
    form, b, _ = FILTERS[fname]
    return 1 if form == "norm" else len(b) // 3


def coefs(fname, kind):
    """(form, b, a) as the kind's coefficient type"""
    form, b, a = FILTERS[fname]
    if np.iscomplexobj(b):
        assert kind == "cccf"
    dt = IM.coef_dtype(kind)
    return form, np.asarray(b, dt), np.asarray(a, dt)


def sections(fname):
    """[(b0, b1, b2, a1, a2)] in float64 / complex128"""
    form, b, a = FILTERS[fname]
    wide = np.complex128 if np.iscomplexobj(b) else np.float64
    b, a = np.asarray(b).astype(wide), np.asarray(a).astype(wide)
    if form == "norm":
        b, a = np.concatenate([b, np.zeros(3 - len(b), wide)]), np.concatenate([a, np.zeros(3 - len(a), wide)])
    return [(b[3 * k], b[3 * k + 1], b[3 * k + 2], a[3 * k + 1], a[3 * k + 2]) for k in range(len(b) // 3)]


# ------------------------------------------------------------------ streams
def level(n, envelope):
    if envelope == "flat":
        return None
    if envelope == "stairs":
        steps = np.array([0.3, 0.7, 0.11, 0.9, 0.05, 0.6])
        return steps[(np.arange(n) // 700) % len(steps)]
    lv = np.full(n, 1e-5 if envelope == "burst" else 0.0)
    for base in range(0, n, 3 * TILE):
        for a, b in ((0, 40), (1000, 1300), (TILE + 17 * RUN - 1, TILE + 17 * RUN + 1),
                     (TILE + 64 * RUN - 1, TILE + 64 * RUN + 1), (TILE - 50, TILE + 1), (2 * TILE - 1, 2 * TILE + 60),
                     (2 * TILE + 1000, 2 * TILE + 1001), (CUT - 30, CUT)):
            lv[base + a:base + b] = 1.0
    lv[n - 5:] = 1.0
    return lv


@functools.lru_cache(maxsize=None)
def stream(kind, n, envelope, seed):
    x = IM.noise_input(kind, n, seed, level(n, envelope))
    x.setflags(write=False)
    return x


def seed_of(fname, kind, envelope):
    return zlib.crc32(("%s %s %s" % (fname, kind, envelope)).encode())


# ------------------------------------------------------------------ the scale
def _shift(v, i):
    if i == 0:
        return v
    o = np.zeros_like(v)
    o[i:] = v[:-i]
    return o


def _absg_len(a1, a2, peak):
    """L: |g| beyond it is dropped; (majorant of the tail) peak <= 2^-24 of 2^-126 U, U >= 1"""
    rho = _pole_modulus(a1, a2)
    want = 2.0 ** -24 * TINY / max(peak, 1e-300)
    L = 8
    while rho ** L * (L * (1 - rho) + 1) / (1 - rho) ** 2 > want:    # sum_{j>=L} (j+1) rho^j
        L += max(8, L // 8)
    return L


def _pole_modulus(a1, a2):
    rho = float(np.max(np.abs(np.roots([1.0, a1, a2])))) * (1 + 1e-12)
    assert rho < 1.0, "a second-order section with a pole on the circle has no finite cut"
    return rho


def _absg_head(a1, a2):
    """J: from here on the majorant (j + 1) rho^j sums to less than 2^-40 (of sum |g| >= 1)"""
    rho = _pole_modulus(a1, a2)
    J = 8
    while rho ** J * (J * (1 - rho) + 1) / (1 - rho) ** 2 > 2.0 ** -40:
        J += max(8, J // 8)
    return J


LONG = 1 << 16     # streams longer than this take |g|'s far part through its majorant


def _absg_conv(a1, a2, r):
    """|g| (*) r, g the impulse response of 1 / (1 + a1 z^-1 + a2 z^-2).  Up to LONG samples: |g| cut
    at _absg_len.  Longer streams: |g| up to J = _absg_head exactly, and beyond J its majorant
    (j + 1) rho^j, which is rational (O(n)): nothing is dropped, the result is an upper bound of the
    exact one, above it by less than 2^-40 of a steady level (by more only deeper than J samples into
    a gap, where what is left of the burst is below 2^-40 of it)."""
    if a2 == 0:
        return lfilter([1.0], [1.0, -abs(a1)], r)
    n = len(r)
    L, J = min(n, _absg_len(a1, a2, float(np.max(r)))), _absg_head(a1, a2)
    far = n > LONG and J < L
    imp = np.zeros(J if far else L, np.complex128 if np.iscomplexobj(np.array([a1, a2])) else np.float64)
    imp[0] = 1.0
    g = np.abs(lfilter([1.0], [1.0, a1, a2], imp))
    out = np.convolve(r, g)[:n]
    if far:     # sum_{i>=0} (J + (i + 1)) rho^(J+i) r[n-J-i]
        rho, rd = _pole_modulus(a1, a2), _shift(r, J)
        out += rho ** J * (J * lfilter([1.0], [1.0, -rho], rd) + lfilter([1.0], [1.0, -2 * rho, rho * rho], rd))
    return out


def scale(fname, x):
    """-> (y64, A, U) for the input x (any float or complex array; float64 / complex128 inside)"""
    sec = sections(fname)
    cplx = np.iscomplexobj(x) or np.iscomplexobj(sec[0][0])
    t = np.asarray(x).astype(np.complex128 if cplx else np.float64)
    n = len(t)
    E, EU = np.zeros(n), np.zeros(n)
    one = np.ones(n)
    for b0, b1, b2, a1, a2 in sec:
        v = lfilter([1.0], [1.0, a1, a2], t)
        av = np.abs(v)
        R = np.abs(t) + abs(a1) * _shift(av, 1) + abs(a2) * _shift(av, 2)
        S = abs(b0) * av + abs(b1) * _shift(av, 1) + abs(b2) * _shift(av, 2)
        Ev = _absg_conv(a1, a2, R + E)
        EvU = _absg_conv(a1, a2, one + EU)
        E = abs(b0) * Ev + abs(b1) * _shift(Ev, 1) + abs(b2) * _shift(Ev, 2) + S
        EU = abs(b0) * EvU + abs(b1) * _shift(EvU, 1) + abs(b2) * _shift(EvU, 2) + one
        t = b0 * v + b1 * _shift(v, 1) + b2 * _shift(v, 2)
    assert np.min(EU) >= 1.0      # what _absg_len's cut relies on
    return t, E, EU


def first_input(x):
    """index of the first non-zero input (len(x) if none)"""
    nz = np.flatnonzero(np.asarray(x) != 0)
    return int(nz[0]) if len(nz) else len(x)


def ratios(y, y64, A, U, k=1.0):
    """|y - y64| / (k 2^-23 A + 2^-126 U) per output; inf where y is not finite"""
    y = np.asarray(y)
    with np.errstate(all="ignore"):
        r = np.abs(y.astype(y64.dtype) - y64) / (k * EPS * A + TINY * U)
    r[~np.isfinite(y)] = np.inf
    return r


def verdict(y, x, y64, A, U, span=slice(None)):
    """-> (ok, r, where): ok = every output of the span is finite, within K 2^-23 A + 2^-126 U, and
    exactly 0 before the first non-zero input; r = the worst ratio with K = 1 and its index"""
    y = np.asarray(y)
    idx = np.arange(len(y64))[span]
    r4 = ratios(y, y64, A, U, K)[span]
    r1 = ratios(y, y64, A, U, 1.0)[span]
    quiet = idx < first_input(x)
    ok = bool(np.all(r4 <= 1.0)) and bool(np.all(y[span][quiet] == 0))
    w = int(np.argmax(r1)) if len(r1) else 0
    return ok, float(r1[w]) if len(r1) else 0.0, int(idx[w]) if len(r1) else 0


# ------------------------------------------------------------------ per (filter, kind, stream), cached
@functools.lru_cache(maxsize=None)
def case(fname, kind, envelope, n=NS):
    """(x, y64, A, U) of the row's stream of n samples"""
    x = stream(kind, n, envelope, seed_of(fname, kind, envelope))
    y64, A, U = scale(fname, x)
    for a in (y64, A, U):
        a.setflags(write=False)
    return x, y64, A, U


@functools.lru_cache(maxsize=4)
def long_case(fname, kind, envelope="burst"):
    """(x, y64, A, U) over FIRST loud samples (the first call) and the long stream after them"""
    seed = seed_of(fname, kind, envelope)
    x = np.concatenate([stream(kind, FIRST, "flat", seed + 1), stream(kind, NLONG, envelope, seed + 2)])
    return (x,) + scale(fname, x)


@functools.lru_cache(maxsize=None)
def model32(fname, kind, envelope):
    """run32 on the short stream"""
    form, b, a = coefs(fname, kind)
    y, _ = IM.run32(kind, form, b, a, case(fname, kind, envelope)[0])
    return y


@functools.lru_cache(maxsize=None)
def r_ref(fname, kind):
    """the largest worst ratio of run32 over the filter's short streams"""
    return max(verdict(model32(fname, kind, e), *case(fname, kind, e))[1] for e in envelopes(fname))


# ------------------------------------------------------------------ float64 with states (for the mutations)
def run64_seg(fname, x, zi=None):
    """x through the sections from the states zi (scipy's, one array per section; None = zero)
    -> (y, zf)"""
    sec = sections(fname)
    cplx = np.iscomplexobj(x) or np.iscomplexobj(sec[0][0])
    t = np.asarray(x).astype(np.complex128 if cplx else np.float64)
    zf = []
    for k, (b0, b1, b2, a1, a2) in enumerate(sec):
        z0 = np.zeros(2, t.dtype) if zi is None else np.asarray(zi[k], t.dtype)
        t, z = lfilter([b0, b1, b2], [1.0, a1, a2], t, zi=z0)
        zf.append(z)
    return t, zf


def run64_spans(fname, x, edges, start_of):
    """the stream in the spans edges[i] .. edges[i+1]; span i starts from start_of(i, true, z):
    true = the states the stream really has there, z = the list of every earlier span's end states
    from zero state (z[j] of span j)"""
    out, true, z = [], None, []
    for i in range(len(edges) - 1):
        seg = x[edges[i]:edges[i + 1]]
        y, _ = run64_seg(fname, seg, start_of(i, true, z))
        out.append(y)
        _, true = run64_seg(fname, seg, true)
        z.append(run64_seg(fname, seg, None)[1])
    return np.concatenate(out)


def df2_state(fname, x, n):
    """the kernels' state before sample n of the stream x: (v_k[n-1], v_k[n-2]) per section"""
    sec = sections(fname)
    cplx = np.iscomplexobj(x) or np.iscomplexobj(sec[0][0])
    t = np.asarray(x[:n]).astype(np.complex128 if cplx else np.float64)
    st = []
    for b0, b1, b2, a1, a2 in sec:
        v = lfilter([1.0], [1.0, a1, a2], t)
        st.append((v[n - 1], v[n - 2]))
        t = b0 * v + b1 * _shift(v, 1) + b2 * _shift(v, 2)
    return st


def zero_input(fname, state, count):
    """count outputs of the cascade from the state (df2_state's layout) with zero input"""
    st = [list(s) for s in state]
    out = np.zeros(count, np.result_type(*[type(v) for s in st for v in s], np.float64))
    for n in range(count):
        t = 0.0
        for k, (b0, b1, b2, a1, a2) in enumerate(sections(fname)):
            v0 = t - a1 * st[k][0] - a2 * st[k][1]
            t = b0 * v0 + b1 * st[k][0] + b2 * st[k][1]
            st[k] = [v0, st[k][0]]
        out[n] = t
    return out
