"""Error bounds local to each bin for spgramcf / spgramf, and the streams that
probe them.

host/spgram.c restated in float64.  The window is w = g window, g = sqrt(2) /
(rms(window) sqrt(nfft)) formed in float32 as create() forms it (the float32
values are the reference's window: the scale is data, not arithmetic under
test).  With ext = (W zeros of history) ++ (every sample written so far),
transform t ends at stream index e_t and reads u_t = ext[e_t + 1 .. e_t + W]
w, zero padded to nfft: X_t = FFT(u_t), P_t = |X_t|^2.

  execute(), execute_psd():  the current window; psd = P + 1e-16.
  accumulate_psd(x, n, a):   a transform each time the sample counter reaches
        W / 2 (it runs on across calls): e_t = (t + 1) W/2 - 1; psd = (1 - a_t)
        psd + a_t P_t from psd = 1, where a_t = 1 for every transform of the
        call that makes the object's first transform and the call's a (as
        float32) after that.
  estimate_psd(x, n):        reset; e_t = (t + 1) delay - 1, delay = max(nfft /
        4, 1), and a last one at n - 1 if delay does not divide n; psd = mean_t P_t.
  Outputs are 10 log10 psd, bin k at (k + nfft / 2) mod nfft.

Outputs are compared in linear power, 10^(dB / 10), bin by bin.  eps = 2^-23.

The bound.  A float32 power-of-two FFT errs per bin by at most the 2-norm of
its error, at most 4 lg nfft eps ||X||_2 = 4 lg nfft eps sqrt(nfft) ||u||_2
(tests/fft_bound.py); the window product adds eps |u_i| per sample, carried
by the transform as at most eps sqrt(nfft) ||u||_2 per bin; |X|^2's own
roundings are relative to P.  So

    d_t = (4 lg nfft + 8) eps sqrt(nfft) ||u_t||_2          |X_t[k] - X64_t[k]| <= d_t
    | |X|^2 - P_t[k] | <= 2 |X_t[k]| d_t + d_t^2

  execute:      |X - X64| <= d_t
  execute_psd:  2 |X| d_t + d_t^2 + conv(P + 1e-16) (the 3 eps of |X|^2 and + 1e-16 inside conv's + 4)
  estimate:     bound[k] = mean_t (2 |X_t[k]| d_t + d_t^2) + (T + 4) eps psd64[k] + conv(psd64[k])
  accumulate:   bound[k] = sum_t c_t [2 |X_t[k]| d_t + d_t^2 + (3 (T_end - t + 1) + 8) eps P_t[k]] + conv(psd64[k])
  conv(p) = eps (|ln p| + 4) p

estimate's middle term: a float32 sum of T non-negative terms in any order
errs by at most (T - 1) u relative to the sum (u = eps / 2), each |X|^2 by 3 u,
the division by 1 u: (T + 4) eps has a factor 2 over that.  conv: the output
is 10 log10f(p); an error of c ulps of the dB value v = 10 log10 p moves 10^(v /
10) by (ln 10 / 10) |v| c u p = |ln p| c u p, and the multiply by 10 and
log10f's own error near p = 1, where |ln p| vanishes, are the + 4.  accumulate:
c_t = a_t prod_{s > t} (1 - a_s) is the weight the recursion gives transform t
at the end of the stream (the initial ones: a transform of its own with P = 1,
d = 0 and c = prod_s (1 - a_s)); every step of the recursion p = (1 - a) p + a v
rounds 1 - a, two products and a sum: 3 u per step relative to the terms it
carries, T_end - t + 1 steps for transform t, and the regrouping by chunks
replaces len steps by one product with powf(1 - a, len), whose error (the
rounding of 1 - a taken to the power len, 2 ulps of powf) stays under the 3 u
per step it replaces; 3 eps per step has the factor 2, and + 8 covers |X|^2
and the two products by a.

The bound's first term is local to a transform, not to a bin: a bin 100 dB
under the tone is held to d_t^2 of the transforms that saw the tone, about
-80 dB.  The tightness comes from the second assertion: the worst ratio of the
code under test must be at most MARGIN = 4 times the oracle's on the same case
(the project's standing margin).  The oracle's serial float32 sum is inside
the (T + 4) eps term but 1.6e-5 normwise at T = 4097, which is why the
comparison is against float64 and not against the oracle.

Streams (complex or real, seeded):
  tone:   level 1 at bin nfft / 4 + 1, bin centred, with a smooth onset over
          the first 2 W samples, over a noise floor of 1e-5: more than 100 dB
          between the strongest and the weakest bin of the float64 reference
          with a Kaiser window, beta = 10.
  bursts: the 1e-5 floor, and level-1 noise over W samples centred on the end
          of transform 63 (so it is in the last transform of chunk 0 and the
          first of chunk 1), of transform 4095 (the last chunk of fold group 0
          and the first of group 1; streams long enough), on every cut between
          calls (the windows that straddle history and input), and the last W
          samples (the final transform).

Shared by tests/test_spgram_bound.py and tests/test_gpu_spgram_bound.py.  No GPU.
"""
import functools
import math

import numpy as np

import liquidmi as LQ

EPS = 2.0 ** -23
MARGIN = 4.0
STREAMS = ["tone", "bursts"]
BETA = 10.0


def kaiser_window(W):
    """The library's own Kaiser window (host code, no GPU), float32."""
    return np.array([LQ.lib().kaiser(i, W, BETA, 0.0) for i in range(W)], np.float32)


def scaled_window(window, nfft):
    """create()'s w in float32 arithmetic, as float64 values."""
    g = np.float32(0)
    for v in window.astype(np.float32):
        g = np.float32(g + np.float32(v * v))
    g = np.float32(math.sqrt(2.0) / float(np.float32(np.sqrt(np.float32(g / np.float32(len(window))))) *
                                          np.sqrt(np.float32(nfft))))
    return (g * window.astype(np.float32)).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------ transform positions
def estimate_ends(nfft, n):
    delay = max(nfft // 4, 1)
    e = np.arange(delay - 1, n, delay, dtype=np.int64)
    return np.concatenate([e, [n - 1]]) if n % delay else e


def accumulate_plan(W, calls):
    """calls: [(samples, alpha)].  Returns (ends, a_t, first): stream indices of
    the transforms, the alpha each is folded in with, and the index of each
    call's first transform (len(calls) + 1 entries)."""
    H = W // 2
    total = sum(n for n, _ in calls)
    ends = np.arange(H - 1, total, H, dtype=np.int64)
    a = np.empty(len(ends))
    first, pos, seen = [0], 0, False
    for n, alpha in calls:
        t0, t1 = first[-1], int(np.searchsorted(ends, pos + n))
        forced = (not seen) and t1 > t0
        a[t0:t1] = 1.0 if forced else float(np.float32(alpha))
        seen = seen or t1 > t0
        first.append(t1)
        pos += n
    return ends, a, first


def weights(a):
    """c_t = a_t prod_{s > t} (1 - a_s), and the initial psd's weight prod_s (1 - a_s)."""
    tail = np.concatenate([np.cumprod((1.0 - a)[::-1])[::-1][1:], [1.0]])
    return a * tail, float(np.prod(1.0 - a))


# ------------------------------------------------------------------ float64 reference and bound
def _chunks(T, nfft):
    step = max((1 << 21) // nfft, 1)
    return [(a, min(a + step, T)) for a in range(0, T, step)]


def _spectra(x, W, w64, nfft, ends):
    """X64_t for the transforms ending at ends, and ||u_t||_2."""
    ext = np.concatenate([np.zeros(W, np.complex128), x.astype(np.complex128)])
    U = ext[(ends[:, None] + 1) + np.arange(W)[None, :]] * w64[None, :]
    return np.fft.fft(U, n=nfft, axis=1), np.sqrt(np.sum(np.abs(U) ** 2, axis=1))


def dfac(nfft):
    return (4 * math.log2(nfft) + 8) * EPS * math.sqrt(nfft)


def conv(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return EPS * (np.abs(np.log(p)) + 4.0) * p


def reference(x, W, w64, nfft, ends, c, steps, c_init=0.0, init_steps=0, shift=True, want_energy=True):
    """psd64[k] = sum_t c_t P_t[k] (+ c_init), and the bound's transform-local
    part sum_t c_t (2 |X| d_t + d_t^2 + steps_t eps P_t); shifted to the
    output's bin order.  Also the energy sum_k P_t[k] per transform."""
    psd, bnd, energy = np.full(nfft, float(c_init)), np.full(nfft, c_init * init_steps * EPS), np.empty(len(ends))
    for a, b in _chunks(len(ends), nfft):
        if np.max(c[a:b]) < 1e-40 and not want_energy:   # under 1e-40 of a transform's power: far below conv()
            energy[a:b] = np.nan
            continue
        X, un = _spectra(x, W, w64, nfft, ends[a:b])
        P, d = np.abs(X) ** 2, dfac(nfft) * un
        energy[a:b] = np.sum(P, axis=1)
        cw = c[a:b]
        psd += cw @ P
        bnd += cw @ (2 * np.sqrt(P) * d[:, None] + (d ** 2)[:, None]) + (cw * steps[a:b] * EPS) @ P
    if shift:
        psd, bnd = np.roll(psd, nfft // 2), np.roll(bnd, nfft // 2)
    return psd, bnd, energy


# ------------------------------------------------------------------ streams
def _noise(r, n, real):
    return r.uniform(-1, 1, n) if real else (r.uniform(-1, 1, n) + 1j * r.uniform(-1, 1, n)) / math.sqrt(2.0)


def stream(name, real, nfft, W, n, spans=(), seed=0):
    """n samples; bursts: level-1 noise over each [a, b) of `spans` (clipped to
    the stream) and over the last W."""
    r = np.random.default_rng(4099 * nfft + 17 * W + 2 * seed + (1 if real else 0) + 7 * STREAMS.index(name))
    x = 1e-5 * _noise(r, n, real)
    if name == "tone":
        ph = 2 * np.pi * (((nfft // 4 + 1) * np.arange(n, dtype=np.int64)) % nfft) / nfft
        # a smooth onset over 2 W samples (the running sum of a Kaiser window): the first
        # windows, part history and part tone, then leak no more than the full ones
        ramp = np.cumsum(np.kaiser(2 * W, 3 * BETA))
        env = np.ones(n)
        m = min(2 * W, n)
        env[:m] = (ramp / ramp[-1])[:m]
        x = x + env * (np.cos(ph) if real else np.exp(1j * ph))
    else:
        for a, b in list(spans) + [(n - W, n)]:
            a, b = max(int(a), 0), min(int(b), n)
            if b > a:
                x[a:b] = _noise(r, b - a, real)
    return x.astype(np.float32 if real else np.complex64)


# ------------------------------------------------------------------ cases
class Case:
    """One stream through estimate_psd or a sequence of accumulate_psd calls.

    mode "estimate": calls = [(n, None)]; mode "accumulate": calls = [(n, alpha), ...].
    """

    def __init__(self, mode, real, nfft, W, calls, name, centres_t=(), want_energy=True):
        self.mode, self.real, self.nfft, self.W, self.calls, self.name = mode, real, nfft, W, list(calls), name
        self.window = kaiser_window(W)
        self.w64 = scaled_window(self.window, nfft)
        n = sum(c[0] for c in calls)
        if mode == "estimate":
            assert len(calls) == 1
            self.ends = estimate_ends(nfft, n)
            T = len(self.ends)
            self.c, self.steps, self.c_init, self.first = np.full(T, 1.0 / T), np.zeros(T), 0.0, [0, T]
        else:
            self.ends, self.a, self.first = accumulate_plan(W, calls)
            T = len(self.ends)
            self.c, self.c_init = weights(self.a)
            self.steps = 3.0 * (T - np.arange(T)) + 8.0
        self.T = T
        cuts = np.cumsum([c[0] for c in calls])[:-1]
        # W samples from half a window before the end of transform t, and on to half a window
        # before the end of transform t + 1 where the hop is longer than that: in both transforms
        spans = [(self.ends[t] - W // 2, max(self.ends[t] - W // 2 + W, self.ends[t + 1] - W // 2 + 1))
                 for t in centres_t if t + 1 < T] + [(c - W // 2, c - W // 2 + W) for c in cuts]
        self.x = stream(name, real, nfft, W, n, spans)
        self.psd64, b, self.energy = reference(self.x, W, self.w64, nfft, self.ends, self.c, self.steps, self.c_init,
                                               3.0 * T + 8.0, True, want_energy)
        self.bound = b + ((T + 4) * EPS * self.psd64 if mode == "estimate" else 0.0) + conv(self.psd64)
        for a in (self.x, self.psd64, self.bound, self.energy):
            a.setflags(write=False)

    def pieces(self):
        edges = np.concatenate([[0], np.cumsum([c[0] for c in self.calls])])
        return [(self.x[a:b], al) for (a, b), (_, al) in zip(zip(edges[:-1], edges[1:]), self.calls)]

    def report(self, db):
        db = np.asarray(db, np.float64)
        assert db.shape == self.psd64.shape
        with np.errstate(over="ignore", invalid="ignore"):
            lin = 10.0 ** (db / 10.0)
        finite = np.isfinite(db) & np.isfinite(lin)     # -inf dB is a zero psd: no stream here has one
        err = np.where(finite, np.abs(lin - self.psd64), np.inf)
        ratio = err / self.bound
        worst = int(np.argmax(ratio))
        return {"worst": float(ratio[worst]), "bin": worst, "failing": int(np.count_nonzero(~(ratio <= 1.0))),
                "nonfinite": int(np.count_nonzero(~finite))}

    def check(self, db, oracle_worst=None, what=""):
        r = self.report(db)
        print("spgram_bound %s %s nfft=%d W=%d %s T=%d %s: worst %.4g of the bound at bin %d (oracle %s), %d of %d "
              "bins fail, %d non-finite" % (self.mode, "real" if self.real else "complex", self.nfft, self.W, self.name,
                                           self.T, what, r["worst"], r["bin"],
                                           "-" if oracle_worst is None else "%.4g" % oracle_worst, r["failing"],
                                           self.nfft, r["nonfinite"]))
        assert r["failing"] == 0 and r["nonfinite"] == 0, (
            "%s nfft=%d W=%d T=%d %s: worst error %.4g x the bound at bin %d; %d bins fail; %d non-finite"
            % (self.mode, self.nfft, self.W, self.T, what, r["worst"], r["bin"], r["failing"], r["nonfinite"]))
        if oracle_worst is not None:
            assert r["worst"] <= MARGIN * oracle_worst, (
                "%s nfft=%d W=%d T=%d %s: worst ratio %.4g at bin %d is more than %g x the oracle's %.4g"
                % (self.mode, self.nfft, self.W, self.T, what, r["worst"], r["bin"], MARGIN, oracle_worst))
        return r


def run_object(g, c):
    """The case's calls through a spgram object of the library or the oracle (host entry points)."""
    if c.mode == "estimate":
        return g.estimate_psd(c.x)
    for x, alpha in c.pieces():
        g.accumulate_psd(x, alpha)
    return g.write_accumulation()


def oracle_worst(c):
    import oracle_lib as O
    return c.check(run_object(O.Spgram(c.nfft, c.window, c.real), c), what="oracle")["worst"]


# ------------------------------------------------------------------ rows
def estimate_n(nfft, T, ragged=True):
    """Samples that make T transforms; ragged: the last one at n - 1, off the delay grid."""
    delay = max(nfft // 4, 1)
    return T * delay - (delay // 3 if ragged and delay > 2 else 0)


def accumulate_calls(W, T, alpha, cuts=False):
    """A first call of two transforms (its alpha is forced to 1) that leaves the
    sample counter at 5, the call of exactly T transforms, and with cuts: calls
    of exactly 64 transforms, of one, of none (shorter than W / 2) and a last
    one of 3 samples whose transform straddles four calls' samples."""
    H = W // 2
    calls = [(2 * H + min(5, H - 1), 0.5), (T * H, alpha)]
    if cuts:
        assert H >= 8
        calls += [(64 * H, alpha), (H, alpha), (H - 6, alpha), (3, alpha)]
    return calls


def transforms_of_calls(W, calls):
    _, _, first = accumulate_plan(W, calls)
    return [b - a for a, b in zip(first[:-1], first[1:])]


SEAMS = (63, 4095)     # transforms whose end a burst is centred on: chunk seam, fold-group seam
PLAIN_T = [63, 64, 65, 4096, 4097, 2 * 4096 + 64 + 3]
ALPHAS = [0.0, 0.05, 1.0]
FUSED_W = [301, 512, 513, 1024]
FUSED_T = [255, 256, 257, 4097]


def _rows():
    """(mode, real, nfft, W, T, alpha, cuts, stream): T the transforms of the
    estimate or of the accumulate stream's main call."""
    R = []
    for T in PLAIN_T:                                   # plain path, nfft = 64, W = 48
        for name in STREAMS:
            R.append(("estimate", False, 64, 48, T, None, False, name))
        for alpha in ALPHAS:
            R.append(("accumulate", False, 64, 48, T, alpha, False, "tone"))
            R.append(("accumulate", False, 64, 48, T, alpha, alpha == 0.05 and T in (65, 4097), "bursts"))
    R.append(("estimate", True, 64, 48, 4097, None, False, "bursts"))
    R.append(("accumulate", True, 64, 48, 4097, 0.05, True, "bursts"))
    for nfft, W in ((256, 256), (2048, 301)):
        for name in STREAMS:
            R.append(("estimate", False, nfft, W, 4097, None, False, name))
        R.append(("estimate", True, nfft, W, 4097, None, False, "tone"))
    for W in FUSED_W:                                   # fused path, nfft = 1024
        for real in (False, True):
            for T in FUSED_T:
                R.append(("estimate", real, 1024, W, T, None, False, STREAMS[(T + W) % 2]))
                R.append(("accumulate", real, 1024, W, T, 0.05, T in (257, 4097), STREAMS[(T + W + 1) % 2]))
    for alpha in (0.0, 1.0):
        R.append(("accumulate", False, 1024, 512, 257, alpha, True, "bursts"))
    return R


ROWS = _rows()


TAIL = 8


def single_transform(row):
    """alpha = 1 on the tone: psd is the stream's last transform alone."""
    return row[0] == "accumulate" and row[5] == 1.0 and row[7] == "tone"


def margin_oracle(row, c):
    """The oracle's worst ratio the margin is taken against.  It is the
    oracle's ratio on the case, but where psd is the stream's last transform of
    the tone alone it is the oracle's worst over the stream cut after each of
    its last TAIL = 8 transforms (the case itself among them).

    Measured on these rows (MI355X and oracle, stage by stage): both transforms
    err alike (|dX| at 0.006 to 0.018 of d_t, |X|^2 at 0.003 to 0.017 of the
    bound), and the worst ratio of either comes from the peak bin, where the dB
    value (14 dB) is rounded to float32: one ulp of it is 1.8 eps of the power,
    0.015 of the bound there.  log10f and the multiply by 10 leave 0.4 to 4
    eps from one transform to the next, so the oracle's ratio on one transform
    is one draw of that rounding (0.004 to 0.034 over the last 16 positions;
    the kernels' 0.007 to 0.035), and the tone's phase against the hop repeats
    every 8 transforms (24 samples at 17 / 64 cycles per sample).  One draw is
    no yardstick; eight are."""
    if not single_transform(row):
        return oracle_worst(c)
    import oracle_lib as O
    assert not row[6] and c.first[-1] == c.T
    H, worst = c.W // 2, 0.0
    (n0, a0), (n1, a1) = c.calls
    for j in range(TAIL):
        g = O.Spgram(c.nfft, c.window, c.real)
        g.accumulate_psd(c.x[:n0], a0)
        g.accumulate_psd(c.x[n0:n0 + n1 - j * H], a1)
        t = c.T - 1 - j
        X, un = _spectra(c.x, c.W, c.w64, c.nfft, c.ends[t:t + 1])
        P, d = np.abs(X[0]) ** 2, dfac(c.nfft) * un[0]
        psd = np.roll(P, c.nfft // 2)
        bnd = np.roll(2 * np.sqrt(P) * d + d * d + c.steps[-1] * EPS * P, c.nfft // 2) + conv(psd)
        lin = 10.0 ** (g.write_accumulation().astype(np.float64) / 10.0)
        r = float(np.max(np.abs(lin - psd) / bnd))
        if j == 0:
            assert abs(r - c.report(10.0 * np.log10(lin))["worst"]) <= 1e-6 * r    # the case's own reference and bound
        worst = max(worst, r)
    print("spgram_bound %s: the oracle's worst over the last %d transforms %.4g" % (row_id(row), TAIL, worst))
    return worst


def row_id(r):
    mode, real, nfft, W, T, alpha, cuts, name = r
    return "%s-%s-nfft%d-W%d-T%d%s%s-%s" % (mode[:3], "real" if real else "cplx", nfft, W, T,
                                           "" if alpha is None else "-a%g" % alpha, "-cuts" if cuts else "", name)


@functools.lru_cache(maxsize=3)
def case(row):
    mode, real, nfft, W, T, alpha, cuts, name = row
    if mode == "estimate":
        return Case("estimate", real, nfft, W, [(estimate_n(nfft, T, T % 2 == 1), None)], name, SEAMS)
    # the seams of the main call: its transforms 63 / 4095 are the stream's 65 / 4097
    return Case("accumulate", real, nfft, W, accumulate_calls(W, T, alpha, cuts), name, tuple(2 + t for t in SEAMS))


def row_path(row):
    """(kernel path, fold levels of the largest call) from the launch's own decisions."""
    mode, real, nfft, W, T, alpha, cuts, name = row
    return LQ.spgram_route(real, nfft, W), fold_levels(min(T, max(LQ.spgram_batch_samples() // nfft, 1)))


def fold_levels(T_call):
    """1 or 2: the fold of a call (or launch batch) of T_call transforms."""
    nch = -(-T_call // LQ.spgram_chunk())
    return 1 if nch <= LQ.spgram_fold_group() else 2


# ------------------------------------------------------------------ closed forms for the launch-geometry rows
def two_sample_terms(x, w64, ends):
    """nfft-point transforms of a two-sample window: X_t[k] = A_t + B_t exp(-2 pi i k / nfft),
    A_t = w0 ext[e_t + 1], B_t = w1 ext[e_t + 2]."""
    ext = np.concatenate([np.zeros(2, np.complex128), x.astype(np.complex128)])
    return w64[0] * ext[ends + 1], w64[1] * ext[ends + 2]


def two_sample_case(nfft, calls, seed):
    """W = 2 (a transform per sample): the stream, float64 psd and bound of
    accumulate calls with the spectra in closed form, over the transforms whose
    weight is at least 1e-40 (below that: far under conv()).  Returns (window,
    x, psd64, bound, T)."""
    W = 2
    win = kaiser_window(W)
    w64 = scaled_window(win, nfft)
    n = sum(c[0] for c in calls)
    r = np.random.default_rng(seed)
    lv = np.where(np.arange(n) % 1000 < 500, 1.0, 1e-3)
    x = ((r.uniform(-1, 1, n) + 1j * r.uniform(-1, 1, n)) * lv).astype(np.complex64)
    ends, a, first = accumulate_plan(W, calls)
    c, c_init = weights(a)
    T = len(ends)
    steps = 3.0 * (T - np.arange(T)) + 8.0
    A, B = two_sample_terms(x, w64, ends)
    keep = np.flatnonzero(c >= 1e-40)
    A, B, ck, sk = A[keep], B[keep], c[keep], steps[keep]
    ph = np.exp(-2j * np.pi * np.arange(nfft) / nfft)
    psd, bnd = np.full(nfft, c_init), np.full(nfft, c_init * (3.0 * T + 8.0) * EPS)
    d = dfac(nfft) * np.sqrt(np.abs(A) ** 2 + np.abs(B) ** 2)
    for lo in range(0, len(keep), 256):
        q = slice(lo, lo + 256)
        P = np.abs(A[q, None] + B[q, None] * ph[None, :]) ** 2
        psd += ck[q] @ P
        bnd += ck[q] @ (2 * np.sqrt(P) * d[q, None] + (d[q] ** 2)[:, None]) + (ck[q] * sk[q] * EPS) @ P
    psd, bnd = np.roll(psd, nfft // 2), np.roll(bnd, nfft // 2)
    return win, x, psd, bnd + conv(psd), T


def check_lin(db, psd, bound, what):
    db = np.asarray(db, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        lin = 10.0 ** (db / 10.0)
    ok = np.isfinite(db)
    r = np.where(ok, np.abs(lin - psd), np.inf) / bound
    print("spgram_bound %s: worst %.4g of the bound at bin %d" % (what, np.max(r), np.argmax(r)))
    assert np.all(ok) and np.max(r) <= 1.0, "%s: worst %.4g x the bound at bin %d" % (what, np.max(r), np.argmax(r))
    return float(np.max(r))


SECOND_BATCH_N = (1 << 13) + 5       # samples a call: 8197 transforms at W = 2 against 8192 a batch at nfft = 4096
GATHER_N = 70000                     # nfft = 4: as many transforms on the gather's grid.y
CHUNKS_N = (1 << 22) + (1 << 12)     # nfft = 2: as many transforms, 65600 chunks on k_spg_part's grid.y


@functools.lru_cache(maxsize=1)
def gather_case():
    return Case("estimate", False, 4, 4, [(GATHER_N, None)], "bursts", SEAMS, want_energy=False)


@functools.lru_cache(maxsize=1)
def chunks_case():
    return Case("estimate", False, 2, 2, [(CHUNKS_N, None)], "bursts", SEAMS, want_energy=False)
