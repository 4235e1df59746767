"""An error bound local to each output frame for the channelizers, and the
cases that probe it.

The normwise checks of the rest of the suite divide the largest error by the
largest output of the whole run, so a frame whose inputs are quieter than the
loudest frame is checked only against that frame's level: at 1e-5 of full
scale the whole content of a quiet frame is about the tolerance.  Here every
output of firpfbch2 and firpfbch, analyzer and synthesizer, is held to a bound
formed from the inputs that output's frame sees, against float64 models that
restate oracle/oracle.c:839-1056.

Notation: H[i, n] = h[i + nM], eps = 2^-23, windows hold the newest sample at
index 0, Z(z) = ||z||_2, lg = log2 of M (of the next power of two where M is
none).

  firpfbch2 analyzer   block b takes M/2 inputs, f = b & 1; they go to windows
      j = base - 1 - i (base = M for f = 1, M/2 for f = 0);
      X[j] = sum_n H[i, n] W[j, n], a[j] = sum_n |H[i, n]| |W[j, n]|,
      j = (i + f M/2) mod M;  Y_b = ifft(X)  (numpy's 1/M is the reference's);
      bound_b = (0.71 2m + 4 lg + 8) eps ||a||_2 / sqrt(M), every channel.
  firpfbch analyzer    x[bM + i] goes to window M - 1 - i;
      v[i] = sum_n H[i, n] W[i, n], a the same over moduli;  Y_b = fft(v[::-1]);
      bound_b = (0.71 T + 4 lg + 8) eps sqrt(M) ||a||_2.
  firpfbch synthesizer z_f = ifft(X_f) M pushed to window i;
      y[i] = sum_n H[i, n] W[i, n];
      bound[f, i] = eps (4 lg sum_n |H[i, n]| Z(z_{f-n})
                         + (0.71 T + 8) sum_n |H[i, n]| |W[i, n]|).
  firpfbch2 synthesizer z_f = ifft(X_f) M/2;  with c = i + f M/2,
      y_f[i] = sum_n H[i, n] z_{f-2n}[c] + sum_n H[i + M/2, n] z_{f-1-2n}[c];
      the bound as above over both dot products, second coefficient
      0.71 4m + 8, each window slot with the Z of the frame that filled it.

T is the number of real terms per output component: p for real taps, 2p for
complex ones (2m and 4m for firpfbch2).

Where the constants come from (u = 2^-24): a float32 dot product of T real
terms per component errs by at most gamma_T A, with the sqrt(2) of a complex
value 0.71 T eps A (as in tests/fir_bound.py).  A power-of-two float32 FFT
errs normwise by at most lg (mu + gamma_4 (sqrt(2) + mu)) ||y||_2 (Higham,
Accuracy and Stability of Numerical Algorithms, Thm 24.2), with twiddles
rounded to float32 below 4 eps per stage.  ||v||_2 <= ||a||_2, and one output
errs by at most the 2-norm of its frame's error.  The + 8 covers the scale
multiplies and an accumulator that truncates.  The direct DFT of the sizes
that are no power of two stays within the next power of two's bound.

An output passes if |y - y64| <= bound; where the bound is exactly 0 the
frame's whole window is zero and the output must be exactly 0 (either sign).
Every output must be finite.  The second assertion of the GPU tests compares
the worst ratio err / bound with the oracle's on the same case.

Shared by tests/test_pfb_bound.py (the oracle meets the bound, the checker is
pinned) and tests/test_gpu_pfb_bound.py (every channelizer kernel).  No GPU.
"""
import collections
import functools
import math
import zlib

import numpy as np

EPS = 2.0 ** -23
FLOOR = {"burst": 1e-5, "gaps": 0.0}
ENVELOPES = ["burst", "gaps"]

# kind: "pfb2" (firpfbch2, q = m) or "pfb" (firpfbch, q = p); an: analyzer;
# t: "crcf" / "cccf"; S: blocks one workgroup run or set covers on the row's
# kernel; mode: None, "few" (calls of at most 16 blocks) or "unaligned" (the
# input at a pointer that is 8 but not 16 bytes aligned, device calls only);
# route: what liquidmi.firpfbch2_route / firpfbch_route must answer for the
# row's stream in one call (for `few' rows: for a call of 16 blocks).  The
# query is the launch's own decision, and tests/test_pfb_bound.py holds every
# row to its route and to run == S, so neither is a comment.
# nb: the stream's length in blocks where it is not 3S + 4 windows + 5 (the
# long-run rows of tests/test_gpu_pfb_bound.py, whose S comes from the query).
Row = collections.namedtuple("Row", "kind an t M q S mode route nb", defaults=(None, None))


def _rows(kind, an, t, specs):
    return [Row(kind, an, t, M, q, S, mode, route) for M, q, S, mode, route in specs]


# firpfbch2 analyzer (M, m, S, mode, route)
PFB2_AN = _rows("pfb2", True, "crcf", [
    (2, 1, 512, None, "pfb2_direct"),         # k_pfb2_an<2>: 1024 / M blocks per workgroup
    (8, 2, 128, None, "pfb2_direct"),         # k_pfb2_an<8>
    (12, 3, 1, None, "pfb2_generic"),         # k_pfb2_an_generic (direct DFT): one block per workgroup
    (4, 1, 256, None, "pfb2_direct"),         # k_pfb2_an<4>
    (64, 9, 16, None, "pfb2_direct"),         # k_pfb2_an<64> (2m > 16): 16 blocks per workgroup
    (1024, 9, 1, None, "pfb2_direct"),        # k_pfb2_an<1024>: one block per workgroup
    (64, 2, 64, None, "pfb2_an_small"),       # k_pfb2_an_small: runs of 32 rows = 64 blocks per set
    (128, 4, 64, None, "pfb2_an_small"),      # k_pfb2_an_small
    (256, 2, 64, None, "pfb2_an256"),         # k_pfb2_an256<L, 1>: runs of 32 rows
    (512, 3, 64, None, "pfb2_an512"),         # k_pfb2_an256<L, 2>
    (1024, 2, 64, None, "pfb2_an1024"),       # k_pfb2_an1024 (streaming): 4 groups of 16 blocks
    (1024, 4, 64, None, "pfb2_an1024"),       # k_pfb2_an1024
    (1024, 2, 16, "few", "pfb2_an1024_few"),  # k_pfb2_an1024_few: one workgroup per call of <= 16 blocks
    (1024, 4, 16, "few", "pfb2_an1024_few"),  # k_pfb2_an1024_few
    (1024, 4, 64, "unaligned", "pfb2_an1024_unpaired"),   # k_pfb2_an1024<L, false>: the unpaired 8-byte loads
    (1024, 3, 48, None, "pfb2_poly+fft"),     # k_pfb2_poly<6>: runs of 4L = 24 rows
    (256, 8, 128, None, "pfb2_poly+fft"),     # k_pfb2_poly<16>: 64 rows
    (8192, 2, 32, None, "pfb2_poly+fft"),     # k_pfb2_poly<4>: 16 rows
    (2048, 2, 64, None, "pfb2_an2048"),       # k_pfb2_an2048: runs of 32 rows
    (4096, 2, 64, None, "pfb2_an4096"),       # k_pfb2_an4096: runs of 32 rows
    (16, 2, 64, None, "pfb2_direct"),         # k_pfb2_an<16>: 64 blocks per workgroup
])
# firpfbch2 synthesizer (M, m, S, mode, route)
PFB2_SYN = _rows("pfb2", False, "crcf", [
    (12, 3, 64, None, "pfb2_two_pass_run"),   # batched transform + k_pfb2_syn_out_run<6>: a lane runs 64 blocks
    (64, 4, 64, None, "pfb2_two_pass_run"),   # batched transform + k_pfb2_syn_out_run<8>
    (256, 2, 64, None, "pfb2_syn_fused"),     # k_pfb2_syn_fused<4, 1>: runs of 64 blocks
    (512, 4, 64, None, "pfb2_syn_fused"),     # k_pfb2_syn_fused<8, 2>
    (1024, 2, 32, None, "pfb2_syn1024"),      # k_pfb2_syn1024<4>: 2 groups of 16 blocks
    (1024, 4, 32, None, "pfb2_syn1024"),      # k_pfb2_syn1024<8>
    (4096, 2, 33, None, "pfb2_syn4096"),      # k_pfb2_syn4096<4>: runs of 33 blocks
    (64, 1, 1, None, "pfb2_two_pass_elem"),   # batched transform + k_pfb2_syn_out (2m = 2 has no ring): per element
    (12, 5, 1, None, "pfb2_two_pass_elem"),   # batched direct DFT + k_pfb2_syn_out (2m = 10)
])
# firpfbch analyzer (M, p, S, mode, route), crcf
PFB_AN = _rows("pfb", True, "crcf", [
    (10, 5, 1, None, "pfb_an_elem+fft"),      # k_pfb_an_X (per element) + batched direct DFT
    (64, 8, 32, None, "pfb_an_small"),        # k_pfb_an_small: runs of 32 blocks
    (256, 4, 32, None, "pfb_an_fused"),       # k_pfb_an_fused
    (1024, 4, 32, None, "pfb_an1024"),        # k_pfb_an1024<4, 16>: 2 groups of 16 blocks
    (1024, 8, 32, None, "pfb_an1024"),        # k_pfb_an1024<8, 8>
    (4096, 4, 32, None, "pfb_an4096"),        # k_pfb_an4096
    (1024, 4, 16, "few", "pfb_an1024_few"),   # k_pfb_an1024_few<4>
    (1024, 8, 16, "few", "pfb_an1024_few"),   # k_pfb_an1024_few<8>
    (2048, 4, 64, None, "pfb_an_run+fft"),    # k_pfb_an_X_run<4, float>: a lane runs 64 blocks; batched transform
    (1024, 4, 32, "unaligned", "pfb_an1024_unpaired"),   # k_pfb_an1024<4, 16, false>: the unpaired 8-byte loads
])
# firpfbch synthesizer (M, p, S, mode, route), crcf
PFB_SYN = _rows("pfb", False, "crcf", [
    (10, 5, 1, None, "pfb_fft+syn_elem"),     # batched direct DFT + k_pfb_syn_out (per element)
    (64, 8, 64, None, "pfb_syn_small"),       # k_pfb_syn_small: runs of 64 blocks
    (256, 4, 64, None, "pfb_syn_fused"),      # k_pfb_syn_fused
    (1024, 4, 32, None, "pfb_syn1024"),       # k_pfb_syn1024<4>: 2 groups of 16 blocks
    (1024, 8, 32, None, "pfb_syn1024"),       # k_pfb_syn1024<8>
    (4096, 4, 33, None, "pfb_syn4096"),       # k_pfb_syn4096: runs of 33 blocks
    # calls of 16 blocks are one group in one workgroup (the query's run is the
    # workgroup's reach, 2 groups): the seams are the calls', S = 16
    (1024, 4, 16, "few", "pfb_syn1024"),      # k_pfb_syn1024<4>; under 3 blocks the two-pass form
    (1024, 8, 16, "few", "pfb_syn1024"),      # k_pfb_syn1024<8>; under 7 blocks batched transform + k_pfb_syn_out_run<8>
    (2048, 4, 64, None, "pfb_fft+syn_run"),   # batched transform + k_pfb_syn_out_run<4, float>: a lane runs 64 blocks
])
# firpfbch with complex taps: the same kernels with float2 coefficients; M = 1024
# has no fast form for them (k_pfb_an_X_run / k_pfb_syn_out_run<4, float2>)
PFB_CCCF = (_rows("pfb", True, "cccf", [(64, 4, 32, None, "pfb_an_small_c"), (256, 4, 32, None, "pfb_an_fused_c"),
                                        (4096, 4, 32, None, "pfb_an4096_c")])
            + _rows("pfb", False, "cccf", [(64, 4, 64, None, "pfb_syn_small_c"), (256, 4, 64, None, "pfb_syn_fused_c"),
                                           (4096, 4, 33, None, "pfb_syn4096_c")])
            + _rows("pfb", True, "cccf", [(1024, 4, 64, None, "pfb_an_run+fft_c"), (10, 5, 1, None, "pfb_an_elem+fft_c")])
            + _rows("pfb", False, "cccf", [(1024, 4, 64, None, "pfb_fft+syn_run_c"),
                                           (10, 5, 1, None, "pfb_fft+syn_elem_c")]))
ROWS = PFB2_AN + PFB2_SYN + PFB_AN + PFB_SYN + PFB_CCCF

# Pieces too short for a row's kernel go down the ladder: {route: (pieces of
# fewer blocks than this, the route they take)}; `_c' routes as their real one.
SHORT = {
    "pfb2_syn1024": (lambda r: 4 * r.q - 1, "pfb2_two_pass_run"),     # the state is 4m - 1 transforms
    "pfb2_syn4096": (lambda r: 4 * r.q - 1, "pfb2_two_pass_run"),
    "pfb2_syn_fused": (lambda r: 16, "pfb2_two_pass_run"),            # one group of 16 blocks
    "pfb_syn1024": (lambda r: r.q - 1, "pfb_fft+syn_run"),            # the state is p - 1 transforms
    "pfb_syn4096": (lambda r: r.q, "pfb_fft+syn_run"),
    "pfb_syn_fused": (lambda r: r.q, "pfb_fft+syn_run"),
    "pfb_syn_small": (lambda r: r.q, "pfb_fft+syn_run"),
}
COPYOUT_MAX = 64 << 10      # liquid_mi355x_copyout_max(): the host calls' pinned completion buffer


def piece_route(r, n, host):
    """The route a call of n blocks of row r's object takes; host: through
    execute_block on host pointers.  The M = 1024 analyzers send calls of at
    most 16 blocks to the few-block kernel, which also raises the completion
    flag of a host call whose output fits COPYOUT_MAX."""
    c = "_c" if r.route.endswith("_c") else ""
    base = r.route[:len(r.route) - len(c)]
    if base in SHORT:
        below, other = SHORT[base]
        return other + c if n < below(r) else r.route
    for fam in ("pfb2_an1024", "pfb_an1024"):
        if base.startswith(fam) and n <= 16:
            return fam + ("_few_signal" if host and n * r.M * 8 <= COPYOUT_MAX else "_few")
    return r.route


def ways(r):
    """How the GPU tests run a row: (name, cuts in blocks, host pointers)."""
    few = few_cuts(r) if r.mode == "few" else []
    if r.mode == "unaligned":
        return [("device", few, False), ("device-ragged", cuts(r), False)]
    return [("one-call", few, True), ("ragged", cuts(r), True), ("device", few, False)]


def pieces(r, at):
    """(first block, blocks) of each call for cuts `at'."""
    e = [0] + list(at) + [n_blocks(r)]
    return list(zip(e[:-1], np.diff(e).tolist()))


def row_id(r):
    return "%s-%s-%s-M%d-%s%d%s%s" % (r.kind, "an" if r.an else "syn", r.t, r.M, "m" if r.kind == "pfb2" else "p", r.q,
                                      "-" + r.mode if r.mode else "", "-S%d-nb%d" % (r.S, r.nb) if r.nb else "")


def window_blocks(r):
    """2m (firpfbch2) or p (firpfbch): the length of the stretch `as long as
    the window'; the stream runs to 3S + 2 * 2 * this + 5 blocks."""
    return 2 * r.q if r.kind == "pfb2" else r.q


def n_blocks(r):
    return r.nb or 3 * r.S + 4 * window_blocks(r) + 5


def nin(r):
    return r.M // 2 if r.kind == "pfb2" and r.an else r.M


def nout(r):
    return r.M // 2 if r.kind == "pfb2" and not r.an else r.M


def lg(M):
    return max(1, math.ceil(math.log2(M)))


# ------------------------------------------------------------------ envelopes
def stretches(S, wl, nb, analyzer):
    """The full-level stretches as {name: (lo, hi)} in blocks.  Fixed: the
    first block, one ending with the last sample before block S, one beginning
    at block S + 1, one straddling block 2S by a block either side, the last
    block.  The others each go to the middle of the largest stretch still
    free, in this order: `window' (wl blocks), `single' (one block far from
    anything) and, for analyzers, `mid' (begins and ends mid-block) and
    `sample' (one sample in the middle of a block)."""
    out = {}
    for name, (a, b) in (("first", (0, 1)), ("before", (S - 2, S)), ("after", (S + 1, S + 3)),
                         ("straddle", (2 * S - 1, 2 * S + 2)), ("last", (nb - 1, nb))):
        a, b = max(a, 0), min(b, nb)
        assert b > a, (name, S, nb)
        out[name] = (a, b)
    for name, w in [("window", wl), ("single", 1)] + ([("mid", 2), ("sample", 1)] if analyzer else []):
        free = np.ones(nb, np.int8)
        for a, b in out.values():
            free[a:b] = 0
        d = np.diff(np.concatenate(([0], free, [0])))
        a, b = max(zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)), key=lambda ab: ab[1] - ab[0])
        assert b - a >= w + 2, "no room for the %s stretch (S %d, wl %d)" % (name, S, wl)
        lo = int(a + (b - a - w) // 2)
        out[name] = (lo, lo + w)
    return out


def envelope(name, r):
    """Per input sample (analyzers) or per input frame (synthesizers), as one
    value per input sample either way; full level 1, floor 1e-5 (burst) or
    exactly 0 (gaps)."""
    nb, n = n_blocks(r), nin(r)
    e = np.full(nb * n, FLOOR[name])
    for k, (a, b) in stretches(r.S, window_blocks(r), nb, r.an).items():
        if k == "mid":       # from the middle of its first block to three quarters of its second
            lo = a * n + n // 2
            e[lo:max(lo + 1, a * n + n + 3 * n // 4)] = 1.0
        elif k == "sample":
            e[a * n + n // 2] = 1.0
        else:
            e[a * n:b * n] = 1.0
    return e


def cuts(r):
    """Way (b): ragged calls that start on both block parities; one cut falls
    right after the `window' stretch, and the call that follows is quiet for
    as long as the stream around it is.  Rows of mode `few': calls of at most
    16 blocks."""
    nb, wl = n_blocks(r), window_blocks(r)
    s = stretches(r.S, wl, nb, r.an)
    wend = s["window"][1]
    quiet = min([a for a, _ in s.values() if a >= wend] + [wend + 2 * wl + 1])   # the next call ends here
    if r.mode == "few":
        c, k, sizes = set([wend]), 0, (16, 7, 16, 1, 12, 15)
        b = 0
        while b < nb:
            c.add(b)
            b += sizes[k % len(sizes)]
            k += 1
    else:
        c = {3, wend, quiet, quiet + (r.S | 1)}
    return sorted(b for b in c if 0 < b < nb)


def few_cuts(r):
    """Way (a) and (c) of a `few' row: calls of 16 blocks."""
    return list(range(16, n_blocks(r), 16))


# ------------------------------------------------------------------ taps, signals
def taps(r):
    """firpfbch2: a float32 windowed sinc of 2Mm + 1 taps, cutoff 1/M
    (analyzer) or 0.5/M, scaled to sum M.  firpfbch: Mp taps uniform in
    [-0.5, 0.5) per component."""
    if r.kind == "pfb2":
        n = 2 * r.M * r.q + 1
        fc = (1.0 if r.an else 0.5) / r.M
        h = np.sinc(2.0 * fc * (np.arange(n) - r.M * r.q)) * np.hamming(n)
        return (h * (r.M / np.sum(h))).astype(np.float32)
    g = np.random.default_rng(zlib.crc32(("taps " + row_id(r)).encode()))
    n = r.M * r.q
    if r.t == "cccf":
        return (g.uniform(-0.5, 0.5, n) + 1j * g.uniform(-0.5, 0.5, n)).astype(np.complex64)
    return g.uniform(-0.5, 0.5, n).astype(np.float32)


def signal(r, name):
    g = np.random.default_rng(zlib.crc32(("%s %s" % (row_id(r), name)).encode()))
    e = envelope(name, r)
    return ((g.uniform(-0.5, 0.5, len(e)) + 1j * g.uniform(-0.5, 0.5, len(e))) * e).astype(np.complex64)


# ------------------------------------------------------------------ float64 models
def _H(h, M, L):
    wide = np.complex128 if np.iscomplexobj(h) else np.float64
    return np.ascontiguousarray(h[:M * L].astype(wide).reshape(L, M).T)   # H[i, n] = h[i + nM]


def _lag(A, k):
    """A[f - k] along the first axis, zero before the stream."""
    if k == 0:
        return A
    B = np.zeros_like(A)
    if k < len(A):
        B[k:] = A[:len(A) - k]
    return B


def pfb2_analyzer_model(h, x, M, m):
    L, M2 = 2 * m, M // 2
    nb = len(x) // M2
    H = _H(h, M, L)
    Hj = (H, np.roll(H, M2, axis=0))       # row j: H[(j - f M/2) mod M]
    aHj = (np.abs(Hj[0]), np.abs(Hj[1]))
    xr = x.astype(np.complex128).reshape(nb, M2)
    W = np.zeros((M, L), np.complex128)
    X = np.empty((nb, M), np.complex128)
    an = np.empty(nb)
    for b in range(nb):
        f = b & 1
        rows = slice(M2, M) if f else slice(0, M2)     # j = base - 1 - i
        W[rows, 1:] = W[rows, :-1].copy()
        W[rows, 0] = xr[b, ::-1]
        X[b] = np.sum(Hj[f] * W, axis=1)
        an[b] = np.linalg.norm(np.sum(aHj[f] * np.abs(W), axis=1))
    K = 0.71 * L + 4 * lg(M) + 8
    bound = np.repeat((K * EPS / math.sqrt(M)) * an, M).reshape(nb, M)
    return np.fft.ifft(X, axis=1), bound


def pfb_analyzer_model(h, x, M, p):
    nb = len(x) // M
    H = _H(h, M, p)
    T = 2 * p if np.iscomplexobj(h) else p
    xw = x.astype(np.complex128).reshape(nb, M)[:, ::-1]    # window i takes x[bM + M - 1 - i]
    v = np.zeros((nb, M), np.complex128)
    a = np.zeros((nb, M))
    for n in range(p):
        v += H[:, n] * _lag(xw, n)
        a += np.abs(H[:, n]) * np.abs(_lag(xw, n))
    K = 0.71 * T + 4 * lg(M) + 8
    bound = np.repeat((K * EPS * math.sqrt(M)) * np.linalg.norm(a, axis=1), M).reshape(nb, M)
    return np.fft.fft(v[:, ::-1], axis=1), bound


def pfb_synthesizer_model(h, X, M, p):
    nb = len(X) // M
    H = _H(h, M, p)
    T = 2 * p if np.iscomplexobj(h) else p
    z = np.fft.ifft(X.astype(np.complex128).reshape(nb, M), axis=1) * M
    Z = np.repeat(np.linalg.norm(z, axis=1), M).reshape(nb, M)
    y = np.zeros((nb, M), np.complex128)
    bz = np.zeros((nb, M))
    bw = np.zeros((nb, M))
    for n in range(p):
        y += H[:, n] * _lag(z, n)
        bz += np.abs(H[:, n]) * _lag(Z, n)
        bw += np.abs(H[:, n]) * np.abs(_lag(z, n))
    return y, EPS * (4 * lg(M) * bz + (0.71 * T + 8) * bw)


def pfb2_synthesizer_model(h, X, M, m):
    L, M2 = 2 * m, M // 2
    nb = len(X) // M
    H = _H(h, M, L)
    z = np.fft.ifft(X.astype(np.complex128).reshape(nb, M), axis=1) * M2
    Zn = np.linalg.norm(z, axis=1)
    y = np.zeros((nb, M2), np.complex128)
    bound = np.zeros((nb, M2))
    odd = (np.arange(nb) & 1).astype(bool)
    for f in (0, 1):                        # the frames of parity f read columns c = i + f M/2
        zc = z[:, f * M2:(f + 1) * M2]
        Zc = np.repeat(Zn, M2).reshape(nb, M2)
        yy = np.zeros((nb, M2), np.complex128)
        bz = np.zeros((nb, M2))
        bw = np.zeros((nb, M2))
        for n in range(L):
            for Hn, k in ((H[:M2, n], 2 * n), (H[M2:, n], 2 * n + 1)):
                yy += Hn * _lag(zc, k)
                bz += np.abs(Hn) * _lag(Zc, k)
                bw += np.abs(Hn) * np.abs(_lag(zc, k))
        sel = odd if f else ~odd
        y[sel] = yy[sel]
        bound[sel] = (EPS * (4 * lg(M) * bz + (0.71 * 4 * m + 8) * bw))[sel]
    return y, bound


def model(r, h, x):
    fn = {("pfb2", True): pfb2_analyzer_model, ("pfb2", False): pfb2_synthesizer_model,
          ("pfb", True): pfb_analyzer_model, ("pfb", False): pfb_synthesizer_model}[(r.kind, r.an)]
    y64, bound = fn(h, x, r.M, r.q)
    return y64.reshape(-1), bound.reshape(-1)


# ------------------------------------------------------------------ the oracle
def oracle_run(r, h, x, at=()):
    """The CPU oracle on the stream, one call per piece (`at' in blocks).
    Complex taps: the oracle has real ones, and the channelizer is linear in
    them, so the two runs on the real and the imaginary taps are combined."""
    import oracle_lib as O

    typ = O.ANALYZER if r.an else O.SYNTHESIZER
    if r.kind == "pfb2":
        o = O.FirPfbch2(typ, r.M, r.q, h=h)
        return np.concatenate([o.execute_block(p) for p in np.split(x, [b * nin(r) for b in at])])
    if r.t == "cccf":
        re = oracle_run(r._replace(t="crcf"), np.ascontiguousarray(h.real), x)
        im = oracle_run(r._replace(t="crcf"), np.ascontiguousarray(h.imag), x)
        return (re + 1j * im).astype(np.complex64)
    o = O.FirPfbch(typ, r.M, p=r.q, h=h)
    return np.concatenate([o.execute(b) for b in x.reshape(-1, r.M)])


# ------------------------------------------------------------------ cases
class Case:
    def __init__(self, r, name):
        self.r, self.name = r, name
        self.h, self.x = taps(r), signal(r, name)
        self.y64, self.bound = model(r, self.h, self.x)
        self.nb = n_blocks(r)
        assert len(self.x) == self.nb * nin(r) and len(self.y64) == self.nb * nout(r)
        for a in (self.h, self.x, self.y64, self.bound):   # shared among tests: left unchanged
            a.setflags(write=False)
        self._oracle = None

    def oracle(self):
        """(output, report) of the oracle in one call, computed once."""
        if self._oracle is None:
            y = oracle_run(self.r, self.h, self.x)
            y.setflags(write=False)
            self._oracle = (y, report(y, self.y64, self.bound))
        return self._oracle

    def frame_level(self):
        """The largest bound of each output frame."""
        return self.bound.reshape(self.nb, -1).max(axis=1)

    def check(self, y, what=""):
        return check("%s %s %s" % (row_id(self.r), self.name, what), y, self.y64, self.bound)


@functools.lru_cache(maxsize=None)
def case(r, name):
    return Case(r, name)


# ------------------------------------------------------------------ the checker
def report(y, y64, bound):
    """Worst ratio to the bound and its index, the number of failing outputs,
    of outputs that must be zero but are not, and of non-finite ones."""
    y = np.asarray(y)
    assert y.shape == y64.shape == bound.shape, (y.shape, y64.shape, bound.shape)
    finite = np.isfinite(y)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(y.astype(np.complex128) - y64)
    err[~finite] = np.inf
    zero = bound == 0
    ok = np.where(zero, y == 0, err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(zero, np.where(y == 0, 0.0, np.inf), err / bound)
    worst = int(np.argmax(ratio))
    return {"worst": float(ratio[worst]), "index": worst, "failing": int(np.count_nonzero(~ok)),
            "nonzero_zeros": int(np.count_nonzero(zero & (y != 0))),
            "nonfinite": int(np.count_nonzero(~finite)), "n": int(len(y)), "zeros": int(np.count_nonzero(zero))}


def check(label, y, y64, bound):
    r = report(y, y64, bound)
    print("pfb_bound %s: worst %.4g of the bound at %d, %d of %d fail, %d nonzero zeros (of %d), %d non-finite"
          % (label, r["worst"], r["index"], r["failing"], r["n"], r["nonzero_zeros"], r["zeros"], r["nonfinite"]))
    assert r["failing"] == 0 and r["nonfinite"] == 0, (
        "%s: worst error %.4g x the bound at output %d; %d of %d outputs fail; %d outputs that must be zero "
        "are not; %d non-finite" % (label, r["worst"], r["index"], r["failing"], r["n"], r["nonzero_zeros"],
                                    r["nonfinite"]))
    return r
