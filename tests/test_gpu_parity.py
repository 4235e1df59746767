"""GPU parity: the HIP path (through the C-ABI) against the reference's golden
vectors and the CPU oracle.  Runs on the MI355X box (`pytest -m gpu`).

Tolerances:
  * golden vectors: the reference runner's own absolute tolerance (1e-3 for
    firfilt/firdecim/fftfilt data files, 1e-6..1e-3 for the known answers);
  * oracle comparisons: normwise max|y_gpu - y_oracle| / max|y_oracle|
    <= NRM = 1e-5 (BASELINE north star "1e-5 relative float error",
    normwise per SURVEY 7.4.7: per-sample relative error is not attainable
    even by the reference itself).
"""
import os
import subprocess

import numpy as np
import pytest

import golden_io as G
import liquidmi as LQ
import oracle_lib as O

pytestmark = pytest.mark.gpu

NRM = 1e-5
TYPES = {"rrrf": O.RRRF, "crcf": O.CRCF, "cccf": O.CCCF}


def rng(seed):
    return np.random.default_rng(seed)


def cx(r, n):
    return (r.uniform(-0.5, 0.5, n) + 1j * r.uniform(-0.5, 0.5, n)).astype(np.complex64)


def samples(r, t, n):
    return r.uniform(-0.5, 0.5, n).astype(np.float32) if t == "rrrf" else cx(r, n)


def coefs(r, t, n):
    return cx(r, n) if t == "cccf" else r.uniform(-0.5, 0.5, n).astype(np.float32)


# ============================================================== golden vectors
@pytest.mark.parametrize("case", G.load("firfilt"), ids=lambda c: c["name"])
def test_firfilt_golden(case):
    h, x, y = G.arr(case["h"]), G.arr(case["x"]), G.arr(case["y"])
    q = LQ.FirFilt(case["type"], h)
    out = []
    for v in x:                       # firfilt_runtest.c:68-95: push + execute
        q.push(v)
        out.append(q.execute())
    assert np.max(np.abs(np.asarray(out) - y)) < case["tol"]
    q2 = LQ.FirFilt(case["type"], h)
    assert np.max(np.abs(q2.execute_block(x) - y)) < case["tol"]


@pytest.mark.parametrize("case", G.load("firdecim"), ids=lambda c: c["name"])
def test_firdecim_golden(case):
    h, x, y = G.arr(case["h"]), G.arr(case["x"]), G.arr(case["y"])
    q = LQ.FirDecim(case["M"], h, t=case["type"])
    out = np.array([q.execute(x[i * case["M"]:(i + 1) * case["M"]]) for i in range(len(y))])
    assert np.max(np.abs(out - y)) < case["tol"]


def _nextpow2(x):
    n, x = 0, x - 1
    while x > 0:
        x >>= 1
        n += 1
    return n


@pytest.mark.parametrize("case", G.load("fftfilt"), ids=lambda c: c["name"])
def test_fftfilt_golden(case):
    h, x, y = G.arr(case["h"]), G.arr(case["x"]), G.arr(case["y"])
    n = 1 << _nextpow2(len(h) - 1)
    nb = -(-len(x) // n)
    xp = np.zeros(nb * n, np.float32 if case["type"] == "rrrf" else np.complex64)
    xp[: len(x)] = x
    q = LQ.FftFilt(h, n, t=case["type"])
    out = np.concatenate([q.execute(xp[b * n:(b + 1) * n]) for b in range(nb)])
    assert np.max(np.abs(out[: len(y)] - y)) < case["tol"]


KA = G.load("known_answers")


@pytest.mark.parametrize("name", [k for k in KA if k.startswith("autotest_dotprod") and "basic" not in k])
def test_dotprod_known_answer(name):
    c = KA[name]
    h, x = G.arr(c["h"]), G.arr(c["x"])
    y = LQ.dotprod_run(c["type"], h, x)
    assert abs(complex(y) - G.scalar(c["y"])) < c["tol"] * 1.5
    q = LQ.DotProd(c["type"], h)
    assert abs(complex(q.execute(x)) - G.scalar(c["y"])) < c["tol"] * 1.5


def test_dotprod_rrrf_basic():
    c = KA["autotest_dotprod_rrrf_basic"]
    q = LQ.DotProd("rrrf", G.arr(c["h"]))
    for case in c["cases"]:
        assert abs(q.execute(G.arr(case["x"])) - case["y"]) < c["tol"]


def test_firinterp_known_answer():
    c = KA["autotest_firinterp_crcf_generic"]
    q = LQ.FirInterp(c["M"], G.arr(c["h"]))
    y = np.concatenate([q.execute(v) for v in G.arr(c["x"])])
    assert np.max(np.abs(y - G.arr(c["y"]))) < 4e-6


# ============================================================== oracle parity
@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("hlen", [1, 7, 16, 33, 64, 100, 300])
def test_firfilt_stream_vs_oracle(t, hlen):
    r = rng(hlen)
    h = coefs(r, t, hlen)
    x = samples(r, t, 30000)
    g = LQ.FirFilt(t, h)
    o = O.FirFilt(TYPES[t], h)
    s = (0.7 - 0.2j) if t == "cccf" else 0.7
    g.set_scale(s)
    o.set_scale(s)
    # ragged call sizes, including 1-sample and sub-halo calls, in-place block
    cuts = [0, 1, 2, 50, 4095, 4096, 9000, 9001, 20000, 30000]
    outs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        outs.append(g.execute_block(x[a:b]))
    y = np.concatenate(outs)
    ref = o.execute_block(x)
    assert G.nrm_err(y, ref) < NRM


def test_firfilt_crcf_baseline_config1_vs_oracle():
    # BASELINE config 1: h = 64, 1M complex samples, one execute_block
    r = rng(11)
    h = r.uniform(-0.5, 0.5, 64).astype(np.float32)
    x = cx(r, 1 << 20)
    y = LQ.FirFilt("crcf", h).execute_block(x)
    ref = O.FirFilt(O.CRCF, h).execute_block(x)
    assert G.nrm_err(y, ref) < NRM


def test_firfilt_mixed_push_execute_block_and_reset():
    r = rng(12)
    h = r.uniform(-0.5, 0.5, 40).astype(np.float32)
    x = cx(r, 3000)
    g, o = LQ.FirFilt("crcf", h), O.FirFilt(O.CRCF, h)
    for rep in range(2):
        ya = [g.execute_block(x[:100])]
        for v in x[100:130]:
            g.push(v)
            ya.append(np.array([g.execute()]))
        ya.append(g.execute_block(x[130:]))
        ref = o.execute_block(x)
        assert G.nrm_err(np.concatenate(ya), ref) < NRM
        g.reset()
        o.reset()


def test_firfilt_device_path_in_place():
    r = rng(13)
    h = r.uniform(-0.5, 0.5, 64).astype(np.float32)
    x = cx(r, 200000)
    g = LQ.FirFilt("crcf", h)
    buf = LQ.DeviceBuffer.from_array(x)
    g.execute_block_dev(buf.p, 120000, buf.p)            # in place, then a second call
    g.execute_block_dev(buf.p + 120000 * 8, 80000, buf.p + 120000 * 8)
    g.synchronize()
    y = buf.to_array(np.complex64, len(x))
    ref = O.FirFilt(O.CRCF, h).execute_block(x)
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("hlen", [33, 45, 64, 65, 100, 128, 129, 192, 193, 256])
def test_firfilt_crcf_matrix_core_path_long_stream(t, hlen):
    # h in 33..64 (every type), 65..128 (crcf: two 64-tap blocks, a
    # 128-sample halo) and 129..256 (crcf: three / four blocks, the A
    # fragments read from LDS), device pointers, not in place: the MFMA kernel
    # (k_firfilt_mx.hip; rrrf / cccf past 64 taps: the VALU kernel).  Several 2048-output chunks per workgroup, a ragged
    # tail, a second call continuing the stream, and a complex scale.  Held to
    # the oracle at the usual bound and to a float64 convolution at 2e-6 (the
    # three-term bf16 split is float32-accurate, not bf16-accurate).
    r = rng(100 + hlen)
    h = coefs(r, t, hlen)
    # every length and call size runs the direct kernels (firfilt has no
    # transform form; tests/test_gpu_fir_bound.py): a short first call, a
    # long one continuing it and an unaligned tail
    n0, n1, n2 = 6000, (3 << 20) + 12345, 777
    x = samples(r, t, n0 + n1 + n2)
    esz = x.itemsize
    g = LQ.FirFilt(t, h)
    s = (0.7 - 0.2j) if t == "cccf" else 0.7
    g.set_scale(s)
    bx = LQ.DeviceBuffer.from_array(x)
    by = LQ.DeviceBuffer(x.nbytes)
    g.execute_block_dev(bx.p, n0, by.p)
    g.execute_block_dev(bx.p + n0 * esz, n1, by.p + n0 * esz)
    g.execute_block_dev(bx.p + (n0 + n1) * esz, n2, by.p + (n0 + n1) * esz)   # 4- or 8-byte aligned: VALU kernel
    g.synchronize()
    y = by.to_array(x.dtype, len(x))
    o = O.FirFilt(TYPES[t], h)
    o.set_scale(s)
    ref = o.execute_block(x)
    assert G.nrm_err(y, ref) < NRM
    ref64 = s * np.convolve(x.astype(np.complex128), h.astype(np.complex128))[: len(x)]
    if t == "rrrf":
        ref64 = ref64.real
    assert G.nrm_err(y, ref64) < 2e-6


def test_firfilt_crcf_unaligned_device_pointers():
    # 8-byte aligned (not 16) device pointers take the VALU kernel
    r = rng(14)
    h = r.uniform(-0.5, 0.5, 64).astype(np.float32)
    x = cx(r, 100001)
    g = LQ.FirFilt("crcf", h)
    bx = LQ.DeviceBuffer.from_array(np.concatenate([x[:1], x]))
    by = LQ.DeviceBuffer(x.nbytes + 8)
    g.execute_block_dev(bx.p + 8, len(x), by.p + 8)
    g.synchronize()
    y = by.to_array(np.complex64, len(x) + 1)[1:]
    ref = O.FirFilt(O.CRCF, h).execute_block(x)
    assert G.nrm_err(y, ref) < NRM


def test_firfilt_kaiser_design_matches_oracle():
    g = LQ.firdes_kaiser(65, 0.2, 60.0, 0.1)
    o = O.firdes_kaiser(65, 0.2, 60.0, 0.1)
    assert np.max(np.abs(g - o)) <= 1e-7


@pytest.mark.parametrize("n", [16, 64, 256, 1024, 7, 33])
@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
def test_dotprod_batch_vs_oracle(t, n):
    r = rng(n)
    h = coefs(r, t, n)
    X = samples(r, t, 4096 * n)
    Y = LQ.DotProd(t, h).execute_batch(X)
    ref = O.dotprod_batch(TYPES[t], h, X)
    assert G.nrm_err(Y, ref) < NRM


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("M,m", [(2, 2), (4, 3), (8, 5), (8, 8), (16, 4), (64, 4)])
def test_firdecim_vs_oracle(M, m, t):
    r = rng(M)
    x = samples(r, t, M * 5000)
    if t == "cccf":   # complex taps
        h = coefs(r, t, 2 * M * m)
        g, o = LQ.FirDecim(M, h, t=t), O.FirDecim(O.CCCF, M, h)
    else:
        g, o = LQ.FirDecim(M, m=m, As=60.0, t=t), O.FirDecim(TYPES[t], M, m=m, As=60.0)
    y = np.concatenate([g.execute_block(x[: M * 1234]), g.execute_block(x[M * 1234:])])
    assert G.nrm_err(y, o.execute_block(x)) < NRM


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("M,hlen", [(1, 7), (3, 29), (2, 80), (5, 333), (7, 8), (200, 801), (8, 2)])
def test_firdecim_ragged_vs_oracle(M, hlen, t):
    """arbitrary taps (hlen not a multiple of M, long filters split in tap
    chunks, one-tap-per-phase filters, decimation factors whose tile exceeds
    the fast kernel's LDS shape) over block sizes that are not tile multiples"""
    r = rng(M * 7 + hlen)
    x = samples(r, t, M * 3001)
    h = coefs(r, t, hlen)
    g, o = LQ.FirDecim(M, h, t=t), O.FirDecim(TYPES[t], M, h)
    cuts = [0, 1, 517, 2048 + 3, 3001]
    y = np.concatenate([g.execute_block(x[M * a: M * b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert G.nrm_err(y, o.execute_block(x)) < NRM


@pytest.mark.parametrize("t", ["rrrf", "crcf"])
def test_firdecim_device_path_unaligned(t):
    """device pointers that are not 16-byte aligned (the staging loop's
    vector loads must not be taken)"""
    M, r = 4, rng(77)
    x = samples(r, t, M * 70001 + 1)
    h = coefs(r, t, 37)
    esz = 4 if t == "rrrf" else 8
    g = LQ.FirDecim(M, h, t=t)
    fn = getattr(LQ.lib(), "firdecim_%s_execute_block_dev" % t)
    bx = LQ.DeviceBuffer.from_array(x)
    by = LQ.DeviceBuffer((70000 + 1) * esz)
    fn(g.q, bx.p + esz, 30001, by.p + esz)
    fn(g.q, bx.p + esz + 30001 * M * esz, 39999, by.p + esz + 30001 * esz)
    LQ.lib().liquid_mi355x_device_synchronize()
    y = by.to_array(np.float32 if t == "rrrf" else np.complex64, 70001)[1:]
    ref = O.FirDecim(TYPES[t], M, h).execute_block(x[1:])[:70000]
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
# M = 4, m = 7, 9, 11, 15: 2m + 1 taps per phase, the register-window kernel's
# 16-, 20-, 24- and 32-tap classes (the rows before reach 8 and 12); m = 16:
# 33 per phase, real taps on the plain kernel
@pytest.mark.parametrize("M,m", [(2, 3), (4, 3), (8, 5), (32, 2), (4, 7), (4, 9), (4, 11), (4, 15), (4, 16)])
def test_firinterp_vs_oracle(M, m, t):
    r = rng(M + 1)
    x = samples(r, t, 5000)
    if t == "cccf":
        h = coefs(r, t, 2 * M * m - 3)     # ragged length: zero-padded to M*L
        g, o = LQ.FirInterp(M, h, t=t), O.FirInterp(O.CCCF, M, h)
    else:
        g, o = LQ.FirInterp(M, m=m, As=60.0, t=t), O.FirInterp(TYPES[t], M, m=m, As=60.0)
    y = np.concatenate([g.execute_block(x[:777])] + [g.execute(v) for v in x[777:780]] + [g.execute_block(x[780:])])
    assert G.nrm_err(y, o.execute_block(x)) < NRM


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("hlen,n", [(4, 4), (23, 32), (512, 2048), (2049, 2048), (2050, 2100), (4097, 4096),
                                    (4098, 4097)])
def test_fftfilt_vs_oracle(hlen, n, t):
    r = rng(hlen)
    h = coefs(r, t, hlen)
    nb = 40 if n <= 32 else 12
    x = samples(r, t, n * nb)
    g, o = LQ.FftFilt(h, n, t=t), O.FftFilt(TYPES[t], h, n)
    s = (1.5 - 0.25j) if t == "cccf" else 1.5
    g.set_scale(s)            # linear: the oracle runs at unit scale and the reference is scaled after
    y = np.concatenate([g.execute(x[b * n:(b + 1) * n]) for b in range(nb)])
    assert G.nrm_err(y, s * o.execute_stream(x)) < NRM


def test_fftfilt_long_stream_block_extension():
    # BASELINE config 3 geometry (h=512, n=2048) on a 1M-sample stream, ragged calls
    r = rng(21)
    h = r.uniform(-0.5, 0.5, 512).astype(np.float32)
    x = cx(r, 1 << 20)
    g = LQ.FftFilt(h, 2048)
    y = np.concatenate([g.execute_block(x[:333333]), g.execute_block(x[333333:])])
    ref = O.FftFilt(O.CRCF, h, 2048).execute_stream(x)
    assert G.nrm_err(y, ref) < NRM


# (4, 1) and the m = 9 cases: k_pfb2_an<M> for M = 4 and for every power of two
# M >= 64 (m > 8 is past the polyphase pass's tap counts)
@pytest.mark.parametrize("M,m", [(2, 1), (8, 2), (12, 3), (64, 4), (256, 2), (1024, 4), (4096, 2),
                                 (4, 1), (64, 9), (128, 9), (256, 9), (512, 9), (1024, 9), (2048, 9), (4096, 9)])
def test_firpfbch2_analyzer_vs_oracle(M, m):
    r = rng(M + m)
    nblocks = 64 if M <= 1024 else 8
    x = cx(r, nblocks * M // 2)
    g = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0)
    o = O.FirPfbch2(O.ANALYZER, M, m, 60.0)
    # odd-sized calls so that calls start on both block parities
    cuts = [0, 1, 4, 5, 30, nblocks]
    step = M // 2
    y = np.concatenate([g.execute_block(x[a * step:b * step]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert G.nrm_err(y, o.execute_block(x)) < NRM


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("dev", [False, True])
def test_firpfbch2_m1024_few_block_calls(m, dev):
    # M = 1024: calls of at most 16 blocks take k_pfb2_an1024_few (the
    # per-call API's path; host-pointer calls of up to 8 blocks also raise
    # the completion flag from the kernel), longer ones the streaming kernel;
    # mixed on one object, both block parities, against the oracle
    M = 1024
    r = rng(400 + m + dev)
    sizes = [1, 1, 2, 3, 16, 17, 1, 5, 8, 9, 100, 1, 15, 2]
    nb = sum(sizes)
    x = cx(r, nb * M // 2)
    g = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0)
    o = O.FirPfbch2(O.ANALYZER, M, m, 60.0)
    ys, a = [], 0
    for k in sizes:
        xs = x[a * M // 2:(a + k) * M // 2]
        if dev:
            dx = LQ.DeviceBuffer.from_array(xs)
            dy = LQ.DeviceBuffer(k * M * 8)
            g.execute_block_dev(dx.p, k, dy.p)
            g.synchronize()
            ys.append(dy.to_array(np.complex64, k * M))
        else:
            ys.append(g.execute_block(xs))
        a += k
    assert G.nrm_err(np.concatenate(ys), o.execute_block(x)) < NRM


# the last five reach k_pfb2_poly<L> for L = 2m = 2, 6, 14 and, at M = 8192
# (no fused form, batched 8192-point transform), L = 4, 8
@pytest.mark.parametrize("M,m", [(64, 4), (128, 1), (256, 4), (512, 3), (1024, 5), (2048, 4), (4096, 6), (256, 8),
                                 (1024, 1), (1024, 3), (64, 7), (8192, 2), (8192, 4)])
def test_firpfbch2_analyzer_polyphase_pass_vs_oracle(M, m):
    # power-of-two M other than the fused M=1024/m=4 path: polyphase pass
    # (column slices x row runs with a warm-up of 2m-1 rows each) + batched
    # transform in place.  Enough blocks for many row runs per slice; ragged
    # calls start on both block parities.
    r = rng(7 * M + m)
    nblocks = max(64, (1 << 21) // M)
    x = cx(r, nblocks * M // 2)
    g = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0)
    o = O.FirPfbch2(O.ANALYZER, M, m, 60.0)
    cuts = [0, 1, 6, 7, nblocks // 2 + 1, nblocks]
    step = M // 2
    y = np.concatenate([g.execute_block(x[a * step:b * step]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert G.nrm_err(y, o.execute_block(x)) < NRM


@pytest.mark.parametrize("M,m", [(64, 1), (64, 2), (64, 3), (64, 4), (128, 2), (128, 4)])
def test_firpfbch2_analyzer_small_fused_vs_oracle(M, m):
    # M = 64 / 128 with m <= 4: the fused kernel (k_pfb2_an_small, several
    # column sets per workgroup, each on its own run of rows); enough blocks
    # for many workgroups and a ragged last run, calls on both block parities
    r = rng(11 * M + m)
    nblocks = (1 << 20) // M + 37
    x = cx(r, nblocks * M // 2)
    g = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0)
    o = O.FirPfbch2(O.ANALYZER, M, m, 60.0)
    cuts = [0, 3, 4, 1001, nblocks - 5, nblocks]
    step = M // 2
    y = np.concatenate([g.execute_block(x[a * step:b * step]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert G.nrm_err(y, o.execute_block(x)) < NRM


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_firpfbch2_analyzer_m2048_fused_vs_oracle(m):
    # M = 2048 with m <= 4: the fused kernel (k_pfb2_an2048, two columns per
    # lane, 4-row groups, register 2048-point transforms in the ring's own
    # buffers); many workgroup runs, a ragged last run, calls on both parities
    M = 2048
    r = rng(7 * M + m)
    nblocks = (1 << 22) // M + 29
    x = cx(r, nblocks * M // 2)
    g = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0)
    o = O.FirPfbch2(O.ANALYZER, M, m, 60.0)
    cuts = [0, 1, 4, 777, nblocks - 3, nblocks]
    step = M // 2
    y = np.concatenate([g.execute_block(x[a * step:b * step]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert G.nrm_err(y, o.execute_block(x)) < NRM


@pytest.mark.parametrize("M,m", [(2048, 2), (2048, 4), (256, 4), (512, 3), (64, 4), (128, 2)])
def test_firpfbch2_analyzer_short_extra_run(M, m):
    # M = 2048: 16 384 blocks + 2 (8 194 rows), 256 runs of 32 rows and one
    # extra run of 2 rows (launch_pfb2_an2048's balance rule); M = 256 / 512:
    # 65 536 blocks + 2, 1024 runs of 32 rows and one of 2 (launch_pfb2_an256);
    # M = 64 / 128: 131 072 blocks + 2 (sets of 40 rows: no extra run there)
    r = rng(11 * M + m)
    nblocks = {2048: 16384, 256: 65536, 512: 65536, 64: 131072, 128: 131072}[M] + 2
    x = cx(r, nblocks * M // 2)
    g = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0)
    o = O.FirPfbch2(O.ANALYZER, M, m, 60.0)
    cuts = [0, 1, nblocks]
    step = M // 2
    y = np.concatenate([g.execute_block(x[a * step:b * step]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert G.nrm_err(y, o.execute_block(x)) < NRM


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_firpfbch2_analyzer_m4096_fused_vs_oracle(m):
    # M = 4096 with m <= 4: the fused kernel (k_pfb2_an4096, four columns per
    # lane, one-row groups, quarter transforms + radix-4 combine, the oldest
    # ring row in LDS); many workgroup runs, a ragged last run, calls on both
    # block parities
    M = 4096
    r = rng(5 * M + m)
    nblocks = (1 << 22) // M + 41
    x = cx(r, nblocks * M // 2)
    g = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0)
    o = O.FirPfbch2(O.ANALYZER, M, m, 60.0)
    cuts = [0, 1, 4, 333, nblocks - 3, nblocks]
    step = M // 2
    y = np.concatenate([g.execute_block(x[a * step:b * step]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert G.nrm_err(y, o.execute_block(x)) < NRM


def test_firpfbch2_analyzer_polyphase_chunks_vs_oracle():
    # a call longer than one polyphase chunk (2^27 / M blocks): the second
    # chunk takes its history from the input before it; odd start parity
    M, m = 4096, 2
    r = rng(4097)
    nb = (1 << 27) // M + 301
    x = cx(r, (nb + 1) * M // 2)
    g = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0)
    o = O.FirPfbch2(O.ANALYZER, M, m, 60.0)
    y = np.concatenate([g.execute_block(x[:M // 2]), g.execute_block(x[M // 2:])])
    assert G.nrm_err(y, o.execute_block(x)) < NRM


@pytest.mark.parametrize("M,m", [(64, 4), (256, 4)])
def test_firpfbch2_analyzer_vs_downconverter_bank(M, m):
    """the GPU analyzer against the reference's down-converter equivalence
    built on the golden-pinned firfilt oracle (golden_io.firpfbch2_downconverter)"""
    r = rng(M * 3 + m)
    nblocks = 40
    x = cx(r, nblocks * M // 2)
    y = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0).execute_block(x).reshape(nblocks, M)
    h = O.firpfbch2_prototype(O.ANALYZER, M, m, 60.0)
    ref = G.firpfbch2_downconverter(x, h, M, m, nblocks, lambda hh, z: O.FirFilt(O.CRCF, hh).execute_block(z))
    assert G.nrm_err(y, ref) < NRM


PFB2_CHANS = [0, 1, 255, 511, 512, 513, 1023]


def test_firpfbch2_config4_vs_downconverter_bank():
    """BASELINE config 4 geometry (M = 1024, m = 4, Kaiser As = 60) on the
    fast kernel k_pfb2_an1024 against the reference's own equivalence method
    (sandbox/firpfbch2_analysis_equivalence_test.c:182-215: mix down, filter
    with the prototype, sample every M/2) built on the golden-pinned firfilt
    oracle, on a channel subset; 32 blocks from a zero state in two calls,
    the second starting at odd block parity"""
    M, m = 1024, 4
    r = rng(1024 * 4 + 1)
    chans = PFB2_CHANS + sorted(int(c) for c in r.choice(np.arange(2, 1023), 9, replace=False))
    nblocks = 32
    x = cx(r, nblocks * M // 2)
    g = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0)
    y = np.concatenate([g.execute_block(x[:7 * M // 2]), g.execute_block(x[7 * M // 2:])]).reshape(nblocks, M)
    h = O.firpfbch2_prototype(O.ANALYZER, M, m, 60.0)
    ref = G.firpfbch2_downconverter(x, h, M, m, nblocks, lambda hh, z: O.FirFilt(O.CRCF, hh).execute_block(z),
                                    channels=chans)
    assert G.nrm_err(y[:, chans], ref) < NRM


def test_firpfbch_analyzer_m1024_vs_downconverter_bank():
    """firpfbch_crcf_analyzer_autotest.c:30-146 (analyzer == mixer + firfilt,
    tol 1e-4) on the GPU's M = 1024, p = 8 fast kernel (random taps, as the
    reference allows), channel subset, two ragged calls"""
    r = rng(1024 + 8)
    M, p, ns = 1024, 8, 24
    chans = PFB2_CHANS + [100, 300, 700, 900, 1022]
    h = r.choice([-1.5, -0.5, 0.5, 1.5], M * p).astype(np.float32)
    x = (0.1 * np.sqrt(0.5) * (r.choice([-1.5, -0.5, 0.5, 1.5], M * ns)
                               + 1j * r.choice([-1.5, -0.5, 0.5, 1.5], M * ns))).astype(np.complex64)
    g = LQ.FirPfbch(LQ.LIQUID_ANALYZER, M, p=p, h=h)
    y = np.concatenate([g.execute_block(x[:5 * M]), g.execute_block(x[5 * M:])]).reshape(ns, M)
    ref = G.firpfbch_downconverter(x, h, M, ns, lambda hh, z: O.FirFilt(O.CRCF, hh).execute_block(z), chans)
    assert np.max(np.abs(y[:, chans] - ref)) < 1e-4


def test_firpfbch2_baseline_config4_slice_vs_oracle():
    # BASELINE config 4 geometry: M=1024, m=4, As=60, 2^20 samples (2048 blocks)
    r = rng(31)
    x = cx(r, 1 << 20)
    y = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, 1024, 4, 60.0).execute_block(x)
    ref = O.FirPfbch2(O.ANALYZER, 1024, 4, 60.0).execute_block(x)
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("M", [8, 16, 32, 64])
def test_firpfbch2_perfect_reconstruction_gpu(M):
    # the reference's own test: src/multichannel/tests/firpfbch2_crcf_autotest.c:28-98
    m = 5
    n = M * 8 * m
    s, p, gg = 1, 524287, 1031
    x = np.zeros(n, np.complex64)
    for i in range(n):
        s = (s * p) % gg
        x[i] = np.float32(s) / np.float32(gg) - np.float32(0.5)
    qa = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0)
    qs = LQ.FirPfbch2(LQ.LIQUID_SYNTHESIZER, M, m, 60.0)
    y = np.zeros(n, np.complex64)
    for i in range(0, n, M // 2):
        y[i:i + M // 2] = qs.execute(qa.execute(x[i:i + M // 2]))
    d = 2 * M * m - M // 2 + 1
    assert np.max(np.abs(y[:d])) < 1e-3
    assert np.max(np.abs(y[d:] - x[: n - d])) < 1e-3


# (8, 4): k_pfb2_syn_out_run<8>; (8, 1): the per-element k_pfb2_syn_out
@pytest.mark.parametrize("M,m", [(8, 2), (64, 3), (1024, 4), (8, 4), (8, 1)])
def test_firpfbch2_synthesizer_vs_oracle(M, m):
    r = rng(M * 3)
    nb = 40
    X = cx(r, nb * M)
    g = LQ.FirPfbch2(LQ.LIQUID_SYNTHESIZER, M, m, 60.0)
    o = O.FirPfbch2(O.SYNTHESIZER, M, m, 60.0)
    y = np.concatenate([g.execute_block(X[: 3 * M]), g.execute_block(X[3 * M:])])
    assert G.nrm_err(y, o.execute_block(X)) < NRM


@pytest.mark.parametrize("M,m", [(256, 4), (256, 1), (512, 3), (512, 2)])
def test_firpfbch2_synthesizer_m256_512_fused(M, m):
    # fused M = 256 / 512 synthesizer: many 64-block runs per call (each
    # warming up on the 16 blocks before it), an odd first call so later
    # calls start on the other block parity, state carried across calls
    r = rng(M + 5 * m)
    nb = 2000 if M == 256 else 1000
    X = cx(r, nb * M)
    g = LQ.FirPfbch2(LQ.LIQUID_SYNTHESIZER, M, m, 60.0)
    o = O.FirPfbch2(O.SYNTHESIZER, M, m, 60.0)
    cuts = [0, 17, 300, nb]
    y = np.concatenate([g.execute_block(X[a * M:b * M]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert G.nrm_err(y, o.execute_block(X)) < NRM


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_firpfbch2_synthesizer_m4096_fused(m):
    # k_pfb2_syn4096 (quarter transforms, radix-4 combine into the lane's
    # columns, L partial outputs per column): many runs per call (each
    # warming up on the blocks before it), an odd first call so the next
    # starts on the other block parity, a short call below 4m-1 blocks
    # (two-pass path) carrying the state between fused calls
    M = 4096
    r = rng(M + 7 * m)
    nb = 1200
    X = cx(r, nb * M)
    g = LQ.FirPfbch2(LQ.LIQUID_SYNTHESIZER, M, m, 60.0)
    o = O.FirPfbch2(O.SYNTHESIZER, M, m, 60.0)
    cuts = [0, 401, 402, nb]
    y = np.concatenate([g.execute_block(X[a * M:b * M]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert G.nrm_err(y, o.execute_block(X)) < NRM


@pytest.mark.parametrize("m", [4, 2])
def test_firpfbch2_synthesizer_m1024_many_workgroups(m):
    # k_pfb2_syn1024: 701 blocks over ~22 workgroups (history rebuilt from the
    # input), odd first call so the second call starts on the other parity,
    # then a short call below 4m-1 blocks (general path, shared state)
    M, nb = 1024, 701
    r = rng(60 + m)
    X = cx(r, (nb + 20 + 3) * M)
    g = LQ.FirPfbch2(LQ.LIQUID_SYNTHESIZER, M, m, 60.0)
    o = O.FirPfbch2(O.SYNTHESIZER, M, m, 60.0)
    y = np.concatenate([g.execute_block(X[: nb * M]), g.execute_block(X[nb * M:(nb + 20) * M]),
                        g.execute_block(X[(nb + 20) * M:])])
    assert G.nrm_err(y, o.execute_block(X)) < NRM


@pytest.mark.parametrize("typ", [LQ.LIQUID_ANALYZER, LQ.LIQUID_SYNTHESIZER])
# p = 2m.  M = 4: the run kernels' p = 2, 8, 10, 12, 14, 16; M = 256: the fused
# M = 256 / 512 kernels' p = 2, 10, 12, 14; M = 64: the fused M = 64 / 128
# kernels' p = 4, 10, 12, 14
@pytest.mark.parametrize("M,m", [(4, 2), (16, 3), (1024, 2), (6, 2),
                                 (4, 1), (4, 4), (4, 5), (4, 6), (4, 7), (4, 8),
                                 (256, 1), (256, 5), (256, 6), (256, 7),
                                 (64, 2), (64, 5), (64, 6), (64, 7)])
def test_firpfbch_vs_oracle(typ, M, m):
    r = rng(M + 7 * typ)
    nb = 30
    x = cx(r, nb * M)
    g = LQ.FirPfbch(typ, M, m=m, As=60.0)
    o = O.FirPfbch(typ, M, m=m, As=60.0)
    y = np.concatenate([g.execute(x[b * M:(b + 1) * M]) for b in range(3)] + [g.execute_block(x[3 * M:])])
    ref = np.concatenate([o.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("typ", [LQ.LIQUID_ANALYZER, LQ.LIQUID_SYNTHESIZER])
@pytest.mark.parametrize("M,m", [(256, 2), (256, 4), (512, 3), (512, 8)])
def test_firpfbch_m256_512_long_stream(typ, M, m):
    # the fused M = 256 / 512 analyzer (16-row groups, runs of rows per
    # workgroup with a 16-row warm-up) and the generic synthesizer over
    # thousands of blocks in ragged calls
    r = rng(M + 31 * m + typ)
    nb = (1 << 20) // M
    x = cx(r, nb * M)
    g = LQ.FirPfbch(typ, M, m=m, As=60.0)
    o = O.FirPfbch(typ, M, m=m, As=60.0)
    cuts = [0, 1, 778, nb]
    y = np.concatenate([g.execute_block(x[a * M:b * M]) for a, b in zip(cuts[:-1], cuts[1:])])
    ref = o.execute_block(x) if hasattr(o, "execute_block") else \
        np.concatenate([o.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("mode", ["host", "dev", "inplace"])
def test_firpfbch_m1024_few_block_calls(m, mode):
    # M = 1024 crcf: calls of at most 16 blocks take k_pfb_an1024_few (host
    # calls of up to 8 blocks raise the completion flag from the kernel),
    # longer ones the streaming kernel; mixed on one object against the
    # oracle, device calls also in place
    M = 1024
    r = rng(500 + m + len(mode))
    sizes = [1, 1, 2, 3, 16, 17, 1, 5, 8, 9, 40, 1, 15]
    nb = sum(sizes)
    x = cx(r, nb * M)
    g = LQ.FirPfbch(LQ.LIQUID_ANALYZER, M, m=m, As=60.0)
    o = O.FirPfbch(O.ANALYZER, M, m=m, As=60.0)
    ys, a = [], 0
    for k in sizes:
        xs = x[a * M:(a + k) * M]
        if mode == "host":
            ys.append(g.execute_block(xs))
        else:
            dx = LQ.DeviceBuffer.from_array(xs)
            dy = dx if mode == "inplace" else LQ.DeviceBuffer(k * M * 8)
            LQ.lib().firpfbch_crcf_execute_block_dev(g.q, dx.p, k, dy.p)
            LQ.lib().liquid_mi355x_device_synchronize()
            ys.append(dy.to_array(np.complex64, k * M))
        a += k
    ref = o.execute_block(x) if hasattr(o, "execute_block") else \
        np.concatenate([o.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(np.concatenate(ys), ref) < NRM


@pytest.mark.parametrize("M,m", [(64, 1), (64, 4), (128, 3), (128, 8)])
def test_firpfbch_analyzer_small_m_long_stream(M, m):
    # the fused M = 64 / 128 analyzer (k_pfb_an_small: several column sets per
    # workgroup, each on its own run of blocks) over thousands of blocks in
    # ragged calls
    r = rng(5 * M + m)
    nb = (1 << 20) // M + 21
    x = cx(r, nb * M)
    g = LQ.FirPfbch(LQ.LIQUID_ANALYZER, M, m=m, As=60.0)
    o = O.FirPfbch(O.ANALYZER, M, m=m, As=60.0)
    cuts = [0, 1, 779, nb - 3, nb]
    y = np.concatenate([g.execute_block(x[a * M:b * M]) for a, b in zip(cuts[:-1], cuts[1:])])
    ref = o.execute_block(x) if hasattr(o, "execute_block") else \
        np.concatenate([o.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_firpfbch_analyzer_m4096_long_stream(m):
    # the fused M = 4096 analyzer (k_pfb_an4096: four columns per lane, one
    # row per group, quarter transforms + radix-4 combine, the oldest ring
    # row in LDS) over many workgroup runs in ragged calls
    M = 4096
    r = rng(3 * M + m)
    nb = (1 << 22) // M + 23
    x = cx(r, nb * M)
    g = LQ.FirPfbch(LQ.LIQUID_ANALYZER, M, m=m, As=60.0)
    o = O.FirPfbch(O.ANALYZER, M, m=m, As=60.0)
    cuts = [0, 1, 333, nb - 3, nb]
    y = np.concatenate([g.execute_block(x[a * M:b * M]) for a, b in zip(cuts[:-1], cuts[1:])])
    ref = o.execute_block(x) if hasattr(o, "execute_block") else \
        np.concatenate([o.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_firpfbch_synthesizer_m4096_long_stream(m):
    # the fused M = 4096 synthesizer (k_pfb_syn4096: quarter transforms
    # loaded straight from X, radix-4 combine into the lane's own columns,
    # register ring): runs warm up on the blocks before them or on the
    # object's state; a short call (fewer blocks than p: two-pass path)
    # carries the state between fused calls
    M = 4096
    r = rng(13 * M + m)
    nb = (1 << 22) // M + 23
    x = cx(r, nb * M)
    g = LQ.FirPfbch(LQ.LIQUID_SYNTHESIZER, M, m=m, As=60.0)
    o = O.FirPfbch(O.SYNTHESIZER, M, m=m, As=60.0)
    cuts = [0, 1, 333, nb - 3, nb]
    y = np.concatenate([g.execute_block(x[a * M:b * M]) for a, b in zip(cuts[:-1], cuts[1:])])
    ref = o.execute_block(x) if hasattr(o, "execute_block") else \
        np.concatenate([o.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("typ", [LQ.LIQUID_ANALYZER, LQ.LIQUID_SYNTHESIZER])
def test_firpfbch_m4096_cccf_complex_taps(typ):
    # the fused M = 4096 kernels with complex taps, pinned by linearity in the taps
    M, p = 4096, 6
    r = rng(4099 + typ)
    h = cx(r, M * p)
    nb = 300
    x = cx(r, nb * M)
    g = LQ.FirPfbch(typ, M, p=p, h=h, t="cccf")
    o_re = O.FirPfbch(typ, M, p=p, h=h.real.copy())
    o_im = O.FirPfbch(typ, M, p=p, h=h.imag.copy())
    y = np.concatenate([g.execute(x[:M]), g.execute_block(x[M:])])
    ref = np.concatenate([o_re.execute(x[b * M:(b + 1) * M]).astype(np.complex128)
                          + 1j * o_im.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(y, ref) < NRM



@pytest.mark.parametrize("M,m", [(64, 1), (64, 4), (128, 3), (128, 8)])
def test_firpfbch_synthesizer_small_m_long_stream(M, m):
    # the fused M = 64 / 128 synthesizer (k_pfb_syn_small): runs of blocks per
    # column set, warm-up on the blocks before a run or on the object's state;
    # ragged calls (short ones take the two-pass path) carry the state across
    r = rng(9 * M + m)
    nb = (1 << 20) // M + 21
    x = cx(r, nb * M)
    g = LQ.FirPfbch(LQ.LIQUID_SYNTHESIZER, M, m=m, As=60.0)
    o = O.FirPfbch(O.SYNTHESIZER, M, m=m, As=60.0)
    cuts = [0, 1, 779, nb - 3, nb]
    y = np.concatenate([g.execute_block(x[a * M:b * M]) for a, b in zip(cuts[:-1], cuts[1:])])
    ref = o.execute_block(x) if hasattr(o, "execute_block") else \
        np.concatenate([o.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(y, ref) < NRM


def test_firpfbch_analyzer_small_m_complex_taps():
    M, p = 64, 6
    r = rng(4242)
    h = cx(r, M * p)
    nb = 4000
    x = cx(r, nb * M)
    g = LQ.FirPfbch(LQ.LIQUID_ANALYZER, M, p=p, h=h, t="cccf")
    o_re = O.FirPfbch(O.ANALYZER, M, p=p, h=h.real.copy())
    o_im = O.FirPfbch(O.ANALYZER, M, p=p, h=h.imag.copy())
    y = np.concatenate([g.execute(x[:M]), g.execute_block(x[M:])])
    ref = np.concatenate([o_re.execute(x[b * M:(b + 1) * M]).astype(np.complex128)
                          + 1j * o_im.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("typ", [LQ.LIQUID_ANALYZER, LQ.LIQUID_SYNTHESIZER])
def test_firpfbch_cccf_m256_complex_taps(typ):
    M, p = 256, 6
    r = rng(999 + typ)
    h = cx(r, M * p)
    nb = 600
    x = cx(r, nb * M)
    g = LQ.FirPfbch(typ, M, p=p, h=h, t="cccf")
    o_re = O.FirPfbch(typ, M, p=p, h=h.real.copy())
    o_im = O.FirPfbch(typ, M, p=p, h=h.imag.copy())
    y = np.concatenate([g.execute(x[:M]), g.execute_block(x[M:])])
    ref = np.concatenate([o_re.execute(x[b * M:(b + 1) * M]).astype(np.complex128)
                          + 1j * o_im.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(y, ref) < NRM


# ============================================================== drop-in programs
# ------------------------------------------------------------------ firpfb / resamp
def test_firpfb_known_answer():
    # firpfb_autotest.c impulse response (rrrf data through the crcf bank, imag = 0)
    c = KA["autotest_firpfb_impulse_response"]
    q = LQ.FirPfb(c["M"], G.arr(c["h"]))
    for v in G.arr(c["x"]):
        q.push(v)
    out = np.array([q.execute(i) for i in range(c["M"])])
    assert np.max(np.abs(out.real - G.arr(c["y"]))) < c["tol"]
    assert np.max(np.abs(out.imag)) == 0.0


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("M,hlen", [(8, 64), (32, 449), (64, 896), (5, 7)])
def test_firpfb_block_and_push_vs_oracle(M, hlen, t):
    r = rng(M * 3 + hlen)
    h = coefs(r, t, hlen)
    x = samples(r, t, 3000)
    g = LQ.FirPfb(M, h, t=t)
    o = O.FirPfb(TYPES[t], M, h)
    s = (0.8 + 0.1j) if t == "cccf" else 0.8
    g.set_scale(s)            # linear: the oracle runs at unit scale and the reference is scaled after
    ref = np.empty((len(x), M), np.float32 if t == "rrrf" else np.complex64)
    for k, v in enumerate(x):
        o.push(v)
        ref[k] = [o.execute(i) for i in range(M)]
    ref = ref * s
    y1 = g.execute_block(x[:2000])
    for v in x[2000:2010]:              # per-sample push/execute after a block call
        g.push(v)
    per = np.array([g.execute(i) for i in range(M)])
    y2 = g.execute_block(x[2010:])
    assert G.nrm_err(y1, ref[:2000]) < NRM
    assert G.nrm_err(per, ref[2009]) < NRM
    assert G.nrm_err(y2, ref[2010:]) < NRM


# -------------------------------------------- per-sample calls on the pinned window
# push() appends to the pinned host window, which moves back to the start of
# its buffer every n + 64 pushes (n = the window length, at most 128 here), and
# the single-output kernels read it in place; block calls in between hand the
# window to the device and back.
@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("hlen", [1, 13, 40, 100])
def test_firfilt_push_execute_across_window_moves(t, hlen):
    r = rng(hlen * 5 + 1)
    h = coefs(r, t, hlen)
    x = samples(r, t, 1600)
    g = LQ.FirFilt(t, h)
    out = []
    for a, b, per in [(0, 100, False), (100, 1100, True), (1100, 1300, False), (1300, 1600, True)]:
        if per:
            for v in x[a:b]:
                g.push(v)
                out.append(np.atleast_1d(g.execute()))
        else:
            out.append(g.execute_block(x[a:b]))
    assert G.nrm_err(np.concatenate(out), O.FirFilt(TYPES[t], h).execute_block(x)) < NRM


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("M,hlen", [(5, 7), (8, 64), (32, 449)])
def test_firpfb_push_execute_across_window_moves(M, hlen, t):
    r = rng(M * 7 + hlen)
    h = coefs(r, t, hlen)
    x = samples(r, t, 700)
    g = LQ.FirPfb(M, h, t=t)
    o = O.FirPfb(TYPES[t], M, h)
    ref = np.empty((len(x), M), np.float32 if t == "rrrf" else np.complex64)
    for k, v in enumerate(x):
        o.push(v)
        ref[k] = [o.execute(i) for i in range(M)]
    y1 = np.asarray(g.execute_block(x[:200])).reshape(-1, M)
    per = []
    for k in range(200, 600):           # one bank per push, cycling through the banks
        g.push(x[k])
        per.append(g.execute(k % M))
    y2 = np.asarray(g.execute_block(x[600:])).reshape(-1, M)
    assert G.nrm_err(y1, ref[:200]) < NRM
    assert G.nrm_err(np.array(per), ref[np.arange(200, 600), np.arange(200, 600) % M]) < NRM
    assert G.nrm_err(y2, ref[600:]) < NRM


# ------------------------------------------------------------ prototype constructors
# *_create_rnyquist / *_create_prototype design taps on the host
# (liquid_firdes_prototype, pinned in tests/test_firdes.py) and hand them to
# the ordinary constructors: check the wiring against the oracle objects built
# from the same taps.
@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("ftype,k,m,beta,mu", [("rkaiser", 2, 7, 0.3, 0.0), ("rrc", 4, 3, 0.5, 0.25),
                                                ("gmsktx", 3, 4, 0.3, -0.5)])
def test_firfilt_create_rnyquist(t, ftype, k, m, beta, mu):
    r = rng(k * 11 + m)
    x = samples(r, t, 5000)
    code = LQ.LIQUID_FIRFILT[ftype]
    g = LQ.FirFilt.construct("_create_rnyquist", (code, k, m, beta, mu), t=t)
    h = LQ.firdes_prototype(ftype, k, m, beta, mu)
    o = O.FirFilt(TYPES[t], h.astype(np.complex64) if t == "cccf" else h)
    assert G.nrm_err(g.execute_block(x), o.execute_block(x)) < NRM


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("ftype,M,m,beta,dt", [("arkaiser", 4, 5, 0.35, 0.0), ("kaiser", 3, 4, 0.3, 0.5),
                                                ("rcos", 8, 2, 0.25, 0.0)])
def test_firdecim_firinterp_create_prototype(t, ftype, M, m, beta, dt):
    r = rng(M * 5 + m)
    code = LQ.LIQUID_FIRFILT[ftype]
    h = LQ.firdes_prototype(ftype, M, m, beta, dt)
    hc = h.astype(np.complex64) if t == "cccf" else h
    x = samples(r, t, 400 * M)
    gd = LQ.FirDecim.construct("_create_prototype", (code, M, m, beta, dt), t=t, M=M)
    od = O.FirDecim(TYPES[t], M, hc)
    assert G.nrm_err(gd.execute_block(x), od.execute_block(x)) < NRM
    xi = samples(r, t, 700)
    gi = LQ.FirInterp.construct("_create_prototype", (code, M, m, beta, dt), t=t, M=M)
    oi = O.FirInterp(TYPES[t], M, hc)
    assert G.nrm_err(gi.execute_block(xi), oi.execute_block(xi)) < NRM


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("deriv", [0, 1])
def test_firpfb_create_rnyquist_drnyquist(t, deriv):
    # firpfb.c:146-240: prototype at M*k samples/symbol; derivative bank = central
    # difference (circular ends) scaled to max|h dh| = 0.06
    M, k, m, beta = 16, 2, 5, 0.35
    code = LQ.LIQUID_FIRFILT["rkaiser"]
    H = LQ.firdes_prototype("rkaiser", M * k, m, beta).astype(np.float64)
    if deriv:
        dH = np.roll(H, -1) - np.roll(H, 1)
        H = dH * 0.06 / np.max(np.abs(H * dH))
    H = H.astype(np.float32)
    ctor = "_create_drnyquist" if deriv else "_create_rnyquist"
    g = LQ.FirPfb.construct(ctor, (code, M, k, m, beta), t=t, M=M)
    o = O.FirPfb(TYPES[t], M, H.astype(np.complex64) if t == "cccf" else H)
    r = rng(77 + deriv)
    x = samples(r, t, 600)
    ref = np.empty((len(x), M), np.float32 if t == "rrrf" else np.complex64)
    for j, v in enumerate(x):
        o.push(v)
        ref[j] = [o.execute(i) for i in range(M)]
    assert G.nrm_err(g.execute_block(x), ref) < 2 * NRM


@pytest.mark.parametrize("typ", [LQ.LIQUID_ANALYZER, LQ.LIQUID_SYNTHESIZER])
@pytest.mark.parametrize("m", [4, 2])
def test_firpfbch_m1024_fast_path_many_workgroups(typ, m):
    # M = 1024 fast kernels (k_pfb_an1024 / k_pfb_syn1024): 700 blocks spread
    # over ~22 workgroups, so every workgroup but the first rebuilds its
    # history from the input; a ragged second call continues the stream
    M, nb = 1024, 700
    r = rng(40 + m + typ)
    x = cx(r, (nb + 9) * M)
    g = LQ.FirPfbch(typ, M, m=m, As=60.0)
    o = O.FirPfbch(typ, M, m=m, As=60.0)
    y = np.concatenate([g.execute_block(x[: nb * M]), g.execute_block(x[nb * M:])])
    ref = np.concatenate([o.execute(x[b * M:(b + 1) * M]) for b in range(nb + 9)])
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("typ", [LQ.LIQUID_ANALYZER, LQ.LIQUID_SYNTHESIZER])
# (4, 1): the run kernels' p = 1 (one tap per branch: explicit taps only)
@pytest.mark.parametrize("M,p", [(8, 4), (64, 6), (6, 3), (4, 1)])
def test_firpfbch_cccf_complex_taps(typ, M, p):
    # the channelizer is linear in its taps over the complex numbers:
    # A(hr + j hi) = A(hr) + j A(hi), so two real-tap oracle runs pin cccf
    r = rng(M * p + typ)
    h = cx(r, M * p)
    nb = 20
    x = cx(r, nb * M)
    g = LQ.FirPfbch(typ, M, p=p, h=h, t="cccf")
    o_re = O.FirPfbch(typ, M, p=p, h=h.real.copy())
    o_im = O.FirPfbch(typ, M, p=p, h=h.imag.copy())
    y = np.concatenate([g.execute(x[:M]), g.execute_block(x[M:])])
    ref = np.concatenate([o_re.execute(x[b * M:(b + 1) * M]).astype(np.complex128)
                          + 1j * o_im.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("t", ["crcf", "cccf"])
@pytest.mark.parametrize("typ", [LQ.LIQUID_ANALYZER, LQ.LIQUID_SYNTHESIZER])
@pytest.mark.parametrize("ftype", ["arkaiser", "rkaiser", "rrc", "hM3"])
def test_firpfbch_create_rnyquist(t, typ, ftype):
    # firpfbch.c:193-256: analyzer taps are the time-reversed first 2Mm (matched filter)
    M, m, beta = 16, 3, 0.4
    h = LQ.firdes_prototype(ftype, M, m, beta)
    g_len = 2 * M * m
    gc = h[:g_len] if typ == LQ.LIQUID_SYNTHESIZER else h[:g_len][::-1]
    g = LQ.FirPfbch(typ, M, t=t, rnyquist=(m, beta, LQ.LIQUID_FIRFILT[ftype]))
    o = O.FirPfbch(typ, M, p=2 * m, h=np.ascontiguousarray(gc))
    r = rng(5 + typ)
    nb = 24
    x = cx(r, nb * M)
    y = g.execute_block(x)
    ref = np.concatenate([o.execute(x[b * M:(b + 1) * M]) for b in range(nb)])
    assert G.nrm_err(y, ref) < NRM


def test_firfilt_freqresponse_groupdelay():
    # firfilt.c:371-404 restated in float64: H = s * sum_i h[n-1-i] e^{j2pi fc i}
    r = rng(3)
    for t in ("rrrf", "crcf", "cccf"):
        h = coefs(r, t, 37)
        g = LQ.FirFilt(t, h)
        s = (0.9 + 0.2j) if t == "cccf" else 0.9
        g.set_scale(s)
        i = np.arange(len(h))
        for fc in (-0.31, 0.0, 0.125, 0.4):
            H = s * np.sum(h[::-1].astype(np.complex128) * np.exp(2j * np.pi * fc * i))
            assert abs(g.freqresponse(fc) - H) <= 1e-5 * max(1.0, abs(H))
            hr = np.real(h).astype(np.float64)
            e = np.exp(2j * np.pi * fc * i)
            gd = np.real(np.sum(hr * e * i) / np.sum(hr * e))
            assert abs(g.groupdelay(fc) - gd) <= 1e-3 * max(1.0, abs(gd))


def _resamp_pair(rate, m=7, fc=0.25, As=60.0, npfb=64):
    rate = float(np.float32(rate))
    return LQ.Resamp(rate, m, fc, As, npfb), O.Resamp(rate, m, fc, As, npfb)


@pytest.mark.parametrize("rate,m,npfb", [(1.037, 7, 64), (0.97, 7, 64), (3.7, 4, 32), (0.5, 7, 64),
                                         (10.3, 3, 64), (0.8131, 3, 37), (2.0, 16, 64), (1.3, 20, 16)])
def test_resamp_vs_oracle_ragged(rate, m, npfb):
    r = rng(int(rate * 1000) + m)
    x = cx(r, 200_000)
    g, o = _resamp_pair(rate, m=m, npfb=npfb)
    cuts = [0, 1, 2, 3, 100, 70_000, 70_001, 140_000, 200_000]
    ys = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b - a == 1:
            ys.append(g.execute(x[a]))
        else:
            ys.append(g.execute_block(x[a:b]))
    y = np.concatenate(ys)
    ref = o.execute_block(x)
    assert len(y) == len(ref)
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("rate,npfb", [(30.0, 64), (58.9, 64), (59.9, 64), (64.0, 64), (100.0, 64), (83.3, 64),
                                       (75.5, 64), (130.7, 64), (57.3, 37)])
def test_resamp_high_rate_vs_oracle(rate, npfb):
    """rates whose 16-input tiles overflow the tiled kernel's 1088 output
    slots (r > ~60) run the per-input kernel; rates above npfb follow the
    reference's unsigned b < npfb test (resamp.c:254), which stops the stream
    once a BOUNDARY update leaves b = -1.  Calls of >= 16 inputs, ragged."""
    r = rng(int(rate * 10) + npfb)
    x = cx(r, 6000)
    g, o = _resamp_pair(rate, m=7, npfb=npfb)
    cuts = [0, 1, 17, 18, 1000, 1001, 4096, 6000]
    ys = [g.execute(x[a]) if b - a == 1 else g.execute_block(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    y = np.concatenate(ys)
    ref = o.execute_block(x)
    assert len(y) == len(ref)
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("rate,m", [(40.0, 12), (45.3, 16), (35.0, 9), (20.0, 16)])
def test_resamp_high_rate_long_filter_vs_oracle(rate, m):
    """high rates shrink the tiles to 16-32 inputs, fewer than the L + 1 =
    2m + 1 window samples: tiles after the first of a call also reach into
    the history (a round-3 kernel read zeros there)"""
    r = rng(int(rate * 7) + m)
    x = cx(r, 3000)
    g, o = _resamp_pair(rate, m=m, npfb=64)
    cuts = [0, 1, 40, 41, 1000, 3000]
    ys = [g.execute(x[a]) if b - a == 1 else g.execute_block(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    y = np.concatenate(ys)
    ref = o.execute_block(x)
    assert len(y) == len(ref)
    assert G.nrm_err(y, ref) < NRM


def test_resamp_reference_autotest_gpu():
    """autotest_resamp_crcf (src/filter/tests/resamp_crcf_autotest.c:29-136)
    on the GPU path: one execute() per input as the reference calls it, then
    the same stream in one execute_block; both pass the reference's rate /
    peak / peak-frequency / side-lobe checks and match the oracle"""
    rr, m, bw, As, npfb, x, check = G.resamp_autotest_case()
    g = LQ.Resamp(rr, m, bw, As, npfb)
    y = np.concatenate([g.execute(v) for v in x])
    assert check(y) == []
    yb = LQ.Resamp(rr, m, bw, As, npfb).execute_block(x)
    assert check(yb) == []
    ref = O.Resamp(rr, m, bw, As, npfb).execute_block(x)
    assert len(y) == len(ref) == len(yb)
    assert G.nrm_err(y, ref) < NRM and G.nrm_err(yb, ref) < NRM


def test_resamp_long_stream_crosses_period():
    # r = 1.037: the timing plan repeats every 1 011 163 inputs; 2.5M inputs in
    # calls of 600k use (and wrap) the periodic plan several times
    r = rng(37)
    x = cx(r, 2_500_000)
    g, o = _resamp_pair(1.037)
    y = np.concatenate([g.execute_block(x[a:a + 600_000]) for a in range(0, len(x), 600_000)])
    ref = o.execute_block(x)
    assert len(y) == len(ref)
    assert G.nrm_err(y, ref) < NRM


def test_resamp_set_rate_adjust_rate_reset():
    r = rng(41)
    x = cx(r, 150_000)
    g, o = _resamp_pair(1.037)
    y, ref = [], []
    y.append(g.execute_block(x[:80_000]))
    ref.append(o.execute_block(x[:80_000]))
    g.set_rate(0.913)
    o.set_rate(float(np.float32(0.913)))
    y.append(g.execute_block(x[80_000:120_000]))
    ref.append(o.execute_block(x[80_000:120_000]))
    g.adjust_rate(0.05)                 # the reference clips the adjusted rate to 0.5
    o.adjust_rate(0.05)
    y.append(g.execute_block(x[120_000:]))
    ref.append(o.execute_block(x[120_000:]))
    for a, b in zip(y, ref):
        assert len(a) == len(b)
        assert G.nrm_err(a, b) < NRM
    g.reset()
    o.reset()
    o.set_rate(0.5)
    g.set_rate(0.5)
    a, b = g.execute_block(x[:5000]), o.execute_block(x[:5000])
    assert len(a) == len(b) and G.nrm_err(a, b) < NRM


@pytest.mark.parametrize("t", [LQ.RRRF, LQ.CCCF])
@pytest.mark.parametrize("rate,m,npfb", [(1.037, 7, 64), (0.8131, 3, 37), (1.3, 20, 16)])
def test_resamp_types_vs_oracle(t, rate, m, npfb):
    # resamp.c:117-132 designs real taps for every type: cccf filters exactly as
    # crcf, and rrrf as crcf on a real signal (imaginary part zero)
    r = rng(int(rate * 100) + m + (7 if t == LQ.RRRF else 0))
    rate = float(np.float32(rate))
    x = cx(r, 150_000)
    if t == LQ.RRRF:
        x = np.ascontiguousarray(x.real)
    g = LQ.Resamp(rate, m, 0.25, 60.0, npfb, t=t)
    o = O.Resamp(rate, m, 0.25, 60.0, npfb)
    cuts = [0, 1, 2, 5000, 80_000, 80_001, 150_000]
    ys = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        ys.append(g.execute(x[a]) if b - a == 1 else g.execute_block(x[a:b]))
    y = np.concatenate(ys)
    ref = o.execute_block(x.astype(np.complex64))
    assert len(y) == len(ref)
    if t == LQ.RRRF:
        assert y.dtype == np.float32
        ref = ref.real
    assert G.nrm_err(y, ref) < NRM


def test_resamp_baseline_config5_device():
    # BASELINE configs[4]: r = 1.037, npfb = 64, m = 7 on 32M samples, device resident
    n = 1 << 25
    r = rng(5)
    x = cx(r, n)
    g, o = _resamp_pair(1.037)
    nout = g.num_output(n)
    assert nout == 34_795_945
    dx = LQ.DeviceBuffer.from_array(x)
    dy = LQ.DeviceBuffer(nout * 8)
    ny = g.execute_block_dev(dx.p, n, dy.p)
    g.synchronize()
    assert ny == nout
    y = dy.to_array(np.complex64, nout)
    ref = o.execute_block(x)
    assert len(ref) == nout
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("src", sorted(f for f in os.listdir(os.path.join(LQ.ROOT, "examples")) if f.endswith(".c")))
def test_examples_run_on_gpu(src, tmp_path):
    inc = os.path.join(LQ.ROOT, "include")
    libdir = os.path.dirname(LQ.LIB_PATH)
    out = tmp_path / "a.out"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-I", inc, os.path.join(LQ.ROOT, "examples", src),
                           "-L", libdir, "-lliquid_mi355x", "-Wl,-rpath," + libdir, "-lm", "-o", str(out)])
    res = subprocess.run([str(out)], capture_output=True, text=True, timeout=120)
    print(res.stdout, res.stderr)
    assert res.returncode == 0


REF_EX = os.path.join(LQ.ROOT, "build", "ref_examples")


@pytest.mark.skipif(not os.path.isdir(REF_EX), reason="reference examples not built (tools/build_ref_examples.sh)")
@pytest.mark.parametrize("exe", sorted(os.listdir(REF_EX)) if os.path.isdir(REF_EX) else [])
@pytest.mark.parametrize("small_calls", ["gpu", "host"])
def test_reference_examples_run(exe, small_calls, tmp_path):
    """liquid-dsp's own example programs, compiled unchanged against the
    drop-in header, run to completion with every call on the GPU
    (LQ_SMALL_CALLS=gpu), and in the library's default mode (single-sample
    calls on the host, block calls on the GPU)."""
    env = dict(os.environ)
    env.pop("LQ_SMALL_CALLS", None)
    if small_calls == "gpu":
        env["LQ_SMALL_CALLS"] = "gpu"
    res = subprocess.run([os.path.join(REF_EX, exe)], capture_output=True, text=True, timeout=120, cwd=tmp_path,
                         env=env)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0
    assert "error" not in res.stderr.lower()


# ------------------------------------------------------------ resamp2 / msresamp2 / msresamp
def _as_oracle_in(x):
    return x.astype(np.complex64)


def _cmp_typed(y, ref, t):
    if t == "rrrf":
        assert y.dtype == np.float32
        ref = ref.real
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("m,f0", [(5, 0.0), (12, 0.13), (2, -0.2)])
def test_resamp2_modes_vs_oracle(t, mode, m, f0):
    r = rng(m * 10 + mode)
    nin = LQ.Resamp2.NIN[mode]
    ncalls = 2000
    x = samples(r, t, ncalls * nin)
    g = LQ.Resamp2(m, f0, 60.0, t=t)
    o = O.Resamp2(m, f0, 60.0, ctaps=(t == "cccf"))
    # ragged: single per-call API calls, then blocks of odd sizes (toggle parity)
    cuts = [0, 1, 2, 3, 700, 701, 1500, ncalls]
    ys0, ys1 = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        xa = x[a * nin:b * nin]
        if b - a == 1:
            res = g.call(mode, xa[0] if nin == 1 else xa)
            if mode == 0:
                ys0.append(np.array([res[0]]))
                ys1.append(np.array([res[1]]))
            else:
                ys0.append(res)
        else:
            res = g.run(mode, xa)
            if mode == 0:
                ys0.append(res[0])
                ys1.append(res[1])
            else:
                ys0.append(res)
    ref = o.run(mode, _as_oracle_in(x))
    if mode == 0:
        _cmp_typed(np.concatenate(ys0), ref[0], t)
        _cmp_typed(np.concatenate(ys1), ref[1], t)
    else:
        _cmp_typed(np.concatenate(ys0), ref, t)


def test_resamp2_mixed_modes_share_windows():
    # the reference's modes push into the same two windows; switching modes on
    # one object continues from that shared state
    r = rng(99)
    g = LQ.Resamp2(6, 0.0, 60.0)
    o = O.Resamp2(6, 0.0, 60.0)
    for mode, n in [(0, 37), (3, 50), (4, 21), (1, 40), (0, 3), (2, 64), (0, 11)]:
        x = cx(r, n * LQ.Resamp2.NIN[mode])
        a, b = g.run(mode, x), o.run(mode, x)
        if mode == 0:
            assert G.nrm_err(a[0], b[0]) < NRM and G.nrm_err(a[1], b[1]) < NRM
        else:
            assert G.nrm_err(a, b) < NRM
    g.clear()
    o.clear()
    x = cx(r, 64)
    assert G.nrm_err(g.run(3, x), o.run(3, x)) < NRM


def test_resamp2_reference_analysis_synthesis_gpu():
    m, n, x, check = G.resamp2_analysis_case()
    g = LQ.Resamp2(m, 0.0, 60.0)
    y = np.concatenate([g.call(LQ.RESAMP2_ANALYZER, x[2 * i:2 * i + 2]) for i in range(n)])
    err, tol = check(y[0::2], y[1::2])
    assert err < tol
    m, n, x, check = G.resamp2_synthesis_case()
    y = LQ.Resamp2(m, 0.0, 60.0).run(LQ.RESAMP2_SYNTHESIZER, x)
    err, tol = check(y)
    assert err < tol


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("typ", [0, 1])
@pytest.mark.parametrize("ns", [0, 1, 3])
def test_msresamp2_vs_oracle(t, typ, ns):
    r = rng(ns * 7 + typ)
    M = 1 << ns
    ncalls = 300
    x = samples(r, t, ncalls * (1 if typ == 0 else M))
    g = LQ.MsResamp2(typ, ns, 0.4, 0.0, 60.0, t=t)
    o = O.MsResamp2(typ, ns, 0.4, 0.0, 60.0)
    step = 1 if typ == 0 else M
    y = np.concatenate([g.execute(x[:step]), g.execute_block(x[step:100 * step]), g.execute_block(x[100 * step:])])
    _cmp_typed(y, o.execute_block(_as_oracle_in(x)), t)


@pytest.mark.parametrize("t", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("rate", [0.127115323, 0.3, 0.77, 1.0, 1.7, 3.3, 10.5])
def test_msresamp_vs_oracle(t, rate):
    r = rng(int(rate * 1000))
    rate = float(np.float32(rate))
    x = samples(r, t, 20_000)
    g = LQ.MsResamp(rate, 60.0, t=t)
    o = O.MsResamp(rate, 60.0)
    cuts = [0, 1, 2, 3, 5, 333, 4000, 4001, 20_000]
    y = np.concatenate([g.execute(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    ref = o.execute(_as_oracle_in(x))
    assert len(y) == len(ref)
    _cmp_typed(y, ref, t)
    assert abs(g.get_delay() - LQ.MsResamp(rate, 60.0, t=t).get_delay()) == 0


def test_msresamp_reference_spectral_gpu():
    r, As, x, check = G.msresamp_spectral_case()
    g = LQ.MsResamp(r, As)
    y = np.concatenate([g.execute(x[i:i + 1]) for i in range(len(x))])
    assert check(y) == []


def test_msresamp_device_long_stream():
    # 4M samples device-resident through a 1/8.3 decimating chain
    n = 1 << 22
    r = rng(123)
    x = cx(r, n)
    rate = float(np.float32(1 / 8.3))
    g = LQ.MsResamp(rate, 60.0)
    o = O.MsResamp(rate, 60.0)
    nout = g.num_output(n)
    dx = LQ.DeviceBuffer.from_array(x)
    dy = LQ.DeviceBuffer(max(1, nout) * 8)
    ny = g.execute_block_dev(dx.p, n, dy.p)
    g.synchronize()
    assert ny == nout
    y = dy.to_array(np.complex64, ny)
    ref = o.execute(x)
    assert len(ref) == ny
    assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("rate,As", [(3.3, 60.0), (2.5, 20.0), (2.2, 40.0), (3.9, 80.0), (7.1, 100.0), (3.3, 120.0)])
def test_msresamp_interp_chain_device_stream(rate, As):
    # the interpolating chain (resampler + first half-band stage fused into
    # k_resamp4, stage m = 3 (As = 20) .. 12; As = 120 gives m = 13: two
    # kernels; r = 7.1: the second stage unfused after the fused one) on a
    # 2M-sample device stream in ragged calls, two objects' outputs compared
    # with the oracle
    rate = float(np.float32(rate))
    n = 1 << 21
    r = rng(int(rate * 100 + As))
    x = cx(r, n)
    o = O.MsResamp(rate, As)
    for t in (LQ.CRCF, LQ.CCCF):
        g = LQ.MsResamp(rate, As, t=t)
        cuts = [0, 1, 7, 300, 301, 70_001, 1_000_000, n]
        dx = LQ.DeviceBuffer.from_array(x)
        ys = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            nout = g.num_output(b - a)
            # cccf: outputs 8 bytes past a 16-byte boundary (the stage's 8-byte stores)
            off = 8 if t == LQ.CCCF else 0
            dy = LQ.DeviceBuffer(max(1, nout) * 8 + 16)
            ny = g.execute_block_dev(dx.p + 8 * a, b - a, dy.p + off)
            g.synchronize()
            assert ny == nout
            yb = np.empty(max(1, nout) + 2, np.complex64)
            LQ.lib().liquid_mi355x_memcpy_d2h(LQ.ptr(yb), dy.p, yb.nbytes)
            ys.append(yb.view(np.uint8)[off:off + 8 * ny].view(np.complex64))
        y = np.concatenate(ys)
        ref = o.execute(x) if t == LQ.CRCF else ref
        assert len(y) == len(ref)
        assert G.nrm_err(y, ref) < NRM


@pytest.mark.parametrize("rate", [40.0, 70.0, 150.0])
def test_msresamp_interp_chain_many_stages(rate):
    # five to seven half-band stages after the fused resampler + first stage:
    # the later stages ping-pong between two buffers that must grow with every
    # stage (stage s writes 2^s times the fused kernel's output count;
    # round-5 advisor finding on host/resamp2.c)
    rate = float(np.float32(rate))
    n = 1 << 15
    r = rng(int(rate))
    x = cx(r, n)
    o = O.MsResamp(rate, 60.0)
    ref = o.execute(x)
    for t in (LQ.CRCF, LQ.CCCF):
        g = LQ.MsResamp(rate, 60.0, t=t)
        dx = LQ.DeviceBuffer.from_array(x)
        ys = []
        for a, b in ((0, 3), (3, 5000), (5000, n)):
            nout = g.num_output(b - a)
            dy = LQ.DeviceBuffer(max(1, nout) * 8)
            ny = g.execute_block_dev(dx.p + 8 * a, b - a, dy.p)
            g.synchronize()
            assert ny == nout
            ys.append(dy.to_array(np.complex64, ny))
        y = np.concatenate(ys)
        assert len(y) == len(ref)
        assert G.nrm_err(y, ref) < NRM


# ------------------------------------------------------------ FFT plan API
FFTG = G.load("fft")
R2RG = G.load("fft_r2r")


@pytest.mark.parametrize("case", FFTG, ids=lambda c: "n%d" % c["n"])
def test_fft_run_golden(case):
    # fft_runtest.c:30-67: forward against the data, backward recovers n x
    x, y = G.arr(case["x"]), G.arr(case["y"])
    Y = LQ.fft_run(x, +1)
    assert np.max(np.abs(Y - y)) < case["tol"]
    z = LQ.fft_run(Y, -1) / len(x)
    assert np.max(np.abs(z - x)) < case["tol"]
    assert G.nrm_err(Y, O.fft(x, +1)) < NRM


@pytest.mark.parametrize("case", R2RG, ids=lambda c: c["name"])
def test_fft_r2r_golden(case):
    y = LQ.fft_r2r(G.arr(case["x"]).real.astype(np.float32), case["type"])
    assert np.max(np.abs(y - np.asarray(case["y"]))) < case["tol"]


@pytest.mark.parametrize("n", [32, 64, 128, 256, 512, 2048, 4096, 8192, 1 << 14, 1 << 15, 65536, 1 << 17, 1 << 20, 1000, 4099, 12345,
                               100003, 17,
                               3 * 4096,
                               2, 4, 8, 16, 1024])   # k_fft_batch<N> and k_fft1024_batch through the plan API
@pytest.mark.parametrize("direction", [+1, -1])
def test_fft_sizes_vs_float64(n, direction):
    r = rng(n)
    batch = 3 if n <= 100003 else 1
    X = (r.standard_normal((batch, n)) + 1j * r.standard_normal((batch, n))).astype(np.complex64)
    Y = LQ.fft_batch(X, direction)
    ref = np.fft.fft(X.astype(np.complex128), axis=1) if direction > 0 else \
        np.fft.ifft(X.astype(np.complex128), axis=1) * n
    for b in range(batch):
        assert G.nrm_err(Y[b], ref[b]) < NRM


@pytest.mark.parametrize("typ", [10, 11, 12, 13, 20, 21, 22, 23])
def test_fft_r2r_large_vs_formula(typ):
    import test_oracle as TO
    r = rng(typ)
    x = r.standard_normal(1000).astype(np.float32)
    assert G.nrm_err(LQ.fft_r2r(x, typ), TO.r2r_np(typ, x)) < NRM


def test_fft_plan_binds_arrays_and_device_batch():
    # fft_create_plan binds x/y; fft_execute reads x at call time
    n = 256
    x = np.zeros(n, np.complex64)
    y = np.zeros(n, np.complex64)
    L = LQ.lib()
    p = L.fft_create_plan(n, LQ.ptr(x), LQ.ptr(y), LQ.LIQUID_FFT_FORWARD if hasattr(LQ, "LIQUID_FFT_FORWARD") else 1, 0)
    r = rng(4)
    for _ in range(3):
        x[:] = cx(r, n)
        L.fft_execute(p)
        assert G.nrm_err(y, np.fft.fft(x.astype(np.complex128))) < NRM
    L.fft_destroy_plan(p)
    # device-resident batch
    X = cx(r, 64 * 1024).reshape(64, 1024)
    dX = LQ.DeviceBuffer.from_array(X)
    q = L.fft_create_plan(1024, None, None, -1, 0)
    L.fft_execute_batch_dev(q, dX.p, dX.p, 64)
    LQ.lib().liquid_mi355x_device_synchronize()
    L.fft_destroy_plan(q)
    Y = dX.to_array(np.complex64, 64 * 1024).reshape(64, 1024)
    assert G.nrm_err(Y, np.fft.ifft(X.astype(np.complex128), axis=1) * 1024) < NRM


@pytest.mark.parametrize("n", [8192, 16384])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("direction", [+1, -1])
def test_fft_one_pass_large_inplace_offsets(n, off, direction):
    # n = 8192 / 16384 run one pass (k_fft8192_batch / k_fft16384_batch:
    # 16-byte pair loads when x is 16-byte aligned, 8-byte loads otherwise);
    # in place on a device batch starting off samples into the allocation
    batch = 37
    r = rng(n + off)
    X = cx(r, batch * n).reshape(batch, n)
    host = np.zeros(batch * n + 1, np.complex64)
    host[off:off + batch * n] = X.reshape(-1)
    dX = LQ.DeviceBuffer.from_array(host)
    L = LQ.lib()
    q = L.fft_create_plan(n, None, None, direction, 0)
    L.fft_execute_batch_dev(q, dX.p + 8 * off, dX.p + 8 * off, batch)
    L.liquid_mi355x_device_synchronize()
    L.fft_destroy_plan(q)
    Y = dX.to_array(np.complex64, batch * n + 1)[off:off + batch * n].reshape(batch, n)
    ref = np.fft.fft(X.astype(np.complex128), axis=1) if direction > 0 else \
        np.fft.ifft(X.astype(np.complex128), axis=1) * n
    assert G.nrm_err(Y, ref) < NRM


# ------------------------------------------------------------ spgram
def _db_close(a, b):
    # dB outputs compared in linear power, normwise (NRM)
    return G.nrm_err(10 ** (np.asarray(a, np.float64) / 10), 10 ** (np.asarray(b, np.float64) / 10)) < NRM


def _kaiser_window(W, beta):
    return np.array([LQ.lib().kaiser(i, W, beta, 0.0) for i in range(W)], np.float32)


@pytest.mark.parametrize("real_in", [False, True])
@pytest.mark.parametrize("nfft,W", [(64, 48), (256, 128), (1000, 1000), (2, 1), (1024, 512), (1024, 1024), (1024, 301)])
def test_spgram_vs_oracle(real_in, nfft, W):
    r = rng(nfft + W + real_in)
    win = _kaiser_window(W, 8.0)
    g = LQ.Spgram(nfft, win, real_in=real_in)
    o = O.Spgram(nfft, win, real_in=real_in)
    sig = (lambda n: r.standard_normal(n).astype(np.float32)) if real_in else (lambda n: cx(r, n))
    # write / push then execute
    x = sig(W + 7)
    g.write(x[:-3])
    for v in x[-3:]:
        g.push(v)
    o.write(x)
    assert G.nrm_err(g.execute(), o.execute()) < NRM
    assert _db_close(g.execute_psd(), o.execute_psd())
    # accumulate in ragged calls (the first call's alpha = 1 rule included)
    for n, a in [(5, 0.2), (3 * W + 1, 0.2), (1, 0.05), (7 * W + 3, 0.05), (0, 0.3), (W // 2 + 2, 0.3)]:
        xs = sig(n)
        g.accumulate_psd(xs, a)
        o.accumulate_psd(xs, a)
    assert _db_close(g.write_accumulation(), o.write_accumulation())
    # estimate: resets, then averages every nfft/4 and at the end
    xs = sig(10 * nfft + 3)
    assert _db_close(g.estimate_psd(xs), o.estimate_psd(xs))
    assert G.nrm_err(g.execute(), o.execute()) < NRM        # window continues after estimate


def test_spgram_default_and_kaiser_constructors():
    r = rng(12)
    x = cx(r, 5000)
    g = LQ.Spgram(512, default=True)
    o = O.Spgram(512, _kaiser_window(256, 10.0))
    assert _db_close(g.estimate_psd(x), o.estimate_psd(x))
    g2 = LQ.Spgram(300, kaiser=(200, 6.0))
    o2 = O.Spgram(300, _kaiser_window(200, 6.0))
    assert _db_close(g2.estimate_psd(x), o2.estimate_psd(x))


def test_spgram_device_estimate_long():
    n, nfft = 1 << 22, 1024
    r = rng(77)
    x = cx(r, n)
    win = _kaiser_window(nfft // 2, 10.0)
    g = LQ.Spgram(nfft, win)
    o = O.Spgram(nfft, win)
    dx = LQ.DeviceBuffer.from_array(x)
    dp = LQ.DeviceBuffer(nfft * 4)
    LQ.lib().spgramcf_estimate_psd_dev(g.q, dx.p, n, dp.p)
    LQ.lib().spgramcf_synchronize(g.q)
    assert _db_close(dp.to_array(np.float32, nfft), o.estimate_psd(x))


def test_spgram_device_estimate_full_round():
    # 2^26 samples, a 512-sample window: 2^19 transforms through the fused
    # kernel (lqk_spgram_fused1024: 8192 chunks of 64, two fold levels)
    n, nfft = (1 << 26) + 12345, 1024
    r = rng(78)
    x = cx(r, n)
    win = _kaiser_window(nfft // 2, 10.0)
    g = LQ.Spgram(nfft, win)
    o = O.Spgram(nfft, win)
    dx = LQ.DeviceBuffer.from_array(x)
    dp = LQ.DeviceBuffer(nfft * 4)
    LQ.lib().spgramcf_estimate_psd_dev(g.q, dx.p, n, dp.p)
    LQ.lib().spgramcf_synchronize(g.q)
    # tolerance 1e-4, not NRM: the oracle (like the reference, spgram.c)
    # sums the 2^19 periodograms serially in float32, whose own rounding is
    # ~sqrt(T) eps ~ 4e-5 relative here; the kernel's two-level fold is the
    # more accurate of the two (observed difference ~1e-5)
    a = 10 ** (dp.to_array(np.float32, nfft).astype(np.float64) / 10)
    b = 10 ** (np.asarray(o.estimate_psd(x), np.float64) / 10)
    assert G.nrm_err(a, b) < 1e-4


# ------------------------------------------------ launch-chunk boundaries
# The fast kernels split very long calls into launches of 2^17 / 2^18 blocks
# (firpfbch / firpfbch2) or 2^27 samples (fftfilt) so that 32-bit buffer
# offsets suffice; a call that crosses such a boundary must equal the same
# stream fed in two calls split elsewhere.  Channelizer blocks do not depend
# on where calls or launches start: bit-exact.  fftfilt segments restart at
# call boundaries: equal to float32 rounding.
@pytest.mark.parametrize("which", ["firpfbch2", "firpfbch"])
def test_channelizer_launch_chunk_boundary(which):
    r = rng(91)
    if which == "firpfbch2":
        M, per, nb, cut = 1024, 512, (1 << 18) + 77, 100003
        make = lambda: LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, 4, 60.0)   # noqa: E731
    else:
        M, per, nb, cut = 1024, 1024, (1 << 17) + 33, 70001
        make = lambda: LQ.FirPfbch(LQ.LIQUID_ANALYZER, M, m=4, As=60.0)   # noqa: E731
    x = cx(r, nb * per)
    y1 = make().execute_block(x)
    q = make()
    y2 = np.concatenate([q.execute_block(x[: cut * per]), q.execute_block(x[cut * per:])])
    assert y1.shape == y2.shape
    assert np.array_equal(y1, y2)
    # a call of several launches, then a short one: the history the first
    # call's kernel writes (on its first launch, from the whole call) carries
    cut2 = nb - 70
    q3 = make()
    y3 = np.concatenate([q3.execute_block(x[: cut2 * per]), q3.execute_block(x[cut2 * per:])])
    assert np.array_equal(y1, y3)


@pytest.mark.parametrize("t", ["crcf", "cccf"])
@pytest.mark.parametrize("hlen", [1, 2, 64, 512, 2049, 2050, 3001, 4097])
@pytest.mark.parametrize("off", [0, 8])
def test_fftfilt_segments_device_stream(t, hlen, off):
    # complex I/O: 4096-point segments up to 2049 taps, 8192-point segments
    # (k_fftfilt8k) up to 4097: 16-byte pair loads / stores when x and y are
    # 16-byte aligned (off = 0), 8-byte ones otherwise; odd stream lengths (a
    # pair straddling the end in the last segment), ragged calls, the first
    # segment's history
    r = rng(hlen * 3 + off)
    h = coefs(r, t, hlen)
    n = 300_001
    x = cx(r, n)
    o = O.FftFilt(TYPES[t], h, max(hlen - 1, 1))
    ref = o.execute_stream(x)
    g = LQ.FftFilt(h, max(hlen - 1, 1), t=t)
    dx = LQ.DeviceBuffer(8 * n + 16)
    LQ.lib().liquid_mi355x_memcpy_h2d(dx.p + off, LQ.ptr(x), x.nbytes)
    dy = LQ.DeviceBuffer(8 * n + 16)
    for a, b in ((0, 7), (7, 70_001), (70_001, 70_002), (70_002, n)):
        g.execute_block_dev(dx.p + off + 8 * a, b - a, dy.p + off + 8 * a)
    LQ.lib().liquid_mi355x_device_synchronize()
    yb = np.empty(n + 2, np.complex64)
    LQ.lib().liquid_mi355x_memcpy_d2h(LQ.ptr(yb), dy.p, yb.nbytes)
    y = yb.view(np.uint8)[off:off + 8 * n].view(np.complex64)
    assert len(ref) > n - 4097
    assert G.nrm_err(y[:len(ref)], ref) < NRM
    # in place: the block call copies the input first (segments read overlapping halos)
    g2 = LQ.FftFilt(h, max(hlen - 1, 1), t=t)
    g2.execute_block_dev(dx.p + off, n, dx.p + off)
    LQ.lib().liquid_mi355x_device_synchronize()
    LQ.lib().liquid_mi355x_memcpy_d2h(LQ.ptr(yb), dx.p, yb.nbytes)
    assert G.nrm_err(yb.view(np.uint8)[off:off + 8 * n].view(np.complex64)[:len(ref)], ref) < NRM


def test_fftfilt_launch_chunk_boundary():
    r = rng(92)
    h = r.uniform(-0.5, 0.5, 512).astype(np.float32)
    n, cut = (1 << 27) + 4097, (1 << 26) + 3
    x = cx(r, n)
    y1 = LQ.FftFilt(h, 2048).execute_block(x)
    q = LQ.FftFilt(h, 2048)
    y2 = np.concatenate([q.execute_block(x[:cut]), q.execute_block(x[cut:])])
    assert G.nrm_err(y1, y2) < 1e-6
    # a two-launch call, then a short one (the history from the first call)
    q3 = LQ.FftFilt(h, 2048)
    cut2 = n - 4001
    y3 = np.concatenate([q3.execute_block(x[:cut2]), q3.execute_block(x[cut2:])])
    assert G.nrm_err(y1, y3) < 1e-6
