"""freqmod / freqdem block calls on the GPU against the numpy model
(tests/freqmodem_model.py).

freqmod: outputs equal the model's bit for bit, table indices included, and the
accumulator after every call equals the stepped model's -- for every call
geometry (TILE and the scan's pass come from the library), for a stream cut
into calls at odd sizes, through host and device pointers, interleaved with
per-sample calls and reset, on half-way products, wrapping sums, increments
near 2^15, out-of-range products and zeros.

freqdem: every output m satisfies |m - ref phi| <= E 2^-23 |ref phi|, E = 5, phi
the float64 argument of the float32 product the model forms, and is zero in
value where phi is zero; the M-channel object equals M lag-1 objects on the
de-interleaved channels bit for bit; M on both sides of the geometry switch.

Inputs and their products are computed once and shared."""
import functools

import numpy as np
import pytest

import freqmodem_model as FM
import liquidmi as LQ

pytestmark = pytest.mark.gpu

f32 = np.float32
FIX = FM.load_fixture()


def cplx(v):
    v = np.asarray(v, np.uint32).view(f32)
    z = np.zeros(len(v) // 2, np.complex64)
    z.real[:], z.imag[:] = v[0::2], v[1::2]
    return z


TABLE = cplx(FIX["table"])
RECORDED = {c["name"]: c for c in FIX["cases"]}
CASES = FM.case_list()
TILE, PASS = LQ.FreqMod.TILE, LQ.FreqMod.SCAN_PASS
DTILE, SWITCH, FRAMES = LQ.FreqDem.TILE, LQ.FreqDem.SWITCH, LQ.FreqDem.FRAMES
N = 3 * TILE + 5
SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, N]
NSCAN = PASS * TILE + 5            # the smallest call whose tile sums take a second scan pass, plus 5
DSIZES = [1, 2, 63, 64, 65, DTILE - 1, DTILE, DTILE + 1, 3 * DTILE + 5]
MS = sorted({1, 2, 3, 64, SWITCH - 1, SWITCH, 1024})
CUTS = ([1, 7, TILE + 1], [TILE] * 3, [63, 1, 64, 65, 2])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def messages(kind, n=N):
    """wide: increments over the whole 16-bit range and beyond, sums that wrap both ways;
    halfway / range: the fixture's special products repeated across the tiles"""
    if kind == "wide":
        return frozen(FM.message(n, 5, 4.0))
    if kind == "small":
        return frozen(FM.message(n, 6, 1.0))
    m = FM.halfway_messages() if kind == "halfway" else FM.range_messages()
    return frozen(np.tile(m, n // len(m) + 1)[:n].copy())


MOD_INPUTS = [("wide", 0.5), ("wide", 1.0), ("small", 0.02), ("small", 0.08), ("halfway", 0.5), ("range", 1.0)]


@functools.lru_cache(maxsize=None)
def mod_expected(kind, kf, n=N):
    """(outputs, accumulator after each sample) from accumulator 0"""
    m = FM.ModModel(kf, TABLE)
    ph = np.cumsum(FM.increments(m.ref, messages(kind, n))) & 0xffff
    return frozen(TABLE[FM.table_index(ph)]), frozen(ph)


def advance(out, ph, start):
    """the expected outputs and accumulators of a stream that starts from accumulator `start`"""
    p = (ph + start) & 0xffff
    return TABLE[FM.table_index(p)], p


# ------------------------------------------------------------------ freqmod
@pytest.mark.parametrize("c", [c for c in CASES if c[1] == "mod"], ids=lambda c: c[0])
def test_freqmod_fixture_case(c):
    name, kind, kf, ops = c
    q = LQ.FreqMod(kf)
    assert same_bits(FM.drive_library(q, kind, ops, blocks=True), cplx(RECORDED[name]["out"]))
    assert q.get_phase() == RECORDED[name]["acc"]


@pytest.mark.parametrize("kind,kf", MOD_INPUTS, ids=lambda v: str(v))
def test_freqmod_geometry(kind, kf):
    m = messages(kind)
    out, ph = mod_expected(kind, kf)
    for n in SIZES:
        q = LQ.FreqMod(kf)
        first = q.modulate(0.37)                      # a per-sample call first: the block starts off zero
        start = q.get_phase()
        assert start == int(FM.increments(FM.mod_ref(kf), np.array([0.37], f32))[0]) and first == TABLE[
            FM.table_index(start)]
        want, p = advance(out[:n], ph[:n], start)
        assert same_bits(q.modulate_block(m[:n]), want), n
        assert q.get_phase() == p[-1], n


def test_freqmod_zero_messages():
    q = LQ.FreqMod(0.3)
    q.modulate(0.1)
    start = q.get_phase()
    s = q.modulate_block(np.zeros(N, f32))
    assert np.all(s == TABLE[FM.table_index(start)]) and q.get_phase() == start
    q.modulate_block(np.zeros(0, f32))
    assert q.get_phase() == start


def test_freqmod_across_the_scan_pass():
    """PASS tiles and one more: the scan of the tile sums carries into its second pass"""
    kf = 0.5
    m = messages("wide", NSCAN)
    out, ph = mod_expected("wide", kf, NSCAN)
    q = LQ.FreqMod(kf)
    assert same_bits(q.modulate_block(m), out)
    assert q.get_phase() == ph[-1]
    # on from there, device pointers, a call of exactly PASS tiles and the rest
    dm, ds = LQ.DeviceBuffer.from_array(m), LQ.DeviceBuffer(8 * NSCAN)
    cut = PASS * TILE
    q.modulate_block_dev(dm.p, cut, ds.p)
    q.modulate_block_dev(dm.p + 4 * cut, NSCAN - cut, ds.p + 8 * cut)
    q.synchronize()
    want, p = advance(out, ph, int(ph[-1]))
    assert same_bits(ds.to_array(np.complex64, NSCAN), want)
    assert q.get_phase() == p[-1]


@pytest.mark.parametrize("kind,kf", [("wide", 0.5), ("halfway", 0.5), ("range", 1.0)], ids=lambda v: str(v))
def test_freqmod_stream_cut_into_calls(kind, kf):
    m = messages(kind)
    out, ph = mod_expected(kind, kf)
    for sizes in CUTS:
        for dev in (False, True):
            q = LQ.FreqMod(kf)
            dm, ds = LQ.DeviceBuffer.from_array(m), LQ.DeviceBuffer(8 * N)
            got, k, sizes_left = np.zeros(N, np.complex64), 0, list(sizes)
            while k < N:
                c = min(sizes_left.pop(0) if sizes_left else N - k, N - k)
                if dev:
                    q.modulate_block_dev(dm.p + 4 * k, c, ds.p + 8 * k)
                else:
                    got[k:k + c] = q.modulate_block(m[k:k + c])
                k += c
                assert q.get_phase() == ph[k - 1], (sizes, dev, k)
            if dev:
                q.synchronize()
                got = ds.to_array(np.complex64, N)
            assert same_bits(got, out), (sizes, dev)


def test_freqmod_interleaved_with_per_sample_calls_and_reset():
    kf = 0.5
    m = messages("wide")
    q, model = LQ.FreqMod(kf), FM.ModModel(kf, TABLE)
    dm, ds = LQ.DeviceBuffer.from_array(m), LQ.DeviceBuffer(8 * N)
    k = 0
    for op, c in (("b", TILE + 5), ("s", 3), ("d", 65), ("s", 1), ("r", 0), ("d", TILE), ("b", 1), ("r", 0), ("s", 2),
                  ("b", 700), ("d", 2), ("d", 1)):
        x = m[k:k + c]
        if op == "r":
            q.reset()
            model.reset()
        elif op == "s":
            assert same_bits(np.array([q.modulate(v) for v in x], np.complex64), model.step(x)), (op, k)
        elif op == "b":
            assert same_bits(q.modulate_block(x), model.block(x)), (op, k)
        else:
            q.modulate_block_dev(dm.p + 4 * k, c, ds.p + 8 * k)
            q.synchronize()
            assert same_bits(ds.to_array(np.complex64, k + c)[k:], model.block(x)), (op, k)
        assert q.get_phase() == model.phase, (op, k)
        k += c


def test_freqmod_unaligned_device_pointers():
    kf, n = 0.5, N - 1
    m = messages("wide")
    out, ph = mod_expected("wide", kf)
    for om, os_ in ((4, 0), (0, 8), (4, 8), (8, 8)):
        q = LQ.FreqMod(kf)
        dm, ds = LQ.DeviceBuffer.from_array(np.concatenate([np.zeros(om // 4, f32), m])), LQ.DeviceBuffer(8 * N + 16)
        q.modulate_block_dev(dm.p + om, n, ds.p + os_)
        q.synchronize()
        assert same_bits(ds.to_array(np.complex64, N + 2)[os_ // 8:os_ // 8 + n], out[:n]), (om, os_)
        assert q.get_phase() == ph[n - 1]


# ------------------------------------------------------------------ freqdem
@functools.lru_cache(maxsize=None)
def samples(n=3 * DTILE + 5, seed=11):
    return frozen(FM.dem_input(n, seed))


def dem_len(M):
    """long enough for a second walk of frames and a ragged last frame"""
    return max(3 * DTILE + 5, (2 * FRAMES + 3) * M + 5)


@functools.lru_cache(maxsize=None)
def products(M, n, seed=11):
    re, im = FM.DemModel(0.08, M).block(samples(n, seed))
    return frozen(re), frozen(im)


WORST = {}


def dem_check(what, m, re, im, ref, blocks=True):
    """blocks: every output came from a block call (the kernel's float64 argument, not the
    host's atan2f): its worst ratio is printed apart, for DESIGN.md"""
    r = FM.check(what, m, re, im, ref)
    if blocks:
        WORST["gpu"] = max(WORST.get("gpu", 0.0), r * FM.E)
        print("freqdem block calls on the GPU so far: worst %.4g of the E = 1 bound" % WORST["gpu"])


@pytest.mark.parametrize("c", [c for c in CASES if c[1] == "dem"], ids=lambda c: c[0])
def test_freqdem_fixture_case(c):
    name, kind, kf, ops = c
    re, im, ref = FM.dem_case_products(kf, ops)
    dem_check("gpu " + name, FM.drive_library(LQ.FreqDem(kf), kind, ops, blocks=True), re, im, ref,
              blocks=all(op == "b" for op, _ in ops))


@pytest.mark.parametrize("M", MS)
def test_freqdem_geometry(M):
    nmax = dem_len(M)
    x, (re, im), ref = samples(nmax), products(M, nmax), FM.dem_ref(0.08)
    for n in DSIZES + [nmax]:
        q = LQ.FreqDem(0.08, M)
        # from a zero state the first M products are those of the whole stream's first M
        dem_check("geometry M=%d n=%d" % (M, n), q.demodulate_block(x[:n]), re[:n], im[:n], ref)


@pytest.mark.parametrize("M", MS)
def test_freqdem_channels_equal_lag_one_objects(M):
    n = dem_len(M)
    x = samples(n)
    got = LQ.FreqDem(0.08, M).demodulate_block(x)
    one = LQ.FreqDem(0.08)
    for ch in range(M):
        one.reset()                     # a reset object is a new one
        assert same_bits(got[ch::M], one.demodulate_block(x[ch::M])), ch


@pytest.mark.parametrize("M", MS)
def test_freqdem_stream_cut_into_calls(M):
    """cuts shorter than M included; host and device pointers give the whole stream's bits"""
    n = 3 * DTILE + 5
    x = samples(n)
    whole = LQ.FreqDem(0.08, M).demodulate_block(x)
    for sizes in CUTS + ([5, M, M - 1 or 1, 1, M + 1, 3],):
        for dev in (False, True):
            q = LQ.FreqDem(0.08, M)
            dx, dm = LQ.DeviceBuffer.from_array(x), LQ.DeviceBuffer(4 * n)
            got, k, left = np.zeros(n, f32), 0, list(sizes)
            while k < n:
                c = min(left.pop(0) if left else n - k, n - k)
                if dev:
                    q.demodulate_block_dev(dx.p + 8 * k, c, dm.p + 4 * k)
                else:
                    got[k:k + c] = q.demodulate_block(x[k:k + c])
                k += c
            if dev:
                q.synchronize()
                got = dm.to_array(f32, n)
            assert same_bits(got, whole), (sizes, dev)


@pytest.mark.parametrize("M", [1, 3, SWITCH])
def test_freqdem_interleaved_with_per_sample_calls_and_reset(M):
    n = 3 * DTILE + 5
    x = samples(n, 12)
    q, model, ref = LQ.FreqDem(0.08, M), FM.DemModel(0.08, M), FM.dem_ref(0.08)
    dx, dm = LQ.DeviceBuffer.from_array(x), LQ.DeviceBuffer(4 * n)
    k = 0
    for op, c in (("b", DTILE + 5), ("s", 3), ("d", 65), ("s", 1), ("d", 2), ("b", 1), ("r", 0), ("d", DTILE), ("s", 2),
                  ("b", 700), ("r", 0), ("s", M + 1), ("d", 2 * M + 1), ("b", 3)):
        xs = x[k:k + c]
        if op == "r":
            q.reset()
            model.reset()
            continue
        if op == "s":
            got = np.array([q.demodulate(v) for v in xs], f32)
        elif op == "b":
            got = q.demodulate_block(xs)
        else:
            q.demodulate_block_dev(dx.p + 8 * k, c, dm.p + 4 * k)
            q.synchronize()
            got = dm.to_array(f32, k + c)[k:]
        re, im = model.block(xs)
        dem_check("interleaved M=%d %s at %d" % (M, op, k), got, re, im, ref, blocks=op != "s")
        k += c


def test_freqdem_unaligned_device_pointers():
    n = 3 * DTILE + 4
    x = samples()
    for M in (1, SWITCH):
        want = LQ.FreqDem(0.08, M).demodulate_block(x[1:1 + n])
        q = LQ.FreqDem(0.08, M)
        dx, dm = LQ.DeviceBuffer.from_array(x), LQ.DeviceBuffer(4 * n + 8)
        q.demodulate_block_dev(dx.p + 8, n, dm.p + 4)
        q.synchronize()
        assert same_bits(dm.to_array(f32, n + 2)[1:1 + n], want), M


# ------------------------------------------------------------------ chains on device pointers
@pytest.mark.parametrize("kf", [0.02, 0.04, 0.08])
def test_roundtrip_on_device_pointers(kf):
    """freqmod -> freqdem with no host copy between: the autotest's message and tolerance"""
    m = FM.cosines(N)
    mod, dem = LQ.FreqMod(kf), LQ.FreqDem(kf)
    dm, ds, dy = LQ.DeviceBuffer.from_array(m), LQ.DeviceBuffer(8 * N), LQ.DeviceBuffer(4 * N)
    mod.modulate_block_dev(dm.p, N, ds.p)
    mod.synchronize()
    dem.demodulate_block_dev(ds.p, N, dy.p)
    dem.synchronize()
    y = dy.to_array(f32, N)
    assert np.max(np.abs(y[1:] - m[1:])) < 5e-2
    s = FM.ModModel(kf, TABLE).block(m)
    assert same_bits(ds.to_array(np.complex64, N), s)
    re, im = FM.DemModel(kf).block(s)
    dem_check("round trip kf=%g" % kf, y, re, im, FM.dem_ref(kf))


def test_channelizer_into_a_freqdem_bank():
    """firpfbch2 analyzer -> freqdem_create_channels on the channelizer's stream, device pointers
    only.  A slow FM signal (deviation within the channel) sits in channel 4; a frame advances
    M / 2 samples, so with kf 32 times the modulator's the bank's slot 4 is the message averaged
    over the frame, delayed by the filter's m M samples = 2 m frames."""
    M, m, kf, frames = 64, 4, 0.004, 400
    n = frames * M // 2
    i = np.arange(n) / 256.0
    msg = (0.3 * np.cos(2 * np.pi * 0.013 * i) + 0.2 * np.cos(2 * np.pi * 0.021 * i + 0.4)
           + 0.4 * np.cos(2 * np.pi * 0.037 * i + 1.7)).astype(f32)
    s = FM.ModModel(kf, TABLE).block(msg)
    x = (s * np.exp(2j * np.pi * 4 / M * np.arange(n))).astype(np.complex64)
    ch = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, m, 60.0)
    dem = LQ.FreqDem(32 * kf, M)
    dx, dc, dy = LQ.DeviceBuffer.from_array(x), LQ.DeviceBuffer(8 * frames * M), LQ.DeviceBuffer(4 * frames * M)
    dem.set_stream(ch.get_stream())
    try:
        ch.execute_block_dev(dx.p, frames, dc.p)
        dem.demodulate_block_dev(dc.p, frames * M, dy.p)
        dem.synchronize()
    finally:
        dem.set_stream(None)
    c, y = dc.to_array(np.complex64, frames * M), dy.to_array(f32, frames * M)
    # every slot is the lag-M discriminator of the channelizer's own output (samples inside the
    # magnitudes the bound is stated for)
    prev = np.concatenate([np.zeros(M, np.complex64), c[:-M]])
    keep = (np.abs(c) >= 2.0 ** -30) & ((np.abs(prev) >= 2.0 ** -30) | (prev == 0))
    assert keep.sum() > frames * M // 2
    re, im = FM.DemModel(32 * kf, M).block(c)
    dem_check("channelizer bank", y[keep], re[keep], im[keep], FM.dem_ref(32 * kf))
    audio, want, lag = y[4::M], msg.reshape(frames, M // 2).mean(1), 2 * m
    assert np.max(np.abs(audio[20:] - want[20 - lag:frames - lag])) < 5e-2
