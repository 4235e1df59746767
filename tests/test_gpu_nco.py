"""nco_crcf block mixing on the GPU against the numpy model (tests/nco_model.py):
every output component within E 2^-24 (|Re x| + |Im x|), E = 5, of the float64
product of the sample with the rotator at the replayed float32 phase, exactly
zero where the sample is zero, and the phase after every call equal to the
stepped model's bit for bit -- for every call geometry of the kernel, however
the stream is cut into calls, in place or not, through host or device pointers,
across state changes, and under both forms of the phase plan.

TILE (samples per workgroup) comes from the library; N = 3 TILE + 5.  Phases
are walked once per frequency and shared."""
import functools

import numpy as np
import pytest

import liquidmi as LQ
import nco_model as NM

pytestmark = pytest.mark.gpu

TILE = LQ.NCO.TILE
N = 3 * TILE + 5
FIX = NM.load_fixture()
TABLE = np.array(FIX["table"], np.uint32).view(np.float32)
f32 = np.float32
PI32 = float(f32(np.pi))
TYPES = [NM.NCO, NM.VCO]
TYPE_IDS = ["nco", "vco"]
SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, N]
FREQS = [0.0, 0.1, -0.7, 3.0, 1e-3, PI32, -PI32]


@functools.lru_cache(maxsize=None)
def stream(n=N, seed=42):
    x = NM.stream_input(n, seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def phases(theta0, d, n=N):
    """the phases before samples 0 .. n-1 and after each of them: n + 1 values"""
    th, last = NM.walk(theta0, d, n)
    th = np.append(th, last).astype(f32)
    th.setflags(write=False)
    return th


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def make(typ, theta0, d, plan=None):
    q = LQ.NCO(typ, plan=plan)
    q.set_phase(theta0)
    q.set_frequency(d)
    return q


def mix(q, x, down, **kw):
    return (q.mix_block_down if down else q.mix_block_up)(x, **kw)


def check(what, typ, th, x, down, y):
    c64, s64 = NM.rotator64(typ, th)
    return NM.check(what, y, NM.mix64(x, c64, s64, down), x)


def run_calls(q, x, sizes, down):
    parts, k = [], 0
    sizes = list(sizes)
    while k < len(x):
        c = min(sizes.pop(0) if sizes else len(x) - k, len(x) - k)
        parts.append(mix(q, x[k:k + c], down))
        k += c
    return np.concatenate(parts)


# ------------------------------------------------------------------ 1 the fixture's cases
@pytest.mark.parametrize("c", FIX["cases"], ids=lambda c: c["name"])
def test_fixture_case(c):
    ops = [(n, a) for n, a in c["ops"]]
    x = NM.stream_input(NM.samples_of(ops), c["seed"])
    ref = np.array(c["out"], np.uint32).view(f32)
    q = LQ.NCO(c["type"])
    vals = NM.drive_library(q, ops, x, blocks=True)
    assert NM.bits(q.get_phase()) == c["phase"]
    assert same_bits(NM.state_values(ops, vals), NM.state_values(ops, ref))
    _, recs = NM.Model(c["type"], TABLE).run(ops, x)
    if recs:
        y64, xs = NM.reference64(c["type"], recs, x)
        NM.check("gpu " + c["name"], NM.mix_outputs(ops, vals), y64, xs)
        if c["type"] == NM.NCO:
            # table lookups and separately rounded products: the reference's own values
            assert np.array_equal(NM.mix_outputs(ops, vals), NM.mix_outputs(ops, ref))


# ------------------------------------------------------------------ 2 geometry
@pytest.mark.parametrize("d", FREQS, ids=lambda d: "d=%.4g" % d)
@pytest.mark.parametrize("down", [0, 1], ids=["up", "down"])
@pytest.mark.parametrize("typ", TYPES, ids=TYPE_IDS)
def test_geometry(typ, down, d):
    th = phases(0.3, d)
    for n in SIZES:
        x = stream()[:n]
        q = make(typ, 0.3, d)
        y = mix(q, x, down)
        assert NM.bits(q.get_phase()) == NM.bits(th[n]), n
        assert np.all(y[x == 0] == 0)
        check("geometry %s %s d=%g n=%d" % (TYPE_IDS[typ], "down" if down else "up", d, n), typ, th[:n], x, down, y)


def test_index_at_a_bin_edge():
    """d_theta = 2.5 from phase 0 meets, within 2^17 samples, a phase whose table index moves if
    theta * K + 512 is fused (tests/test_nco_model.py): the kernel's index must not"""
    n = 1 << 17
    th = phases(0.0, 2.5, n)
    moved = np.nonzero(NM.index(th[:n]) != NM.index_contracted(th[:n]))[0]
    assert len(moved) >= 1
    x = stream(n, 5).copy()
    x[moved] = 1 + 1j
    for plan in ("direct", "periodic"):
        q = make(NM.NCO, 0.0, 2.5, plan)
        y = mix(q, x, 0)
        assert NM.bits(q.get_phase()) == NM.bits(th[n])
        check("bin edge %s" % plan, NM.NCO, th[:n], x, 0, y)
        k = NM.index(th[:n])
        assert np.array_equal(y, NM.mix32(x, TABLE[(k + 64) & 0xff], TABLE[k], False))


# ------------------------------------------------------------------ 3 splitting
@pytest.mark.parametrize("d", [0.1, -0.7, PI32], ids=lambda d: "d=%.4g" % d)
@pytest.mark.parametrize("typ", TYPES, ids=TYPE_IDS)
def test_splitting(typ, d):
    x = stream()
    whole = mix(make(typ, 0.3, d), x, 0)
    check("whole", typ, phases(0.3, d)[:N], x, 0, whole)
    for sizes in ([1, 7, TILE + 1], [TILE] * 3, [63, 1, 64, 65, 2]):
        q = make(typ, 0.3, d)
        assert same_bits(run_calls(q, x, sizes, 0), whole), sizes
        assert NM.bits(q.get_phase()) == NM.bits(phases(0.3, d)[N])


# ------------------------------------------------------------------ 4 in place, host and device pointers
@pytest.mark.parametrize("down", [0, 1], ids=["up", "down"])
@pytest.mark.parametrize("typ", TYPES, ids=TYPE_IDS)
def test_in_place_and_device_pointers(typ, down):
    x, d = stream(), -0.7
    y = mix(make(typ, 0.3, d), x, down)
    check("host pointers", typ, phases(0.3, d)[:N], x, down, y)
    assert same_bits(mix(make(typ, 0.3, d), x, down, inplace=True), y)
    # device pointers, out of place and in place
    q = make(typ, 0.3, d)
    dx, dy = LQ.DeviceBuffer.from_array(x), LQ.DeviceBuffer(x.nbytes)
    mix(q, dx, down, y=dy)
    q.synchronize()
    assert same_bits(dy.to_array(np.complex64, N), y)
    assert same_bits(dx.to_array(np.complex64, N), x)
    q = make(typ, 0.3, d)
    mix(q, dx, down)
    q.synchronize()
    assert same_bits(dx.to_array(np.complex64, N), y)
    assert NM.bits(q.get_phase()) == NM.bits(phases(0.3, d)[N])
    # pointers that are not 16-byte aligned (8-byte accesses), and mixed alignment
    pad = np.concatenate([np.zeros(1, np.complex64), x])
    for ox, oy in ((8, 8), (8, 0), (0, 8)):
        q = make(typ, 0.3, d)
        dx, dy = LQ.DeviceBuffer.from_array(pad), LQ.DeviceBuffer(pad.nbytes)
        (q.mix_block_down_dev if down else q.mix_block_up_dev)(dx.p + ox, dy.p + oy, N - 1)
        q.synchronize()
        got = dy.to_array(np.complex64, N + 1)[oy // 8:oy // 8 + N - 1]
        want = mix(make(typ, 0.3, d), pad[ox // 8:ox // 8 + N - 1], down)
        assert same_bits(got, want), (ox, oy)


# ------------------------------------------------------------------ 5 state changes between blocks
@pytest.mark.parametrize("plan", [None, "direct", "periodic"], ids=["auto", "direct", "periodic"])
@pytest.mark.parametrize("typ", TYPES, ids=TYPE_IDS)
def test_state_changes(typ, plan):
    b = lambda v: NM.bits(f32(v))   # noqa: E731
    ops = [("P", b(0.3)), ("F", b(0.1)), ("U", TILE + 5), ("g", 0), ("F", b(-0.7)), ("D", 100), ("g", 0),
           ("p", b(1.0)), ("U", 65), ("g", 0), ("L", b(0.2)), ("U", 64), ("g", 0), ("S", 3), ("U", 10), ("g", 0),
           ("S", 70), ("D", 9), ("g", 0), ("m", 0), ("U", 7), ("g", 0), ("R", 0), ("g", 0), ("F", b(1e-3)), ("U", 130),
           ("g", 0), ("R", 0), ("F", b(1e-3)), ("D", 131), ("g", 0)]
    x = stream(NM.samples_of(ops), 7)
    q = LQ.NCO(typ, plan=plan)
    vals = NM.drive_library(q, ops, x, blocks=True)
    m = NM.Model(typ, TABLE)
    mv, recs = m.run(ops, x)
    assert NM.bits(q.get_phase()) == NM.bits(m.theta)
    assert same_bits(NM.state_values(ops, vals), NM.state_values(ops, mv))
    y64, xs = NM.reference64(typ, recs, x)
    NM.check("state changes %s %s" % (TYPE_IDS[typ], plan), NM.mix_outputs(ops, vals), y64, xs)


# ------------------------------------------------------------------ 6 plan kinds
@functools.lru_cache(maxsize=None)
def orbit():
    """d_theta = 0.1 from phase 0: pre-period and period from the model, not assumed"""
    return NM.cycle(0.0, 0.1)


@pytest.mark.parametrize("typ", TYPES, ids=TYPE_IDS)
def test_plan_kinds(typ):
    pre, per = orbit()
    n = pre + 2 * per + TILE + 5
    x, th = stream(n, 9), phases(0.0, 0.1, n)
    runs = {}
    for plan, sizes in (("direct", []), ("periodic", []), (None, []), ("periodic", [pre + per, per]),
                        ("periodic", [pre + per - 1, 2, per - 1]), ("direct", [pre + per, per]),
                        ("periodic", [pre, per, per])):
        q = make(typ, 0.0, 0.1, plan)
        runs[(plan, tuple(sizes))] = run_calls(q, x, sizes, 1)
        assert NM.bits(q.get_phase()) == NM.bits(th[n]), (plan, sizes)
    first = runs[("direct", ())]
    check("plan kinds %s" % TYPE_IDS[typ], typ, th[:n], x, 1, first)
    for k, y in runs.items():
        assert same_bits(y, first), k


def test_unforced_plan_across_its_switch():
    """an object left to itself walks direct plans first and builds the periodic one once they
    have covered 2^22 positions of an orbit: three calls of 2^22 + 3 samples cross that point,
    and give the bits and phases of an object held to direct plans; the last phase is the one
    the library's own plan walk serves (checked against the model in tests/test_nco_model.py)"""
    n = (1 << 22) + 3
    x = np.tile(stream(), n // N + 1)[:n]
    free, held = make(NM.NCO, 0.3, 0.1), make(NM.NCO, 0.3, 0.1, "direct")
    for _ in range(3):
        assert same_bits(mix(free, x, 1), mix(held, x, 1))
        assert NM.bits(free.get_phase()) == NM.bits(held.get_phase())
    th = LQ.nco_walk(LQ.LIQUID_NCO, 0.3, 0.1, 3 * n + 1, False)[0]
    assert NM.bits(free.get_phase()) == NM.bits(th[3 * n])


# ------------------------------------------------------------------ 7 beyond the kernel's range
@pytest.mark.parametrize("typ", TYPES, ids=TYPE_IDS)
def test_large_frequency_runs_in_the_host_loop(typ):
    q = make(typ, 0.3, 7.0)
    assert not q.device_eligible
    assert make(typ, 0.3, 3.0).device_eligible
    n = 300
    x, th = stream()[:n], phases(0.3, 7.0)
    y = mix(q, x, 0)
    assert NM.bits(q.get_phase()) == NM.bits(th[n])
    if typ == NM.VCO:      # the NCO type's index is undefined out there, as in the reference
        check("host loop", typ, th[:n], x, 0, y)
    dx = LQ.DeviceBuffer.from_array(x)
    q = make(typ, 0.3, 7.0)
    mix(q, dx, 0)
    q.synchronize()
    assert same_bits(dx.to_array(np.complex64, n), y)
