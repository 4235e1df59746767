"""nco_crcf without a GPU: the numpy model (tests/nco_model.py) equals what the
reference returned (tests/golden/nco.json) bit for bit, the recorded outputs
meet the per-output bound (it is reachable), two wrong models miss it (the
checker is pinned), the library's per-sample interface equals the fixture bit
for bit with no device, its phase plan serves the stepped phases, and the
library exports the whole interface.

LIQUID_VCO outputs depend on the C library's sinf / cosf, which numpy does not
restate: for that type phases and frequencies are compared bit for bit and
outputs against the bound."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import liquidmi as LQ
import nco_model as NM

FIX = NM.load_fixture()
TABLE = np.array(FIX["table"], np.uint32).view(np.float32)
CASES = FIX["cases"]
f32 = np.float32


def case_ops(c):
    return [(n, a) for n, a in c["ops"]]


def case_input(c):
    return NM.stream_input(NM.samples_of(case_ops(c)), c["seed"])


def recorded(c):
    return np.array(c["out"], np.uint32).view(f32)


def compare(what, c, vals, phase):
    """bit for bit (nco), or phases / frequencies bit for bit and outputs within the bound (vco)"""
    ops, ref = case_ops(c), recorded(c)
    assert len(vals) == len(ref)
    assert NM.bits(phase) == c["phase"], what
    if c["type"] == NM.NCO:
        assert np.array_equal(np.asarray(vals, f32).view(np.uint32), ref.view(np.uint32)), what
        return
    assert np.array_equal(NM.state_values(ops, vals).view(np.uint32), NM.state_values(ops, ref).view(np.uint32)), what
    x = case_input(c)
    _, recs = NM.Model(c["type"], TABLE).run(ops, x)
    if recs:
        y64, xs = NM.reference64(c["type"], recs, x)
        NM.check(what, NM.mix_outputs(ops, vals), y64, xs)


def test_fixture_shape():
    assert len(TABLE) == 256 and len(CASES) == 14
    assert all(NM.samples_of(case_ops(c)) <= 4096 for c in CASES)
    assert {c["type"] for c in CASES} == {NM.NCO, NM.VCO}
    assert [NM.bits(f32(d)) for d in NM.LONG_D] == [e["d"] for e in FIX["long"]]


def test_table_is_the_sine_of_the_rounded_angle():
    """tab[i] = sinf(a_i), a_i the float32 angle: within one unit of the float64 sine of a_i,
    and up to a few units away from the sine of the exact angle"""
    a = NM.table_angles().astype(np.float64)
    assert np.max(np.abs(TABLE.astype(np.float64) - np.sin(a))) <= NM.U24
    ideal = np.sin(2 * np.pi * np.arange(256) / 256)
    print("nco table: up to %.3g 2^-24 from the sine of the exact angle"
          % (np.max(np.abs(TABLE.astype(np.float64) - ideal)) / NM.U24))
    assert np.array_equal(NM.index(NM.table_phases()), np.arange(256))


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_model_equals_the_fixture(c):
    m = NM.Model(c["type"], TABLE)
    vals, _ = m.run(case_ops(c), case_input(c))
    compare("model " + c["name"], c, vals, m.theta)


@pytest.mark.parametrize("c", [c for c in CASES if NM.samples_of(case_ops(c))], ids=lambda c: c["name"])
def test_reference_meets_the_bound(c):
    ops, x = case_ops(c), case_input(c)
    _, recs = NM.Model(c["type"], TABLE).run(ops, x)
    y64, xs = NM.reference64(c["type"], recs, x)
    NM.check("reference " + c["name"], NM.mix_outputs(ops, recorded(c)), y64, xs)


@pytest.mark.parametrize("e", FIX["long"], ids=lambda e: "d=%g" % NM.unbits(e["d"]))
def test_long_walk(e):
    assert NM.bits(NM.walk(0.0, NM.unbits(e["d"]), NM.LONG_STEPS)[1]) == e["phase"]


def test_contracted_index_misses_the_bound():
    """theta * K + 512 fused moves an index at a bin edge: d_theta = 2.5 meets one within 2^17 samples"""
    n = 1 << 17
    th, _ = NM.walk(0.0, 2.5, n)
    good, bad = NM.index(th), NM.index_contracted(th)
    moved = np.nonzero(good != bad)[0]
    assert len(moved) >= 1
    x = NM.stream_input(n, 5)
    x[moved] = 1 + 1j
    c64, s64 = NM.rotator64(NM.NCO, th)
    y64 = NM.mix64(x, c64, s64, False)
    NM.check("separately rounded index", NM.mix32(x, TABLE[(good + 64) & 0xff], TABLE[good], False), y64, x)
    r = NM.report(NM.mix32(x, TABLE[(bad + 64) & 0xff], TABLE[bad], False), y64, x)
    print("nco contracted index: %d of %d indices move, worst %.4g x the bound" % (len(moved), n, r))
    assert r > 100


@pytest.mark.parametrize("typ", [NM.NCO, NM.VCO], ids=["nco", "vco"])
def test_float64_phase_misses_the_bound(typ):
    n = 4096
    th, _ = NM.walk(0.3, 0.1, n)
    th64 = NM.walk64(0.3, 0.1, n)
    x = NM.stream_input(n, 6)
    c64, s64 = NM.rotator64(typ, th)
    y64 = NM.mix64(x, c64, s64, True)
    c, s = NM.rotator32(typ, th, TABLE)
    NM.check("float32 phase", NM.mix32(x, c, s, True), y64, x)
    c, s = NM.rotator32(typ, th64.astype(f32), TABLE)
    r = NM.report(NM.mix32(x, c, s, True), y64, x)
    print("nco float64 phase accumulator (%s): worst %.4g x the bound" % ("nco" if typ == NM.NCO else "vco", r))
    assert r > 10


# ------------------------------------------------------------------ the library's host interface (no GPU)
def test_library_table():
    q = LQ.NCO(LQ.LIQUID_NCO)
    got = np.empty(256, f32)
    for i, phi in enumerate(NM.table_phases()):
        q.set_phase(phi)
        got[i] = q.sin()
    assert np.array_equal(got.view(np.uint32), TABLE.view(np.uint32))


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_library_per_sample_equals_the_fixture(c):
    """block ops as per-sample loops (the reference's own definition of them): no device is touched"""
    q = LQ.NCO(c["type"])
    vals = NM.drive_library(q, case_ops(c), case_input(c), blocks=False)
    compare("library " + c["name"], c, vals, q.get_phase())


@pytest.mark.parametrize("e", FIX["long"], ids=lambda e: "d=%g" % NM.unbits(e["d"]))
def test_library_long_walk(e):
    q = LQ.NCO(LQ.LIQUID_VCO)
    q.set_frequency(NM.unbits(e["d"]))
    step, h = LQ.lib().nco_crcf_step, q.q
    for _ in range(NM.LONG_STEPS):
        step(h)
    assert NM.bits(q.get_phase()) == e["phase"]


def test_library_unwrap(capfd):
    t = NM.unwrap_input()
    assert np.array_equal(LQ.unwrap_phase(t).view(np.uint32), np.array(FIX["unwrap"]["basic"], np.uint32))
    capfd.readouterr()
    assert np.array_equal(LQ.unwrap_phase(t, advanced=True).view(np.uint32),
                          np.array(FIX["unwrap"]["advanced"], np.uint32))
    assert "warning: liquid_unwrap_phase2() has not yet been tested!" in capfd.readouterr().err


def test_library_runs_without_a_device():
    """create, the per-sample interface and print in a process that cannot see a GPU"""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import liquidmi as LQ\n"
            "q = LQ.NCO(LQ.LIQUID_NCO); q.set_frequency(0.1); q.pll_step(0.2); q.step(); q.mix_up(1 + 0j)\n"
            "LQ.lib().nco_crcf_print(q.q); print(q.device_eligible)\n")
    e = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code, LQ.HERE], capture_output=True, text=True, env=e, timeout=60)
    assert out.returncode == 0, out.stderr
    assert "nco [type: nco" in out.stdout and "True" in out.stdout.split()


@pytest.fixture(scope="module")
def orbit():
    """d_theta = 0.1 from phase 0: pre-period, period (from the model, not assumed) and the
    stepped phases over pre-period + 2 periods + 5 positions"""
    pre, per = NM.cycle(0.0, 0.1)
    n = pre + 2 * per + 5
    return pre, per, n, NM.walk(0.0, 0.1, n)[0]


@pytest.mark.parametrize("periodic", [0, 1], ids=["direct", "periodic"])
def test_walk_equals_the_stepped_model(orbit, periodic):
    pre, per, n, th = orbit
    got = LQ.nco_walk(LQ.LIQUID_NCO, 0.0, 0.1, n, periodic)
    assert got is not None
    gth, gidx, gpre, gper = got
    assert np.array_equal(gth.view(np.uint32), th.view(np.uint32))
    assert np.array_equal(gidx.astype(np.int64), NM.index(th))
    assert (gpre, gper) == ((pre, per) if periodic else (0, 0))


@pytest.mark.parametrize("theta0,d", [(0.3, 0.0), (0.0, float(f32(np.pi / 2))), (3.0, -3.0), (-1.0, 2.5)])
def test_walk_short_orbits(theta0, d):
    n = 3000
    th = NM.walk(theta0, d, n)[0]
    for periodic in (0, 1):
        got = LQ.nco_walk(LQ.LIQUID_VCO, theta0, d, n, periodic)
        if got is None:      # no period within the limit: allowed for the periodic form only
            assert periodic
            continue
        assert np.array_equal(got[0].view(np.uint32), th.view(np.uint32))


def test_library_exports_the_interface():
    names = [n for n in LQ.header_functions() if n.startswith("nco_crcf_")]
    want = ["create", "destroy", "print", "reset", "get_frequency", "set_frequency", "adjust_frequency", "get_phase",
            "set_phase", "adjust_phase", "step", "sin", "cos", "sincos", "cexpf", "pll_set_bandwidth", "pll_step",
            "mix_up", "mix_down", "mix_block_up", "mix_block_down", "mix_block_up_dev", "mix_block_down_dev",
            "device_eligible", "set_stream", "synchronize"]
    assert sorted(names) == sorted("nco_crcf_" + w for w in want)
    L = ctypes.CDLL(LQ.LIB_PATH)
    extra = ["liquid_unwrap_phase", "liquid_unwrap_phase2", "liquid_mi355x_nco_tile", "liquid_mi355x_nco_checkpoint",
             "liquid_mi355x_nco_walk"]
    for n in names + extra:
        assert hasattr(L, n), n
        assert n in LQ.header_functions(), n
    assert LQ.NCO.TILE >= 64 and LQ.NCO.TILE % LQ.NCO.CHECKPOINT == 0
    hdr = open(LQ.HEADER).read()
    assert re.search(r"typedef enum \{ LIQUID_NCO = 0, LIQUID_VCO \} liquid_ncotype;", hdr)
    assert "typedef struct nco_crcf_s *nco_crcf;" in hdr


def test_reference_program_compiles_and_links(tmp_path):
    """a C program written against liquid.h's nco interface, compiled against include/liquid.h"""
    src = tmp_path / "t.c"
    src.write_text('#include <complex.h>\n#include "liquid.h"\n'
                   "int main(void) {\n"
                   "    nco_crcf q = nco_crcf_create(LIQUID_VCO);\n"
                   "    liquid_float_complex x[4] = {1, 1, 1, 1}, y[4];\n"
                   "    float s, c, t[3] = {0, 3, -3};\n"
                   "    nco_crcf_set_frequency(q, 0.1f); nco_crcf_set_phase(q, 0.2f); nco_crcf_adjust_phase(q, 0.1f);\n"
                   "    nco_crcf_adjust_frequency(q, 0.1f); nco_crcf_pll_set_bandwidth(q, 0.1f); nco_crcf_pll_step(q, 0.1f);\n"
                   "    nco_crcf_step(q); nco_crcf_sincos(q, &s, &c); nco_crcf_cexpf(q, y); nco_crcf_mix_up(q, x[0], y);\n"
                   "    nco_crcf_mix_down(q, x[0], y); s = nco_crcf_sin(q) + nco_crcf_cos(q) + nco_crcf_get_phase(q)\n"
                   "        + nco_crcf_get_frequency(q);\n"
                   "    if (s > 1e9f) { nco_crcf_mix_block_up(q, x, y, 4); nco_crcf_mix_block_down(q, x, y, 4); }\n"
                   "    liquid_unwrap_phase(t, 3); nco_crcf_print(q); nco_crcf_reset(q); nco_crcf_destroy(q);\n"
                   "    return 0;\n}\n")
    libdir = os.path.dirname(LQ.LIB_PATH)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-I", os.path.join(LQ.ROOT, "include"),
                           str(src), "-L", libdir, "-lliquid_mi355x", "-Wl,-rpath," + libdir, "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("nco [type: vco")
