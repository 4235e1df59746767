"""freqmod / freqdem without a GPU: the numpy model (tests/freqmodem_model.py)
equals what the reference returned (tests/golden/freqmodem.json) -- freqmod
outputs and accumulator bit for bit, freqdem outputs within the bound --, two
wrong roundings miss the half-way case (the checker is pinned), the library's
per-sample calls equal the fixture with no device, the library exports the
interface, a program written against liquid.h compiles and links, and the
reference's round-trip autotest holds through the library's host calls."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import freqmodem_model as FM
import liquidmi as LQ

FIX = FM.load_fixture()
f32 = np.float32


def cplx(v):
    v = np.asarray(v, np.uint32).view(f32)
    z = np.zeros(len(v) // 2, np.complex64)
    z.real[:], z.imag[:] = v[0::2], v[1::2]
    return z


TABLE = cplx(FIX["table"])
RECORDED = {c["name"]: c for c in FIX["cases"]}
CASES = FM.case_list()
MOD = [c for c in CASES if c[1] == "mod"]
DEM = [c for c in CASES if c[1] == "dem"]
ids = lambda c: c[0]   # noqa: E731


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_fixture_shape():
    assert len(TABLE) == 1024 and [c["name"] for c in FIX["cases"]] == [c[0] for c in CASES]
    for name, kind, kf, ops in CASES:
        n = len(FM.case_inputs(ops))
        assert n <= 256 and len(RECORDED[name]["out"]) == (2 * n if kind == "mod" else n)
        assert RECORDED[name]["kf"] == int(FM.bits(np.array([kf], f32))[0])
    assert {kf for _, _, kf, _ in CASES} == set(FM.KFS)
    assert os.path.getsize(FM.FIXTURE) < 170000


def test_table():
    """cexpf of the float32 angle: within a unit of the float64 cosine and sine of that angle"""
    t64 = FM.table64()
    assert np.max(np.abs(TABLE.real.astype(np.float64) - t64.real)) <= 2.0 ** -24
    assert np.max(np.abs(TABLE.imag.astype(np.float64) - t64.imag)) <= 2.0 ** -24
    assert TABLE[0] == 1 and len({(a, b) for a, b in zip(FM.bits(TABLE.real), FM.bits(TABLE.imag))}) == 1024


@pytest.mark.parametrize("c", MOD, ids=ids)
def test_freqmod_model_equals_the_fixture(c):
    name, _, kf, ops = c
    want = cplx(RECORDED[name]["out"])
    stepped, summed = FM.ModModel(kf, TABLE), FM.ModModel(kf, TABLE)
    a = np.concatenate([stepped.step(x) for _, x in ops])
    b = np.concatenate([summed.block(x) for _, x in ops])
    assert same_bits(a, want) and same_bits(b, want)
    assert stepped.phase == summed.phase == RECORDED[name]["acc"]


@pytest.mark.parametrize("inc", [FM.increments_rint, FM.increments_add_half], ids=["rintf", "add_half"])
def test_wrong_rounding_misses_the_halfway_case(inc):
    name, _, kf, ops = next(c for c in MOD if c[0] == "halfway")
    m = FM.ModModel(kf, TABLE, inc)
    got = np.concatenate([m.block(x) for _, x in ops])
    assert not same_bits(got, cplx(RECORDED[name]["out"]))
    assert m.phase != RECORDED[name]["acc"]


def test_out_of_range_products_add_nothing():
    name, _, kf, ops = next(c for c in MOD if c[0] == "range")
    m = FM.range_messages()
    inc = FM.increments(FM.mod_ref(kf), m)
    big = ~(np.abs(m.astype(np.float64) * 65536.0) < 2.0 ** 31)
    assert big.sum() >= 8 and np.all(inc[big] == 0) and np.all(inc[~big & (m != 0)] != 0)


@pytest.mark.parametrize("c", DEM, ids=ids)
def test_reference_freqdem_meets_the_bound(c):
    name, _, kf, ops = c
    re, im, ref = FM.dem_case_products(kf, ops)
    FM.check("reference " + name, np.array(RECORDED[name]["out"], np.uint32).view(f32), re, im, ref)
    FM.check("float32 model " + name, FM.reference32(re, im, ref), re, im, ref)


def test_zero_state_third_quadrant_is_pi():
    """the product of a zero state with a third-quadrant sample is (-0, +0): pi ref, not 0"""
    name, _, kf, ops = next(c for c in DEM if c[0] == "quadrants")
    re, im, ref = FM.dem_case_products(kf, ops)
    out = np.array(RECORDED[name]["out"], np.uint32).view(f32)
    assert np.signbit(re[2]) and re[2] == 0 and not np.signbit(im[2]) and im[2] == 0
    assert out[2] == f32(np.pi) * ref and out[0] == 0


@pytest.mark.parametrize("kf", [0.02, 0.04, 0.08])
def test_reference_roundtrip(kf):
    c = RECORDED["roundtrip_mod_kf%g" % kf]
    re, im = FM.DemModel(kf).block(cplx(c["out"]))
    y = np.array(c["dem"], np.uint32).view(f32)
    FM.check("reference round trip kf=%g" % kf, y, re, im, FM.dem_ref(kf))
    assert np.max(np.abs(y[1:] - FM.cosines(256)[1:])) < 5e-2


# ------------------------------------------------------------------ the library's host interface (no GPU)
def test_library_table():
    assert same_bits(LQ.FreqMod(0.1).get_table(), TABLE)


@pytest.mark.parametrize("c", MOD, ids=ids)
def test_library_freqmod_per_sample_equals_the_fixture(c):
    name, kind, kf, ops = c
    q = LQ.FreqMod(kf)
    assert same_bits(FM.drive_library(q, kind, ops, blocks=False), cplx(RECORDED[name]["out"]))
    assert q.get_phase() == RECORDED[name]["acc"]
    q.reset()
    assert q.get_phase() == 0


@pytest.mark.parametrize("c", DEM, ids=ids)
def test_library_freqdem_per_sample_meets_the_bound(c):
    name, kind, kf, ops = c
    re, im, ref = FM.dem_case_products(kf, ops)
    FM.check("library " + name, FM.drive_library(LQ.FreqDem(kf), kind, ops, blocks=False), re, im, ref)


@pytest.mark.parametrize("M", [2, 3, 64])
def test_library_freqdem_channels_per_sample(M):
    """the lag-M object, per-sample calls: M independent lag-1 objects on the de-interleaved channels"""
    x = FM.dem_input(5 * M + 1, 31)
    q = LQ.FreqDem(0.08, M)
    assert q.get_channels() == M and LQ.FreqDem(0.08).get_channels() == 1
    got = np.array([q.demodulate(v) for v in x], f32)
    for ch in range(M):
        one = LQ.FreqDem(0.08)
        assert same_bits(got[ch::M], np.array([one.demodulate(v) for v in x[ch::M]], f32))


@pytest.mark.parametrize("kf", [0.02, 0.04, 0.08])
def test_autotest_roundtrip_through_the_host_calls(kf):
    """src/modem/tests/freqmodem_autotest.c: 1024 samples of three cosines, tolerance 5e-2, the
    first sample skipped"""
    m = FM.cosines(1024)
    mod, dem = LQ.FreqMod(kf), LQ.FreqDem(kf)
    y = np.array([dem.demodulate(mod.modulate(v)) for v in m], f32)
    assert np.max(np.abs(y[1:] - m[1:])) < 5e-2


def test_library_runs_without_a_device():
    """create, the per-sample calls, reset and print in a process that cannot see a GPU"""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import liquidmi as LQ\n"
            "m, d = LQ.FreqMod(0.04), LQ.FreqDem(0.04, 3)\n"
            "print(d.demodulate(m.modulate(0.5)), m.get_phase()); m.reset(); d.reset()\n"
            "LQ.lib().freqmod_print(m.q); LQ.lib().freqdem_print(d.q)\n")
    e = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code, LQ.HERE], capture_output=True, text=True, env=e, timeout=60)
    assert out.returncode == 0, out.stderr
    assert "freqmod:" in out.stdout and "freqdem:" in out.stdout and "1311" in out.stdout.split()


@pytest.mark.parametrize("what", ["freqmod", "freqdem"])
@pytest.mark.parametrize("kf", [0.0, -0.1, 1.5])
def test_kf_out_of_range_exits(what, kf):
    code = "import sys; sys.path.insert(0, sys.argv[1]); import liquidmi as LQ; LQ.lib().%s_create(%r)" % (what, kf)
    out = subprocess.run([sys.executable, "-c", code, LQ.HERE], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1
    assert "error: %s_create(), modulation factor" % what in out.stderr and "out of range [0,1]" in out.stderr


def test_library_exports_the_interface():
    names = [n for n in LQ.header_functions() if n.startswith(("freqmod_", "freqdem_"))]
    want = ["freqmod_" + w for w in ("create", "destroy", "print", "reset", "modulate", "modulate_block",
                                     "modulate_block_dev", "get_phase", "get_table", "set_stream", "synchronize")]
    want += ["freqdem_" + w for w in ("create", "create_channels", "get_channels", "destroy", "print", "reset",
                                      "demodulate", "demodulate_block", "demodulate_block_dev", "set_stream",
                                      "synchronize")]
    assert sorted(names) == sorted(want)
    L = ctypes.CDLL(LQ.LIB_PATH)
    extra = ["liquid_mi355x_freqmod_tile", "liquid_mi355x_freqmod_scan_pass", "liquid_mi355x_freqdem_tile",
             "liquid_mi355x_freqdem_switch", "liquid_mi355x_freqdem_frames"]
    for n in names + extra:
        assert hasattr(L, n), n
        assert n in LQ.header_functions(), n
    assert LQ.FreqMod.TILE >= 64 and LQ.FreqMod.SCAN_PASS >= 1 and LQ.FreqDem.TILE >= 64
    assert LQ.FreqMod.TILE * LQ.FreqMod.SCAN_PASS < 1 << 24      # the scan's carry is reachable in a test
    assert 1 < LQ.FreqDem.SWITCH <= 1024
    hdr = open(LQ.HEADER).read()
    assert "typedef struct freqmod_s *freqmod;" in hdr and "typedef struct freqdem_s *freqdem;" in hdr


def test_reference_program_compiles_and_links(tmp_path):
    """a C program written against liquid.h's freqmod / freqdem interface alone"""
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <complex.h>\n#include "liquid.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "    freqmod mod = freqmod_create(0.1f);\n"
                   "    freqdem dem = freqdem_create(0.1f);\n"
                   "    float m[4] = {0.1f, 0.2f, -0.3f, 0.4f}, y[4];\n"
                   "    liquid_float_complex s[4];\n"
                   "    for (int i = 0; i < 4; i++) { freqmod_modulate(mod, m[i], &s[i]); freqdem_demodulate(dem, s[i], &y[i]); }\n"
                   "    if (argc > 7) { freqmod_modulate_block(mod, m, 4, s); freqdem_demodulate_block(dem, s, 4, y); }\n"
                   '    printf("%.3f %.3f %.3f\\n", y[1], y[2], y[3]);\n'
                   "    freqmod_print(mod); freqdem_print(dem); freqmod_reset(mod); freqdem_reset(dem);\n"
                   "    freqmod_destroy(mod); freqdem_destroy(dem);\n"
                   "    return 0;\n}\n")
    libdir = os.path.dirname(LQ.LIB_PATH)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-I", os.path.join(LQ.ROOT, "include"),
                           str(src), "-L", libdir, "-lliquid_mi355x", "-Wl,-rpath," + libdir, "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    y = [float(v) for v in out.stdout.splitlines()[0].split()]
    assert max(abs(a - b) for a, b in zip(y, (0.2, -0.3, 0.4))) < 5e-3
    assert "freqmod:" in out.stdout and "freqdem:" in out.stdout
