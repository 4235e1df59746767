"""iirfilt without a GPU: the models are pinned to the reference, and the
host-only parts of the library are checked.

* The float32 model of tests/iirfilt_model.py (run32: the reference's
  statement order, one rounding per operation) reproduces every output
  liquid-dsp's iirfilt gave for the fixture's streams (tests/golden/iirfilt.json,
  recorded by tests/golden/gen_iirfilt.py) bit for bit, and the reference's own
  autotest vectors within their tolerance of 0.001.
* The fixture's own normwise error against the float64 model is printed per
  case: it is the e_ref of the GPU tests' criterion.
* The design helpers (iirdes_pll_active_lag, iirdes_pll_active_PI,
  iirdes_dzpk2sosf, iir_group_delay) need no GPU and are checked against the
  fixture here as well.
* The library exports every iirfilt symbol, the header declares them (and
  does not declare create_prototype / create_lowpass), the Python binding has
  IirFilt, the header compiles as C99 and C++, and the reference's two
  examples compile unchanged into build/ref_examples_iir/.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import iirfilt_model as IM
import liquidmi as LQ

ROOT = LQ.ROOT
KINDS = ("rrrf", "crcf", "cccf")
SYMBOLS = ["iirfilt_%s_%s" % (t, s) for t in KINDS for s in (
    "create", "create_sos", "create_dc_blocker", "create_pll", "create_integrator", "create_differentiator",
    "destroy", "print", "reset", "execute", "execute_block", "execute_block_dev", "get_length", "freqresponse",
    "groupdelay", "device_eligible", "set_stream", "synchronize")] + [
    "iirdes_pll_active_lag", "iirdes_pll_active_PI", "iirdes_dzpk2sosf", "iir_group_delay"]


@functools.lru_cache(maxsize=None)
def fixture():
    return IM.load_fixture()


def names(key):
    with open(IM.FIXTURE) as f:
        return re.findall(r'"name":"([^"]+)"', f.read().split('"vectors"')[0 if key == "cases" else 1])


def bits(a):
    return np.ascontiguousarray(a).view(np.float32).view(np.uint32)


def test_fixture_has_every_case():
    d = fixture()
    got = [c["name"] for c in d["cases"]]
    for want in ("dc_blocker_0.01_crcf", "dc_blocker_1e-3_rrrf", "pll_rrrf", "integrator_rrrf", "integrator_crcf",
                 "differentiator_rrrf", "differentiator_crcf", "butter4_crcf", "butter4_rrrf", "ellip5_crcf",
                 "cpoles1_cccf", "cpoles2_cccf", "a0_is_2_rrrf", "radius_1.01_crcf"):
        assert want in got
    for c in d["cases"]:
        assert len(c["y"]) == c["n"] == (200 if c["name"].startswith("radius") else IM.NOUT)
    assert sorted(v["name"] for v in d["vectors"]) == sorted(
        "iirfilt_%s_data_h%dx64" % (t, h) for t in KINDS for h in (3, 5, 7))
    assert os.path.getsize(IM.FIXTURE) < 200 * 1024


@pytest.mark.parametrize("k", range(len(names("cases"))), ids=names("cases"))
def test_model_reproduces_reference_stream(k):
    c = fixture()["cases"][k]
    x = IM.case_input(c)
    y32, _ = IM.run32(c["kind"], c["form"], c["b"], c["a"], x)
    same = np.array_equal(bits(y32), bits(c["y"]))
    if np.all(np.isfinite(c["y"])):
        y64 = IM.run64(c["kind"], c["form"], c["b"], c["a"], x)
        print("iirfilt %-24s reference e_ref = max|y - y64| / max|y64| = %.3e" % (c["name"], IM.err(c["y"], y64)))
    else:   # the reference's integrator: its gain is negative and its fourth root is not a number
        print("iirfilt %-24s reference outputs are not finite" % c["name"])
    assert same, "float32 model differs from the recorded reference outputs"


@pytest.mark.parametrize("k", range(9), ids=names("vectors"))
def test_model_reproduces_autotest_vectors(k):
    v = fixture()["vectors"][k]
    y32, _ = IM.run32(v["kind"], "norm", v["bn"], v["an"], v["x"])
    e = float(np.max(np.abs(y32 - v["y"])))
    print("%s: max |model - expected| %.3g (tolerance %g)" % (v["name"], e, v["tol"]))
    assert v["tol"] == 0.001 and e < v["tol"]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def test_pll_helpers_match_reference():
    n = 0
    for h in fixture()["helpers"]:
        if h["fn"] not in ("lag", "pi"):
            continue
        fn = LQ.iirdes_pll_active_lag if h["fn"] == "lag" else LQ.iirdes_pll_active_PI
        b, a = fn(h["w"], h["zeta"], h["K"])
        assert rel(b, h["b"]) <= 1e-6 and rel(a, h["a"]) <= 1e-6, (h, b, a)
        n += 1
    assert n == 4


def test_dzpk2sosf_matches_reference():
    n = 0
    for h in fixture()["helpers"]:
        if h["fn"] != "zpk":
            continue
        z = np.array(h["z"], np.float32).view(np.complex64)
        p = np.array(h["p"], np.float32).view(np.complex64)
        B, A = LQ.iirdes_dzpk2sosf(z, p, h["k"])
        assert rel(B, h["b"]) <= 1e-6 and rel(A, h["a"]) <= 1e-6, (h, B, A)
        n += 1
    assert n == 2


def test_pll_case_coefficients_come_from_active_lag():
    c = next(c for c in fixture()["cases"] if c["name"] == "pll_rrrf")
    b, a = LQ.iirdes_pll_active_lag(c["w"], c["zeta"], c["K"])
    assert rel(b / a[0], c["b"]) <= 1e-6 and rel(a / a[0], c["a"]) <= 1e-6


def test_iir_group_delay_against_float64():
    c = next(c for c in fixture()["cases"] if c["name"] == "butter4_rrrf")
    b, a = c["b"][:3].astype(np.float64), c["a"][:3].astype(np.float64)
    for fc in (0.0, 0.05, 0.2, 0.45):
        w = 2 * np.pi * fc
        # group delay = -d arg H / dw, H = B(e^{-jw}) / A(e^{-jw})
        k = np.arange(3)
        e = np.exp(-1j * w * k)
        gd = np.real(np.sum(k * b * e) / np.sum(b * e)) - np.real(np.sum(k * a * e) / np.sum(a * e))
        got = LQ.iir_group_delay(c["b"][:3], c["a"][:3], fc)
        assert abs(got - gd) <= 1e-4 * max(1.0, abs(gd)), (fc, got, gd)


# ------------------------------------------------------------------ the boundary
def test_library_exports_iirfilt():
    L = C.CDLL(LQ.LIB_PATH)
    missing = [n for n in SYMBOLS if not hasattr(L, n)]
    assert not missing, missing
    declared = set(LQ.header_functions())
    assert not [n for n in SYMBOLS if n not in declared]
    # the prototype designs are a later step: a caller must fail at link time
    for t in KINDS:
        for s in ("create_prototype", "create_lowpass"):
            assert "iirfilt_%s_%s" % (t, s) not in declared and not hasattr(L, "iirfilt_%s_%s" % (t, s))


def test_python_binding_has_iirfilt():
    for name in ("sos", "dc_blocker", "pll", "integrator", "differentiator", "execute", "execute_block",
                 "execute_block_dev", "reset", "freqresponse", "groupdelay", "get_length"):
        assert callable(getattr(LQ.IirFilt, name))
    assert isinstance(LQ.IirFilt.__dict__["device_eligible"], property)
    L = LQ.lib()
    for n in SYMBOLS:
        assert getattr(L, n).argtypes is not None, n
    src = open(os.path.join(ROOT, "liquid-dsp_amd", "csrc", "lq_kernels.h")).read()
    for attr, macro in (("RUN", "LQK_IIRFILT_RUN"), ("TILE", "LQK_IIRFILT_TILE"), ("SCAN", "LQK_IIRFILT_SCAN")):
        assert getattr(LQ.IirFilt, attr) == int(re.search(r"#define %s (\d+)" % macro, src).group(1))
    assert LQ.IirFilt.TILE % LQ.IirFilt.RUN == 0


@pytest.mark.parametrize("code,msg", [
    ("L.iirfilt_crcf_create(None, 0, None, 1)", "error: iirfilt_crcf_create(), numerator length cannot be zero\n"),
    ("L.iirfilt_rrrf_create(None, 2, None, 0)", "error: iirfilt_rrrf_create(), denominator length cannot be zero\n"),
    ("L.iirfilt_cccf_create_sos(None, None, 0)",
     "error: iirfilt_cccf_create_sos(), filter must have at least one 2nd-order section\n"),
    ("L.iirfilt_rrrf_create_pll(ctypes.c_float(1.5), ctypes.c_float(0.7), ctypes.c_float(10))",
     "error: iirfilt_rrrf_create_pll(), bandwidth must be in (0,1)\n"),
])
def test_create_rejects_like_the_reference(code, msg):
    """iirfilt.c:85-91,154-157,387-396: the reference's messages, exit status
    1 (checked before any GPU is looked for; in a child process)."""
    prog = "import ctypes,sys; L=ctypes.CDLL(sys.argv[1]); %s; print('returned')" % code
    out = subprocess.run([sys.executable, "-c", prog, LQ.LIB_PATH], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "returned" not in out.stdout
    assert out.stderr == msg


def test_header_with_iirfilt_compiles_as_c_and_cxx(tmp_path):
    inc = os.path.join(ROOT, "include")
    body = ("float b[3] = {1, 0, 0}, a[3] = {1, 0, 0}; liquid_float_complex x[2], H;\n"
            "iirfilt_crcf q = iirfilt_crcf_create_sos(b, a, 1); iirfilt_crcf_execute_block(q, x, 2, x);\n"
            "iirfilt_crcf_execute_block_dev(q, x, 0, x); iirfilt_crcf_freqresponse(q, 0.1f, &H);\n"
            "iirfilt_rrrf p = iirfilt_rrrf_create_dc_blocker(0.1f); float y; iirfilt_rrrf_execute(p, 1.0f, &y);\n"
            "iirdes_pll_active_lag(0.1f, 0.7f, 10.0f, b, a); iirfilt_rrrf_destroy(p); iirfilt_crcf_destroy(q);\n")
    c = tmp_path / "t.c"
    c.write_text('#include "liquid.h"\nint main(void){' + body + "return 0;}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(c)])
    cc = tmp_path / "t.cc"
    cc.write_text('#include <complex>\n#include "liquid.h"\nint main(){' + body + "return 0;}\n")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-fsyntax-only", "-I", inc, str(cc)])


@pytest.mark.skipif(not os.path.isdir(os.path.join(os.environ.get("LIQUID_REFERENCE", "/root/reference"), "examples")),
                    reason="reference sources not present")
def test_reference_iirfilt_examples_compile_unchanged():
    subprocess.check_call(["bash", os.path.join(ROOT, "tools", "build_ref_examples_iir.sh")])
    built = sorted(os.listdir(os.path.join(ROOT, "build", "ref_examples_iir")))
    assert built == ["iirfilt_crcf_dcblocker_example", "pll_example"]
