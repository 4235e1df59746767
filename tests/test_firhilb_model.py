"""firhilbf without a GPU: the checker is pinned to the reference, and the
drop-in boundary has the new object.

* The float64 model of tests/firhilb_model.py, with the fixture's taps,
  reproduces every output liquid-dsp's firhilbf gave for the fixture's
  streams (tests/golden/firhilb.json, recorded by tests/golden/gen_firhilb.py)
  at the bar: delay outputs bit for bit, dot outputs within
  (2m + 8) 2^-23 A and exactly zero where A = 0.  So the bar can be met, and
  the checker the GPU tests use agrees with the reference.
* The model reproduces the two known-answer vectors of the reference's
  firhilb_autotest.c within its tolerance.
* The library exports every firhilbf symbol, the Python binding has FirHilb,
  the header still compiles as C99 and C++, and the reference's three firhilb
  examples compile unchanged into build/ref_examples_firhilb/.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import firhilb_model as FM
import liquidmi as LQ

ROOT = LQ.ROOT

SYMBOLS = ["firhilbf_" + s for s in (
    "create", "destroy", "print", "reset", "r2c_execute", "c2r_execute", "decim_execute", "decim_execute_block",
    "interp_execute", "interp_execute_block", "r2c_execute_block", "c2r_execute_block",
    "decim_execute_block_dev", "interp_execute_block_dev", "r2c_execute_block_dev", "c2r_execute_block_dev",
    "set_stream", "synchronize")]


@functools.lru_cache(maxsize=None)
def fixture():
    return FM.load_fixture()


def case_ids():
    return ["m%d" % m for m, _ in FM.CASES]


def test_fixture_has_every_case():
    d = fixture()
    assert [(c["m"], c["As"]) for c in d["cases"]] == FM.CASES
    assert d["calls"] == FM.CALLS
    for c in d["cases"]:
        m = c["m"]
        assert len(c["hq"]) == 2 * m
        assert np.array_equal(c["hq"], -c["hq"][::-1])      # exactly antisymmetric
        for mode in FM.MODES:
            assert len(c[mode]) == 2 * FM.CALLS
        assert len(c["mixed"]) == 2 * sum(len(x.view(np.float32)) // FM.NIN[md] for md, x in FM.mixed_ops(m))


def test_fixture_inputs_have_bursts_and_zeros():
    x = FM.stream_input(5, "decim")
    a = np.abs(x)
    assert a.max() > 0.4 and np.count_nonzero(a == 0) > 50 and np.count_nonzero((a > 0) & (a < 1e-5)) > 50
    assert not np.signbit(x[x == 0]).any()


@pytest.mark.parametrize("k", range(len(FM.CASES)), ids=case_ids())
@pytest.mark.parametrize("mode", FM.MODES)
def test_model_reproduces_reference_stream(mode, k):
    c = fixture()["cases"][k]
    FM.check(c["m"], c["hq"], [(mode, FM.stream_input(c["m"], mode))], c[mode], "reference " + mode)


@pytest.mark.parametrize("k", range(len(FM.CASES)), ids=case_ids())
def test_model_reproduces_reference_mixed(k):
    c = fixture()["cases"][k]
    FM.check(c["m"], c["hq"], FM.mixed_ops(c["m"]), c["mixed"], "reference mixed")


@pytest.mark.parametrize("mode", ["decim", "interp"])
def test_model_reproduces_autotest_vectors(mode):
    d = fixture()
    ka = d["known_answers"]
    assert (ka["m"], ka["As"], ka["tol"]) == (5, 60.0, 0.005)
    hq = next(c["hq"] for c in d["cases"] if (c["m"], c["As"]) == (5, 60.0))
    ops, want = FM.known_answer_ops(d, mode)
    assert len(want) == 32
    val, _, _ = FM.Model(5, hq).run_ops(ops)
    err = np.max(np.abs(val - want))
    print("autotest %s: max |model - expected| %.3g (tolerance %g)" % (mode, err, ka["tol"]))
    assert err <= ka["tol"]


def test_checker_rejects_what_misses_the_bar():
    """one ulp on a delay output, a dot output past the bound, a nonzero
    where A = 0: each is caught"""
    c = fixture()["cases"][1]
    ops = [("decim", FM.stream_input(c["m"], "decim"))]
    val, A, dot = FM.Model(c["m"], c["hq"]).run_ops(ops)
    good = c["decim"]
    assert FM.report(c["m"], c["hq"], ops, good)["delay_bad"] == 0
    i_delay = int(np.argmax(~dot & (good != 0)))
    i_dot = int(np.argmax(dot & (A > 0.1)))
    i_zero = int(np.argmax(dot & (A == 0)))
    assert dot[i_zero] and A[i_zero] == 0
    for i, v, key in ((i_delay, np.nextafter(good[i_delay], np.float32(2)), "delay_bad"),
                      (i_dot, good[i_dot] + np.float32(2 * (2 * c["m"] + 8) * FM.EPS * A[i_dot]), "dot_bad"),
                      (i_zero, np.float32(1e-30), "nonzero_zeros")):
        y = good.copy()
        y[i] = v
        assert FM.report(c["m"], c["hq"], ops, y)[key] == 1


# ------------------------------------------------------------------ the boundary
def test_library_exports_firhilbf():
    L = C.CDLL(LQ.LIB_PATH)
    missing = [n for n in SYMBOLS if not hasattr(L, n)]
    assert not missing, missing
    declared = set(LQ.header_functions())
    assert not [n for n in SYMBOLS if n not in declared]


def test_python_binding_has_firhilb():
    assert hasattr(LQ, "FirHilb")
    for name in ("decim_block", "interp_block", "r2c_block", "c2r_block", "decim", "interp", "r2c", "reset",
                 "decim_block_dev", "interp_block_dev", "r2c_block_dev", "c2r_block_dev"):
        assert callable(getattr(LQ.FirHilb, name))
    L = LQ.lib()
    for n in SYMBOLS:
        assert getattr(L, n).argtypes is not None, n


def test_create_rejects_short_filter_like_the_reference():
    """firhilb.c:71-74: m < 2 prints the reference's message and exits with
    status 1 (checked before any GPU is looked for; in a child process)."""
    code = ("import ctypes,sys; L=ctypes.CDLL(sys.argv[1]); L.firhilbf_create.restype=ctypes.c_void_p; "
            "L.firhilbf_create(ctypes.c_uint(1), ctypes.c_float(60.0)); print('returned')")
    out = subprocess.run([sys.executable, "-c", code, LQ.LIB_PATH], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "returned" not in out.stdout
    assert out.stderr == "error: firhilb_create(), filter semi-length (m) must be at least 2\n"


def test_header_with_firhilbf_compiles_as_c_and_cxx(tmp_path):
    inc = os.path.join(ROOT, "include")
    body = ("firhilbf q = firhilbf_create(5, 60.0f); liquid_float_complex y; float x[2] = {0, 0};\n"
            "firhilbf_decim_execute(q, x, &y); firhilbf_r2c_execute_block_dev(q, x, 0, &y); firhilbf_destroy(q);\n")
    c = tmp_path / "t.c"
    c.write_text('#include "liquid.h"\nint main(void){' + body + "return 0;}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(c)])
    cc = tmp_path / "t.cc"
    cc.write_text('#include <complex>\n#include "liquid.h"\nint main(){' + body + "return 0;}\n")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-fsyntax-only", "-I", inc, str(cc)])


@pytest.mark.skipif(not os.path.isdir(os.path.join(os.environ.get("LIQUID_REFERENCE", "/root/reference"), "examples")),
                    reason="reference sources not present")
def test_reference_firhilb_examples_compile_unchanged():
    subprocess.check_call(["bash", os.path.join(ROOT, "tools", "build_ref_examples_firhilb.sh")])
    built = sorted(os.listdir(os.path.join(ROOT, "build", "ref_examples_firhilb")))
    assert built == ["firhilb_decim_example", "firhilb_example", "firhilb_interp_example"]
