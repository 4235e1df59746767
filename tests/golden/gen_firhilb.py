#!/usr/bin/env python3
"""Record liquid-dsp's firhilbf as a JSON fixture (tests/golden/firhilb.json).

Runs ONLY where the reference sources are present: it copies them to a
temporary directory, builds libliquid.a there by SURVEY Appendix A's recipe
(-msse4.1), drives firhilbf through the small C program below and records
what it returned.  Nothing compiled and none of the reference's text is kept:
the fixture holds numbers only.

Contents, for (m, As) in CASES:
  hq      the quadrature taps, read as the decimator's impulse response
          (unit impulse at x[0]: Im y[i] = hq[2m-1-i])
  decim / interp / r2c
          the outputs of one stream of CALLS calls per stateful mode
  mixed   one object: decim, an odd number of r2c calls, interp, r2c again
and the two known-answer vectors of src/filter/tests/firhilb_autotest.c
(m = 5, As = 60, 16 calls each, tolerance 0.005), copied as data.

The streams' inputs are not stored: tests/firhilb_model.py (stream_input)
regenerates them from integer arithmetic alone -- a 32-bit LCG gives 16-bit
values v, the sample is float32((v - 32768) / 65536) times a burst envelope
(level 1 in a few runs, 1e-5 elsewhere, a stretch of exact zeros) -- and this
script imports that function, so both sides use the same samples.  Outputs
are written with the shortest decimal text that reads back to the same
float32, so every recorded output is exact.

Usage:  python tests/golden/gen_firhilb.py [reference-directory]
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import firhilb_model as FM  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LIQUID_REFERENCE", "/root/reference")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <complex.h>
#include "liquid.h"
/* stdin: "m As" then ops "D n" / "I n" / "R n", each followed by its input
 * floats as uint32 bit patterns; stdout: the output floats the same way */
static float rd(void) { uint32_t b; float f; if (scanf("%u", &b) != 1) exit(2); memcpy(&f, &b, 4); return f; }
static void wr(float f) { uint32_t b; memcpy(&b, &f, 4); printf("%u\n", b); }
int main(void)
{
    unsigned m; float As; char op[4]; unsigned n;
    if (scanf("%u %f", &m, &As) != 2) return 2;
    firhilbf q = firhilbf_create(m, As);
    while (scanf("%3s %u", op, &n) == 2) {
        for (unsigned i = 0; i < n; i++) {
            if (op[0] == 'D') {
                float x[2]; float complex y;
                x[0] = rd(); x[1] = rd();
                firhilbf_decim_execute(q, x, &y);
                wr(crealf(y)); wr(cimagf(y));
            } else if (op[0] == 'I') {
                float re = rd(), im = rd(), y[2];
                firhilbf_interp_execute(q, re + _Complex_I * im, y);
                wr(y[0]); wr(y[1]);
            } else {
                float complex y;
                firhilbf_r2c_execute(q, rd(), &y);
                wr(crealf(y)); wr(cimagf(y));
            }
        }
    }
    firhilbf_destroy(q);
    return 0;
}
"""

CONFIG_H = """
#define HAVE_MMINTRIN_H 1
#define HAVE_XMMINTRIN_H 1
#define HAVE_EMMINTRIN_H 1
#define HAVE_PMMINTRIN_H 1
#define HAVE_COMPLEX_H 1
#define HAVE_MATH_H 1
#define HAVE_STDIO_H 1
#define HAVE_STDLIB_H 1
#define HAVE_STRING_H 1
#define SIZEOF_INT 4
#define SIZEOF_UNSIGNED_INT 4
"""

MMX = " ".join("src/dotprod/src/%s.mmx.o" % s for s in ("dotprod_cccf", "dotprod_crcf", "dotprod_rrrf", "sumsq"))
VEC = " ".join("src/vector/src/vector%s_%s.port.o" % (t, s) for t in ("f", "cf") for s in ("add", "norm", "mul", "trig"))
SUBST = {"PACKAGE_NAME": "liquid-dsp", "PACKAGE_VERSION": "1.2.0", "PACKAGE_BUGREPORT": "x", "srcdir": ".",
         "libdir": "/nonexistent/lib", "prefix": "/nonexistent", "exec_prefix": "/nonexistent", "CC": "gcc",
         "SED": "sed", "GREP": "grep", "CFLAGS": "-g -O2", "DEBUG_OPTION": "", "ARCH_OPTION": "-msse4.1",
         "LDFLAGS": "", "LIBS": "-lm -lc", "SH_LIB": "libliquid.so", "MLIBS_DOTPROD": MMX, "MLIBS_VECTOR": VEC}


def build_reference(tmp):
    src = os.path.join(tmp, "liqref")
    shutil.copytree(REF, src)
    subprocess.check_call(["chmod", "-R", "u+w", src])
    mk = open(os.path.join(src, "makefile.in")).read()
    mk = re.sub(r"@(\w+)@", lambda m: SUBST.get(m.group(1), ""), mk)
    open(os.path.join(src, "makefile"), "w").write(mk)
    open(os.path.join(src, "config.h"), "w").write(CONFIG_H)
    subprocess.check_call(["make", "-s", "-j16", "libliquid.a"], cwd=src, stdout=subprocess.DEVNULL)
    drv = os.path.join(tmp, "drive.c")
    open(drv, "w").write(DRIVER)
    exe = os.path.join(tmp, "drive")
    subprocess.check_call(["gcc", "-O2", "-msse4.1", "-I", os.path.join(src, "include"), drv,
                           os.path.join(src, "libliquid.a"), "-lm", "-o", exe])
    return exe


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def drive(exe, m, As, ops):
    """ops: [(mode, input array)]; returns the list of float32 output arrays."""
    txt = ["%d %r" % (m, float(As))]
    for mode, x in ops:
        flat = np.ascontiguousarray(x).view(np.float32)
        n = len(flat) if mode == "r2c" else len(flat) // 2
        txt.append("%s %d" % ({"decim": "D", "interp": "I", "r2c": "R"}[mode], n))
        txt.append(" ".join(str(int(b)) for b in bits(flat)))
    out = subprocess.run([exe], input="\n".join(txt) + "\n", capture_output=True, text=True, check=True).stdout
    y = np.array([int(t) for t in out.split()], np.uint32).view(np.float32)
    res, k = [], 0
    for mode, x in ops:
        flat = np.ascontiguousarray(x).view(np.float32)
        n = len(flat) if mode == "r2c" else len(flat) // 2
        res.append(y[k:k + 2 * n].copy())
        k += 2 * n
    assert k == len(y)
    return res


def num(v):
    """shortest decimal text that reads back to the same float32"""
    v = np.float32(v)
    s = np.format_float_scientific(v, unique=True, trim="-") if v != 0 else ("-0.0" if np.signbit(v) else "0")
    assert np.float32(float(s)) == v and np.signbit(np.float32(float(s))) == np.signbit(v)
    m, e = s.split("e") if "e" in s else (s, "0")
    return m + ("e%d" % int(e) if int(e) else "")


def known_answers():
    src = open(os.path.join(REF, "src", "filter", "tests", "firhilb_autotest.c")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    arrays = re.findall(r"float(\s+complex)?\s+(x|test)\[\d+\]\s*=\s*\{(.*?)\}\s*;", src, re.S)
    assert [a[1] for a in arrays] == ["x", "test", "x", "test"]

    def parse(cplx, body):
        if not cplx:
            return [float(t) for t in body.split(",") if t.strip()]
        out = []
        for t in body.split(","):
            if t.strip():
                r, i = t.split("+J*")
                out += [float(r), float(i)]
        return out
    vals = [parse(c.strip(), b) for c, _, b in arrays]
    return {"m": 5, "As": 60.0, "tol": 0.005,
            "decim": {"x": vals[0], "y": vals[1]},      # y: (re, im) pairs
            "interp": {"x": vals[2], "y": vals[3]}}     # x: (re, im) pairs


def main():
    tmp = tempfile.mkdtemp(prefix="gen_firhilb_")
    try:
        exe = build_reference(tmp)
        cases = []
        for m, As in FM.CASES:
            imp = np.zeros(4 * m, np.float32)
            imp[0] = 1.0
            y = drive(exe, m, As, [("decim", imp)])[0]
            hq = y[1::2][::-1].copy()                   # Im y[i] = hq[2m-1-i]
            assert np.array_equal(hq, -hq[::-1]), "taps not antisymmetric"
            case = {"m": m, "As": As, "hq": hq}
            for mode in FM.MODES:
                case[mode] = drive(exe, m, As, [(mode, FM.stream_input(m, mode))])[0]
            ops = FM.mixed_ops(m)
            case["mixed"] = np.concatenate(drive(exe, m, As, ops))
            cases.append(case)
        # the model meets the bar on everything just recorded (what
        # tests/test_firhilb_model.py asserts): say so before writing
        for c in cases:
            for mode in FM.MODES:
                FM.check(c["m"], c["hq"], [(mode, FM.stream_input(c["m"], mode))], c[mode], "gen %s" % mode)
            FM.check(c["m"], c["hq"], FM.mixed_ops(c["m"]), c["mixed"], "gen mixed")
        body = []
        for c in cases:
            f = ['"m":%d' % c["m"], '"As":%s' % num(c["As"])]
            for k in ("hq",) + FM.MODES + ("mixed",):
                f.append('"%s":[%s]' % (k, ",".join(num(v) for v in c[k])))
            body.append("{" + ",\n".join(f) + "}")
        txt = '{"calls":%d,\n"cases":[\n%s\n],\n"known_answers":%s}\n' % (
            FM.CALLS, ",\n".join(body), json.dumps(known_answers(), separators=(",", ":")))
        json.loads(txt)
        out = os.path.join(HERE, "firhilb.json")
        open(out, "w").write(txt)
        print("wrote %s: %d bytes" % (out, len(txt)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
