#!/usr/bin/env python3
"""Record liquid-dsp's iirfilt as a JSON fixture (tests/golden/iirfilt.json).

Runs ONLY where the reference sources are present: as gen_firhilb.py, it
copies them to a temporary directory, builds libliquid.a there (-msse4.1),
drives iirfilt through the small C program below and records what it
returned.  Nothing compiled and none of the reference's text is kept: the
fixture holds numbers only.

Contents:
  cases    per stream: the constructor and its arguments, the float32
           coefficients the object holds after normalisation (the driver reads
           them out of the object and divides a section by its a[0] in the
           coefficient type, as the object does), and NOUT outputs of
           execute_block.  Inputs are not stored: tests/iirfilt_model.py
           (stream_input) regenerates them from integer arithmetic.
  helpers  iirdes_pll_active_lag / _PI and iirdes_dzpk2sosf on recorded
           arguments.
  vectors  the reference's own iirfilt_{rrrf,crcf,cccf}_data_h{3,5,7}x64
           (src/filter/tests/data), copied as data, with the normalised
           coefficients and the autotest's tolerance.
Outputs are written with the shortest decimal text that reads back to the same
float32.  The Butterworth and elliptic coefficients of cases 5 and 6 come from
the reference's liquid_iirdes.

Usage:  python tests/golden/gen_iirfilt.py [reference-directory]
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
import gen_firhilb as GF  # noqa: E402  (the reference build recipe)
import iirfilt_model as IM  # noqa: E402

REF = GF.REF

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <complex.h>
#include "liquid.h"
/* stdin: one command; floats travel as uint32 bit patterns both ways */
static float rd(void) { uint32_t b; float f; if (scanf("%u", &b) != 1) exit(2); memcpy(&f, &b, 4); return f; }
static void wr(float f) { uint32_t b; memcpy(&b, &f, 4); printf("%u\n", b); }
static void rdn(float *p, unsigned n) { for (unsigned i = 0; i < n; i++) p[i] = rd(); }
static void wrn(const float *p, unsigned n) { for (unsigned i = 0; i < n; i++) wr(p[i]); }
/* the object's fields (iirfilt.c: b, a, v, n, nb, na, type, qsos, nsos) */
#define RUN(NAME, TC, TI, CW, SW)                                                                  \
    struct NAME##_fields { TC *b, *a; TI *v; unsigned n, nb, na; int type; void *qsos; unsigned nsos; }; \
    static void run_##NAME(void)                                                                   \
    {                                                                                              \
        char ctor[16]; NAME q = NULL; unsigned n;                                                  \
        if (scanf("%15s", ctor) != 1) exit(2);                                                     \
        if (!strcmp(ctor, "create")) {                                                             \
            unsigned nb, na; if (scanf("%u %u", &nb, &na) != 2) exit(2);                           \
            TC b[nb], a[na]; rdn((float *)b, nb * CW); rdn((float *)a, na * CW);                   \
            q = NAME##_create(b, nb, a, na);                                                       \
        } else if (!strcmp(ctor, "create_sos")) {                                                  \
            unsigned ns; if (scanf("%u", &ns) != 1) exit(2);                                       \
            TC B[3 * ns], A[3 * ns]; rdn((float *)B, 3 * ns * CW); rdn((float *)A, 3 * ns * CW);   \
            q = NAME##_create_sos(B, A, ns);                                                       \
        } else if (!strcmp(ctor, "dc_blocker")) { q = NAME##_create_dc_blocker(rd());              \
        } else if (!strcmp(ctor, "pll")) { float w = rd(), z = rd(), K = rd(); q = NAME##_create_pll(w, z, K); \
        } else if (!strcmp(ctor, "integrator")) { q = NAME##_create_integrator();                  \
        } else if (!strcmp(ctor, "differentiator")) { q = NAME##_create_differentiator();          \
        } else exit(3);                                                                            \
        struct NAME##_fields *f = (struct NAME##_fields *)q;                                       \
        if (f->type == 0) {                                                                        \
            printf("0 %u %u\n", f->nb, f->na);                                                     \
            wrn((float *)f->b, f->nb * CW); wrn((float *)f->a, f->na * CW);                        \
        } else {                                                                                   \
            unsigned ns = f->n / 2;                                                                \
            printf("1 %u %u\n", 3 * ns, 3 * ns);                                                   \
            for (int pass = 0; pass < 2; pass++)                                                   \
                for (unsigned k = 0; k < 3 * ns; k++) {                                            \
                    TC c = (pass ? f->a : f->b)[k] / f->a[3 * (k / 3)];                            \
                    wrn((float *)&c, CW);                                                          \
                }                                                                                  \
            wrn((float *)f->b, 3 * ns * CW); wrn((float *)f->a, 3 * ns * CW);                      \
        }                                                                                          \
        if (scanf("%u", &n) != 1) exit(2);                                                         \
        TI *x = malloc((n + 1) * sizeof(TI)), *y = malloc((n + 1) * sizeof(TI));                   \
        rdn((float *)x, n * SW);                                                                   \
        NAME##_execute_block(q, x, n, y);                                                          \
        wrn((float *)y, n * SW);                                                                   \
        NAME##_destroy(q);                                                                         \
    }
RUN(iirfilt_rrrf, float, float, 1, 1)
RUN(iirfilt_crcf, float, float complex, 1, 2)
RUN(iirfilt_cccf, float complex, float complex, 2, 2)
int main(void)
{
    char cmd[16];
    if (scanf("%15s", cmd) != 1) return 2;
    if (!strcmp(cmd, "rrrf")) run_iirfilt_rrrf();
    else if (!strcmp(cmd, "crcf")) run_iirfilt_crcf();
    else if (!strcmp(cmd, "cccf")) run_iirfilt_cccf();
    else if (!strcmp(cmd, "des")) {       /* ftype order fc Ap As -> B, A (sos) */
        int ft; unsigned order; if (scanf("%d %u", &ft, &order) != 2) return 2;
        float fc = rd(), Ap = rd(), As = rd();
        unsigned ns = (order + 1) / 2; float B[3 * ns], A[3 * ns];
        liquid_iirdes(ft, LIQUID_IIRDES_LOWPASS, LIQUID_IIRDES_SOS, order, fc, 0.0f, Ap, As, B, A);
        wrn(B, 3 * ns); wrn(A, 3 * ns);
    } else if (!strcmp(cmd, "lag") || !strcmp(cmd, "pi")) {
        float w = rd(), z = rd(), K = rd(), b[3], a[3];
        if (cmd[0] == 'l') iirdes_pll_active_lag(w, z, K, b, a); else iirdes_pll_active_PI(w, z, K, b, a);
        wrn(b, 3); wrn(a, 3);
    } else if (!strcmp(cmd, "zpk")) {
        unsigned n; if (scanf("%u", &n) != 1) return 2;
        float complex z[n], p[n], k; rdn((float *)z, 2 * n); rdn((float *)p, 2 * n); rdn((float *)&k, 2);
        unsigned ns = (n + 1) / 2; float B[3 * ns], A[3 * ns];
        iirdes_dzpk2sosf(z, p, n, k, B, A);
        wrn(B, 3 * ns); wrn(A, 3 * ns);
    } else return 3;
    return 0;
}
"""


def build(tmp):
    GF.DRIVER = DRIVER
    return GF.build_reference(tmp)


def bits(a):
    return " ".join(str(int(v)) for v in np.ascontiguousarray(a).view(np.float32).ravel().view(np.uint32))


def call(exe, text):
    out = subprocess.run([exe], input=text + "\n", capture_output=True, text=True, check=True).stdout.split()
    return out


def floats(tokens):
    return np.array([int(t) for t in tokens], np.uint32).view(np.float32)


def run_case(exe, kind, ctor, args, x):
    """-> dict(form, b, a normalised; raw_b, raw_a for sos), outputs"""
    cw, sw = (2 if kind == "cccf" else 1), (1 if kind == "rrrf" else 2)
    x = np.ascontiguousarray(x, IM.sample_dtype(kind))
    out = call(exe, "%s %s %s %d %s" % (kind, ctor, args, len(x), bits(x)))
    form, nb, na = int(out[0]), int(out[1]), int(out[2])
    k = 3
    b = floats(out[k:k + nb * cw]); k += nb * cw
    a = floats(out[k:k + na * cw]); k += na * cw
    res = {"form": "sos" if form else "norm", "b": b, "a": a}
    if form:
        res["held_b"] = floats(out[k:k + nb * cw]); k += nb * cw
        res["held_a"] = floats(out[k:k + na * cw]); k += na * cw
    y = floats(out[k:])
    assert len(y) == len(x) * sw
    return res, y


def num(v):
    v = np.float32(v)
    if not np.isfinite(v):
        return "NaN" if np.isnan(v) else ("Infinity" if v > 0 else "-Infinity")
    return GF.num(v)


def arr(a):
    return "[" + ",".join(num(v) for v in np.ascontiguousarray(a).view(np.float32).ravel()) + "]"


def parse_vectors(exe):
    vec = []
    for kind in ("rrrf", "crcf", "cccf"):
        for h in (3, 5, 7):
            name = "iirfilt_%s_data_h%dx64" % (kind, h)
            src = open(os.path.join(REF, "src", "filter", "tests", "data", name + ".c")).read()
            src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
            src = re.sub(r"//[^\n]*", "", src)
            got = {}
            for m in re.finditer(r"float(\s+complex)?\s+%s_(\w)\[\]\s*=\s*\{(.*?)\}\s*;" % name, src, re.S):
                vals = []
                for t in m.group(3).split(","):
                    if not t.strip():
                        continue
                    if m.group(1):
                        r, i = t.split("*_Complex_I")[0].rsplit("+", 1)
                        vals += [float(r), float(i)]
                    else:
                        vals.append(float(t))
                got[m.group(2)] = np.array(vals, np.float32)
            assert sorted(got) == ["a", "b", "x", "y"], sorted(got)
            cw = 2 if kind == "cccf" else 1
            assert len(got["b"]) == h * cw and len(got["a"]) == h * cw
            res, _ = run_case(exe, kind, "create", "%d %d %s %s" % (h, h, bits(got["b"]), bits(got["a"])),
                              np.zeros(0, IM.sample_dtype(kind)))
            vec.append({"name": name, "kind": kind, "b": got["b"], "a": got["a"], "bn": res["b"], "an": res["a"],
                        "x": got["x"], "y": got["y"]})
    return vec


def main():
    tmp = tempfile.mkdtemp(prefix="gen_iirfilt_")
    try:
        exe = build(tmp)
        f32 = lambda *v: np.array(v, np.float32)  # noqa: E731
        butter = floats(call(exe, "des 0 4 %s" % bits(f32(0.1, 0.1, 60.0))))
        ellip = floats(call(exe, "des 3 5 %s" % bits(f32(0.2, 0.1, 60.0))))
        bB, bA = butter[:6], butter[6:]
        eB, eA = ellip[:9], ellip[9:]
        # case 7: poles 0.95 e^{+-j0.3} e^{j0.2} -> z^2 + a1 z + a2 (complex coefficients)
        p = 0.95 * np.exp(1j * np.array([0.3, -0.3])) * np.exp(1j * 0.2)
        c1A = np.array([1.0, -(p[0] + p[1]), p[0] * p[1]], np.complex64)
        c1B = np.array([0.05, 0.1, 0.05], np.complex64)
        p2 = 0.8 * np.exp(1j * np.array([1.1, -0.9]))
        c2A = np.concatenate([c1A, np.array([1.0, -(p2[0] + p2[1]), p2[0] * p2[1]], np.complex64)])
        c2B = np.array([0.05 + 0.02j, 0.1 - 0.03j, 0.05 + 0.01j, 0.3 - 0.1j, 0.2 + 0.25j, -0.1 + 0.05j], np.complex64)
        # case 9: one section, poles at radius 1.01
        ua = f32(1.0, -2 * 1.01 * np.cos(0.4), 1.01 * 1.01)
        plan = [
            # name, kind, ctor, args text, ctor arguments for the tests, n
            ("dc_blocker_0.01", "crcf", "dc_blocker", bits(f32(0.01)), {"alpha": 0.01}, IM.NOUT),
            ("dc_blocker_1e-3", "rrrf", "dc_blocker", bits(f32(1e-3)), {"alpha": 1e-3}, IM.NOUT),
            ("pll", "rrrf", "pll", bits(f32(0.01, 0.707, 1000.0)), {"w": 0.01, "zeta": 0.707, "K": 1000.0}, IM.NOUT),
            ("integrator", "rrrf", "integrator", "", {}, IM.NOUT),
            ("integrator", "crcf", "integrator", "", {}, IM.NOUT),
            ("differentiator", "rrrf", "differentiator", "", {}, IM.NOUT),
            ("differentiator", "crcf", "differentiator", "", {}, IM.NOUT),
            ("butter4", "crcf", "create_sos", "2 %s %s" % (bits(bB), bits(bA)), {"B": bB, "A": bA}, IM.NOUT),
            ("butter4", "rrrf", "create_sos", "2 %s %s" % (bits(bB), bits(bA)), {"B": bB, "A": bA}, IM.NOUT),
            ("ellip5", "crcf", "create_sos", "3 %s %s" % (bits(eB), bits(eA)), {"B": eB, "A": eA}, IM.NOUT),
            ("cpoles1", "cccf", "create_sos", "1 %s %s" % (bits(c1B), bits(c1A)), {"B": c1B, "A": c1A}, IM.NOUT),
            ("cpoles2", "cccf", "create_sos", "2 %s %s" % (bits(c2B), bits(c2A)), {"B": c2B, "A": c2A}, IM.NOUT),
            ("a0_is_2", "rrrf", "create", "3 3 %s %s" % (bits(f32(0.2, 0.4, 0.2)), bits(f32(2.0, -1.6, 0.9))),
             {"B": f32(0.2, 0.4, 0.2), "A": f32(2.0, -1.6, 0.9)}, IM.NOUT),
            ("radius_1.01", "crcf", "create_sos", "1 %s %s" % (bits(f32(1.0, 0.5, 0.25)), bits(ua)),
             {"B": f32(1.0, 0.5, 0.25), "A": ua}, 200),
        ]
        body = []
        for idx, (name, kind, ctor, args, cargs, n) in enumerate(plan):
            seed = 4000 + 17 * idx
            res, y = run_case(exe, kind, ctor, args, IM.stream_input(kind, n, seed))
            f = ['"name":"%s_%s"' % (name, kind), '"kind":"%s"' % kind, '"ctor":"%s"' % ctor, '"form":"%s"' % res["form"],
                 '"n":%d' % n, '"seed":%d' % seed]
            for k, v in cargs.items():
                f.append('"%s":%s' % ("raw_" + k.lower() if k in ("B", "A") else k,
                                      arr(v) if isinstance(v, np.ndarray) else num(v)))
            f += ['"b":%s' % arr(res["b"]), '"a":%s' % arr(res["a"]), '"y":%s' % arr(y)]
            body.append("{" + ",\n".join(f) + "}")
            # the float32 model on what was just recorded (what tests/test_iirfilt_model.py asserts)
            cb = res["b"].view(np.complex64) if kind == "cccf" else res["b"]
            ca = res["a"].view(np.complex64) if kind == "cccf" else res["a"]
            ym, _ = IM.run32(kind, res["form"], cb, ca, IM.stream_input(kind, n, seed))
            same = np.array_equal(ym.view(np.float32).view(np.uint32), y.view(np.uint32))
            print("%-24s %s: float32 model %s" % (name, kind, "bit for bit" if same else "DIFFERS"))
        # helpers
        hl = []
        for cmd, w, z, K in (("lag", 0.01, 0.707, 1000.0), ("lag", 0.2, 0.3, 10.0), ("pi", 0.01, 0.707, 1000.0),
                             ("pi", 0.35, 0.9, 2.5)):
            r = floats(call(exe, "%s %s" % (cmd, bits(f32(w, z, K)))))
            hl.append('{"fn":"%s","w":%s,"zeta":%s,"K":%s,"b":%s,"a":%s}' % (cmd, num(w), num(z), num(K), arr(r[:3]),
                                                                         arr(r[3:])))
        zs = np.array([-1.0, 0.3 + 0.8j, 0.3 - 0.8j, -0.5 + 0.1j, -0.5 - 0.1j], np.complex64)
        ps = np.array([0.7, 0.2 - 0.6j, 0.2 + 0.6j, 0.5 + 0.5j, 0.5 - 0.5j], np.complex64)
        for n, k in ((5, 0.02), (4, 0.3)):
            r = floats(call(exe, "zpk %d %s %s %s" % (n, bits(zs[5 - n:]), bits(ps[5 - n:]), bits(f32(k, 0.0)))))
            ns = (n + 1) // 2
            hl.append('{"fn":"zpk","z":%s,"p":%s,"k":%s,"b":%s,"a":%s}' % (arr(zs[5 - n:]), arr(ps[5 - n:]), num(k),
                                                                       arr(r[:3 * ns]), arr(r[3 * ns:])))
        vb = []
        for v in parse_vectors(exe):
            vb.append('{"name":"%s","kind":"%s","tol":0.001,\n%s}' % (
                v["name"], v["kind"], ",\n".join('"%s":%s' % (k, arr(v[k])) for k in ("b", "a", "bn", "an", "x", "y"))))
        txt = '{"cases":[\n%s\n],\n"helpers":[\n%s\n],\n"vectors":[\n%s\n]}\n' % (",\n".join(body), ",\n".join(hl),
                                                                              ",\n".join(vb))
        json.loads(txt)
        out = os.path.join(HERE, "iirfilt.json")
        open(out, "w").write(txt)
        print("wrote %s: %d bytes" % (out, len(txt)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
