#!/usr/bin/env python3
"""Record liquid-dsp's recursive filter designs and its iirdecim / iirinterp
as a JSON fixture (tests/golden/iirdes.json).

Runs ONLY where the reference sources are present: as gen_iirfilt.py, it uses
gen_firhilb.py's recipe (the sources copied to a temporary directory,
libliquid.a built there), drives the library through the small C program
below and records what it returned.  Nothing compiled and none of the
reference's text is kept: the fixture holds numbers only.

Contents:
  designs   liquid_iirdes on recorded arguments: B, A
  azpk      the five analog prototypes for n = 4 and 5: zeros, poles, gain
  bilinear  bilinear_zpkf on one of them
  stable    iirdes_isstable on the reference's two autotest cases and on two
            of the designs in TF form
  cplxpair  the reference's autotest vectors (n = 6 and n = 20), copied as
            data with their tolerance
  streams   iirdecim and iirinterp: the constructor and its arguments, the
            coefficients of the filter inside (from liquid_iirdes on the same
            arguments, or as given to create) and the first NOUT outputs of
            execute_block.  Inputs are not stored: tests/iirfilt_model.py
            (stream_input) regenerates them.
Floats are written with the shortest decimal text that reads back to the same
float32.  For every stream the generator prints whether the float32 model
(iirfilt_model.run32: the decimator is run32(x)[::M], the interpolator run32
of the stuffed input) reproduces the recorded outputs bit for bit.

Usage:  python tests/golden/gen_iirdes.py [reference-directory]
"""
import json
import os
import re
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gen_firhilb as GF  # noqa: E402  (the reference build recipe)
import gen_iirfilt as GI  # noqa: E402  (bits, call, floats, num, arr)
import iirfilt_model as IM  # noqa: E402

REF = GF.REF
NOUT = IM.NOUT

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <complex.h>
#include "liquid.h"
/* stdin: one command; floats travel as uint32 bit patterns both ways */
static float rd(void) { uint32_t b; float f; if (scanf("%u", &b) != 1) exit(2); memcpy(&f, &b, 4); return f; }
static unsigned ru(void) { unsigned v; if (scanf("%u", &v) != 1) exit(2); return v; }
static void wr(float f) { uint32_t b; memcpy(&b, &f, 4); printf("%u\n", b); }
static void rdn(float *p, unsigned n) { for (unsigned i = 0; i < n; i++) p[i] = rd(); }
static void wrn(const float *p, unsigned n) { for (unsigned i = 0; i < n; i++) wr(p[i]); }
static unsigned deslen(int bt, int fmt, unsigned order)
{
    unsigned N = (bt >= 2) ? 2 * order : order;
    return fmt == LIQUID_IIRDES_SOS ? 3 * ((N + 1) / 2) : N + 1;
}
#define RATE(OBJ, FILT, TC, TI, CW, SW, DECIM)                                                     \
    static void run_##OBJ(void)                                                                    \
    {                                                                                              \
        char ctor[16]; OBJ q = NULL; unsigned M;                                                   \
        if (scanf("%15s %u", ctor, &M) != 2) exit(2);                                              \
        if (!strcmp(ctor, "default")) { unsigned o = ru(); q = OBJ##_create_default(M, o);         \
        } else if (!strcmp(ctor, "proto")) {                                                       \
            int ft = ru(), bt = ru(), fm = ru(); unsigned o = ru();                                \
            float fc = rd(), f0 = rd(), Ap = rd(), As = rd();                                      \
            q = OBJ##_create_prototype(M, ft, bt, fm, o, fc, f0, Ap, As);                          \
        } else {                                                                                   \
            unsigned nb = ru(), na = ru(); TC b[nb], a[na];                                        \
            rdn((float *)b, nb * CW); rdn((float *)a, na * CW);                                    \
            q = OBJ##_create(M, b, nb, a, na);                                                     \
        }                                                                                          \
        unsigned n = ru(), nin = DECIM ? n * M : n, nout = DECIM ? n : n * M;                      \
        TI *x = malloc((nin + 1) * sizeof(TI)), *y = malloc((nout + 1) * sizeof(TI));              \
        rdn((float *)x, nin * SW);                                                                 \
        OBJ##_execute_block(q, x, n, y);                                                           \
        wrn((float *)y, nout * SW);                                                                \
        OBJ##_destroy(q);                                                                          \
    }
RATE(iirdecim_rrrf, iirfilt_rrrf, float, float, 1, 1, 1)
RATE(iirdecim_crcf, iirfilt_crcf, float, float complex, 1, 2, 1)
RATE(iirdecim_cccf, iirfilt_cccf, float complex, float complex, 2, 2, 1)
RATE(iirinterp_rrrf, iirfilt_rrrf, float, float, 1, 1, 0)
RATE(iirinterp_crcf, iirfilt_crcf, float, float complex, 1, 2, 0)
RATE(iirinterp_cccf, iirfilt_cccf, float complex, float complex, 2, 2, 0)
int main(void)
{
    char cmd[24];
    if (scanf("%23s", cmd) != 1) return 2;
    if (!strcmp(cmd, "iirdecim_rrrf")) run_iirdecim_rrrf();
    else if (!strcmp(cmd, "iirdecim_crcf")) run_iirdecim_crcf();
    else if (!strcmp(cmd, "iirdecim_cccf")) run_iirdecim_cccf();
    else if (!strcmp(cmd, "iirinterp_rrrf")) run_iirinterp_rrrf();
    else if (!strcmp(cmd, "iirinterp_crcf")) run_iirinterp_crcf();
    else if (!strcmp(cmd, "iirinterp_cccf")) run_iirinterp_cccf();
    else if (!strcmp(cmd, "des")) {       /* ftype btype format order fc f0 Ap As -> B, A */
        int ft = ru(), bt = ru(), fm = ru(); unsigned order = ru();
        float fc = rd(), f0 = rd(), Ap = rd(), As = rd();
        unsigned n = deslen(bt, fm, order); float B[n + 1], A[n + 1];
        liquid_iirdes(ft, bt, fm, order, fc, f0, Ap, As, B, A);
        wrn(B, n); wrn(A, n);
    } else if (!strcmp(cmd, "azpk")) {    /* which n [parameters] -> z (2 floor(n/2) values), p, k */
        int which = ru(); unsigned n = ru();
        float complex z[n + 2], p[n + 2], k = 0;   /* the Bessel routine writes n + 1 poles */
        memset(z, 0, sizeof(z));
        if (which == 0) butter_azpkf(n, z, p, &k);
        else if (which == 1) { float ep = rd(); cheby1_azpkf(n, ep, z, p, &k); }
        else if (which == 2) { float es = rd(); cheby2_azpkf(n, es, z, p, &k); }
        else if (which == 3) { float ep = rd(), es = rd(); ellip_azpkf(n, ep, es, z, p, &k); }
        else bessel_azpkf(n, z, p, &k);
        wrn((float *)z, 2 * 2 * (n / 2)); wrn((float *)p, 2 * n); wrn((float *)&k, 2);
    } else if (!strcmp(cmd, "bil")) {     /* nza npa za pa ka m -> zd, pd, kd */
        unsigned nza = ru(), npa = ru(); float complex za[nza + 1], pa[npa], zd[npa], pd[npa], ka, kd;
        rdn((float *)za, 2 * nza); rdn((float *)pa, 2 * npa); rdn((float *)&ka, 2);
        float m = rd();
        bilinear_zpkf(za, nza, pa, npa, ka, m, zd, pd, &kd);
        wrn((float *)zd, 2 * npa); wrn((float *)pd, 2 * npa); wrn((float *)&kd, 2);
    } else if (!strcmp(cmd, "stab")) {
        unsigned n = ru(); float b[n], a[n]; rdn(b, n); rdn(a, n);
        printf("%d\n", iirdes_isstable(b, a, n));
    } else return 3;
    return 0;
}
"""

FT = {"butter": 0, "cheby1": 1, "cheby2": 2, "ellip": 3, "bessel": 4}
BT = {"lowpass": 0, "highpass": 1, "bandpass": 2, "bandstop": 3}
FM = {"sos": 0, "tf": 1}

# name, ftype, btype, format, order, fc, f0, Ap, As
DESIGNS = [
    ("butter2_tf", "butter", "lowpass", "tf", 2, 0.25, 0.0, 1.0, 40.0),      # the reference's autotest
    ("butter4", "butter", "lowpass", "sos", 4, 0.1, 0.0, 0.1, 60.0),
    ("butter7", "butter", "lowpass", "sos", 7, 0.15, 0.0, 0.1, 60.0),
    ("cheby1_5", "cheby1", "lowpass", "sos", 5, 0.2, 0.0, 0.5, 60.0),
    ("cheby2_6", "cheby2", "lowpass", "sos", 6, 0.2, 0.0, 0.1, 50.0),
    ("ellip5", "ellip", "lowpass", "sos", 5, 0.2, 0.0, 0.1, 60.0),
    ("ellip8", "ellip", "lowpass", "sos", 8, 0.12, 0.0, 0.2, 50.0),
    ("bessel4", "bessel", "lowpass", "sos", 4, 0.15, 0.0, 0.1, 60.0),
    ("butter3_hp", "butter", "highpass", "sos", 3, 0.3, 0.0, 0.1, 60.0),
    ("butter4_bp", "butter", "bandpass", "sos", 4, 0.1, 0.25, 0.1, 60.0),
    ("butter3_bs", "butter", "bandstop", "sos", 3, 0.1, 0.2, 0.1, 60.0),
    ("ellip4_hp", "ellip", "highpass", "sos", 4, 0.25, 0.0, 0.1, 60.0),
    ("ellip3_bp", "ellip", "bandpass", "sos", 3, 0.08, 0.2, 0.1, 40.0),
    ("ellip4_bs", "ellip", "bandstop", "sos", 4, 0.12, 0.3, 0.1, 40.0),
    ("butter4_tf", "butter", "lowpass", "tf", 4, 0.2, 0.0, 0.1, 60.0),
]
AZPK = [("butter", ()), ("cheby1", (0.35,)), ("cheby2", (0.01,)), ("ellip", (0.35, 1000.0)), ("bessel", ())]

f32 = lambda *v: np.array(v, np.float32)  # noqa: E731


def design(exe, d):
    _, ft, bt, fm, order, fc, f0, Ap, As = d
    r = GI.floats(GI.call(exe, "des %d %d %d %d %s" % (FT[ft], BT[bt], FM[fm], order, GI.bits(f32(fc, f0, Ap, As)))))
    return r[:len(r) // 2], r[len(r) // 2:]


def parse_cplxpair():
    src = open(os.path.join(REF, "src", "filter", "tests", "iirdes_autotest.c")).read()
    out = []
    for n in (6, 20):
        body = src[src.index("autotest_iirdes_cplxpair_n%d" % n):]
        got = {}
        for key in ("r", "ptest"):
            m = re.search(r"float complex %s\[%d\]\s*=\s*\{(.*?)\};" % (key, n), body, re.S)
            vals = []
            for t in m.group(1).split(","):
                mm = re.match(r"\s*(-?[\d.]+)\s*([+-])\s*([\d.]+)\s*\*\s*_Complex_I", t)
                vals += [float(mm.group(1)), float(mm.group(2) + mm.group(3))]
            got[key] = np.array(vals, np.float32)
        out.append((n, got["r"], got["ptest"]))
    return out


def stuffed(x, M):
    z = np.zeros(len(x) * M, x.dtype)
    z[::M] = x
    return z


def main():
    tmp = tempfile.mkdtemp(prefix="gen_iirdes_")
    try:
        GF.DRIVER = DRIVER
        exe = GF.build_reference(tmp)
        num, arr = GI.num, GI.arr
        des, rec = [], {}
        for d in DESIGNS:
            B, A = design(exe, d)
            rec[d[0]] = (B, A)
            des.append('{"name":"%s","ftype":"%s","btype":"%s","format":"%s","order":%d,"fc":%s,"f0":%s,"Ap":%s,"As":%s,\n'
                       '"b":%s,\n"a":%s}' % (d[:5] + tuple(num(v) for v in d[5:]) + (arr(B), arr(A))))
        az, keep = [], None
        for n in (4, 5):
            for which, (name, par) in enumerate(AZPK):
                r = GI.floats(GI.call(exe, "azpk %d %d %s" % (which, n, GI.bits(f32(*par)) if par else "")))
                nz = 2 * (n // 2) if name in ("cheby2", "ellip") else 0
                z, p, k = r[:2 * nz], r[4 * (n // 2):4 * (n // 2) + 2 * n], r[-2:]
                az.append('{"fn":"%s","n":%d,"par":%s,"z":%s,"p":%s,"k":%s}' % (name, n, arr(f32(*par)), arr(z), arr(p),
                                                                            arr(k)))
                if name == "ellip" and n == 5:
                    keep = (z, p)
        m = np.float32(0.5)
        r = GI.floats(GI.call(exe, "bil 4 5 %s %s %s %s" % (GI.bits(keep[0]), GI.bits(keep[1]), GI.bits(f32(1.0, 0.0)),
                                                          GI.bits(m))))
        bil = '{"za":%s,"pa":%s,"ka":[1,0],"m":%s,"zd":%s,"pd":%s,"kd":%s}' % (arr(keep[0]), arr(keep[1]), num(m),
                                                                         arr(r[:10]), arr(r[10:20]), arr(r[20:]))
        st = []
        auto_b = f32(0.292893218813452, 0.585786437626905, 0.292893218813452)
        for name, b, a in (("autotest_n2_yes", auto_b, f32(1.0, 0.0, 0.171572875253810)),
                           ("autotest_n2_no", auto_b, f32(1.0, 0.0, 1.171572875253810)),
                           ("butter2_tf",) + rec["butter2_tf"], ("butter4_tf",) + rec["butter4_tf"]):
            v = int(GI.call(exe, "stab %d %s %s" % (len(a), GI.bits(b), GI.bits(a)))[0])
            st.append('{"name":"%s","b":%s,"a":%s,"stable":%d}' % (name, arr(b), arr(a), v))
        cp = ['{"n":%d,"tol":1e-8,"pair_tol":1e-6,"z":%s,"p":%s}' % (n, arr(z), arr(p)) for n, z, p in parse_cplxpair()]

        # streams
        with open(IM.FIXTURE) as f:
            c1 = next(c for c in json.load(f)["cases"] if c["name"] == "cpoles1_cccf")
        c1b, c1a = f32(*c1["raw_b"]), f32(*c1["raw_a"])
        hp = ("hp", "butter", "highpass", "sos", 4, 0.3, 0.0, 0.1, 60.0)
        plan = [("default", "crcf", 2, 4), ("default", "crcf", 3, 5), ("default", "crcf", 5, 8), ("default", "rrrf", 4, 3),
                ("create", "cccf", 3, None), ("proto", "crcf", 4, hp)]
        body = []
        for idx, (ctor, kind, M, arg) in enumerate(plan):
            if ctor == "default":
                dd = ("d", "butter", "lowpass", "sos", arg, float(np.float32(0.5) / np.float32(M)), 0.0, 0.1, 60.0)
                B, A = design(exe, dd)
                form, text, extra = "sos", "default %d %d" % (M, arg), '"order":%d' % arg
            elif ctor == "proto":
                B, A = design(exe, arg)
                form = "sos"
                text = "proto %d %d %d %d %d %s" % (M, FT[arg[1]], BT[arg[2]], FM[arg[3]], arg[4], GI.bits(f32(*arg[5:])))
                extra = '"ftype":"%s","btype":"%s","format":"%s","order":%d,"fc":%s,"f0":%s,"Ap":%s,"As":%s' % (
                    arg[1:5] + tuple(num(v) for v in arg[5:]))
            else:
                B, A, form = c1b, c1a, "norm"
                text = "create %d 3 3 %s %s" % (M, GI.bits(B), GI.bits(A))
                extra = '"raw_b":%s,"raw_a":%s' % (arr(B), arr(A))
            cb = B.view(np.complex64) if kind == "cccf" else B
            ca = A.view(np.complex64) if kind == "cccf" else A
            for obj in ("iirdecim", "iirinterp"):
                seed = 6000 + 13 * (2 * idx + (obj == "iirinterp"))
                n = NOUT if obj == "iirdecim" else (NOUT + M - 1) // M
                x = IM.stream_input(kind, n * M if obj == "iirdecim" else n, seed)
                y = GI.floats(GI.call(exe, "%s_%s %s %d %s" % (obj, kind, text, n, GI.bits(x))))
                y = y[:NOUT * (1 if kind == "rrrf" else 2)]
                full, _ = IM.run32(kind, form, cb, ca, x if obj == "iirdecim" else stuffed(x, M))
                ym = np.ascontiguousarray((full[::M] if obj == "iirdecim" else full)[:NOUT])
                same = np.array_equal(ym.view(np.float32).view(np.uint32), y.view(np.uint32))
                name = "%s_%s_%s_M%d" % (obj, ctor, kind, M)
                print("%-32s float32 model %s" % (name, "bit for bit" if same else "DIFFERS"))
                body.append('{"name":"%s","obj":"%s","kind":"%s","ctor":"%s","M":%d,%s,\n"form":"%s","n":%d,"seed":%d,\n'
                            '"b":%s,\n"a":%s,\n"y":%s}' % (name, obj, kind, ctor, M, extra, form, n, seed, arr(B), arr(A),
                                                         arr(y)))
        txt = ('{"designs":[\n%s\n],\n"azpk":[\n%s\n],\n"bilinear":%s,\n"stable":[\n%s\n],\n"cplxpair":[\n%s\n],\n'
               '"streams":[\n%s\n]}\n' % (",\n".join(des), ",\n".join(az), bil, ",\n".join(st), ",\n".join(cp),
                                         ",\n".join(body)))
        json.loads(txt)
        out = os.path.join(HERE, "iirdes.json")
        open(out, "w").write(txt)
        print("wrote %s: %d bytes" % (out, len(txt)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
