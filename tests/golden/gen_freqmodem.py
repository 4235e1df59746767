#!/usr/bin/env python3
"""Record liquid-dsp's freqmod and freqdem as a JSON fixture (tests/golden/freqmodem.json).

Runs ONLY where the reference sources are present: as gen_nco.py, it copies
them to a temporary directory, builds libliquid.a there with the recipe of
gen_firhilb.py, drives the two objects through the small C program below and
records what they returned.  Nothing compiled and none of the reference's text
is kept: the fixture holds numbers only, every float as its uint32 bit pattern.

Contents:
  table    the 1024 table entries (re, im), read with increments of 64 from 0
  cases    per case of tests/freqmodem_model.py's case_list: the outputs of its
           calls in order (freqmod: re, im per sample; freqdem: one float) and,
           for freqmod, the accumulator after the case.  The interface does not
           show the accumulator: it is read from a second run of the case
           followed by 64 samples that each add 1 (freqmodem_model.
           phase_from_probe).  The inputs are not stored: case_list regenerates
           them from integer arithmetic.
           mod_kf* / dem_kf*   256 samples per kf: a block, per-sample calls, a block
           roundtrip_mod_kf*   the autotest's three cosines, modulated; "dem":
                               that output demodulated by a fresh freqdem
           halfway, range      exact half-way products; products beyond 2^31,
                               infinite and NaN
           quadrants, zeros    freqdem: first samples after reset in the four
                               quadrants; samples next to exact zeros

Usage:  python tests/golden/gen_freqmodem.py [reference-directory]
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gen_firhilb as GF  # noqa: E402  (the reference build recipe)
import freqmodem_model as FM  # noqa: E402

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <complex.h>
#include "liquid.h"
/* stdin: "M kf" (freqmod) or "D kf" (freqdem), then ops "b n" (one block call),
 * "s n" (n per-sample calls), each followed by its input floats, and "r 0"
 * (reset); every float a uint32 bit pattern; stdout: the outputs the same way */
static float fb(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static float rd(void) { uint32_t b; if (scanf("%u", &b) != 1) exit(2); return fb(b); }
static void wr(float f) { uint32_t b; memcpy(&b, &f, 4); printf("%u\n", b); }
int main(void)
{
    char kind[4], op[4]; unsigned kfb, n;
    if (scanf("%3s %u", kind, &kfb) != 2) return 2;
    freqmod mod = kind[0] == 'M' ? freqmod_create(fb(kfb)) : NULL;
    freqdem dem = kind[0] == 'D' ? freqdem_create(fb(kfb)) : NULL;
    while (scanf("%3s %u", op, &n) == 2) {
        if (op[0] == 'r') { if (mod) freqmod_reset(mod); else freqdem_reset(dem); continue; }
        float *m = malloc((n + 1) * sizeof(float));
        float complex *s = malloc((n + 1) * sizeof(float complex));
        if (mod) {
            for (unsigned i = 0; i < n; i++) m[i] = rd();
            if (op[0] == 'b') freqmod_modulate_block(mod, m, n, s);
            else for (unsigned i = 0; i < n; i++) freqmod_modulate(mod, m[i], &s[i]);
            for (unsigned i = 0; i < n; i++) { wr(crealf(s[i])); wr(cimagf(s[i])); }
        } else {
            /* the parts are stored, not added: re + I * im loses the sign of a zero */
            for (unsigned i = 0; i < n; i++) { float *z = (float *)&s[i]; z[0] = rd(); z[1] = rd(); }
            if (op[0] == 'b') freqdem_demodulate_block(dem, s, n, m);
            else for (unsigned i = 0; i < n; i++) freqdem_demodulate(dem, s[i], &m[i]);
            for (unsigned i = 0; i < n; i++) wr(m[i]);
        }
        free(m); free(s);
    }
    if (mod) freqmod_destroy(mod); else freqdem_destroy(dem);
    return 0;
}
"""


def drive(exe, kind, kf, ops):
    txt = ["%s %d" % ("M" if kind == "mod" else "D", int(FM.bits(np.array([kf], np.float32))[0]))]
    for op, x in ops:
        if op == "r":
            txt.append("r 0")
            continue
        txt.append("%s %d" % (op, len(x)))
        txt.append(" ".join(str(int(b)) for b in FM.bits(x)))
    out = subprocess.run([exe], input="\n".join(txt) + "\n", capture_output=True, text=True, check=True).stdout.split()
    return np.array([int(t) for t in out], np.uint32)


def cplx(v):
    f = v.view(np.float32)
    return (f[0::2] + 1j * f[1::2]).astype(np.complex64)


def ints(a):
    return "[%s]" % ",".join(str(int(v)) for v in a)


def main():
    tmp = tempfile.mkdtemp(prefix="gen_freqmodem_")
    try:
        GF.DRIVER = DRIVER
        exe = GF.build_reference(tmp)
        # kf = 1 (ref = 65536): the first sample adds 0, every other one exactly 64, which is one
        # table entry: the outputs are entries 0, 1, ..., 1023
        walk = np.full(FM.TABLE_LEN, 64.0 / 65536.0, np.float32)
        walk[0] = 0
        table_bits = drive(exe, "mod", 1.0, [("b", walk)])
        table = cplx(table_bits)
        worst = max(np.max(np.abs(table.real.astype(float) - FM.table64().real)),
                    np.max(np.abs(table.imag.astype(float) - FM.table64().imag)))
        print("table: %d entries differ in bits from the float64-rounded one, worst %.3g 2^-24"
              % (np.count_nonzero(FM.bits(table) != FM.bits(FM.table64())), worst / 2.0 ** -24))
        body, ratio = [], 0.0
        for name, kind, kf, ops in FM.case_list():
            vals = drive(exe, kind, kf, ops)
            rec = '{"name":"%s","kind":"%s","kf":%d,\n"out":%s' % (name, kind, int(FM.bits(np.array([kf], np.float32))[0]),
                                                                    ints(vals))
            if kind == "mod":
                both = cplx(drive(exe, kind, kf, ops + [("s", FM.probe_message(kf))]))
                acc = FM.phase_from_probe(table, both[-65], both[-64:])
                rec += ',\n"acc":%d' % acc
                m = FM.ModModel(kf, table)
                mv = np.concatenate([m.block(x) if op == "b" else m.step(x) for op, x in ops])
                print("%-22s model outputs %s, accumulator %s" % (
                    name, "equal" if np.array_equal(FM.bits(mv), vals) else "DIFFER",
                    "equal" if m.phase == acc else "DIFFERS (%d, %d)" % (m.phase, acc)))
                if name.startswith("roundtrip"):
                    dv = drive(exe, "dem", kf, [("b", cplx(vals))])
                    rec += ',\n"dem":%s' % ints(dv)
                    re, im = FM.DemModel(kf).block(cplx(vals))
                    ratio = max(ratio, FM.report(dv.view(np.float32), re, im, FM.dem_ref(kf), e=1.0))
            else:
                m, parts = FM.DemModel(kf), []
                for op, x in ops:
                    if op == "r":
                        m.reset()
                    else:
                        parts.append(m.block(x))
                re, im = (np.concatenate([p[i] for p in parts]) for i in (0, 1))
                r1 = FM.report(vals.view(np.float32), re, im, m.ref, e=1.0)
                rn = FM.report(FM.reference32(re, im, m.ref), re, im, m.ref, e=1.0)
                ratio = max(ratio, r1)
                print("%-22s reference %.3g of the E = 1 bound, numpy float32 %.3g" % (name, r1, rn))
            body.append(rec + "}")
        print("worst ratio of the recorded freqdem outputs against E = 1: %.4g" % ratio)
        txt = '{"table":%s,\n"cases":[\n%s\n]}\n' % (ints(table_bits), ",\n".join(body))
        json.loads(txt)
        out = os.path.join(HERE, "freqmodem.json")
        open(out, "w").write(txt)
        print("wrote %s: %d bytes" % (out, len(txt)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
