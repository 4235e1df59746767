#!/usr/bin/env python3
"""Record liquid-dsp's nco_crcf as a JSON fixture (tests/golden/nco.json).

Runs ONLY where the reference sources are present: as gen_autocorr.py, it
copies them to a temporary directory, builds libliquid.a there with the recipe
of gen_firhilb.py, drives nco_crcf through the small C program below and
records what it returned.  Nothing compiled and none of the reference's text
is kept: the fixture holds numbers only, every float as its uint32 bit pattern.

Contents:
  table    the 256 sine table values, read with set_phase / cexpf
  cases    per case of tests/nco_model.py's case_ops: the type (0 nco, 1 vco),
           the op sequence (nco_model's docstring has the op names), the values
           it returned and the phase after it.  The samples are not stored:
           nco_model.stream_input regenerates them from integer arithmetic.
           The phase-, frequency- and pll- cases re-run the scenarios of the
           reference's autotests of those names (set a phase and read sin / cos;
           step a tone and read it; lock a loop onto a tone).
  long     the phase after 200 000 steps from 0, per frequency of nco_model.LONG_D
  unwrap   liquid_unwrap_phase and liquid_unwrap_phase2 of nco_model.unwrap_input

Usage:  python tests/golden/gen_nco.py [reference-directory]
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
import nco_model as NM  # noqa: E402

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <complex.h>
#include "liquid.h"
/* stdin: the type (0 nco, 1 vco; 8 / 9: unwrap / unwrap2 of "n" floats), then
 * ops "name arg", sample ops followed by their input floats, every float a
 * uint32 bit pattern; stdout: the recorded floats the same way, then the phase */
static float fb(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static float rd(void) { uint32_t b; if (scanf("%u", &b) != 1) exit(2); return fb(b); }
static void wr(float f) { uint32_t b; memcpy(&b, &f, 4); printf("%u\n", b); }
static void wrc(float complex y) { wr(crealf(y)); wr(cimagf(y)); }
int main(void)
{
    unsigned type, arg; char op[4];
    if (scanf("%u", &type) != 1) return 2;
    if (type >= 8) {
        unsigned n;
        if (scanf("%u", &n) != 1) return 2;
        float *t = malloc((n + 1) * sizeof(float));
        for (unsigned i = 0; i < n; i++) t[i] = rd();
        if (type == 8) liquid_unwrap_phase(t, n); else liquid_unwrap_phase2(t, n);
        for (unsigned i = 0; i < n; i++) wr(t[i]);
        return 0;
    }
    nco_crcf q = nco_crcf_create(type ? LIQUID_VCO : LIQUID_NCO);
    while (scanf("%3s %u", op, &arg) == 2) {
        float complex y, *x;
        switch (op[0]) {
        case 'F': nco_crcf_set_frequency(q, fb(arg)); break;
        case 'f': nco_crcf_adjust_frequency(q, fb(arg)); break;
        case 'P': nco_crcf_set_phase(q, fb(arg)); break;
        case 'p': nco_crcf_adjust_phase(q, fb(arg)); break;
        case 'B': nco_crcf_pll_set_bandwidth(q, fb(arg)); break;
        case 'L': nco_crcf_pll_step(q, fb(arg)); break;
        case 'R': nco_crcf_reset(q); break;
        case 'S': for (unsigned i = 0; i < arg; i++) nco_crcf_step(q); break;
        case 'U': case 'D':
            x = malloc((arg + 1) * sizeof(float complex));
            for (unsigned i = 0; i < arg; i++) { float re = rd(), im = rd(); x[i] = re + _Complex_I * im; }
            if (op[0] == 'U') nco_crcf_mix_block_up(q, x, x, arg); else nco_crcf_mix_block_down(q, x, x, arg);
            for (unsigned i = 0; i < arg; i++) wrc(x[i]);
            free(x);
            break;
        case 'u': case 'd':
            for (unsigned i = 0; i < arg; i++) {
                float re = rd(), im = rd();
                if (op[0] == 'u') nco_crcf_mix_up(q, re + _Complex_I * im, &y);
                else nco_crcf_mix_down(q, re + _Complex_I * im, &y);
                nco_crcf_step(q);
                wrc(y);
            }
            break;
        case 'm': { float re = rd(), im = rd(); nco_crcf_mix_up(q, re + _Complex_I * im, &y); wrc(y); } break;
        case 'c': nco_crcf_cexpf(q, &y); wrc(y); break;
        case 'g': wr(nco_crcf_get_phase(q)); wr(nco_crcf_get_frequency(q)); break;
        default: return 3;
        }
    }
    wr(nco_crcf_get_phase(q));
    nco_crcf_destroy(q);
    return 0;
}
"""


def drive(exe, typ, ops, x):
    """returns (recorded values as uint32, phase bits)"""
    txt, k = [str(typ)], 0
    for name, arg in ops:
        txt.append("%s %d" % (name, arg))
        n = arg if name in "UDud" else 1 if name == "m" else 0
        if n:
            txt.append(" ".join(str(int(b)) for b in x[k:k + n].view(np.uint32)))
            k += n
    out = subprocess.run([exe], input="\n".join(txt) + "\n", capture_output=True, text=True, check=True).stdout.split()
    v = np.array([int(t) for t in out], np.uint32)
    return v[:-1], int(v[-1])


def drive_unwrap(exe, which, t):
    txt = "%d %d\n%s\n" % (which, len(t), " ".join(str(int(b)) for b in t.view(np.uint32)))
    out = subprocess.run([exe], input=txt, capture_output=True, text=True, check=True).stdout.split()
    return np.array([int(v) for v in out], np.uint32)


def ints(a):
    return "[%s]" % ",".join(str(int(v)) for v in a)


def main():
    tmp = tempfile.mkdtemp(prefix="gen_nco_")
    try:
        GF.DRIVER = DRIVER
        exe = GF.build_reference(tmp)
        ops = [op for phi in NM.table_phases() for op in (("P", NM.bits(phi)), ("c", 0))]
        vals, _ = drive(exe, NM.NCO, ops, np.zeros(0, np.complex64))
        table = vals[1::2].copy()                       # cexpf returns (cos, sin)
        tab32 = table.view(np.float32)
        body = []
        for idx, (name, typ, ops) in enumerate(NM.case_ops(tab32)):
            seed = NM.case_seed(idx)
            x = NM.stream_input(NM.samples_of(ops), seed)
            assert len(x) <= 4096
            vals, phase = drive(exe, typ, ops, x)
            body.append('{"name":"%s","type":%d,"seed":%d,\n"ops":%s,\n"out":%s,\n"phase":%d}'
                        % (name, typ, seed, json.dumps([[n, int(a)] for n, a in ops], separators=(",", ":")),
                           ints(vals), phase))
            # what tests/test_nco_model.py asserts, on what was just recorded
            m = NM.Model(typ, tab32)
            mv, recs = m.run(ops, x)
            same = np.array_equal(mv.view(np.uint32), vals)
            worst = 0.0
            if recs:
                y64, xs = NM.reference64(typ, recs, x)
                worst = NM.report(NM.mix_outputs(ops, vals.view(np.float32)), y64, xs)
            print("%-14s %4d samples: model %s, phase %s, worst %.3g of the bound"
                  % (name, len(x), "equal" if same else "DIFFERS", "equal" if NM.bits(m.theta) == phase else "DIFFERS",
                     worst))
        longs = []
        for d in NM.LONG_D:
            _, phase = drive(exe, NM.NCO, [("F", NM.bits(np.float32(d))), ("S", NM.LONG_STEPS)], np.zeros(0, np.complex64))
            longs.append('{"d":%d,"phase":%d}' % (NM.bits(np.float32(d)), phase))
        t = NM.unwrap_input()
        txt = ('{"table":%s,\n"cases":[\n%s\n],\n"long":[%s],\n"unwrap":{"basic":%s,"advanced":%s}}\n'
               % (ints(table), ",\n".join(body), ",".join(longs), ints(drive_unwrap(exe, 8, t)),
                  ints(drive_unwrap(exe, 9, t))))
        json.loads(txt)
        out = os.path.join(HERE, "nco.json")
        open(out, "w").write(txt)
        print("wrote %s: %d bytes" % (out, len(txt)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
