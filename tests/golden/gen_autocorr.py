#!/usr/bin/env python3
"""Record liquid-dsp's autocorr as a JSON fixture (tests/golden/autocorr.json).

Runs ONLY where the reference sources are present: as gen_iirfilt.py, it
copies them to a temporary directory, builds libliquid.a there with the recipe
of gen_firhilb.py, drives autocorr_cccf / autocorr_rrrf through the small C
program below and records what they returned.  Nothing compiled and none of
the reference's text is kept: the fixture holds numbers only.

Contents, per stream of tests/autocorr_model.py's CASES: the type, window,
delay, how the object was driven ("block": one execute_block; "push": a push
and an execute per sample), the NOUT outputs and get_energy after the last
sample.  Inputs are not stored: autocorr_model.stream_input regenerates them
from integer arithmetic.  Outputs are written with the shortest decimal text
that reads back to the same float32.

Usage:  python tests/golden/gen_autocorr.py [reference-directory]
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
import autocorr_model as AM  # noqa: E402

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <complex.h>
#include "liquid.h"
/* stdin: "kind W d drive n" then the input floats as uint32 bit patterns;
 * stdout: the output floats, then get_energy, the same way */
static float rd(void) { uint32_t b; float f; if (scanf("%u", &b) != 1) exit(2); memcpy(&f, &b, 4); return f; }
static void wr(float f) { uint32_t b; memcpy(&b, &f, 4); printf("%u\n", b); }
#define RUN(NAME, T, SW)                                                                           \
    static void run_##NAME(unsigned W, unsigned d, int push, unsigned n)                           \
    {                                                                                              \
        T *x = malloc((n + 1) * sizeof(T)), *y = malloc((n + 1) * sizeof(T));                      \
        for (unsigned i = 0; i < n * SW; i++) ((float *)x)[i] = rd();                              \
        NAME q = NAME##_create(W, d);                                                              \
        if (push)                                                                                  \
            for (unsigned i = 0; i < n; i++) { NAME##_push(q, x[i]); NAME##_execute(q, &y[i]); }   \
        else                                                                                       \
            NAME##_execute_block(q, x, n, y);                                                      \
        for (unsigned i = 0; i < n * SW; i++) wr(((float *)y)[i]);                                 \
        wr(NAME##_get_energy(q));                                                                  \
        NAME##_destroy(q);                                                                         \
    }
RUN(autocorr_cccf, float complex, 2)
RUN(autocorr_rrrf, float, 1)
int main(void)
{
    char kind[8], drive[8]; unsigned W, d, n;
    if (scanf("%7s %u %u %7s %u", kind, &W, &d, drive, &n) != 5) return 2;
    if (!strcmp(kind, "cccf")) run_autocorr_cccf(W, d, !strcmp(drive, "push"), n);
    else if (!strcmp(kind, "rrrf")) run_autocorr_rrrf(W, d, !strcmp(drive, "push"), n);
    else return 3;
    return 0;
}
"""


def run_case(exe, kind, W, d, drive, x):
    flat = np.ascontiguousarray(x, AM.sample_dtype(kind)).view(np.float32)
    text = "%s %d %d %s %d\n%s\n" % (kind, W, d, drive, len(x), " ".join(str(int(b)) for b in flat.view(np.uint32)))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    y = np.array([int(t) for t in out], np.uint32).view(np.float32)
    assert len(y) == len(flat) + 1
    return y[:-1].copy(), y[-1]


def main():
    tmp = tempfile.mkdtemp(prefix="gen_autocorr_")
    try:
        GF.DRIVER = DRIVER
        exe = GF.build_reference(tmp)
        body = []
        for idx, (kind, W, d, drive) in enumerate(AM.CASES):
            seed = AM.case_seed(idx)
            x = AM.stream_input(kind, AM.NOUT, seed)
            y, energy = run_case(exe, kind, W, d, drive, x)
            body.append('{"kind":"%s","W":%d,"d":%d,"drive":"%s","n":%d,"seed":%d,\n"energy":%s,\n"y":[%s]}'
                        % (kind, W, d, drive, AM.NOUT, seed, GF.num(energy), ",".join(GF.num(v) for v in y)))
            # what tests/test_autocorr_model.py asserts, on what was just recorded
            y64, A, e64 = AM.reference64(kind, W, d, x)
            yy = y.view(np.complex64) if AM.is_complex(kind) else y
            r = AM.report(kind, W, yy, y64, A)
            print("%s W=%d d=%d %-5s: worst %.3g of the bound, %d fail; energy %.9g against %.9g in float64"
                  % (kind, W, d, drive, r["worst"], r["failing"], energy, e64[-1]))
        txt = '{"cases":[\n%s\n]}\n' % ",\n".join(body)
        json.loads(txt)
        out = os.path.join(HERE, "autocorr.json")
        open(out, "w").write(txt)
        print("wrote %s: %d bytes" % (out, len(txt)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
