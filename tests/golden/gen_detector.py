#!/usr/bin/env python3
"""Record liquid-dsp's detector_cccf as a JSON fixture (tests/golden/detector.json).

Runs ONLY where the reference sources are present: as gen_autocorr.py, it
copies them to a temporary directory, builds libliquid.a there with the recipe
of gen_firhilb.py (that library holds the framing objects), drives
detector_cccf_correlate sample by sample through the small C program below and
records what it returned.  Nothing compiled and none of the reference's text is
kept: the fixture holds numbers only.

Contents, per case of tests/detector_model.py's CASES: the geometry (sequence
length, threshold, dphi_max, carrier offset, stream length, preamble
positions), the seed, the number of correlators the reference printed, and its
detections as (index, tau_hat, dphi_hat, gamma_hat), the three estimates
written with the shortest decimal text that reads back to the same float32.
Inputs are not stored: detector_model.case_stream regenerates them from integer
arithmetic.  A case whose decisions are not separated by the model's margin
(detector_model.check_margin) is refused.

Usage:  python tests/golden/gen_detector.py [reference-directory]
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
import detector_model as DM  # noqa: E402

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <complex.h>
#include "liquid.h"
/* stdin: "n threshold-bits dphi_max-bits N", the sequence and the stream as
 * uint32 bit patterns; stdout: the object's print, then per detection
 * "DET index tau dphi gamma" (bit patterns) */
static float rd(void) { uint32_t b; float f; if (scanf("%u", &b) != 1) exit(2); memcpy(&f, &b, 4); return f; }
static unsigned bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
int main(void)
{
    unsigned n, N;
    if (scanf("%u", &n) != 1) return 2;
    float thr = rd(), dphi_max = rd();
    if (scanf("%u", &N) != 1) return 2;
    float complex *s = malloc(n * sizeof(*s)), *x = malloc(N * sizeof(*x));
    for (unsigned i = 0; i < n; i++) { float a = rd(), b = rd(); s[i] = a + _Complex_I * b; }
    for (unsigned i = 0; i < N; i++) { float a = rd(), b = rd(); x[i] = a + _Complex_I * b; }
    detector_cccf q = detector_cccf_create(s, n, thr, dphi_max);
    detector_cccf_print(q);
    for (unsigned i = 0; i < N; i++) {
        float tau = 0, dphi = 0, gamma = 0;
        if (detector_cccf_correlate(q, x[i], &tau, &dphi, &gamma))
            printf("DET %u %u %u %u\n", i, bits(tau), bits(dphi), bits(gamma));
    }
    detector_cccf_destroy(q);
    return 0;
}
"""


def words(a):
    return " ".join(str(int(b)) for b in np.ascontiguousarray(a).view(np.uint32).ravel())


def run_case(exe, s, thr, dphi_max, x):
    text = "%d %s %d\n%s\n%s\n" % (len(s), words(np.array([thr, dphi_max], np.float32)), len(x),
                                   words(np.asarray(s, np.complex64)), words(np.asarray(x, np.complex64)))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    m = int(re.search(r"num\. correlators\s*:\s*(\d+)", out).group(1))
    dets = []
    for line in out.splitlines():
        if line.startswith("DET "):
            i, a, b, c = (int(t) for t in line.split()[1:])
            est = np.array([a, b, c], np.uint32).view(np.float32)
            dets.append((i, est[0], est[1], est[2]))
    return m, dets


def main():
    tmp = tempfile.mkdtemp(prefix="gen_detector_")
    try:
        GF.DRIVER = DRIVER
        exe = GF.build_reference(tmp)
        body = []
        for case in DM.CASES:
            name, n, thr, dphi_max, carrier, N, pos = case
            bank, s, x, r64, E64, bound, dets64 = DM.case_model(case)   # asserts the margin: refuses the case
            m, dets = run_case(exe, s, thr, dphi_max, x)
            assert m == bank.m, (name, m, bank.m)
            # what tests/test_detector_model.py asserts, on what was just recorded
            DM.check_detections("reference " + name, dets, bank, r64, E64, bound, thr)
            body.append('{"name":"%s","n":%d,"threshold":%r,"dphi_max":%r,"carrier":%r,"N":%d,"positions":[%s],'
                        '"seed":%d,"m":%d,\n"detections":[%s]}'
                        % (name, n, thr, dphi_max, carrier, N, ",".join(str(p) for p in pos), DM.SEEDS[name], m,
                           ",".join("[%d,%s,%s,%s]" % (i, GF.num(a), GF.num(b), GF.num(c)) for i, a, b, c in dets)))
        txt = '{"cases":[\n%s\n]}\n' % ",\n".join(body)
        json.loads(txt)
        out = os.path.join(HERE, "detector.json")
        open(out, "w").write(txt)
        print("wrote %s: %d bytes" % (out, len(txt)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
