#!/usr/bin/env python3
"""Record liquid-dsp's qdetector_cccf as a JSON fixture (tests/golden/qdetector.json).

Runs ONLY where the reference sources are present: as gen_detector.py, it
copies them to a temporary directory, builds libliquid.a there with the recipe
of gen_firhilb.py, drives qdetector_cccf_execute sample by sample through the
small C program below and records what it returned.  Nothing compiled and none
of the reference's text is kept: the fixture holds numbers only.

Contents, per case of tests/qdetector_model.py's CASE_NAMES: s_len and nfft as
the reference reports them, and every frame as (index of the sample at which
execute returned the buffer, tau_hat, gamma_hat, dphi_hat, phi_hat), the four
estimates as float32 bit patterns.  The ten linear cases go through
qdetector_cccf_create_linear with the autotest's parameters; the three plain
cases through qdetector_cccf_create.  Inputs are not stored:
qdetector_model.case_inputs regenerates them from integer arithmetic.  A case
whose decisions are not separated by the model's margin
(qdetector_model.check_margin) is refused.

Usage:  python tests/golden/gen_qdetector.py [reference-directory]
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
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "liquid-dsp_amd"))
import gen_firhilb as GF  # noqa: E402  (the reference build recipe)
import qdetector_model as QM  # noqa: E402

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <complex.h>
#include "liquid.h"
/* stdin: "linear n range-bits N" (range-bits 0: the default range), the n
 * symbols or template samples and the N stream samples as uint32 bit patterns;
 * stdout: "LEN s_len nfft", then per frame "DET index tau gamma dphi phi" (bit patterns) */
static float rd(void) { uint32_t b; float f; if (scanf("%u", &b) != 1) exit(2); memcpy(&f, &b, 4); return f; }
static unsigned bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
int main(void)
{
    unsigned linear, n, N;
    if (scanf("%u %u", &linear, &n) != 2) return 2;
    float dmax = rd();
    if (scanf("%u", &N) != 1) return 2;
    float complex *s = malloc(n * sizeof(*s)), *x = malloc(N * sizeof(*x));
    for (unsigned i = 0; i < n; i++) { float a = rd(), b = rd(); s[i] = a + _Complex_I * b; }
    for (unsigned i = 0; i < N; i++) { float a = rd(), b = rd(); x[i] = a + _Complex_I * b; }
    qdetector_cccf q = linear ? qdetector_cccf_create_linear(s, n, LIQUID_FIRFILT_ARKAISER, 2, 7, 0.3f)
                              : qdetector_cccf_create(s, n);
    if (dmax != 0.0f) qdetector_cccf_set_range(q, dmax);
    printf("LEN %u %u\n", qdetector_cccf_get_seq_len(q), qdetector_cccf_get_buf_len(q));
    for (unsigned i = 0; i < N; i++)
        if (qdetector_cccf_execute(q, x[i]))
            printf("DET %u %u %u %u %u\n", i, bits(qdetector_cccf_get_tau(q)), bits(qdetector_cccf_get_gamma(q)),
                   bits(qdetector_cccf_get_dphi(q)), bits(qdetector_cccf_get_phi(q)));
    qdetector_cccf_destroy(q);
    return 0;
}
"""


def words(a):
    return " ".join(str(int(b)) for b in np.ascontiguousarray(a).view(np.uint32).ravel())


def run_case(exe, kind, a, x, dmax):
    text = "%d %d %s %d\n%s\n%s\n" % (kind == "linear", len(a), words(np.array([dmax or 0.0], np.float32)), len(x),
                                      words(np.asarray(a, np.complex64)), words(np.asarray(x, np.complex64)))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    s_len = nfft = None
    dets = []
    for line in out.splitlines():
        if line.startswith("LEN "):
            s_len, nfft = (int(t) for t in line.split()[1:])
        if line.startswith("DET "):
            dets.append([int(t) for t in line.split()[1:]])
    return s_len, nfft, dets


def main():
    tmp = tempfile.mkdtemp(prefix="gen_qdetector_")
    try:
        GF.DRIVER = DRIVER
        exe = GF.build_reference(tmp)
        body = []
        for name in QM.CASE_NAMES:
            kind, a, x, dmax = QM.case_inputs(name)
            T, _, rng, wins, dets64 = QM.case_model(name)   # asserts the margin: refuses the case
            s_len, nfft, dets = run_case(exe, kind, a, x, dmax)
            assert (s_len, nfft) == (T.s_len, T.nfft), (name, s_len, nfft)
            # what tests/test_qdetector_model.py asserts, on what was just recorded
            got = [(d[0], dict(zip(QM.EST, (float(v) for v in np.array(d[1:], np.uint32).view(np.float32)))))
                   for d in dets]
            QM.check_detections("reference " + name, got, dets64)
            body.append('{"name":"%s","s_len":%d,"nfft":%d,"detections":[%s]}'
                        % (name, s_len, nfft, ",".join("[%s]" % ",".join(str(v) for v in d) for d in dets)))
            print(name, s_len, nfft, got)
        txt = '{"cases":[\n%s\n]}\n' % ",\n".join(body)
        json.loads(txt)
        out = os.path.join(HERE, "qdetector.json")
        open(out, "w").write(txt)
        print("wrote %s: %d bytes" % (out, len(txt)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
