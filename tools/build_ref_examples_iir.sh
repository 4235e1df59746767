#!/bin/bash
# Compile liquid-dsp's iirfilt DC-blocker example and its PLL example (whose
# loop filter is iirfilt_rrrf_create_pll), unchanged, against include/liquid.h
# (our drop-in header) and libliquid_mi355x.so.  As
# tools/build_ref_examples_firhilb.sh, with a directory of its own
# (build/ref_examples_iir/, git-ignored): tests/test_gpu_iirfilt.py runs the
# binaries on the GPU.
set -euo pipefail
cd "$(dirname "$0")/.."
REF=${LIQUID_REFERENCE:-/root/reference}
[ -d "$REF/examples" ] || { echo "no reference examples at $REF: skipped"; exit 0; }
OUT=build/ref_examples_iir
mkdir -p "$OUT"
LIBDIR=$PWD/liquid-dsp_amd/lib
for e in iirfilt_crcf_dcblocker pll; do
  gcc -std=gnu99 -O2 -w -I include "$REF/examples/${e}_example.c" -L "$LIBDIR" -lliquid_mi355x \
      -Wl,-rpath,"$LIBDIR" -Wl,-rpath,'$ORIGIN/../../liquid-dsp_amd/lib' -lm -o "$OUT/${e}_example"
done
echo "built $(ls $OUT | wc -l) iirfilt reference examples into $OUT"
