// lq_pfb.h -- what the two channelizer banks (k_firpfbch2.hip, k_firpfbch.hip)
// share, and the batched transform of k_fft_batch.hip they both finish their
// two-pass paths with.  Private to csrc/; the exported C ABI is lq_kernels.h.
#pragma once

#include "lq_device.h"

// y[b] = FFT_dir(x[b]) (* s1 if u1) (* s2 if u2), power-of-two n <= 16384 (else a
// direct DFT, n <= 8192); k_fft_batch.hip.  The banks pass their own u1 / u2
// (lqk_fft_batch_scaled always multiplies twice).
void lq_fft_batch_scaled(unsigned n, int dir, const void *x, void *y, long long batch, float s1, float s2, int u1,
                         int u2, hipStream_t st);

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// sample t of the stream [history (HL samples) | x]
__device__ __forceinline__ float2 ext_load(const float2 *__restrict__ hist, int HL, const float2 *__restrict__ x,
                                           long long t)
{
    return t < 0 ? hist[HL + t] : x[t];
}

// M = 4096 fused kernels: a block buffer is four 1024-point quarters
constexpr int A4_QS = 1092;            // quarter stride: 1088-float2 transform scratch; 1092 * 8 = 32 mod 128 B
constexpr int A4_BSTR = 4 * A4_QS;     //   puts the four quarters of a dot-phase write on distinct bank groups

// ---------------------------------------------------------------- run kernels
// One lane per (column, run of RUN consecutive blocks): the column's taps stay
// in registers and a P-deep shift register of the column's history slides
// along the run, so each input is loaded ~(RUN + P - 1)/RUN times instead of
// P times and each tap once per run (the per-element kernels re-load both for
// every output).
constexpr int RUN = 64;
constexpr int RPF = 4;   // column samples kept in flight by the run kernels

} // namespace
