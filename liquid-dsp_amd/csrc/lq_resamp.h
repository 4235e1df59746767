// lq_resamp.h -- what the arbitrary-rate resampler kernel files (k_resamp.hip,
// k_resamp4.hip) share: the reference's float32 timing recurrence and its
// replay, the host layout of the pair table, and the un-paired LDS read.
// Private to csrc/; the exported C ABI is lq_kernels.h.
#pragma once

#include "lq_device.h"

namespace {

// LDS of a CU: the launchers size their resident workgroups per CU against it
constexpr size_t RS_CU_LDS = 160 * 1024;

// run-time tap count L = 2m -> f(std::integral_constant<int, L>): the even L
// up to 32 that k_resamp3, k_resamp and k_resamp4 are instantiated for
template <class F>
bool rs_taps(unsigned L, F &&f)
{
    return lq_switch<2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32>((int)L, f);
}

// ---- timing (resamp.c:245-363).  Every piece is IEEE float32 with
// contraction off: the replay is bit-exact or it is wrong.
struct rs_state {
    float tau, mu;
    int b, st; // st: 1 INTERP, 0 BOUNDARY
};

// the reference's update_timing_state (resamp.c:352-363)
__device__ __forceinline__ void rs_advance(rs_state &s, float del, float fnpfb)
{
#pragma clang fp contract(off)
    s.tau = s.tau + del;
    const float bf = s.tau * fnpfb;
    const float fb = __builtin_floorf(bf);
    s.b = (int)fb;
    s.mu = bf - fb;
}

// the state a power-of-two bank count derives from tau (host/resamp_plan.c
// rs_from_tau): BOUNDARY iff tau < 0, b = floor(tau npfb), mu its fraction
__device__ __forceinline__ void rs_derive(float tau, float fnpfb, rs_state &s)
{
#pragma clang fp contract(off)
    const float bf = tau * fnpfb;
    const float fb = __builtin_floorf(bf);
    s.tau = tau;
    s.mu = bf - fb;
    s.st = tau >= 0.0f ? 1 : 0;
    s.b = s.st ? (int)fb : 0;
}

// One input of the recurrence (resamp.c:253-307): emit(s) once per output, s
// the state it is computed from (INTERP: banks s.b, s.b + 1; BOUNDARY: bank
// npfb - 1 on the window one input older, and bank 0).  END: also end the
// input (tau -= 1): the state before the next one; a caller that replays a
// single input has no use for it.
template <bool END = true, class F>
__device__ __forceinline__ void rs_input(rs_state &s, float del, float fnpfb, int npfb, F &&emit)
{
    while ((unsigned)s.b < (unsigned)npfb) {   // unsigned, as resamp.c:254 (int b vs unsigned npfb)
        if (s.st && s.b == npfb - 1) {         // last filter: finish with the next input
            if (END) {
                s.st = 0;
                s.b = npfb;
            }
            break;
        }
        emit(s);
        rs_advance(s, del, fnpfb);
        s.st = 1;
    }
    if (END) {
        s.tau -= 1.0f;
        s.b = (int)((unsigned)s.b - (unsigned)npfb);
    }
}

// Power-of-two banks replay tau alone (host/resamp_plan.c rs_step_p2): an
// input adds del until tau reaches z = 1 - 1/npfb, one output each, then
// subtracts 1.  Returns tau `skip` inputs on from x and counts their outputs
// into the caller's own counter k (k_resamp3: its 64-bit one, directly).
template <class K>
__device__ __forceinline__ float rs_skip_p2(float x, int skip, float del, float z, K &k)
{
#pragma clang fp contract(off)
    for (int i = 0; i < skip; i++) {
        while (x < z) {
            x = x + del;
            k++;
        }
        x = x - 1.0f;
    }
    return x;
}

// ---- the pair table.  Host layout (host/resamp.c): taps2[b * LP + p],
// b <= npfb, p <= L, the two banks an output blends, (h_b[p], h_{b+1}[p]) on
// one window; row npfb is the BOUNDARY pair.  The kernels keep it in LDS as
// (h, h' - h), so a tap is c = fma(mu, h' - h, h): rs_pair(taps2, b * rs_lp<L>()
// + p) (the index formed in here commutes an address add in k_resamp4).
template <int L>
constexpr int rs_lp() { return (L + 3) & ~1; }   // pair stride of a row
__device__ __forceinline__ float2 rs_pair(const float2 *taps2, int i)
{
    const float2 v = taps2[i];
    return make_float2(v.x, v.y - v.x);
}

// ---- one LDS read of 4 or 8 bytes as a relaxed workgroup-scope atomic: the
// compiler issues it as its own ds_read_b64 / _b32 (2 LDS cycles per wave)
// and never pairs two into a ds_read2_b64 (8 cycles, CDNA4 LDS table).  (A
// volatile read, k_resamp4's earlier form, compiles to the same instructions
// in every kernel of both files.)
template <typename T>
__device__ __forceinline__ T lds_rd(const T *p)
{
    if constexpr (sizeof(T) == 8) {
        const unsigned long long u = __hip_atomic_load(reinterpret_cast<unsigned long long *>(const_cast<T *>(p)),
                                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return __builtin_bit_cast(T, u);
    } else {
        const unsigned u = __hip_atomic_load(reinterpret_cast<unsigned *>(const_cast<T *>(p)), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_WORKGROUP);
        return __builtin_bit_cast(T, u);
    }
}

} // namespace
