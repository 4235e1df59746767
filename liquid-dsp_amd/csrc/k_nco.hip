// k_nco.hip -- nco_crcf block mixer: y[i] = x[i] (cos th_i +- j sin th_i) with
// the oscillator's float32 phase replayed bit for bit (src/nco/src/nco.c:134-138,
// 355-361: th += d_theta in float32, then one wrap by 2 pi computed in double).
//
// The phase recurrence is serial but does not depend on the data: the host
// tabulates it (host/nco_plan.c) as a checkpoint every LQK_NCO_CK positions,
// and a workgroup replays its tile of LQK_NCO_TILE samples from them:
//
//   replay   lane t takes the RUN = 8 consecutive samples t*8 .. t*8+7 of the
//            tile: it loads the checkpoint at or before its first position and
//            steps forward (< LQK_NCO_CK steps), then walks its run, loading a
//            checkpoint again where the walk meets one and th_pre where it
//            crosses the seam of a periodic plan -- no phase is more than
//            LQK_NCO_CK - 1 dependent steps from a table value.  It leaves per
//            sample the phase (VCO) or the reference's table index (NCO,
//            nco.c:372: three separately rounded float32 operations) in LDS.
//   mix      the lanes change roles: lane t takes sample pairs (j*256 + t)*2,
//            one 16-byte load and store each, so a wave's accesses are
//            contiguous; it reads the pair's phases or indices from LDS, forms
//            the rotator (NCO: two reads of the 256-entry sine table in LDS;
//            VCO: sincosf) and multiplies: two rounded products and a rounded
//            sum per component, the reference's arithmetic.
//
// LDS: the replay writes are 8 words per lane; one pad word per 8 makes the
// lane stride 9 words (conflict-free ds_write_b32), and the mix reads are then
// at most 2-way conflicted.  Pointers that are not 16-byte aligned take the
// same kernel with 8-byte accesses.
#include <cstdio>
#include <cstdlib>

#include "lq_device.h"

// The phase step, the table index and the mixing products are the reference's
// separately rounded float32 operations.  hipcc contracts a * b + c into an FMA
// by default -- also through __fmul_rn / __fadd_rn, which this toolchain defines
// as the plain operators -- and a fused index moves at bin edges (an output
// error of 2.5e-2 |x|): no contraction in this file.
#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr unsigned TILE = LQK_NCO_TILE, CK = LQK_NCO_CK;
constexpr int RUN = TILE / NT;
static_assert(RUN == 8 && TILE % CK == 0, "runs of 8 samples (the LDS padding), whole checkpoint intervals per tile");

constexpr double NCO_PI = 3.14159265358979323846;

__device__ __forceinline__ float nco_step(float th, float d)
{
    th = th + d;
    const double t = (double)th;
    if (t > NCO_PI) th = (float)(t - 2.0 * NCO_PI);
    else if (t < -NCO_PI) th = (float)(t + 2.0 * NCO_PI);
    return th;
}

__device__ __forceinline__ unsigned nco_index(float th)
{
    return ((unsigned)(th * 40.743665f + 512.0f + 0.5f)) & 0xffu;
}

__device__ __forceinline__ unsigned pad(unsigned j) { return j + (j >> 3); }

template <bool VCO>
__device__ __forceinline__ float2 nco_rot(float2 v, unsigned w, const float *stab, int down)
{
    float s, c;
    if (VCO) {
        sincosf(__uint_as_float(w), &s, &c);
    } else {
        s = stab[w];
        c = stab[(w + 64u) & 0xffu];
    }
    if (down) s = -s;
    return make_float2(v.x * c - v.y * s, v.x * s + v.y * c);
}

template <bool VCO, bool V16>
__global__ __launch_bounds__(NT) void k_nco_mix(const float *__restrict__ tab, unsigned p0, unsigned pre, unsigned P,
                                                float d, float th_pre, const float *__restrict__ sintab, const float2 *x,
                                                float2 *y, unsigned n, int down)
{
    __shared__ unsigned ph[TILE + TILE / 8];
    __shared__ float stab[256];
    const unsigned t = threadIdx.x, base = blockIdx.x * TILE;
    if (!VCO) stab[t] = sintab[t];

    const unsigned i0 = base + t * RUN;
    if (i0 < n) {
        const unsigned seam = pre + P;
        unsigned p = p0 + i0;
        if (P && p >= seam) p = pre + (p - pre) % P;
        float th = tab[p / CK];
        for (unsigned s = p % CK; s; s--) th = nco_step(th, d);
#pragma unroll
        for (int k = 0; k < RUN; k++) {
            ph[pad(t * RUN + k)] = VCO ? __float_as_uint(th) : nco_index(th);
            if (i0 + k + 1 >= n) break;
            p++;
            if (P && p == seam) {
                p = pre;
                th = th_pre;
            } else if (p % CK == 0) {
                th = tab[p / CK];
            } else {
                th = nco_step(th, d);
            }
        }
    }
    __syncthreads();

    if (V16) {
        float4 v[RUN / 2];
#pragma unroll
        for (int j = 0; j < RUN / 2; j++) {
            const unsigned gi = base + 2 * (j * NT + t);
            if (gi + 1 < n) v[j] = *reinterpret_cast<const float4 *>(x + gi);
            else if (gi < n) v[j] = make_float4(x[gi].x, x[gi].y, 0.0f, 0.0f);
        }
#pragma unroll
        for (int j = 0; j < RUN / 2; j++) {
            const unsigned li = 2 * (j * NT + t), gi = base + li;
            if (gi >= n) continue;
            const float2 a = nco_rot<VCO>(make_float2(v[j].x, v[j].y), ph[pad(li)], stab, down);
            if (gi + 1 < n) {
                const float2 b = nco_rot<VCO>(make_float2(v[j].z, v[j].w), ph[pad(li + 1)], stab, down);
                *reinterpret_cast<float4 *>(y + gi) = make_float4(a.x, a.y, b.x, b.y);
            } else {
                y[gi] = a;
            }
        }
    } else {
        float2 v[RUN];
#pragma unroll
        for (int j = 0; j < RUN; j++) {
            const unsigned gi = base + j * NT + t;
            if (gi < n) v[j] = x[gi];
        }
#pragma unroll
        for (int j = 0; j < RUN; j++) {
            const unsigned li = j * NT + t, gi = base + li;
            if (gi < n) y[gi] = nco_rot<VCO>(v[j], ph[pad(li)], stab, down);
        }
    }
}

template <bool VCO, bool V16>
void nco_launch(const lqk_nco_plan *pl, const float *sintab, const void *x, void *y, unsigned n, int down, hipStream_t st)
{
    hipLaunchKernelGGL((k_nco_mix<VCO, V16>), dim3((n + TILE - 1) / TILE), dim3(NT), 0, st, pl->tab, (unsigned)pl->p0,
                       (unsigned)pl->pre, (unsigned)pl->P, pl->d_theta, pl->th_pre, sintab, (const float2 *)x,
                       (float2 *)y, n, down);
    LQ_CHECK_LAUNCH();
}

} // namespace

extern "C" void lqk_nco_mix(int vco, int down, const lqk_nco_plan *pl, const float *sintab, const void *x, void *y,
                            unsigned long long n, void *stream)
{
    if (n == 0) return;
    // positions are 32-bit in the kernel: p0 + n and pre + P stay below 2^31
    if (n > LQK_NCO_MAXN || pl->p0 >= (1ull << 30) || pl->pre + pl->P >= (1ull << 30) ||
        (pl->P && pl->p0 >= pl->pre + pl->P)) {
        fprintf(stderr, "error: lqk_nco_mix: call of %llu samples at plan position %llu outside the kernel's range\n", n,
                pl->p0);
        exit(1);
    }
    hipStream_t st = (hipStream_t)stream;
    const bool v16 = (((uintptr_t)x | (uintptr_t)y) & 15u) == 0;
    if (vco) {
        if (v16) nco_launch<true, true>(pl, sintab, x, y, (unsigned)n, down, st);
        else nco_launch<true, false>(pl, sintab, x, y, (unsigned)n, down, st);
    } else {
        if (v16) nco_launch<false, true>(pl, sintab, x, y, (unsigned)n, down, st);
        else nco_launch<false, false>(pl, sintab, x, y, (unsigned)n, down, st);
    }
}
