// k_fft_batch.hip -- batched transforms, power-of-two n <= 16384 (a direct
// DFT for the other sizes up to 8192): the transform pass of the channelizers'
// two-pass paths (lq_fft_batch_scaled, lq_pfb.h) and, through lqk_fft_batch /
// lqk_fft_batch_scaled, of fftfilt, spgram, the FFT plan API and the M = 1024
// channelizers' state updates (k_pfb2_fast.hip).
#include "lq_device.h"
#include "lq_fft1024.h"
#include "lq_kernels.h"
#include "lq_pfb.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace {

constexpr int NT = 256;

// y[b] = FFT_dir(x[b]) * s1 * s2 (two separate roundings, as the reference
// synthesizer scales twice: firpfbch2.c:303-307); s == 1 skips the multiply.
template <int N, int NB>
__global__ __launch_bounds__(NT) void k_fft_batch(const float2 *__restrict__ x, float2 *__restrict__ y,
                                                  long long batch, int dir, float s1, float s2, int use_s1,
                                                  int use_s2, const float2 *__restrict__ tw)
{
    __shared__ __attribute__((aligned(16))) float2 a[NB * N];
    __shared__ __attribute__((aligned(16))) float2 b[NB * N];
    const long long b0 = (long long)blockIdx.x * NB;
    for (int e = threadIdx.x; e < NB * N; e += NT) {
        const long long gb = b0 + e / N;
        a[e] = gb < batch ? x[b0 * N + e] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    float2 *res = lds_fft<N, NB, NT>(a, b, tw, dir);
    for (int e = threadIdx.x; e < NB * N; e += NT) {
        const long long gb = b0 + e / N;
        if (gb >= batch) continue;
        float2 v = res[e];
        if (use_s1) v = cscale(v, s1);
        if (use_s2) v = cscale(v, s2);
        y[b0 * N + e] = v;
    }
}

// direct DFT for non power-of-two sizes (small M channelizers)
__global__ void k_dft_batch(int N, const float2 *__restrict__ x, float2 *__restrict__ y, long long batch, int dir,
                            float s1, float s2, int use_s1, int use_s2)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *xb = reinterpret_cast<float2 *>(smem); // staged: x may alias y
    const long long gb = blockIdx.x;
    for (int j = threadIdx.x; j < N; j += blockDim.x) xb[j] = x[gb * N + j];
    __syncthreads();
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        float2 acc = make_float2(0.f, 0.f);
        for (int j = 0; j < N; j++) {
            double s, c;
            sincospi(-2.0 * dir * (double)(((long long)j * k) % N) / (double)N, &s, &c);
            acc = cadd(acc, cmul(xb[j], make_float2((float)c, (float)s)));
        }
        if (use_s1) acc = cscale(acc, s1);
        if (use_s2) acc = cscale(acc, s2);
        y[gb * N + k] = acc;
    }
}

// batched 1024-point transforms, one wave each (lq_fft1024.h); 4 waves per workgroup
template <int DIR>
__global__ __launch_bounds__(256) void k_fft1024_batch(const float2 *__restrict__ x, float2 *__restrict__ y,
                                                        long long batch, float s1, float s2, int use_s1,
                                                        int use_s2, const float2 *__restrict__ tw4096)
{
    __shared__ __attribute__((aligned(16))) float2 buf[4 * 1088];
    __shared__ __attribute__((aligned(16))) float2 tw1[1024];
    __shared__ __attribute__((aligned(16))) float2 tw2[64];
    f1k_tables<DIR>(tw1, tw2, tw4096);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float2 *B = buf + wave * 1088;
    for (long long b = (long long)blockIdx.x * 4 + wave; b < batch; b += (long long)gridDim.x * 4) {
        float2 v[16];
        const float2 *xb = x + b * 1024;
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = xb[lane + 64 * k];
        fft1024_wave<DIR>(v, B, tw1, tw2, lane);
        typedef float v4f __attribute__((ext_vector_type(4)));
        v4f *yb = reinterpret_cast<v4f *>(y + b * 1024);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int o = 2 * (lane + 64 * q);
            v4f val = *reinterpret_cast<const v4f *>(B + o + 4 * (o >> 8));
            if (use_s1) val = val * s1;
            if (use_s2) val = val * s2;
            yb[o >> 1] = val;
        }
        lq_wave_fence();   // B is reused by the next transform of this wave
    }
}

// batched 4096-point transforms, one 256-thread workgroup each (fft4096_r16);
// the register transform needs ~2 waves/SIMD worth of VGPRs
template <int DIR>
__global__ __launch_bounds__(256, 2) void k_fft4096_batch(const float2 *__restrict__ x, float2 *__restrict__ y,
                                                           long long batch, float s1, float s2, int use_s1,
                                                           int use_s2, const float2 *__restrict__ tw4096)
{
    __shared__ __attribute__((aligned(16))) float2 lds[FFT4096_LDS];
    const int t = threadIdx.x;
    const tw16x2 w16 = fft4096_tw(tw4096, t);
    for (long long b = blockIdx.x; b < batch; b += gridDim.x) {
        float2 v[16];
        const float2 *xb = x + b * 4096;
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = xb[t + 256 * k];
        fft4096_r16<DIR>(v, lds, w16, t);
        float2 *yb = y + b * 4096;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            float2 w = v[k];
            if (use_s1) w = cscale(w, s1);
            if (use_s2) w = cscale(w, s2);
            yb[t + 256 * k] = w;
        }
        lq_lds_sync();   // lds is reused by the next transform
    }
}

// batched 8192-point transforms in one pass, one 256-thread workgroup each:
// decimation in time over two 4096-point register transforms, X[j] = E[j] +
// W_8192^j O[j], X[j + 4096] = E[j] - W_8192^j O[j] (E, O: the transforms of
// the even / odd samples).  Thread t loads the pairs (x[2i], x[2i+1]), i = t +
// 256 n, as 16-byte loads, runs fft4096_r16 on each half through the same LDS
// scratch and combines in registers (E[t + 256 k], O[t + 256 k] are its own):
// one read and one write of the data, where the four-step form
// (fft_four_step) makes two of each.  W_8192^(t + 256 k) = W_8192^t W_32^k:
// the first from sincospi in double once per thread, the second constants.
__device__ __constant__ float2 c_w32[16] = {
    {1.000000000f, -0.000000000f},  {0.980785280f, -0.195090322f},  {0.923879533f, -0.382683432f},
    {0.831469612f, -0.555570233f},  {0.707106781f, -0.707106781f},  {0.555570233f, -0.831469612f},
    {0.382683432f, -0.923879533f},  {0.195090322f, -0.980785280f},  {0.000000000f, -1.000000000f},
    {-0.195090322f, -0.980785280f}, {-0.382683432f, -0.923879533f}, {-0.555570233f, -0.831469612f},
    {-0.707106781f, -0.707106781f}, {-0.831469612f, -0.555570233f}, {-0.923879533f, -0.382683432f},
    {-0.980785280f, -0.195090322f}};
template <int DIR, bool A16>
__global__ __launch_bounds__(256, 2) void k_fft8192_batch(const float2 *__restrict__ x, float2 *__restrict__ y,
                                                           long long batch, float s1, float s2, int use_s1,
                                                           int use_s2, const float2 *__restrict__ tw4096)
{
    __shared__ __attribute__((aligned(16))) float2 lds[FFT4096_LDS];
    typedef float v4f __attribute__((ext_vector_type(4)));
    const int t = threadIdx.x;
    const tw16x2 w16 = fft4096_tw(tw4096, t);
    double sn, cs;
    sincospi((double)t / 4096.0, &sn, &cs);
    const float2 wt = make_float2((float)cs, DIR > 0 ? (float)-sn : (float)sn);
    for (long long b = blockIdx.x; b < batch; b += gridDim.x) {
        float2 ve[16], vo[16];
        if constexpr (A16) {
            const v4f *xb = reinterpret_cast<const v4f *>(x + b * 8192);
#pragma unroll
            for (int n = 0; n < 16; n++) {
                const v4f q = xb[t + 256 * n];
                ve[n] = make_float2(q.x, q.y);
                vo[n] = make_float2(q.z, q.w);
            }
        } else {   // x only 8-byte aligned
            const float2 *xb = x + b * 8192;
#pragma unroll
            for (int n = 0; n < 16; n++) {
                ve[n] = xb[2 * (t + 256 * n)];
                vo[n] = xb[2 * (t + 256 * n) + 1];
            }
        }
        fft4096_r16<DIR>(ve, lds, w16, t);
        fft4096_r16<DIR>(vo, lds, w16, t);
        float2 *yb = y + b * 8192;
        float2 wtv = wt;   // through an empty asm: the twiddles are not hoisted out of the loop
        asm volatile("" : "+v"(wtv.x), "+v"(wtv.y));
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const float2 c = c_w32[k];
            const float2 o = cmul(vo[k], cmul(wtv, make_float2(c.x, DIR > 0 ? c.y : -c.y)));
            float2 u0 = cadd(ve[k], o), u1 = csub(ve[k], o);
            if (use_s1) {
                u0 = cscale(u0, s1);
                u1 = cscale(u1, s1);
            }
            if (use_s2) {
                u0 = cscale(u0, s2);
                u1 = cscale(u1, s2);
            }
            yb[t + 256 * k] = u0;
            yb[4096 + t + 256 * k] = u1;
        }
        lq_lds_sync();   // lds is reused by the next transform
    }
}

// batched 16384-point transforms in one pass, one 512-thread workgroup each:
// radix-4 decimation in time over four 4096-point register transforms F_r of
// x[4i + r].  Half h of the workgroup (threads 256 h ..) loads the pairs
// (x[4i + 2h], x[4i + 2h + 1]) and transforms both (F_2h, F_2h+1, each half
// on its own LDS scratch); with G_r = W_16384^(r k) F_r[k], k = t + 256 m,
//   X[k + 4096 q] = P_q + Q_q,  P_q = G_0 + (-j)^q G_1,  Q_q = (-1)^q G_2 + j^q G_3
// (forward; the inverse conjugates), so half 0 forms P, half 1 Q, and each
// hands the other the two it needs (P_2, P_3 / Q_0, Q_1) through the LDS the
// transforms used, eight m at a time (64 KB); half 0 writes X[k], X[k+4096],
// half 1 X[k+8192], X[k+12288].  252 VGPRs: one workgroup per CU.
__device__ __constant__ float2 c_w64[16] = {
    {1.000000000f, -0.000000000f}, {0.995184727f, -0.098017140f}, {0.980785280f, -0.195090322f},
    {0.956940336f, -0.290284677f}, {0.923879533f, -0.382683432f}, {0.881921264f, -0.471396737f},
    {0.831469612f, -0.555570233f}, {0.773010453f, -0.634393284f}, {0.707106781f, -0.707106781f},
    {0.634393284f, -0.773010453f}, {0.555570233f, -0.831469612f}, {0.471396737f, -0.881921264f},
    {0.382683432f, -0.923879533f}, {0.290284677f, -0.956940336f}, {0.195090322f, -0.980785280f},
    {0.098017140f, -0.995184727f}};
constexpr int FFT16K_LDS = 2 * FFT4096_LDS > 8192 ? 2 * FFT4096_LDS : 8192;
template <int DIR, bool A16>
__global__ __launch_bounds__(512, 1) void k_fft16384_batch(const float2 *__restrict__ x, float2 *__restrict__ y,
                                                            long long batch, float s1, float s2, int use_s1,
                                                            int use_s2, const float2 *__restrict__ tw4096)
{
    __shared__ __attribute__((aligned(16))) float2 lds[FFT16K_LDS];
    typedef float v4f __attribute__((ext_vector_type(4)));
    // h is wave-uniform: in a scalar register its branches are scalar
    const int h = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8), t = threadIdx.x & 255;
    const tw16x2 w16 = fft4096_tw(tw4096, t);
    double sn, cs;
    sincospi((double)t / 8192.0, &sn, &cs);
    const float2 wt = make_float2((float)cs, DIR > 0 ? (float)-sn : (float)sn);   // W_16384^t
    // P_q / Q_q of 8 m go to xch[(q' 8 + m') 256 + t], q' = 0, 1 (half 0
    // writes P_2, P_3 at 0, half 1 Q_0, Q_1 at 4096)
    float2 *xch = lds;
    // the next transform's loads are issued right after this one's register
    // transforms, so they are in flight during the exchange and the stores
    // (0.275 -> 0.264 ms per 2^26 points; issued before the transforms, with
    // 64 more VGPRs live through them: 0.292; the same prefetch in the 8192
    // kernel: 0.2105 -> 0.2146, not kept)
    auto load = [&](long long bb, float2 (&a)[16], float2 (&c)[16]) {
        if constexpr (A16) {
            const v4f *xb = reinterpret_cast<const v4f *>(x + bb * 16384 + 2 * h);
#pragma unroll
            for (int n = 0; n < 16; n++) {
                const v4f q = xb[2 * (t + 256 * n)];
                a[n] = make_float2(q.x, q.y);
                c[n] = make_float2(q.z, q.w);
            }
        } else {
            const float2 *xb = x + bb * 16384 + 2 * h;
#pragma unroll
            for (int n = 0; n < 16; n++) {
                a[n] = xb[4 * (t + 256 * n)];
                c[n] = xb[4 * (t + 256 * n) + 1];
            }
        }
    };
    float2 na[16], nb[16];
    if (blockIdx.x < batch) load(blockIdx.x, na, nb);
    for (long long b = blockIdx.x; b < batch; b += gridDim.x) {
        float2 va[16], vb[16];
#pragma unroll
        for (int n = 0; n < 16; n++) {
            va[n] = na[n];
            vb[n] = nb[n];
        }
        float2 *scr = lds + h * FFT4096_LDS;
        fft4096_r16<DIR>(va, scr, w16, t);
        fft4096_r16<DIR>(vb, scr, w16, t);
        if (b + gridDim.x < batch) load(b + gridDim.x, na, nb);
        float2 *yb = y + b * 16384 + 8192 * h;
        // P_q / Q_q of k = t + 256 m: g0, g1 = G_2h, G_2h+1; jg = (-j) g1
        // forward, j g1 inverse.  Half 0: P_0 = g0 + g1, P_1 = g0 + jg,
        // P_2 = g0 - g1, P_3 = g0 - jg; half 1: Q_0 = g0 + g1, Q_1 = -g0 - jg,
        // Q_2 = g0 - g1, Q_3 = -g0 + jg.  sel 0: the two this half sends, 1:
        // the two it keeps (recomputed after the exchange rather than held:
        // 32 VGPRs)
        // wt through an empty asm: the twiddles stay inside the batch loop
        // (hoisted, 48 of them took 96 VGPRs and spilled)
        float2 wtv = wt;
        asm volatile("" : "+v"(wtv.x), "+v"(wtv.y));
        auto pq = [&](int m, int sel, float2 &a, float2 &c) {
            const float2 cw = c_w64[m];
            const float2 w1 = cmul(wtv, make_float2(cw.x, DIR > 0 ? cw.y : -cw.y));   // W^k
            float2 g0, g1;
            if (h == 0) {
                g0 = va[m];
                g1 = cmul(vb[m], w1);
            } else {
                const float2 w2 = cmul(w1, w1);
                g0 = cmul(va[m], w2);
                g1 = cmul(vb[m], cmul(w2, w1));
            }
            const float2 jg = DIR > 0 ? make_float2(g1.y, -g1.x) : make_float2(-g1.y, g1.x);
            const bool first = (h == 0) == (sel == 1);   // P_0, P_1 / Q_0, Q_1
            if (first) {
                a = cadd(g0, g1);
                c = h == 0 ? cadd(g0, jg) : make_float2(-g0.x - jg.x, -g0.y - jg.y);
            } else {
                a = csub(g0, g1);
                c = h == 0 ? csub(g0, jg) : make_float2(-g0.x + jg.x, -g0.y + jg.y);
            }
        };
#pragma unroll
        for (int r = 0; r < 2; r++) {
            lq_lds_sync();   // the transforms' (or the previous round's) LDS reads are done
#pragma unroll
            for (int mm = 0; mm < 8; mm++) {
                float2 a, c;
                pq(8 * r + mm, 0, a, c);
                xch[4096 * h + mm * 256 + t] = a;
                xch[4096 * h + 2048 + mm * 256 + t] = c;
            }
            lq_lds_sync();
#pragma unroll
            for (int mm = 0; mm < 8; mm++) {
                const int k = t + 256 * (8 * r + mm);
                float2 a, c;
                pq(8 * r + mm, 1, a, c);
                float2 u0 = cadd(a, xch[4096 * (1 - h) + mm * 256 + t]);
                float2 u1 = cadd(c, xch[4096 * (1 - h) + 2048 + mm * 256 + t]);
                if (use_s1) {
                    u0 = cscale(u0, s1);
                    u1 = cscale(u1, s1);
                }
                if (use_s2) {
                    u0 = cscale(u0, s2);
                    u1 = cscale(u1, s2);
                }
                yb[k] = u0;
                yb[4096 + k] = u1;
            }
        }
        lq_lds_sync();   // lds is reused by the next transform
    }
}

// batched N = 256 R point transforms (R = 1, 2, 8: 256, 512, 2048 points),
// 16 R threads per transform, 16 / R transforms per 256-thread workgroup,
// register passes (fft_r16x16xR); persistent over the batch
template <int R, int DIR>
__global__ __launch_bounds__(256, 2) void k_fftr16_batch(const float2 *__restrict__ x, float2 *__restrict__ y,
                                                          long long batch, float s1, float s2, int use_s1,
                                                          int use_s2, const float2 *__restrict__ tw4096)
{
    constexpr int T = 16 * R, N = 16 * T, G = 256 / T, P = FFTR16_LDS<R>();
    __shared__ __attribute__((aligned(16))) float2 lds[G * P];
    const int g = threadIdx.x / T, t = threadIdx.x % T;
    const tw16x2 w16 = fftr16_tw<R>(tw4096, t);
    for (long long b0 = (long long)blockIdx.x * G; b0 < batch; b0 += (long long)gridDim.x * G) {
        const long long b = b0 + g;
        const bool in = b < batch;
        float2 v[16];
        const float2 *xb = x + (in ? b : 0) * N;
#pragma unroll
        for (int n = 0; n < 16; n++) v[n] = in ? xb[t + T * n] : make_float2(0.f, 0.f);
        fft_r16x16xR<R, DIR>(v, lds + g * P, w16, t);
        if (in) {
            float2 *yb = y + b * N;
#pragma unroll
            for (int s = 0; s < 16 / R; s++)
#pragma unroll
                for (int q = 0; q < R; q++) {
                    float2 w = v[s * R + q];
                    if (use_s1) w = cscale(w, s1);
                    if (use_s2) w = cscale(w, s2);
                    yb[t + T * s + 256 * q] = w;
                }
        }
    }
}

// batched 32 / 64 / 128-point transforms (fft_small16xR): R lanes per
// transform, 256 / R transforms per workgroup, persistent over the batch
template <int R, int DIR>
__global__ __launch_bounds__(256) void k_fftsmall_batch(const float2 *__restrict__ x, float2 *__restrict__ y,
                                                         long long batch, float s1, float s2, int use_s1,
                                                         int use_s2, const float2 *__restrict__ tw4096)
{
    constexpr int N = 16 * R, G = 256 / R, P = FFTS_LDS<R>();
    __shared__ __attribute__((aligned(16))) float2 lds[G * P];
    const int g = threadIdx.x / R, t = threadIdx.x % R;
    const int e = t * (4096 / N);
    const float2 a1 = tw4096[e & 4095], a4 = tw4096[(4 * e) & 4095];
    for (long long b0 = (long long)blockIdx.x * G; b0 < batch; b0 += (long long)gridDim.x * G) {
        const long long b = b0 + g;
        const bool in = b < batch;
        float2 v[16];
        const float2 *xb = x + (in ? b : 0) * N;
#pragma unroll
        for (int n = 0; n < 16; n++) v[n] = in ? xb[t + R * n] : make_float2(0.f, 0.f);
        fft_small16xR<R, DIR>(v, lds + g * P, a1, a4, t);
        if (in) {
            float2 *yb = y + b * N;
#pragma unroll
            for (int u = 0; u < 16 / R; u++)
#pragma unroll
                for (int q = 0; q < R; q++) {
                    float2 w = v[u * R + q];
                    if (use_s1) w = cscale(w, s1);
                    if (use_s2) w = cscale(w, s2);
                    yb[t * (16 / R) + u + 16 * q] = w;
                }
        }
        lq_lds_sync();   // lds is reused by the next batch of transforms
    }
}

template <int R>
void launch_fftsmall(const void *x, void *y, long long batch, int dir, float s1, float s2, int u1, int u2,
                     hipStream_t st)
{
    constexpr int G = 256 / R;
    const long long gb = (batch + G - 1) / G;
    const unsigned grid = lqrt_grid((unsigned long long)gb, 4096);
    lq_switch<+1, -1>(dir > 0 ? +1 : -1, [&](auto d) {
        hipLaunchKernelGGL((k_fftsmall_batch<R, d>), dim3(grid), dim3(256), 0, st, (const float2 *)x, (float2 *)y,
                           batch, s1, s2, u1, u2, (const float2 *)lqrt_twiddles());
    });
    LQ_CHECK_LAUNCH();
}

template <int R>
void launch_fftr16(const void *x, void *y, long long batch, int dir, float s1, float s2, int u1, int u2,
                   hipStream_t st)
{
    constexpr int G = 16 / R;
    const long long g = (batch + G - 1) / G;
    const unsigned grid = lqrt_grid((unsigned long long)g, 2048);
    lq_switch<+1, -1>(dir > 0 ? +1 : -1, [&](auto d) {
        hipLaunchKernelGGL((k_fftr16_batch<R, d>), dim3(grid), dim3(256), 0, st, (const float2 *)x, (float2 *)y,
                           batch, s1, s2, u1, u2, (const float2 *)lqrt_twiddles());
    });
    LQ_CHECK_LAUNCH();
}

template <int N>
void launch_fft_batch(const void *x, void *y, long long batch, int dir, float s1, float s2, int u1, int u2,
                      hipStream_t st)
{
    constexpr int NB = N >= 1024 ? 1 : 1024 / N;
    const long long grid = (batch + NB - 1) / NB;
    hipLaunchKernelGGL((k_fft_batch<N, NB>), dim3((unsigned)grid), dim3(NT), 0, st, (const float2 *)x,
                       (float2 *)y, batch, dir, s1, s2, u1, u2, (const float2 *)lqrt_twiddles());
    LQ_CHECK_LAUNCH();
}

void launch_fft1024(const void *x, void *y, long long batch, int dir, float s1, float s2, int u1, int u2,
                    hipStream_t st)
{
    const long long g = (batch + 3) / 4;
    const unsigned grid = lqrt_grid((unsigned long long)g, 4096);
    lq_switch<+1, -1>(dir > 0 ? +1 : -1, [&](auto d) {
        hipLaunchKernelGGL(k_fft1024_batch<d>, dim3(grid), dim3(256), 0, st, (const float2 *)x, (float2 *)y, batch,
                           s1, s2, u1, u2, (const float2 *)lqrt_twiddles());
    });
    LQ_CHECK_LAUNCH();
}

void launch_fft4096(const void *x, void *y, long long batch, int dir, float s1, float s2, int u1, int u2,
                    hipStream_t st)
{
    const unsigned grid = lqrt_grid((unsigned long long)batch, 2048);
    lq_switch<+1, -1>(dir > 0 ? +1 : -1, [&](auto d) {
        hipLaunchKernelGGL(k_fft4096_batch<d>, dim3(grid), dim3(256), 0, st, (const float2 *)x, (float2 *)y, batch,
                           s1, s2, u1, u2, (const float2 *)lqrt_twiddles());
    });
    LQ_CHECK_LAUNCH();
}

// 8192 and 16384: 16-byte loads where x allows them
void launch_fft8192(const void *x, void *y, long long batch, int dir, float s1, float s2, int u1, int u2,
                    bool a16, hipStream_t st)
{
    const unsigned grid = lqrt_grid((unsigned long long)batch, 2048);
    lq_switch<+1, -1>(dir > 0 ? +1 : -1, [&](auto d) {
        lq_switch<1, 0>(a16, [&](auto a) {
            hipLaunchKernelGGL((k_fft8192_batch<d, a != 0>), dim3(grid), dim3(256), 0, st, (const float2 *)x,
                               (float2 *)y, batch, s1, s2, u1, u2, (const float2 *)lqrt_twiddles());
        });
    });
    LQ_CHECK_LAUNCH();
}

void launch_fft16384(const void *x, void *y, long long batch, int dir, float s1, float s2, int u1, int u2,
                     bool a16, hipStream_t st)
{
    const unsigned grid = lqrt_grid((unsigned long long)batch, 1024);
    lq_switch<+1, -1>(dir > 0 ? +1 : -1, [&](auto d) {
        lq_switch<1, 0>(a16, [&](auto a) {
            hipLaunchKernelGGL((k_fft16384_batch<d, a != 0>), dim3(grid), dim3(512), 0, st, (const float2 *)x,
                               (float2 *)y, batch, s1, s2, u1, u2, (const float2 *)lqrt_twiddles());
        });
    });
    LQ_CHECK_LAUNCH();
}

// the one-pass kernels' dispatch: the family lq_fft_batch_scaled launches for
// n points read from a pointer that is or is not 16-byte aligned
int fft_batch_family(unsigned n)
{
    if (n == 0) return LQK_FFT_REFUSED;
    if (n & (n - 1)) return n <= 8192 ? LQK_FFT_DFT : LQK_FFT_REFUSED;   // one workgroup per transform, n points of LDS
    if (n == 1) return LQK_FFT_DFT;
    if (n <= 16) return LQK_FFT_BATCH;
    if (n <= 128) return LQK_FFT_SMALL;
    switch (n) {
    case 256:
    case 512:
    case 2048: return LQK_FFT_R16;
    case 1024: return LQK_FFT_1024;
    case 4096: return LQK_FFT_4096;
    case 8192: return LQK_FFT_8192;
    case 16384: return LQK_FFT_16384;
    default: return LQK_FFT_REFUSED;
    }
}

} // namespace

extern "C" lqk_fft_route_t lqk_fft_route(unsigned int n, int aligned16)
{
    lqk_fft_route_t r = {LQK_FFT_REFUSED, 0, 0, 0, 0, 0};
    const bool pow2 = n != 0 && (n & (n - 1)) == 0;
    if (n == 0 || (pow2 && n > (1u << 24)) || (!pow2 && n > (1u << 23))) return r;
    if ((pow2 && n <= 16384) || (!pow2 && n <= 16)) {   // one pass
        r.family = fft_batch_family(n);
        r.a16 = (r.family == LQK_FFT_8192 || r.family == LQK_FFT_16384) && aligned16;
        return r;
    }
    // two passes over N1 x N2 points: the transform itself, or Bluestein's M >= 2n - 1
    unsigned long long M = n;
    if (!pow2) {
        M = 1;
        while (M < 2ull * n - 1) M <<= 1;
        r.M = M;
        if (M <= 4096) {   // chirp multiply, lq_fft_batch_scaled's M-point kernels, multiply, back
            r.family = LQK_FFT_BLUESTEIN;
            return r;
        }
    }
    int lg = 0;
    while ((1ull << lg) < M) lg++;
    // the larger factor on the column pass (N2 <= N1 <= 4096 for M <= 2^24)
    r.N1 = 1u << ((lg + 1) / 2);
    r.N2 = (unsigned)(M / r.N1);
    r.family = pow2 ? LQK_FFT_FOUR_STEP : LQK_FFT_BLUESTEIN_FUSED;
    r.rows_s = r.N2 < 256;   // the row pass in k_bs_rows_s (registers, 16 x R points)
    return r;
}

void lq_fft_batch_scaled(unsigned n, int dir, const void *x, void *y, long long batch, float s1, float s2, int u1,
                         int u2, hipStream_t st)
{
    if (batch <= 0) return;
    const bool a16 = ((uintptr_t)x & 15) == 0;
    switch (fft_batch_family(n)) {
    case LQK_FFT_BATCH:
        lq_switch<2, 4, 8, 16>(n, [&](auto N) { launch_fft_batch<N>(x, y, batch, dir, s1, s2, u1, u2, st); });
        return;
    case LQK_FFT_SMALL:
        lq_switch<32, 64, 128>(n, [&](auto N) { launch_fftsmall<N / 16>(x, y, batch, dir, s1, s2, u1, u2, st); });
        return;
    case LQK_FFT_R16:
        lq_switch<256, 512, 2048>(n, [&](auto N) { launch_fftr16<N / 256>(x, y, batch, dir, s1, s2, u1, u2, st); });
        return;
    case LQK_FFT_1024: launch_fft1024(x, y, batch, dir, s1, s2, u1, u2, st); return;
    case LQK_FFT_4096: launch_fft4096(x, y, batch, dir, s1, s2, u1, u2, st); return;
    case LQK_FFT_8192: launch_fft8192(x, y, batch, dir, s1, s2, u1, u2, a16, st); return;
    case LQK_FFT_16384: launch_fft16384(x, y, batch, dir, s1, s2, u1, u2, a16, st); return;
    case LQK_FFT_DFT:
        hipLaunchKernelGGL(k_dft_batch, dim3((unsigned)batch), dim3(n == 1 ? 64 : 256),
                           n == 1 ? 16 : (size_t)n * sizeof(float2), st, (int)n, (const float2 *)x, (float2 *)y, batch,
                           dir, s1, s2, u1, u2);
        LQ_CHECK_LAUNCH();
        return;
    default:
        fprintf(stderr, "error: liquid-mi355x: non power-of-two transform size %u not supported\n", n);
        exit(1);
    }
}

extern "C" void lqk_fft_batch(unsigned int n, int dir, const void *x, void *y, unsigned long long batch,
                              void *stream)
{
    lq_fft_batch_scaled(n, dir, x, y, (long long)batch, 1.f, 1.f, 0, 0, (hipStream_t)stream);
}

extern "C" void lqk_fft_batch_scaled(unsigned int n, int dir, const void *x, void *y, unsigned long long batch,
                                     float s1, float s2, void *stream)
{
    lq_fft_batch_scaled(n, dir, x, y, (long long)batch, s1, s2, 1, 1, (hipStream_t)stream);
}

