// k_autocorr.hip -- windowed delay autocorrelation (autocorr_cccf / autocorr_rrrf,
// src/filter/src/autocorr.c) as one data-parallel kernel per block call.
//
//   p[k]   = x[k] conj(x[k-d])            (rrrf: x[k] x[k-d])
//   rxx[i] = sum_{k=i-W+1..i} p[k],   e2[i] = sum_{k=i-W+1..i} |x[k]|^2
//
// Every output is the sum of the W products of its own window and of nothing
// else: no running sum across outputs and no difference of prefix sums (either
// would leave the rounding error of a loud stretch in every later output;
// DESIGN.md, "autocorr").  The cost per output still does not grow with W:
//
//   A workgroup produces TILE outputs i0 .. i0+TILE.  Its elements u = 0 ..
//   cover the samples k = i0 - WH + u, WH = W - 1 rounded up to a multiple of
//   four (so that runs of four elements start on 16-byte boundaries of x).
//   The elements are cut into segments of W: [0, W), [W, 2W), ...  Inside each
//   segment an inclusive prefix sum P and an inclusive suffix sum S are taken.
//   The window of the output at element u, [u-W+1, u], is either one whole
//   segment (then rxx = P[u]) or the tail of one segment and the head of the
//   next: rxx = S[u-W+1] + P[u].
//
//   The two segmented scans run in three levels with the operator
//   (f1, v1) + (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2), f = "a segment starts
//   here" (ends, for the suffix): a lane scans its run of four elements in
//   registers, a wave scans its 64 runs (one chunk of 256 elements) with
//   shuffles, and wave 0 scans the chunk totals.  P and S go to LDS with the
//   first two levels applied; the chunk-level carry is added when an output is
//   formed, to the elements whose segment began before their chunk did (ended
//   after it, for S) -- which is plain index arithmetic.
//
// Samples before the call come from the history buffer (the last H = W + d
// samples, oldest first), the rest from x, through one index rule (ac_at).
// The delay only moves the second read; it is not limited.  The new history
// is written by the same launch (lq_hist_job_run).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "lq_device.h"
#include "lq_kernels.h"

namespace {

constexpr int NT = 512;
constexpr int TILE = LQK_AUTOCORR_TILE;
constexpr int R = 4;                 // elements per run (one lane)
constexpr int CH = 64 * R;           // elements per chunk (one wave)
constexpr int WMAX = LQK_AUTOCORR_MAXW;
constexpr int MAXCH = (TILE + WMAX + R + CH - 1) / CH;
static_assert(TILE % R == 0 && TILE <= R * NT, "the output phase takes one whole run per lane");
static_assert(MAXCH <= 64, "wave 0 scans the chunk totals in one pass");

typedef float v4f __attribute__((ext_vector_type(4)));

template <bool CX> struct ac_t;
template <> struct ac_t<true> {
    typedef float2 T;
    static constexpr int NS = 2;
};
template <> struct ac_t<false> {
    typedef float T;
    static constexpr int NS = 1;
};

// sample k of the stream: history (k < 0, H samples), x (k < n), zero outside both
template <bool CX>
__device__ __forceinline__ typename ac_t<CX>::T ac_at(const typename ac_t<CX>::T *__restrict__ hist,
                                                      const typename ac_t<CX>::T *__restrict__ x, long long H,
                                                      long long n, long long k)
{
    typedef typename ac_t<CX>::T T;
    if (k >= n || k < -H) return T{};
    return k < 0 ? hist[H + k] : x[k];
}

// the four samples k0 .. k0+3 as floats (re, im interleaved for complex):
// 16-byte loads where the run lies in x and its address allows, else the
// widest aligned pieces (an odd delay puts complex samples 8 bytes off), and
// the index rule per sample at the edges of x
template <bool CX>
__device__ __forceinline__ void ac_load4(const typename ac_t<CX>::T *__restrict__ hist,
                                         const typename ac_t<CX>::T *__restrict__ x, long long H, long long n,
                                         long long k0, float (&s)[R * ac_t<CX>::NS])
{
    typedef typename ac_t<CX>::T T;
    if (k0 >= 0 && k0 + R <= n) {
        const T *p = x + k0;
        const unsigned a = (unsigned)(uintptr_t)p;
        if constexpr (CX) {
            if ((a & 15) == 0) {
                const v4f v0 = *reinterpret_cast<const v4f *>(p), v1 = *reinterpret_cast<const v4f *>(p + 2);
                s[0] = v0.x; s[1] = v0.y; s[2] = v0.z; s[3] = v0.w;
                s[4] = v1.x; s[5] = v1.y; s[6] = v1.z; s[7] = v1.w;
            } else {   /* 8 bytes off: one sample, an aligned pair, one sample */
                const float2 a0 = p[0], a3 = p[3];
                const v4f v = *reinterpret_cast<const v4f *>(p + 1);
                s[0] = a0.x; s[1] = a0.y; s[2] = v.x; s[3] = v.y;
                s[4] = v.z; s[5] = v.w; s[6] = a3.x; s[7] = a3.y;
            }
        } else {
            if ((a & 15) == 0) {
                const v4f v = *reinterpret_cast<const v4f *>(p);
                s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
            } else if ((a & 7) == 0) {
                const float2 v0 = *reinterpret_cast<const float2 *>(p), v1 = *reinterpret_cast<const float2 *>(p + 2);
                s[0] = v0.x; s[1] = v0.y; s[2] = v1.x; s[3] = v1.y;
            } else {
#pragma unroll
                for (int e = 0; e < R; e++) s[e] = p[e];
            }
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < R; e++) {
        const T v = ac_at<CX>(hist, x, H, n, k0 + e);
        if constexpr (CX) {
            s[2 * e] = v.x;
            s[2 * e + 1] = v.y;
        } else {
            s[e] = v;
        }
    }
}

// inclusive scan over the wave's 64 runs with the segmented operator, then
// the carry into each lane (exclusive).  UP: towards higher lanes (prefix),
// else towards lower lanes (suffix).  On return (f, v) is the carry into the
// lane; (tf, tv) the total of the whole wave, valid in every lane.
template <int NC, bool UP>
__device__ __forceinline__ void ac_wave_scan(int lane, int &f, float (&v)[NC], int &tf, float (&tv)[NC])
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int of = UP ? __shfl_up(f, off) : __shfl_down(f, off);
        float ov[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) ov[c] = UP ? __shfl_up(v[c], off) : __shfl_down(v[c], off);
        const bool has = UP ? lane >= off : lane + off < 64;
        if (has) {
            if (!f) {
#pragma unroll
                for (int c = 0; c < NC; c++) v[c] = UP ? ov[c] + v[c] : v[c] + ov[c];
            }
            f |= of;
        }
    }
    const int last = UP ? 63 : 0;
    tf = __shfl(f, last);
#pragma unroll
    for (int c = 0; c < NC; c++) tv[c] = __shfl(v[c], last);
    const int cf = UP ? __shfl_up(f, 1) : __shfl_down(f, 1);
    float cv[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) cv[c] = UP ? __shfl_up(v[c], 1) : __shfl_down(v[c], 1);
    const bool edge = UP ? lane == 0 : lane == 63;
    f = edge ? 0 : cf;
#pragma unroll
    for (int c = 0; c < NC; c++) v[c] = edge ? 0.0f : cv[c];
}

// CX: complex samples; E2: the energy output is wanted.  NC sums per element:
// the product (1 or 2 floats) and |x|^2.
template <bool CX, bool E2>
__global__ __launch_bounds__(NT) void k_autocorr(int W, long long d, long long H, long long n,
                                                 const typename ac_t<CX>::T *__restrict__ hist,
                                                 const typename ac_t<CX>::T *__restrict__ x,
                                                 typename ac_t<CX>::T *__restrict__ rxx, float *__restrict__ e2,
                                                 lqk_hist_job job)
{
    typedef typename ac_t<CX>::T T;
    constexpr int NS = ac_t<CX>::NS;
    constexpr int NC = NS + (E2 ? 1 : 0);
    __shared__ __attribute__((aligned(16))) float sP[NC][TILE];
    __shared__ __attribute__((aligned(16))) float sS[NC][TILE + 2 * R];   // by element: reads run R - 1 past a run
    __shared__ float totP[MAXCH][NC + 1], totS[MAXCH][NC + 1];   // [.][NC]: the flag
    __shared__ float carP[MAXCH][NC], carS[MAXCH][NC];

    lq_hist_job_run<T>(job);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long i0 = (long long)blockIdx.x * TILE;
    const int tn = (int)(n - i0 < TILE ? n - i0 : TILE);   // outputs of this tile
    const int WH = (W - 1 + R - 1) & ~(R - 1);
    const int U = WH + tn;                                 // elements of this tile
    const int nch = (U + CH - 1) / CH;
    const long long kb = i0 - WH;                          // sample of element 0

    for (int q = 0; q * (NT / 64) + wave < nch; q++) {     // wave-uniform
        const int chunk = q * (NT / 64) + wave;
        const int u0 = chunk * CH + lane * R;
        float xs[R * NS], ds[R * NS];
        ac_load4<CX>(hist, x, H, n, kb + u0, xs);
        ac_load4<CX>(hist, x, H, n, kb + u0 - d, ds);
        float v[R][NC];
#pragma unroll
        for (int e = 0; e < R; e++) {
            if constexpr (CX) {
                const float xr = xs[2 * e], xi = xs[2 * e + 1], dr = ds[2 * e], di = ds[2 * e + 1];
                v[e][0] = xr * dr + xi * di;
                v[e][1] = xi * dr - xr * di;
                if constexpr (E2) v[e][2] = xr * xr + xi * xi;
            } else {
                v[e][0] = xs[e] * ds[e];
                if constexpr (E2) v[e][1] = xs[e] * xs[e];
            }
        }
        // position of each element in its segment
        int m[R];
        m[0] = (int)((unsigned)u0 % (unsigned)W);
#pragma unroll
        for (int e = 1; e < R; e++) m[e] = m[e - 1] + 1 == W ? 0 : m[e - 1] + 1;
        // the run: prefix from the left, suffix from the right; open = no
        // segment boundary between the run's edge and the element
        float lp[R][NC], ls[R][NC], run[NC];
        bool op[R], os[R];
        bool open = true;
#pragma unroll
        for (int c = 0; c < NC; c++) run[c] = 0.0f;
#pragma unroll
        for (int e = 0; e < R; e++) {
            const bool st = m[e] == 0;
            open = open && !st;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                run[c] = st ? v[e][c] : run[c] + v[e][c];
                lp[e][c] = run[c];
            }
            op[e] = open;
        }
        int fP = open ? 0 : 1;
        float vP[NC], tvP[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) vP[c] = run[c];
        open = true;
#pragma unroll
        for (int c = 0; c < NC; c++) run[c] = 0.0f;
#pragma unroll
        for (int e = R - 1; e >= 0; e--) {
            const bool en = m[e] == W - 1;
            open = open && !en;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                run[c] = en ? v[e][c] : v[e][c] + run[c];
                ls[e][c] = run[c];
            }
            os[e] = open;
        }
        int fS = open ? 0 : 1;
        float vS[NC], tvS[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) vS[c] = run[c];
        int tfP, tfS;
        ac_wave_scan<NC, true>(lane, fP, vP, tfP, tvP);
        ac_wave_scan<NC, false>(lane, fS, vS, tfS, tvS);
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                totP[chunk][c] = tvP[c];
                totS[chunk][c] = tvS[c];
            }
            totP[chunk][NC] = (float)tfP;
            totS[chunk][NC] = (float)tfS;
        }
        // P is read at elements WH .. WH+tn (index u - WH), S at elements
        // WH-W+1 .. (index u: WH-W+1 < R); runs are aligned for both
        const int jp = u0 - WH;
        if (jp >= 0 && jp < TILE) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                v4f o;
                o.x = op[0] ? vP[c] + lp[0][c] : lp[0][c];
                o.y = op[1] ? vP[c] + lp[1][c] : lp[1][c];
                o.z = op[2] ? vP[c] + lp[2][c] : lp[2][c];
                o.w = op[3] ? vP[c] + lp[3][c] : lp[3][c];
                *reinterpret_cast<v4f *>(&sP[c][jp]) = o;
            }
        }
        if (u0 < TILE + R) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                v4f o;
                o.x = os[0] ? ls[0][c] + vS[c] : ls[0][c];
                o.y = os[1] ? ls[1][c] + vS[c] : ls[1][c];
                o.z = os[2] ? ls[2][c] + vS[c] : ls[2][c];
                o.w = os[3] ? ls[3][c] + vS[c] : ls[3][c];
                *reinterpret_cast<v4f *>(&sS[c][u0]) = o;
            }
        }
    }
    __syncthreads();
    if (wave == 0) {   // the chunk totals: carry into each chunk, from the left (P) and from the right (S)
        int fP = 0, fS = 0, tf;
        float vP[NC], vS[NC], tv[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) vP[c] = vS[c] = 0.0f;
        if (lane < nch) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                vP[c] = totP[lane][c];
                vS[c] = totS[lane][c];
            }
            fP = totP[lane][NC] != 0.0f;
            fS = totS[lane][NC] != 0.0f;
        }
        ac_wave_scan<NC, true>(lane, fP, vP, tf, tv);
        ac_wave_scan<NC, false>(lane, fS, vS, tf, tv);
        if (lane < nch) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                carP[lane][c] = vP[c];
                carS[lane][c] = vS[c];
            }
        }
    }
    __syncthreads();
    // outputs: lane t takes the run j0 .. j0+3; its S values lie sh = WH-W+1
    // elements into two aligned runs of S
    const int sh = WH - W + 1;
    for (int j0 = t * R; j0 < tn; j0 += NT * R) {
        float o[R][NC], pv[NC][R], sv[NC][R];
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const v4f p4 = *reinterpret_cast<const v4f *>(&sP[c][j0]);
            const v4f s0 = *reinterpret_cast<const v4f *>(&sS[c][j0]);
            const v4f s1 = *reinterpret_cast<const v4f *>(&sS[c][j0 + R]);
            const float a[2 * R] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
            pv[c][0] = p4.x; pv[c][1] = p4.y; pv[c][2] = p4.z; pv[c][3] = p4.w;
#pragma unroll
            for (int e = 0; e < R; e++)
                sv[c][e] = sh == 0 ? a[e] : (sh == 1 ? a[e + 1] : (sh == 2 ? a[e + 2] : a[e + 3]));
        }
        int mu = (int)((unsigned)(WH + j0) % (unsigned)W);
#pragma unroll
        for (int e = 0; e < R; e++) {
            const int j = j0 + e, u = WH + j, us = u - W + 1;
            const int cu = u / CH, cs = us / CH;
            const bool whole = mu == W - 1;
            const int ms = whole ? 0 : mu + 1;                     // us % W
            const bool needP = u - mu < cu * CH;                   // the segment began before the chunk
            const bool needS = us - ms + W - 1 > cs * CH + CH - 1; // ... ends after the chunk
#pragma unroll
            for (int c = 0; c < NC; c++) {
                float p = pv[c][e];
                if (needP) p = carP[cu][c] + p;
                float s = sv[c][e];
                if (needS) s = s + carS[cs][c];
                o[e][c] = whole ? p : s + p;
            }
            mu = whole ? 0 : mu + 1;
        }
        T *yp = rxx + i0 + j0;
        const bool full = j0 + R <= tn;
        if (full && ((unsigned)(uintptr_t)yp & 15) == 0) {
            if constexpr (CX) {
                reinterpret_cast<v4f *>(yp)[0] = v4f{o[0][0], o[0][1], o[1][0], o[1][1]};
                reinterpret_cast<v4f *>(yp)[1] = v4f{o[2][0], o[2][1], o[3][0], o[3][1]};
            } else {
                reinterpret_cast<v4f *>(yp)[0] = v4f{o[0][0], o[1][0], o[2][0], o[3][0]};
            }
        } else {
#pragma unroll
            for (int e = 0; e < R; e++) {
                if (j0 + e < tn) {
                    if constexpr (CX) yp[e] = make_float2(o[e][0], o[e][1]);
                    else yp[e] = o[e][0];
                }
            }
        }
        if constexpr (E2) {
            float *ep = e2 + i0 + j0;
            if (full && ((unsigned)(uintptr_t)ep & 15) == 0) {
                reinterpret_cast<v4f *>(ep)[0] = v4f{o[0][NS], o[1][NS], o[2][NS], o[3][NS]};
            } else {
#pragma unroll
                for (int e = 0; e < R; e++)
                    if (j0 + e < tn) ep[e] = o[e][NS];
            }
        }
    }
}

// One output from the history alone (autocorr_execute, get_energy): the window
// is its last W samples, the delayed window starts d samples earlier.  out:
// rxx (1 or 2 floats) then e2, in pinned host memory when flag is given.  A
// fixed tree: the same history gives the same bits.
template <bool CX>
__global__ __launch_bounds__(256) void k_autocorr_single(int W, long long d, long long H,
                                                         const typename ac_t<CX>::T *__restrict__ hist, float *out,
                                                         unsigned *flag, unsigned seq)
{
    constexpr int NC = ac_t<CX>::NS + 1;
    __shared__ float part[NC][256];
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0f;
    const long long w0 = H - W;   // first sample of the window
    for (int i = threadIdx.x; i < W; i += 256) {
        if constexpr (CX) {
            const float2 a = hist[w0 + i], b = hist[w0 + i - d];
            acc[0] += a.x * b.x + a.y * b.y;
            acc[1] += a.y * b.x - a.x * b.y;
            acc[2] += a.x * a.x + a.y * a.y;
        } else {
            const float a = hist[w0 + i], b = hist[w0 + i - d];
            acc[0] += a * b;
            acc[1] += a * a;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; c++) part[c][threadIdx.x] = acc[c];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int c = 0; c < NC; c++) part[c][threadIdx.x] += part[c][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) out[c] = part[c][0];
        lq_signal(flag, seq);
    }
}

template <bool CX, bool E2>
void ac_launch(unsigned int W, unsigned long long d, const void *hist, const void *x, unsigned long long n, void *rxx,
               float *e2, void *hist_new, hipStream_t st)
{
    typedef typename ac_t<CX>::T T;
    const unsigned long long H = (unsigned long long)W + d;   // fits the job's 32-bit length (lqk_autocorr)
    const lqk_hist_job job = {hist, x, n, hist_new, (unsigned int)H};
    hipLaunchKernelGGL((k_autocorr<CX, E2>), dim3((unsigned)((n + TILE - 1) / TILE)), dim3(NT), 0, st, (int)W,
                       (long long)d, (long long)H, (long long)n, (const T *)hist, (const T *)x, (T *)rxx, e2, job);
    LQ_CHECK_LAUNCH();
}

} // namespace

extern "C" void lqk_autocorr(int cx, unsigned int W, unsigned long long d, const void *hist, const void *x,
                             unsigned long long n, void *rxx, float *e2, void *hist_new, void *stream)
{
    if (n == 0) return;
    if (W == 0 || W > LQK_AUTOCORR_MAXW || (unsigned long long)W + d > 0x7fffffffull) {
        fprintf(stderr, "error: lqk_autocorr: window %u / delay %llu outside the kernel's range\n", W, d);
        exit(1);
    }
    hipStream_t st = (hipStream_t)stream;
    if (cx) {
        if (e2) ac_launch<true, true>(W, d, hist, x, n, rxx, e2, hist_new, st);
        else ac_launch<true, false>(W, d, hist, x, n, rxx, e2, hist_new, st);
    } else {
        if (e2) ac_launch<false, true>(W, d, hist, x, n, rxx, e2, hist_new, st);
        else ac_launch<false, false>(W, d, hist, x, n, rxx, e2, hist_new, st);
    }
}

extern "C" void lqk_autocorr_single(int cx, unsigned int W, unsigned long long d, const void *hist, float *out,
                                    unsigned *flag, unsigned seq, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const long long H = (long long)W + (long long)d;
    if (cx)
        hipLaunchKernelGGL(k_autocorr_single<true>, dim3(1), dim3(256), 0, st, (int)W, (long long)d, H,
                           (const float2 *)hist, out, flag, seq);
    else
        hipLaunchKernelGGL(k_autocorr_single<false>, dim3(1), dim3(256), 0, st, (int)W, (long long)d, H,
                           (const float *)hist, out, flag, seq);
    LQ_CHECK_LAUNCH();
}
