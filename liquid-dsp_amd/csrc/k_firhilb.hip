// k_firhilb.hip -- Hilbert transform filter (firhilbf, src/filter/src/firhilb.c)
// as one data-parallel kernel per block of calls.
//
// The object keeps two windows w0, w1 of 2m real samples and 2m quadrature
// taps hq[j] = h[4m-1-2j].  As in k_resamp2.hip each window is the virtual
// sequence E_p = hist_p (2m samples) ++ this block's pushes, so call i is a
// pure function of E_0, E_1 -- one lane per call, no state:
//   decim  : w1 <- x[2i],    yq = dot(w1);  w0 <- x[2i+1], yi = delay(w0)
//   interp : w0 <- Im x[i],  y[2i] = delay(w0);  w1 <- Re x[i], y[2i+1] = dot(w1)
//   r2c    : p = (t0+i)&1:   w_p <- x[i], yi = delay(w_p), yq = dot(w_{1-p})
// with delay(w) the sample pushed m pushes before the newest and
// dot(w) = sum_j hq[j] w[j], w oldest first.
//
// Decim and interp are the same map on bits: call i reads the 8-byte element
// (a, b) = (x[2i], x[2i+1]) or (Re x[i], Im x[i]), a goes to w1 (the dot
// window), b to w0 (the delay window), and the call writes the 8-byte element
// (delay, dot) = (Re y[i], Im y[i]) or (y[2i], y[2i+1]).  One kernel,
// k_firhilb_pair, serves both.
//
// Every dot product is one fmaf chain, j ascending from 0, in both kernels:
// an output does not depend on how the stream is cut into calls or tiles.
#include <hip/hip_runtime.h>

#include "lq_device.h"
#include "lq_kernels.h"

namespace {

constexpr int NT = 256;
constexpr int R = 4;
constexpr int CT = NT * R;   // calls per tile (LQK_FIRHILB_TILE)
static_assert(CT == LQK_FIRHILB_TILE, "tile size is part of the interface (tests cut blocks at it)");

typedef float v2nt __attribute__((ext_vector_type(2)));

// Range-checked view (lq_buf) of `count` elements of `esz` bytes from p: loads
// past the end (or at a negative element, whose 32-bit offset is huge) return
// 0.  The view is made per tile, so offsets stay within a tile plus its halo
// and a launch has no length limit of its own.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t fh_view(const void *p, long long count, int esz)
{
    return lq_buf(p, (int)(count * esz));
}

// n calls of decim / interp.  Tile i0: the elements c = i0 - W + u, u < CT + W,
// are staged once, .x into d[u] (pushes of w1) and .y into e[u] (pushes of
// w0); elements c < 0 are the histories' E_p[c + W].  Call i0 + l then reads
// d[l + 1 + j] (j < W) and e[l + W - m].
__global__ __launch_bounds__(NT) void k_firhilb_pair(int m, long long n, const float *__restrict__ taps,
                                                     const float *__restrict__ hist0,
                                                     const float *__restrict__ hist1, const float2 *__restrict__ x,
                                                     float2 *__restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fh_smem[];
    const int W = 2 * m, t = threadIdx.x;
    float *th = reinterpret_cast<float *>(fh_smem);
    float *d = th + W;
    float *e = d + CT + W;
    const long long i0 = (long long)blockIdx.x * CT;
    const long long c0 = i0 - W;                 // element of slot 0
    const long long cb = c0 > 0 ? c0 : 0;        // first element of the view
    const long long left = n - cb;
    const __amdgpu_buffer_rsrc_t rx = fh_view(x + cb, left < CT + W ? left : CT + W, 8);
    auto ld = [&](int u) -> float2 {
        const unsigned off = (unsigned)(int)((c0 - cb + u) * 8);
        return lq_buf_ld<float2>(rx, off);
    };
    for (int j = t; j < W; j += NT) th[j] = taps[j];
    // all of a lane's loads are issued before its first LDS store (the loop
    // over the W slots past CT waits for its own load, and with it for the
    // R before it, which return in order)
    float2 v[R];
#pragma unroll
    for (int q = 0; q < R; q++) v[q] = ld(t + q * NT);
    for (int u = CT + t; u < CT + W; u += NT) {
        const float2 a = ld(u);
        d[u] = a.x;
        e[u] = a.y;
    }
#pragma unroll
    for (int q = 0; q < R; q++) {
        d[t + q * NT] = v[q].x;
        e[t + q * NT] = v[q].y;
    }
    if (c0 < 0) {   // the first tiles: slots u < -c0 hold history (same lane as the slot's x store)
        for (int u = t; u < -c0; u += NT) {
            d[u] = hist1[i0 + u];
            e[u] = hist0[i0 + u];
        }
    }
    __syncthreads();
    // lane t takes calls t, t + NT, ...: a wave's window reads are consecutive
    // (conflict-free) and every store instruction writes 2 KB contiguous
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0f;
    for (int j = 0; j < W; j++) {
        const float hj = th[j];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = fmaf(hj, d[t + NT * r + 1 + j], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        const long long i = i0 + t + NT * r;
        if (i >= n) break;
        const float yd = e[t + NT * r + W - m];
        __builtin_nontemporal_store(v2nt{yd, acc[r]}, reinterpret_cast<v2nt *>(y + i));
    }
}

// n calls of r2c, the toggle t0 before the first.  The calls of parity b push
// into window t0 ^ b, so S_b = hist_{t0^b} ++ x[b], x[b+2], ... and, with
// c = i >> 1,
//   i even: yi = S_0[W + c - m], yq = sum_j hq[j] S_1[c + j]
//   i odd : yi = S_1[W + c - m], yq = sum_j hq[j] S_0[c + 1 + j].
// Tile i0 (even), c0 = i0 / 2: the pushes cc = c0 - W + v, v < CT/2 + W, of both
// sequences are staged from the CT + 2W consecutive floats x[2 (c0 - W) + u],
// slot u going to s_{u&1}[u >> 1].
__global__ __launch_bounds__(NT) void k_firhilb_r2c(int m, int t0, long long n, const float *__restrict__ taps,
                                                    const float *__restrict__ hist0,
                                                    const float *__restrict__ hist1, const float *__restrict__ x,
                                                    float2 *__restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fh_smem[];
    const int W = 2 * m, t = threadIdx.x;
    float *th = reinterpret_cast<float *>(fh_smem);
    float *s0 = th + W;
    float *s1 = s0 + CT / 2 + W;
    const long long i0 = (long long)blockIdx.x * CT;
    const long long c0 = i0 / 2;
    const long long e0 = 2 * (c0 - W);           // float of slot 0
    const long long eb = e0 > 0 ? e0 : 0;
    const long long left = n - eb;
    const __amdgpu_buffer_rsrc_t rx = fh_view(x + eb, left < CT + 2 * W ? left : CT + 2 * W, 4);
    auto ld = [&](int u) -> float {
        const unsigned off = (unsigned)(int)((e0 - eb + u) * 4);
        return lq_buf_ld<float>(rx, off);
    };
    auto slot = [&](int u) -> float * { return ((u & 1) ? s1 : s0) + (u >> 1); };
    for (int j = t; j < W; j += NT) th[j] = taps[j];
    float v[R];
#pragma unroll
    for (int q = 0; q < R; q++) v[q] = ld(t + q * NT);
    for (int u = CT + t; u < CT + 2 * W; u += NT) *slot(u) = ld(u);
#pragma unroll
    for (int q = 0; q < R; q++) *slot(t + q * NT) = v[q];
    if (e0 < 0) {   // slots u < -e0 hold history (same lane as the slot's x store)
        const float *hp0 = t0 ? hist1 : hist0, *hp1 = t0 ? hist0 : hist1;
        for (int u = t; u < -e0; u += NT) *slot(u) = ((u & 1) ? hp1 : hp0)[c0 + (u >> 1)];
    }
    __syncthreads();
    const int b = t & 1;                          // NT is even: a lane's calls share their parity
    const float *sq = b ? s0 : s1;                // the window this call does not push into
    const float *sd = b ? s1 : s0;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0f;
    for (int j = 0; j < W; j++) {
        const float hj = th[j];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = fmaf(hj, sq[((t + NT * r) >> 1) + b + j], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        const long long i = i0 + t + NT * r;
        if (i >= n) break;
        const float yd = sd[((t + NT * r) >> 1) + W - m];
        __builtin_nontemporal_store(v2nt{yd, acc[r]}, reinterpret_cast<v2nt *>(y + i));
    }
}

// new histories: out_p[k] = E_p[pushes_p + k], k < 2m
__global__ __launch_bounds__(NT) void k_firhilb_hist(int mode, int m, int t0, long long n,
                                                     const float *__restrict__ hist0,
                                                     const float *__restrict__ hist1, const float *__restrict__ x,
                                                     float *__restrict__ out0, float *__restrict__ out1)
{
    const int k = blockIdx.x * NT + threadIdx.x;
    const int W = 2 * m;
    if (k >= 2 * W) return;
    const int p = k >= W;
    const int kk = p ? k - W : k;
    // window p receives x[2c + sp], c < pushes
    int sp;
    long long pushes;
    if (mode == LQK_FH_R2C) {
        sp = (p + t0) & 1;
        pushes = sp ? n / 2 : (n + 1) / 2;
    } else {
        sp = p ? 0 : 1;
        pushes = n;
    }
    const long long idx = pushes + kk;
    (p ? out1 : out0)[kk] = idx < W ? (p ? hist1 : hist0)[idx] : x[2 * (idx - W) + sp];
}

__global__ __launch_bounds__(NT) void k_firhilb_c2r(long long n, const float2 *__restrict__ x, float *__restrict__ y)
{
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i < n) y[i] = x[i].x;
}

} // namespace

extern "C" void lqk_firhilb(int mode, unsigned int m, int t0, const void *taps, const void *hist0, const void *hist1,
                            void *hist0_new, void *hist1_new, const void *x, unsigned long long n, void *y,
                            void *stream)
{
    if (n == 0) return;
    hipStream_t st = (hipStream_t)stream;
    const int W = 2 * (int)m;
    const unsigned grid = (unsigned)((n + CT - 1) / CT);
    if (mode == LQK_FH_R2C) {
        const size_t lds = (size_t)(W + 2 * (CT / 2 + W)) * sizeof(float);
        hipLaunchKernelGGL(k_firhilb_r2c, dim3(grid), dim3(NT), lds, st, (int)m, t0 & 1, (long long)n,
                           (const float *)taps, (const float *)hist0, (const float *)hist1, (const float *)x,
                           (float2 *)y);
    } else {
        const size_t lds = (size_t)(W + 2 * (CT + W)) * sizeof(float);
        hipLaunchKernelGGL(k_firhilb_pair, dim3(grid), dim3(NT), lds, st, (int)m, (long long)n, (const float *)taps,
                           (const float *)hist0, (const float *)hist1, (const float2 *)x, (float2 *)y);
    }
    LQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_firhilb_hist, dim3((unsigned)((2 * W + NT - 1) / NT)), dim3(NT), 0, st, mode, (int)m, t0 & 1,
                       (long long)n, (const float *)hist0, (const float *)hist1, (const float *)x,
                       (float *)hist0_new, (float *)hist1_new);
    LQ_CHECK_LAUNCH();
}

extern "C" void lqk_firhilb_c2r(const void *x, unsigned long long n, void *y, void *stream)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_firhilb_c2r, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream,
                       (long long)n, (const float2 *)x, (float *)y);
    LQ_CHECK_LAUNCH();
}
