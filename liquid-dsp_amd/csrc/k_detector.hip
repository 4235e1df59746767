// k_detector.hip -- the correlator bank of detector_cccf
// (src/framing/src/detector_cccf.c) as one launch per block call.
//
//   c_k[t] = sum_{i<len} p_k[i] w_t[i],  E[t] = sum_{i<len} |w_t[i]|^2,
//   r_k[t] = |c_k[t]| / sqrt(len E[t])        w_t = s[t-len+1 .. t], k < m
//
// Every output is a float32 sum of the len terms of its own window, taken in
// the order i = 0 .. len-1 (one fused multiply-add per real product): no
// running sum across outputs and no difference of prefix sums, so an output
// depends on the samples of its window alone and not on how the stream is cut
// into calls or tiles.
//
// A workgroup produces TILE consecutive samples' rows.  It stages the TILE +
// len - 1 samples they read once in LDS -- history (the len samples before the
// call) and x through one index rule (dt_at), pairs of samples by 16-byte loads
// where they lie in x.  A lane owns R = 4 consecutive outputs and keeps their
// m complex sums and energy sums in registers; walking the taps it holds a
// sliding window of 2R staged samples, so each sample it reads from LDS feeds
// 4 m R multiply-adds, issued as packed pairs (re, im).  Samples are stored in runs of R with one slot of
// padding after each run: the lanes of a wave read one sample each at a stride
// of R + 1 slots, which spreads them over all banks.  Every lane needs the
// same template values at the same time: they are read tap-major through the
// scalar cache (constant address space, wave-uniform addresses) and never
// touch LDS, so a bank of 2048 x 16 (256 KB) costs no LDS either.
//
// The decision pass needs only the rows near a threshold crossing
// (host/detector.c): the kernel marks the samples whose largest r_k exceeds the
// threshold, their two neighbours in the tile, and the first and last sample of
// the call, and appends (t, E, row) of each marked sample to a device list
// through one atomic counter.  A tile's first and last sample have a neighbour
// that another workgroup holds: their records go to fixed slots of a second
// array, with one word of flags per tile, and the host fetches the few it needs
// (a row above the threshold on the other side of the seam).  Rows go to drxy
// only when asked.  The new history is written by the same launch
// (lq_hist_job_run).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "lq_device.h"
#include "lq_kernels.h"

namespace {

constexpr int NT = 512;
constexpr int R = 4;                       // consecutive outputs per lane
constexpr int TILE = LQK_DETECTOR_TILE;
constexpr int MAXLEN = LQK_DETECTOR_MAXLEN;
constexpr int HEAD = LQK_DETECTOR_LIST_HEAD;
static_assert(NT * R == TILE, "one run of R outputs per lane");
static_assert(MAXLEN % R == 0, "the padded length of the longest sequence is MAXLEN");
constexpr int SF_MAX = TILE + MAXLEN + R;                 // staged positions (read: < TILE + padded len + R)
constexpr int LDS_X = (SF_MAX / R + 1) * (R + 1);

typedef float v4f __attribute__((ext_vector_type(4)));
typedef const v2f __attribute__((address_space(4))) *dt_cptr;

// LDS slot of staged position s: runs of R, one slot of padding after each
__device__ __forceinline__ int dt_slot(int s) { return (s >> 2) * (R + 1) + (s & (R - 1)); }

// sample k of the stream: history (k < 0, len samples), x (k < n), zero outside both
__device__ __forceinline__ float2 dt_at(const float2 *__restrict__ hist, const float2 *__restrict__ x, long long len,
                                        long long n, long long k)
{
    if (k >= n || k < -len) return make_float2(0.0f, 0.0f);
    return k < 0 ? hist[len + k] : x[k];
}

// acc += p * v for complex p (a wave-uniform template value, in scalar registers)
// and v, acc = (re, im) in a register pair: two packed multiply-adds whose operand
// selects do the swaps and the sign,
//   (re, im) += p.x * (v.x, v.y);   (re, im) += (-p.y, p.y) * (v.y, v.x)
// the same two roundings per component, in the same order, as the chain
// fma(p.x, v.x, re), fma(-p.y, v.y, re) / fma(p.x, v.y, im), fma(p.y, v.x, im).
__device__ __forceinline__ void dt_cmac(v2f &acc, v2f p, v2f v)
{
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "s"(p), "v"(v));
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "+v"(acc) : "s"(p), "v"(v));
}

// a^2 + b^2 with both squares rounded before the sum, as the energy's two halves are
__device__ __forceinline__ float dt_sumsq(float a, float b)
{
#pragma clang fp contract(off)
    const float aa = a * a, bb = b * b;
    return aa + bb;
}

// taps i .. i+NI of correlators K0 .. K0+MC of a bank of M against the window
// lo ++ hi (R samples each): output e reads sample ii + e of it at tap i + ii.
// WE: the energy too, the squares of the real and of the imaginary parts in
// the two halves of Ep
template <int M, int K0, int MC, int NI, bool WE>
__device__ __forceinline__ void dt_taps(const float2 *pg, const v2f (&lo)[R], const v2f (&hi)[R], v2f (&acc)[MC][R],
                                        v2f (&Ep)[R])
{
    // Wave-uniform addresses in the constant address space: scalar loads.  They go through the
    // scalar cache, which is not coherent with stores: the templates must not be written while
    // a launch that reads them may be in flight (host/detector.c writes them once, before the
    // first launch, and waits for the copy).
    const dt_cptr pp = reinterpret_cast<dt_cptr>((uintptr_t)pg);
#pragma unroll
    for (int ii = 0; ii < NI; ii++) {
#pragma unroll
        for (int k = 0; k < MC; k++) {
            const v2f p = pp[ii * M + K0 + k];
#pragma unroll
            for (int e = 0; e < R; e++) dt_cmac(acc[k][e], p, ii + e < R ? lo[(ii + e) % R] : hi[(ii + e) % R]);
        }
        if constexpr (WE) {
#pragma unroll
            for (int e = 0; e < R; e++) {
                const v2f v = ii + e < R ? lo[(ii + e) % R] : hi[(ii + e) % R];
                Ep[e] = __builtin_elementwise_fma(v, v, Ep[e]);
            }
        }
    }
}

__device__ __forceinline__ void dt_load_run(const float2 *run, v2f (&w)[R])
{
#pragma unroll
    for (int e = 0; e < R; e++) w[e] = v2f{run[e].x, run[e].y};
}

// One walk over the taps for correlators K0 .. K0+MC: their sums in registers,
// then r_k.  The first walk (WE) also forms the energies, which later walks use.
// The window is two runs of R samples that swap roles from one tap block to
// the next, so nothing is moved between them.
template <int M, int K0, int MC, bool WE>
__device__ __forceinline__ void dt_walk(const float2 *__restrict__ pt, const float2 *run, int len, float (&rk)[M][R],
                                        float (&E)[R])
{
    const int nbf = len / R, rem = len - nbf * R;   // whole tap blocks, taps of the last one
    v2f acc[MC][R], Ep[R], wa[R], wb[R];
#pragma unroll
    for (int k = 0; k < MC; k++)
#pragma unroll
        for (int e = 0; e < R; e++) acc[k][e] = v2f{0.0f, 0.0f};
#pragma unroll
    for (int e = 0; e < R; e++) Ep[e] = v2f{0.0f, 0.0f};
    dt_load_run(run, wa);
    int ib = 0;
    for (; ib + 2 <= nbf; ib += 2) {
        dt_load_run(run + (R + 1), wb);
        dt_taps<M, K0, MC, R, WE>(pt + (size_t)ib * R * M, wa, wb, acc, Ep);
        run += 2 * (R + 1);
        dt_load_run(run, wa);
        dt_taps<M, K0, MC, R, WE>(pt + (size_t)(ib + 1) * R * M, wb, wa, acc, Ep);
    }
    if (ib < nbf) {   // an odd number of whole blocks: one more, and the roles stay swapped
        dt_load_run(run + (R + 1), wb);
        dt_taps<M, K0, MC, R, WE>(pt + (size_t)ib * R * M, wa, wb, acc, Ep);
        run += R + 1;
#pragma unroll
        for (int e = 0; e < R; e++) wa[e] = wb[e];
    }
    if (rem) {   // the last taps: wave-uniform
        dt_load_run(run + (R + 1), wb);
        const float2 *pp = pt + (size_t)nbf * R * M;
        if (rem == 1) dt_taps<M, K0, MC, 1, WE>(pp, wa, wb, acc, Ep);
        else if (rem == 2) dt_taps<M, K0, MC, 2, WE>(pp, wa, wb, acc, Ep);
        else dt_taps<M, K0, MC, 3, WE>(pp, wa, wb, acc, Ep);
    }
#pragma unroll
    for (int e = 0; e < R; e++) {
        if constexpr (WE) E[e] = Ep[e].x + Ep[e].y;
        const float den = sqrtf((float)len * E[e]);
#pragma unroll
        for (int k = 0; k < MC; k++) {
            // the squares summed as the energy sums them: a one-tap bank of unit templates gives exactly 1
            const float mag = sqrtf(dt_sumsq(acc[k][e].x, acc[k][e].y));
            rk[K0 + k][e] = E[e] > 0.0f ? mag / den : 0.0f;
        }
    }
}

// The walks of a bank of M: NW = ceil(M / DT_MC_MAX) of them, as even as M allows
#ifndef DT_MC_MAX
#define DT_MC_MAX 12
#endif
template <int M, int K0>
__device__ __forceinline__ void dt_walks(const float2 *__restrict__ pt, const float2 *run, int len, float (&rk)[M][R],
                                         float (&E)[R])
{
    constexpr int left = M - K0, nw = (left + DT_MC_MAX - 1) / DT_MC_MAX, mc = (left + nw - 1) / nw;
    dt_walk<M, K0, mc, K0 == 0>(pt, run, len, rk, E);
    if constexpr (K0 + mc < M) dt_walks<M, K0 + mc>(pt, run, len, rk, E);
}

// M: correlators; ROWS: the rows are wanted in drxy
template <int M, bool ROWS>
__global__ __launch_bounds__(NT) void k_detector(int len, float thr, const float2 *__restrict__ pt,
                                                 const float2 *__restrict__ hist, const float2 *__restrict__ x,
                                                 long long n, float *__restrict__ drxy, unsigned *__restrict__ list,
                                                 unsigned cap, unsigned *__restrict__ edge, lqk_hist_job job)
{
    __shared__ float2 sx[LDS_X];
    __shared__ float smax[TILE + 2];   // [1 + j]: the largest r_k of output j

    lq_hist_job_run<float2>(job);

    const int t = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * TILE;
    const int tn = (int)(n - i0 < TILE ? n - i0 : TILE);   // outputs of this tile
    const int S = tn + len - 1;                            // staged samples some output reads
    const int SF = TILE + ((len + R - 1) / R) * R + R;      // staged positions the lanes load
    const long long k0 = i0 - (len - 1);                   // stream sample at position 0

    // stage: pairs (k, k + 1) that start on a 16-byte boundary of x
    {
        const long long a = (long long)(((uintptr_t)x >> 3) & 1);
        const long long ks = k0 - ((k0 + a) & 1);
        for (int p = t;; p += NT) {
            const long long k = ks + 2 * (long long)p;
            const int s = (int)(k - k0);
            if (s >= SF) break;
            float2 v0, v1;
            if (k >= 0 && k + 2 <= n) {
                const v4f v = *reinterpret_cast<const v4f *>(x + k);
                v0 = make_float2(v.x, v.y);
                v1 = make_float2(v.z, v.w);
            } else {
                v0 = dt_at(hist, x, len, n, k);
                v1 = dt_at(hist, x, len, n, k + 1);
            }
            const float2 z = make_float2(0.0f, 0.0f);
            if (s >= 0) sx[dt_slot(s)] = s < S ? v0 : z;
            if (s + 1 < SF) sx[dt_slot(s + 1)] = s + 1 < S ? v1 : z;
        }
    }
    if (t == 0) smax[0] = smax[tn + 1] = 0.0f;
    __syncthreads();

    const int j0 = t * R;
    float rk[M][R], E[R];
#pragma unroll
    for (int e = 0; e < R; e++) E[e] = 0.0f;
    if (j0 < tn) {
        // a lane's 8 accumulators per correlator limit how many it takes along at once: a
        // wider bank takes several walks over the taps (dt_walks)
        const float2 *run = sx + t * (R + 1);   // the run of R samples at position j0
        dt_walks<M, 0>(pt, run, len, rk, E);
#pragma unroll
        for (int e = 0; e < R; e++) {
            float rmax = 0.0f;
#pragma unroll
            for (int k = 0; k < M; k++) rmax = fmaxf(rmax, rk[k][e]);
            if (j0 + e < tn) smax[1 + j0 + e] = rmax;
        }
        if constexpr (ROWS) {
            float *o = drxy + (size_t)(i0 + j0) * M;
            float flat[R * M];
#pragma unroll
            for (int e = 0; e < R; e++)
#pragma unroll
                for (int k = 0; k < M; k++) flat[e * M + k] = rk[k][e];
            if (j0 + R <= tn && ((uintptr_t)o & 15) == 0) {
#pragma unroll
                for (int c = 0; c < R * M / 4; c++)
                    reinterpret_cast<v4f *>(o)[c] = v4f{flat[4 * c], flat[4 * c + 1], flat[4 * c + 2], flat[4 * c + 3]};
            } else {
#pragma unroll
                for (int c = 0; c < R * M; c++)
                    if (j0 + c / M < tn) o[c] = flat[c];
            }
        }
    }
    __syncthreads();
    // Marked: a row maximum above the threshold, a neighbour of one in this tile, the first and
    // the last sample of the call.  The tile's own first and last sample also go to fixed slots
    // of edge (their other neighbour belongs to another workgroup), with one word of flags per
    // tile for the host: bit 0 / 2: the first / last row's maximum is above the threshold; bit
    // 1 / 3: that sample is in the list already.
    const bool head = blockIdx.x == 0, tail = blockIdx.x == gridDim.x - 1;
    if (t == 0) {
        const bool fh = smax[1] > thr, lh = smax[tn] > thr;
        const bool fl = fh || smax[2] > thr || head || (tail && tn == 1);
        const bool ll = lh || smax[tn - 1] > thr || tail || (head && tn == 1);
        list[HEAD + blockIdx.x] = (fh ? 1u : 0u) | (fl ? 2u : 0u) | (lh ? 4u : 0u) | (ll ? 8u : 0u);
    }
    if (j0 < tn) {
#pragma unroll
        for (int e = 0; e < R; e++) {
            const int j = j0 + e;
            if (j >= tn) continue;
            if (j == 0 || j == tn - 1) {
                for (int side = (j == 0 ? 0 : 1); side <= (j == tn - 1 ? 1 : 0); side++) {
                    unsigned *rec = edge + ((size_t)blockIdx.x * 2 + side) * (2 + M);
                    rec[0] = (unsigned)(i0 + j);
                    rec[1] = __float_as_uint(E[e]);
#pragma unroll
                    for (int k = 0; k < M; k++) rec[2 + k] = __float_as_uint(rk[k][e]);
                }
            }
            const bool mark = (head && j == 0) || (tail && j == tn - 1) || smax[j] > thr || smax[j + 1] > thr ||
                              smax[j + 2] > thr;
            if (!mark) continue;
            const unsigned slot = atomicAdd(list, 1u);
            if (slot >= cap) continue;
            unsigned *rec = list + HEAD + gridDim.x + (size_t)slot * (2 + M);
            rec[0] = (unsigned)(i0 + j);
            rec[1] = __float_as_uint(E[e]);
#pragma unroll
            for (int k = 0; k < M; k++) rec[2 + k] = __float_as_uint(rk[k][e]);
        }
    }
}

template <int M, bool ROWS>
void dt_launch(unsigned int len, float thr, const void *pt, const void *hist, const void *x, unsigned long long n,
               float *drxy, unsigned int *list, unsigned int cap, unsigned int *edge, void *hist_new, hipStream_t st)
{
    const lqk_hist_job job = {hist, x, n, hist_new, len};
    hipLaunchKernelGGL((k_detector<M, ROWS>), dim3((unsigned)((n + TILE - 1) / TILE)), dim3(NT), 0, st, (int)len, thr,
                       (const float2 *)pt, (const float2 *)hist, (const float2 *)x, (long long)n, drxy, list, cap, edge,
                       job);
    LQ_CHECK_LAUNCH();
}

} // namespace

extern "C" void lqk_detector(unsigned int len, unsigned int m, float thr, const void *pt, const void *hist,
                             const void *x, unsigned long long n, float *drxy, unsigned int *list, unsigned int cap,
                             unsigned int *edge, void *hist_new, void *stream)
{
    if (n == 0) return;
    hipStream_t st = (hipStream_t)stream;
    bool ok = len >= 1 && len <= LQK_DETECTOR_MAXLEN && n < (1ull << 31);
    if (ok) {
        LQ_CHECK(hipMemsetAsync(list, 0, HEAD * sizeof(unsigned int), st));
        ok = lq_switch<2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>((int)m, [&](auto mm) {
            constexpr int M = decltype(mm)::value;
            if (drxy) dt_launch<M, true>(len, thr, pt, hist, x, n, drxy, list, cap, edge, hist_new, st);
            else dt_launch<M, false>(len, thr, pt, hist, x, n, drxy, list, cap, edge, hist_new, st);
        });
    }
    if (!ok) {
        fprintf(stderr, "error: lqk_detector: length %u / %u correlators / %llu samples outside the kernel's range\n",
                len, m, n);
        exit(1);
    }
}
