// k_qdetector.hip -- qdetector_cccf's device work (host/qdetector.c).
//
// The stream a call sees is ext = carry (clen samples held by the object) ++
// x; seek window w of a launch is ext[pos + w nfft/2 .. + nfft).  Its record:
//   E = e0 + e1, each half's |x|^2 summed in a fixed order of its own;
//   for offset in [-range, range], lag i: r = IFFT(X[k] conj(S[(k - offset) mod nfft]))[i];
//   (m2, offset, lag) = the first maximum of |r|^2 in (offset, lag) order;
//   peak = sqrt(m2) g, g = 1 / (nfft sqrt(E) sqrt(s_len / nfft) sqrt(s2_sum)); (0, 0, 0) where E == 0.
//
// Fused kernel (nfft = 1024): one wave owns a window.  It loads x[lane + 64 k],
// forms both half energies, runs fft1024_wave and keeps conj(X) in 16 register
// pairs in that same layout.  S sits once per workgroup in LDS; per offset the
// lane multiplies its 16 values by S at the shifted index, transforms forward
// again -- FFT(conj(X) S') = conj(IFFT(X conj(S'))), the same magnitudes, so one
// direction's twiddle tables serve both -- and reads the natural-order result
// back from the wave's LDS buffer at lag = lane + 64 k, keeping (max, key).
// No row leaves the CU; a window's samples are read from HBM once.
//
// Fused kernel (nfft = 512): 32 lanes own a window, see k_qd_fused512.
//
// Composed path (every other nfft, and any nfft on request): gather + energies, lqk_fft_any forward,
// the shifted products for a batch of offsets, lqk_fft_any backward in place,
// and a reduction that folds the batch into the window's running (max, key).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "lq_device.h"
#include "lq_fft1024.h"
#include "lq_kernels.h"

namespace {

constexpr int NT = 256;

struct qd_best {
    float m2;
    unsigned int key;   // (offset + range) * nfft + lag
};

// the reference scans offsets, then lags, and replaces on a strictly larger value
__device__ __forceinline__ bool qd_better(float m2, unsigned key, float bm2, unsigned bkey)
{
    return m2 > bm2 || (m2 == bm2 && key < bkey);
}

__device__ __forceinline__ float2 qd_ext(const float2 *__restrict__ c, long long clen, const float2 *__restrict__ x,
                                         long long p)
{
    return p < clen ? c[p] : x[p - clen];
}

__device__ __forceinline__ void qd_write_record(unsigned int *rec, float m2, unsigned key, float E, int nfft,
                                                int range, unsigned s_len, float s2_sum)
{
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    v4u out = {0u, 0u, 0u, __float_as_uint(E)};
    if (E > 0.0f) {
        const float g0 = sqrtf(E) * sqrtf((float)s_len / (float)nfft);
        const float g = 1.0f / ((float)nfft * g0 * sqrtf(s2_sum));
        out.x = __float_as_uint(sqrtf(m2) * g);
        out.y = key % (unsigned)nfft;
        out.z = (unsigned)((int)(key / (unsigned)nfft) - range);
    }
    *reinterpret_cast<v4u *>(rec) = out;
}

// block-wide fixed-order sum of one value per thread (NT threads)
__device__ __forceinline__ float qd_block_sum(float v, float *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ void qd_block_best(float &m2, unsigned &key, float *shm, unsigned *shk)
{
    shm[threadIdx.x] = m2;
    shk[threadIdx.x] = key;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && qd_better(shm[threadIdx.x + s], shk[threadIdx.x + s], shm[threadIdx.x], shk[threadIdx.x])) {
            shm[threadIdx.x] = shm[threadIdx.x + s];
            shk[threadIdx.x] = shk[threadIdx.x + s];
        }
        __syncthreads();
    }
    m2 = shm[0];
    key = shk[0];
    __syncthreads();
}

// ---------------------------------------------------------------- composed path

// W[w][i] = ext[pos + w h + i], E[w] = e0 + e1; one workgroup per window
__global__ __launch_bounds__(NT) void k_qd_gather(const float2 *__restrict__ c, long long clen,
                                                   const float2 *__restrict__ x, long long pos, int nfft,
                                                   float2 *__restrict__ W, float *__restrict__ E)
{
    __shared__ float sh[NT];
    const long long w = blockIdx.x;
    const int h = nfft >> 1;
    const long long p0 = pos + w * h;
    float e[2];
    for (int half = 0; half < 2; half++) {
        float acc = 0.0f;
        for (int i = threadIdx.x; i < h; i += NT) {
            const float2 v = qd_ext(c, clen, x, p0 + half * h + i);
            W[w * nfft + half * h + i] = v;
            acc += v.x * v.x + v.y * v.y;
        }
        e[half] = qd_block_sum(acc, sh);
    }
    if (threadIdx.x == 0) E[w] = e[0] + e[1];
}

// P[(w nb + ob)][i] = X[w][i] conj(S[(i - (off0 + ob)) mod nfft])
__global__ __launch_bounds__(NT) void k_qd_mul(const float2 *__restrict__ X, const float2 *__restrict__ S, int nfft,
                                                int off0, int nb, float2 *__restrict__ P)
{
    const long long w = blockIdx.x;
    const int ob = blockIdx.y;
    const int off = off0 + ob;
    const float2 *xr = X + w * nfft;
    float2 *pr = P + (w * nb + ob) * (long long)nfft;
    for (int i = threadIdx.x; i < nfft; i += NT) {
        const float2 s = S[(i + nfft - off) & (nfft - 1)];
        pr[i] = cmul(xr[i], make_float2(s.x, -s.y));
    }
}

// fold the nb rows of window w (offsets boff - range ..) into run[w]; the last batch writes the record
__global__ __launch_bounds__(NT) void k_qd_reduce(const float2 *__restrict__ P, int nfft, int nb, int boff, int first,
                                                   int last, qd_best *__restrict__ run, const float *__restrict__ E,
                                                   int range, unsigned s_len, float s2_sum,
                                                   unsigned int *__restrict__ rec)
{
    __shared__ float shm[NT];
    __shared__ unsigned shk[NT];
    const long long w = blockIdx.x;
    const float2 *pr = P + w * nb * (long long)nfft;
    float m2 = 0.0f;
    unsigned key = (unsigned)range * (unsigned)nfft;   // the reference's initial (0, index 0, offset 0)
    const long long tot = (long long)nb * nfft;
    for (long long e = threadIdx.x; e < tot; e += NT) {
        const float2 v = pr[e];
        const float a = v.x * v.x + v.y * v.y;
        if (a > m2) {
            m2 = a;
            key = (unsigned)boff * (unsigned)nfft + (unsigned)e;
        }
    }
    qd_block_best(m2, key, shm, shk);
    if (threadIdx.x == 0) {
        if (!first) {
            const qd_best b = run[w];
            if (!qd_better(m2, key, b.m2, b.key)) {
                m2 = b.m2;
                key = b.key;
            }
        }
        if (last) qd_write_record(rec + 4 * w, m2, key, E[w], nfft, range, s_len, s2_sum);
        else run[w] = qd_best{m2, key};
    }
}

// ---------------------------------------------------------------- fused seek, nfft = 1024

constexpr int FW = 4;   // waves (windows) per workgroup

__global__ __launch_bounds__(64 * FW) void k_qd_fused1024(const float2 *__restrict__ c, long long clen,
                                                           const float2 *__restrict__ x, long long pos,
                                                           long long nw, const float2 *__restrict__ S, int range,
                                                           unsigned s_len, float s2_sum,
                                                           const float2 *__restrict__ tw4096,
                                                           unsigned int *__restrict__ rec)
{
    __shared__ __attribute__((aligned(16))) float2 buf[FW * 1088];
    __shared__ __attribute__((aligned(16))) float2 tw1[1024];
    __shared__ __attribute__((aligned(16))) float2 tw2[64];
    __shared__ __attribute__((aligned(16))) float2 Ss[1024];
    f1k_tables<1>(tw1, tw2, tw4096);
    for (int e = threadIdx.x; e < 1024; e += 64 * FW) Ss[e] = S[e];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float2 *B = buf + wave * 1088;
    const long long w = (long long)blockIdx.x * FW + wave;
    if (w >= nw) return;   // no workgroup barrier below
    const long long p0 = pos + w * 512;
    float2 v[16], xc[16];
    float e0 = 0.0f, e1 = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        v[k] = qd_ext(c, clen, x, p0 + lane + 64 * k);
        const float a = v[k].x * v[k].x + v[k].y * v[k].y;
        if (k < 8) e0 += a;
        else e1 += a;
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        e0 += __shfl_xor(e0, s);
        e1 += __shfl_xor(e1, s);
    }
    const float E = e0 + e1;
    fft1024_wave<1>(v, B, tw1, tw2, lane);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int K = lane + 64 * k;
        const float2 X = B[K + 4 * (K >> 8)];
        xc[k] = make_float2(X.x, -X.y);
    }
    lq_wave_fence();
    float m2 = 0.0f;
    unsigned key = (unsigned)range * 1024u;
    for (int off = -range; off <= range; off++) {
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = cmul(xc[k], Ss[(lane + 64 * k + 1024 - off) & 1023]);
        fft1024_wave<1>(v, B, tw1, tw2, lane);
        const unsigned kb = (unsigned)(off + range) * 1024u;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int K = lane + 64 * k;
            const float2 r = B[K + 4 * (K >> 8)];
            const float a = r.x * r.x + r.y * r.y;
            if (a > m2) {
                m2 = a;
                key = kb + (unsigned)K;
            }
        }
        lq_wave_fence();
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const float om = __shfl_xor(m2, s);
        const unsigned ok = __shfl_xor(key, s);
        if (qd_better(om, ok, m2, key)) {
            m2 = om;
            key = ok;
        }
    }
    if (lane == 0) qd_write_record(rec + 4 * w, m2, key, E, 1024, range, s_len, s2_sum);
}

// ---------------------------------------------------------------- fused seek, nfft = 512

// 32 lanes own a window (fft_r16x16xR<2>, the register transform of k_fftr16_batch),
// eight windows per 256-thread workgroup.  Lane t holds x[t + 32 n] in v[n]; the
// transform leaves X[t + 32 s + 256 q] in v[2 s + q], which is input slot n = s + 8 q
// of the next transform: conj(X) moves between the two layouts as a renaming of
// registers, and after each offset's transform the lane reads its 16 magnitudes
// where they are, lag = t + 32 s + 256 q.  The transform synchronises the
// workgroup, so every lane runs every offset; a window past the launch's last
// works on that last window again and writes nothing.
constexpr int G512 = 8, P512 = FFTR16_LDS<2>();

__global__ __launch_bounds__(256) void k_qd_fused512(const float2 *__restrict__ c, long long clen,
                                                      const float2 *__restrict__ x, long long pos, long long nw,
                                                      const float2 *__restrict__ S, int range, unsigned s_len,
                                                      float s2_sum, const float2 *__restrict__ tw4096,
                                                      unsigned int *__restrict__ rec)
{
    __shared__ __attribute__((aligned(16))) float2 lds[G512 * P512];
    __shared__ __attribute__((aligned(16))) float2 Ss[512];
    for (int e = threadIdx.x; e < 512; e += 256) Ss[e] = S[e];
    const int g = threadIdx.x >> 5, t = threadIdx.x & 31;
    const tw16x2 w16 = fftr16_tw<2>(tw4096, t);
    float2 *L = lds + g * P512;
    const long long w0 = (long long)blockIdx.x * G512 + g;
    const bool in = w0 < nw;
    const long long p0 = pos + (in ? w0 : nw - 1) * 256;
    float2 v[16], xc[16];
    float e0 = 0.0f, e1 = 0.0f;
#pragma unroll
    for (int n = 0; n < 16; n++) {
        v[n] = qd_ext(c, clen, x, p0 + t + 32 * n);
        const float a = v[n].x * v[n].x + v[n].y * v[n].y;
        if (n < 8) e0 += a;
        else e1 += a;
    }
#pragma unroll
    for (int s = 1; s < 32; s <<= 1) {
        e0 += __shfl_xor(e0, s);
        e1 += __shfl_xor(e1, s);
    }
    const float E = e0 + e1;
    fft_r16x16xR<2, 1>(v, L, w16, t);   // its first barrier also covers Ss
#pragma unroll
    for (int s = 0; s < 8; s++)
#pragma unroll
        for (int q = 0; q < 2; q++) xc[s + 8 * q] = make_float2(v[2 * s + q].x, -v[2 * s + q].y);
    float m2 = 0.0f;
    unsigned key = (unsigned)range * 512u;
    for (int off = -range; off <= range; off++) {
#pragma unroll
        for (int n = 0; n < 16; n++) v[n] = cmul(xc[n], Ss[(t + 32 * n + 512 - off) & 511]);
        fft_r16x16xR<2, 1>(v, L, w16, t);
        const unsigned kb = (unsigned)(off + range) * 512u;
        // ascending lag: q, then s
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int s = 0; s < 8; s++) {
                const float2 r = v[2 * s + q];
                const float a = r.x * r.x + r.y * r.y;
                if (a > m2) {
                    m2 = a;
                    key = kb + (unsigned)(t + 32 * s + 256 * q);
                }
            }
    }
#pragma unroll
    for (int s = 1; s < 32; s <<= 1) {
        const float om = __shfl_xor(m2, s);
        const unsigned ok = __shfl_xor(key, s);
        if (qd_better(om, ok, m2, key)) {
            m2 = om;
            key = ok;
        }
    }
    if (in && t == 0) qd_write_record(rec + 4 * w0, m2, key, E, 512, range, s_len, s2_sum);
}

// ---------------------------------------------------------------- align stage

// F[i] = ext[pos + i]; V[i] = F[i] conj(s[i]) for i < s_len, else 0
__global__ __launch_bounds__(NT) void k_qd_align_prep(const float2 *__restrict__ c, long long clen,
                                                       const float2 *__restrict__ x, long long pos, int nfft,
                                                       const float2 *__restrict__ s, int s_len,
                                                       float2 *__restrict__ F, float2 *__restrict__ V)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= nfft) return;
    const float2 v = qd_ext(c, clen, x, pos + i);
    F[i] = v;
    float2 p = make_float2(0.0f, 0.0f);
    if (i < s_len) p = cmul(v, make_float2(s[i].x, -s[i].y));
    V[i] = p;
}

// out: R[nfft-1], R[0], R[1] (6 floats), i0 = the first arg-max of |Vf|^2 (from 0, strictly larger), then
// Vf[i0-1], Vf[i0], Vf[i0+1] (indices modulo nfft): 13 words
__global__ __launch_bounds__(NT) void k_qd_align_pick(const float2 *__restrict__ R, const float2 *__restrict__ Vf,
                                                       int nfft, unsigned int *__restrict__ out)
{
    __shared__ float shm[NT];
    __shared__ unsigned shk[NT];
    float m2 = 0.0f;
    unsigned key = 0;
    for (int i = threadIdx.x; i < nfft; i += NT) {
        const float2 v = Vf[i];
        const float a = v.x * v.x + v.y * v.y;
        if (a > m2) {
            m2 = a;
            key = (unsigned)i;
        }
    }
    qd_block_best(m2, key, shm, shk);
    if (threadIdx.x < 13) {
        const int t = threadIdx.x;
        unsigned val;
        if (t < 6) {
            const float2 r = R[(nfft - 1 + (t >> 1)) & (nfft - 1)];
            val = __float_as_uint((t & 1) ? r.y : r.x);
        } else if (t == 6) {
            val = key;
        } else {
            const int u = t - 7;
            const float2 r = Vf[((int)key + nfft - 1 + (u >> 1)) & (nfft - 1)];
            val = __float_as_uint((u & 1) ? r.y : r.x);
        }
        out[t] = val;
    }
}

// out = sum_{i < s_len} V[i] exp(-j dphi i): a fixed-order sum (one workgroup)
__global__ __launch_bounds__(NT) void k_qd_metric(const float2 *__restrict__ V, int s_len, float dphi,
                                                   float *__restrict__ out)
{
    __shared__ float sh[NT];
    float ar = 0.0f, ai = 0.0f;
    for (int i = threadIdx.x; i < s_len; i += NT) {
        float sn, cs;
        sincosf(-(dphi * (float)i), &sn, &cs);
        const float2 p = cmul(V[i], make_float2(cs, sn));
        ar += p.x;
        ai += p.y;
    }
    ar = qd_block_sum(ar, sh);
    ai = qd_block_sum(ai, sh);
    if (threadIdx.x == 0) {
        out[0] = ar;
        out[1] = ai;
    }
}

} // namespace

extern "C" int lqk_qdetector_route(unsigned int nfft)
{
    return nfft == 1024 || nfft == 512 ? LQK_QD_ROUTE_FUSED : LQK_QD_ROUTE_COMPOSED;
}

static size_t qd_pad(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" size_t lqk_qdetector_scratch_bytes(unsigned int nfft, int range, unsigned long long nw, unsigned int *nb)
{
    const unsigned noff = 2u * (unsigned)range + 1u;
    unsigned long long b = LQK_QD_PRODUCT_SAMPLES / (nw * nfft);
    if (b < 1) b = 1;
    if (b > noff) b = noff;
    if (b > LQ_GRID_Y_MAX) b = LQ_GRID_Y_MAX;
    *nb = (unsigned)b;
    // W / X (nw x nfft), P (nw x nb x nfft), run (nw), E (nw), the transforms' own scratch
    const size_t fw = lqk_fft_work_bytes(nfft, nw * b), fw1 = lqk_fft_work_bytes(nfft, nw);
    return qd_pad((size_t)nw * nfft * 8) + qd_pad((size_t)nw * b * nfft * 8) + qd_pad((size_t)nw * 8) +
           qd_pad((size_t)nw * 4) + (fw > fw1 ? fw : fw1);
}

extern "C" void lqk_qdetector_seek(int route, unsigned int nfft, unsigned int s_len, float s2_sum, int range,
                                   const void *S, const void *carry, unsigned long long clen, const void *x,
                                   unsigned long long pos, unsigned long long nw, void *scratch, void *rec,
                                   void *stream)
{
    if (nw == 0) return;
    hipStream_t st = (hipStream_t)stream;
    if (nfft < 2 || (nfft & (nfft - 1)) || range < 0 || 2ull * range + 1 > nfft || nw > (1ull << 30)) {
        fprintf(stderr, "error: lqk_qdetector_seek: nfft %u / range %d / %llu windows outside the kernels' range\n",
                nfft, range, nw);
        exit(1);
    }
    if (route == LQK_QD_ROUTE_FUSED) {
        if (nfft == 512) {
            hipLaunchKernelGGL(k_qd_fused512, dim3((unsigned)((nw + G512 - 1) / G512)), dim3(256), 0, st,
                               (const float2 *)carry, (long long)clen, (const float2 *)x, (long long)pos,
                               (long long)nw, (const float2 *)S, range, s_len, s2_sum,
                               (const float2 *)lqrt_twiddles(), (unsigned int *)rec);
            LQ_CHECK_LAUNCH();
            return;
        }
        if (nfft != 1024) {
            fprintf(stderr, "error: lqk_qdetector_seek: no fused kernel for nfft %u\n", nfft);
            exit(1);
        }
        hipLaunchKernelGGL(k_qd_fused1024, dim3((unsigned)((nw + FW - 1) / FW)), dim3(64 * FW), 0, st,
                           (const float2 *)carry, (long long)clen, (const float2 *)x, (long long)pos, (long long)nw,
                           (const float2 *)S, range, s_len, s2_sum, (const float2 *)lqrt_twiddles(),
                           (unsigned int *)rec);
        LQ_CHECK_LAUNCH();
        return;
    }
    unsigned nb;
    lqk_qdetector_scratch_bytes(nfft, range, nw, &nb);
    // the layout lqk_qdetector_scratch_bytes sizes
    unsigned char *p = (unsigned char *)scratch;
    float2 *W = (float2 *)p;
    p += qd_pad((size_t)nw * nfft * 8);
    float2 *P = (float2 *)p;
    p += qd_pad((size_t)nw * nb * nfft * 8);
    qd_best *run = (qd_best *)p;
    p += qd_pad((size_t)nw * 8);
    float *E = (float *)p;
    p += qd_pad((size_t)nw * 4);
    void *work = p;
    hipLaunchKernelGGL(k_qd_gather, dim3((unsigned)nw), dim3(NT), 0, st, (const float2 *)carry, (long long)clen,
                       (const float2 *)x, (long long)pos, (int)nfft, W, E);
    LQ_CHECK_LAUNCH();
    lqk_fft_any(nfft, +1, W, W, nw, lqk_fft_work_bytes(nfft, nw) ? work : NULL, stream);
    const int noff = 2 * range + 1;
    for (int o = 0; o < noff; o += (int)nb) {
        const int cnt = noff - o < (int)nb ? noff - o : (int)nb;
        hipLaunchKernelGGL(k_qd_mul, dim3((unsigned)nw, (unsigned)cnt), dim3(NT), 0, st, W, (const float2 *)S,
                           (int)nfft, o - range, cnt, P);
        LQ_CHECK_LAUNCH();
        lqk_fft_any(nfft, -1, P, P, nw * (unsigned long long)cnt,
                    lqk_fft_work_bytes(nfft, nw * (unsigned long long)cnt) ? work : NULL, stream);
        hipLaunchKernelGGL(k_qd_reduce, dim3((unsigned)nw), dim3(NT), 0, st, P, (int)nfft, cnt, o, o == 0,
                           o + cnt >= noff, run, E, range, s_len, s2_sum, (unsigned int *)rec);
        LQ_CHECK_LAUNCH();
    }
}

extern "C" void lqk_qdetector_spectrum(unsigned int nfft, const void *s_padded, void *S, void *work, void *stream)
{
    lqk_fft_any(nfft, +1, s_padded, S, 1, work, stream);
}

extern "C" void lqk_qdetector_align(unsigned int nfft, unsigned int s_len, int offset, const void *S, const void *s,
                                    const void *carry, unsigned long long clen, const void *x, unsigned long long pos,
                                    void *frame, void *scratch, void *out13, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    float2 *V = (float2 *)scratch, *Xf = V + nfft, *R = Xf + nfft;
    void *work = R + nfft;
    void *wk = lqk_fft_work_bytes(nfft, 1) ? work : NULL;
    hipLaunchKernelGGL(k_qd_align_prep, dim3((nfft + NT - 1) / NT), dim3(NT), 0, st, (const float2 *)carry,
                       (long long)clen, (const float2 *)x, (long long)pos, (int)nfft, (const float2 *)s, (int)s_len,
                       (float2 *)frame, V);
    LQ_CHECK_LAUNCH();
    lqk_fft_any(nfft, +1, frame, Xf, 1, wk, stream);
    hipLaunchKernelGGL(k_qd_mul, dim3(1, 1), dim3(NT), 0, st, Xf, (const float2 *)S, (int)nfft, offset, 1, R);
    LQ_CHECK_LAUNCH();
    lqk_fft_any(nfft, -1, R, R, 1, wk, stream);
    lqk_fft_any(nfft, +1, V, Xf, 1, wk, stream);
    hipLaunchKernelGGL(k_qd_align_pick, dim3(1), dim3(NT), 0, st, R, Xf, (int)nfft, (unsigned int *)out13);
    LQ_CHECK_LAUNCH();
}

extern "C" size_t lqk_qdetector_align_bytes(unsigned int nfft)
{
    return (size_t)nfft * 8 * 3 + lqk_fft_work_bytes(nfft, 1);
}

extern "C" void lqk_qdetector_metric(unsigned int s_len, float dphi, const void *scratch, void *out2, void *stream)
{
    hipLaunchKernelGGL(k_qd_metric, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const float2 *)scratch, (int)s_len,
                       dphi, (float *)out2);
    LQ_CHECK_LAUNCH();
}
