// k_firpfbch.hip -- critically sampled polyphase channelizer (firpfbch),
// analyzer and synthesizer, every size but the M = 1024 fast paths
// (k_pfb2_fast.hip).
//
// Reference semantics restated, not translated:
//  firpfbch analyzer src/multichannel/src/firpfbch.c:346-409:
//        X_b[j] = sum_{n<p} h[(M-1-j) + nM] x[(b-n)M + j],  Y_b = FFT_forward(X_b)
//  firpfbch synthesizer firpfbch.c:314-336: z_b = IFFT(X_b),
//        y_b[i] = sum_{n<p} h[i+nM] z_{b-n}[i]
// Taps are real (crcf, TC = float) or complex (cccf, TC = float2).
#include "lq_device.h"
#include "lq_fft1024.h"
#include "lq_kernels.h"
#include "lq_pfb.h"

#include <cstdio>
#include <cstdlib>

namespace {

// ------------------------------------------------------------------ firpfbch analyzer (X build)
// tap x sample: real taps (crcf) or complex taps (cccf, no conjugation, as dotprod_cccf)
__device__ __forceinline__ float2 pfb_mac(float h, float2 v, float2 a)
{
    return make_float2(fmaf(h, v.x, a.x), fmaf(h, v.y, a.y));
}
__device__ __forceinline__ float2 pfb_mac(float2 h, float2 v, float2 a)
{
    return make_float2(fmaf(h.x, v.x, fmaf(-h.y, v.y, a.x)), fmaf(h.x, v.y, fmaf(h.y, v.x, a.y)));
}

template <typename TC>
__global__ void k_pfb_an_X(int M, int p, const TC *__restrict__ hsub, const float2 *__restrict__ hist,
                           const float2 *__restrict__ x, long long nblocks, float2 *__restrict__ X)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nblocks * M) return;
    const long long b = e / M;
    const int j = (int)(e - b * M);
    const int i = M - 1 - j;
    const int HL = (p - 1) * M;
    float2 acc = make_float2(0.f, 0.f);
    for (int n = 0; n < p; n++) {
        const float2 v = ext_load(hist, HL, x, (b - n) * M + j);
        acc = pfb_mac(hsub[i * p + n], v, acc);
    }
    X[e] = acc;
}

// firpfbch synthesizer output: Z = [p-1 history z | nblocks new z]
template <typename TC>
__global__ void k_pfb_syn_out(int M, int p, const TC *__restrict__ hsub, const float2 *__restrict__ Z,
                              long long nblocks, float2 *__restrict__ y)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nblocks * M) return;
    const long long b = e / M;
    const int i = (int)(e - b * M);
    const long long zb = (p - 1) + b;
    float2 acc = make_float2(0.f, 0.f);
    for (int n = 0; n < p; n++) {
        acc = pfb_mac(hsub[i * p + n], Z[(zb - n) * M + i], acc);
    }
    y[e] = acc;
}

// firpfbch analyzer X (firpfbch.c:346-409): X[b][j] = sum_n h[i*P + n] x[(b-n)M + j], i = M-1-j
template <int P, typename TC>
__global__ __launch_bounds__(256) void k_pfb_an_X_run(int M, const TC *__restrict__ hsub,
                                                      const float2 *__restrict__ hist, const float2 *__restrict__ x,
                                                      long long nblocks, float2 *__restrict__ X)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int j = (int)(e % M);
    const long long b0 = (e / M) * RUN;
    if (b0 >= nblocks) return;
    const int i = M - 1 - j, HL = (P - 1) * M;
    TC h[P];
#pragma unroll
    for (int n = 0; n < P; n++) h[n] = hsub[i * P + n];
    float2 w[P];   // w[n] = x[(b - n) M + j]
#pragma unroll
    for (int n = 1; n < P; n++) w[n] = ext_load(hist, HL, x, (b0 - n) * M + j);
    const long long be = b0 + RUN < nblocks ? b0 + RUN : nblocks;
    // the next RPF samples of the column are in flight (clamped indices, no
    // branch): one load latency per RPF blocks instead of per block
    float2 nx[RPF];
#pragma unroll
    for (int d = 0; d < RPF; d++) nx[d] = x[(b0 + d < be ? b0 + d : be - 1) * M + j];
    for (long long b = b0; b < be; b += RPF) {
#pragma unroll
        for (int d = 0; d < RPF; d++) {
            if (b + d >= be) break;
            w[0] = nx[d];
            const long long bn = b + d + RPF;
            nx[d] = x[(bn < be ? bn : be - 1) * M + j];
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int n = 0; n < P; n++) acc = pfb_mac(h[n], w[n], acc);
            X[(b + d) * M + j] = acc;
#pragma unroll
            for (int n = P - 1; n > 0; n--) w[n] = w[n - 1];
        }
    }
}

// firpfbch synthesizer output (firpfbch.c:314-336): y[b][i] = sum_n h[i*P + n] Z[(P-1+b-n) M + i]
template <int P, typename TC>
__global__ __launch_bounds__(256) void k_pfb_syn_out_run(int M, const TC *__restrict__ hsub,
                                                         const float2 *__restrict__ Z, long long nblocks,
                                                         float2 *__restrict__ y)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(e % M);
    const long long b0 = (e / M) * RUN;
    if (b0 >= nblocks) return;
    TC h[P];
#pragma unroll
    for (int n = 0; n < P; n++) h[n] = hsub[i * P + n];
    float2 w[P];   // w[n] = Z[(P-1+b-n) M + i]
#pragma unroll
    for (int n = 1; n < P; n++) w[n] = Z[(P - 1 + b0 - n) * M + i];
    const long long be = b0 + RUN < nblocks ? b0 + RUN : nblocks;
    float2 nz[RPF];   // next RPF transforms' column samples in flight
#pragma unroll
    for (int d = 0; d < RPF; d++) nz[d] = Z[(P - 1 + (b0 + d < be ? b0 + d : be - 1)) * M + i];
    for (long long b = b0; b < be; b += RPF) {
#pragma unroll
        for (int d = 0; d < RPF; d++) {
            if (b + d >= be) break;
            w[0] = nz[d];
            const long long bn = b + d + RPF;
            nz[d] = Z[(P - 1 + (bn < be ? bn : be - 1)) * M + i];
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int n = 0; n < P; n++) acc = pfb_mac(h[n], w[n], acc);
            y[(b + d) * M + i] = acc;
#pragma unroll
            for (int n = P - 1; n > 0; n--) w[n] = w[n - 1];
        }
    }
}

// firpfbch analyzer, M = 256 R (R = 1, 2), fused like k_pfb2_an256: a lane
// per column j with the column's P taps (h[(M-1-j) + nM]) and a 16-row
// register ring, X of each 16-row group's 16 blocks in LDS, then 16 forward
// M-point transforms in registers and one store of Y (16 B per sample
// instead of the two-pass 48).
template <int P, typename TC, int R>
__global__ __launch_bounds__(256 * R, R == 1 ? 2 : 1) void k_pfb_an_fused(const TC *__restrict__ hsub,
                                                                          const float2 *__restrict__ hist,
                                                                          const float2 *__restrict__ x, int n_in,
                                                                          int nb, int S, float2 *__restrict__ Y,
                                                                          const float2 *__restrict__ tw4096)
{
    constexpr int M = 256 * R, HL = (P - 1) * M, NS = 16;
    constexpr bool TIGHT = R > 1;
    constexpr int PS = FFTR16_LDS<R, TIGHT>();
    __shared__ __attribute__((aligned(16))) float2 xr[NS * M];
    __shared__ __attribute__((aligned(16))) float2 scr[16 * PS];
    const int j = threadIdx.x;
    TC h[P];
#pragma unroll
    for (int n = 0; n < P; n++) h[n] = hsub[(M - 1 - j) * P + n];
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)Y, (short)0, nb * M * 8, 0x00020000);
    const float2 *zero = tw4096 + LQ_TW_N;   // lqrt_zeros(): the table's zero tail
    auto row_sample = [&](int b) -> float2 {
        const int t = b * M + j;
        return lq_load_hx(hist + HL, x, zero, t, HL, n_in);
    };
    const int g = threadIdx.x / (16 * R), t = threadIdx.x % (16 * R);
    const tw16x2 w16 = fftr16_tw<R>(tw4096, t);
    const int cs = (int)blockIdx.x * S;
    const int ce = cs + S < nb ? cs + S : nb;
    float2 w[NS], pf[NS];
#pragma unroll
    for (int u = 0; u < NS; u++) w[u] = row_sample(cs - NS + u);
#pragma unroll
    for (int u = 0; u < NS; u++) pf[u] = row_sample(cs + u);
    for (int r0 = cs; r0 < ce; r0 += NS) {
#pragma unroll
        for (int u = 0; u < NS; u++) {
            w[u] = pf[u];
            pf[u] = row_sample(r0 + NS + u);
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int n = 0; n < P; n++) acc = pfb_mac(h[n], w[(u - n) & (NS - 1)], acc);
            xr[u * M + j] = acc;
        }
        lq_lds_sync();
        float2 v[16];
#pragma unroll
        for (int n = 0; n < 16; n++) v[n] = xr[g * M + t + 16 * R * n];
        fft_r16x16xR<R, +1, TIGHT>(v, scr + g * PS, w16, t);
        const int b = r0 + g;
        const unsigned base = b < ce ? (unsigned)b * (unsigned)(M * 8) : 0xFFFFF000u;
#pragma unroll
        for (int sidx = 0; sidx < 16 / R; sidx++)
#pragma unroll
            for (int q = 0; q < R; q++)
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v[sidx * R + q]), ry,
                                                      base + (unsigned)(t + 16 * R * sidx + 256 * q) * 8u, 0, 0);
    }
}

template <typename TC>
void launch_pfb_an_fused(int M, int p, const void *hsub, const void *hist, const void *x, long long nb, void *Y,
                         long long S, unsigned grid, hipStream_t st)
{
    lq_switch<2, 4, 6, 8, 10, 12, 14, 16>(p, [&](auto P) {
        lq_switch<256, 512>(M, [&](auto MM) {
            hipLaunchKernelGGL((k_pfb_an_fused<P, TC, MM / 256>), dim3(grid), dim3(MM), 0, st, (const TC *)hsub,
                               (const float2 *)hist, (const float2 *)x, (int)(nb * M), (int)nb, (int)S,
                               (float2 *)Y, (const float2 *)lqrt_twiddles());
        });
        LQ_CHECK_LAUNCH();
    });
}

// firpfbch analyzer, M = 4096 fused (the two-pass path moved 48 B per
// sample): the structure of k_pfb2_an4096 for the critically sampled bank
// (firpfbch.c:262-312).  Lane t owns columns t + 1024 q with their P taps
// h[(M-1-col) + nM]; row b of the input is block b's polyphase row, and a
// group of G = 3 rows fills three block buffers, whose twelve 1024-point
// quarters (columns = r mod 4) waves 0-11 forward-transform (one row per
// group: 0.72 ms per 2^27 samples at m = 4, four waves busy); all 16 waves
// then combine
//     Y[k + 1024 s] = sum_r W_4096^(r k) Q_r[k] (-i)^(r s)
// into 8-byte coalesced stores.  The ring keeps its oldest row in LDS.
template <int P, typename TC, int G = 3>
__global__ __launch_bounds__(1024, 1) void k_pfb_an4096(const TC *__restrict__ hsub, const float2 *__restrict__ hist,
                                                        const float2 *__restrict__ x, int n_in, int nb, int S,
                                                        float2 *__restrict__ Y, const float2 *__restrict__ tw4096)
{
    constexpr int M = 4096, HL = (P - 1) * M, NS = P;
    static_assert(P >= 2, "ring of at least two rows");
    static_assert(G * A4_BSTR * 8 + 4 * 1024 * 8 + 512 <= 160 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) float2 xr[G * A4_BSTR];
    __shared__ __attribute__((aligned(16))) float2 tw2[64];
    __shared__ __attribute__((aligned(16))) float2 wold[4 * 1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) tw2[tid] = tw4096[(64 * (tid & 3) * (tid >> 2)) & 4095];   // W_64^{+b r} (forward)
    const float2 a1 = tw4096[(4 * lane) & 4095], a4 = tw4096[(16 * lane) & 4095];
    // column t + 1024 q sits in quarter t & 3 at index (t >> 2) + 256 q
    const int pq = (tid & 3) * A4_QS + (tid >> 2);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)Y, (short)0, nb * M * 8, 0x00020000);
    const float2 *zero = tw4096 + LQ_TW_N;
    auto row_sample = [&](int b, int col) -> float2 {
        return lq_load_hx(hist + HL, x, zero, b * M + col, HL, n_in);
    };
    // ring of column q: rows (newest - NS + 2 + u) in w[q][u], the oldest in
    // wold (private to the lane); pf: the next group's rows, loaded after the
    // transforms so they never sit beside a transform and the ring
    float2 w[4][NS - 1], pf[G][4], wo[4];
    const int cs = (int)blockIdx.x * S;
    const int ce = cs + S < nb ? cs + S : nb;
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int u = 0; u < NS - 1; u++) w[q][u] = row_sample(cs - NS + 1 + u, tid + 1024 * q);   // rows cs-P+1 .. cs-1
        wold[q * 1024 + tid] = row_sample(cs - NS + 1, tid + 1024 * q);
#pragma unroll
        for (int g = 0; g < G; g++) pf[g][q] = row_sample(cs + g, tid + 1024 * q);
    }
    __syncthreads();   // tw2 ready
    for (int b0 = cs; b0 < ce; b0 += G) {
#pragma unroll
        for (int g = 0; g < G; g++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                wo[q] = wold[q * 1024 + tid];   // row b - P + 1
#pragma unroll
                for (int u = 0; u < NS - 2; u++) w[q][u] = w[q][u + 1];
                w[q][NS - 2] = pf[g][q];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int o = (M - 1 - (tid + 1024 * q)) * P;
                asm volatile("" : "+v"(o));   // taps re-read each row (L1 / L2 hits), not held across the transforms
                const TC *h = hsub + o;
                float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                for (int n = 0; n < NS; n++) acc = pfb_mac(h[n], n < NS - 1 ? w[q][NS - 2 - n] : wo[q], acc);
                xr[g * A4_BSTR + pq + 256 * q] = acc;
                asm volatile("" ::: "memory");
            }
            // the next row's oldest (row b - P + 2) waits in LDS
#pragma unroll
            for (int q = 0; q < 4; q++) wold[q * 1024 + tid] = w[q][0];
        }
        lq_lds_sync();
        if (wave < 4 * G) {   // block b0 + wave / 4, quarter wave % 4
            float2 *Bq = xr + (wave >> 2) * A4_BSTR + (wave & 3) * A4_QS;
            float2 v[16];
#pragma unroll
            for (int n = 0; n < 16; n++) v[n] = Bq[lane + 64 * n];
            fft1024_wave_rt<+1>(v, Bq, a1, a4, tw2, lane);   // natural order at k + 4 (k >> 8)
        }
        lq_lds_sync();
#pragma unroll
        for (int g = 0; g < G; g++)
#pragma unroll
            for (int q = 0; q < 4; q++) pf[g][q] = row_sample(b0 + G + g, tid + 1024 * q);
        {
            const int k = tid;   // bin k of each quarter -> outputs k + 1024 s
            const int pos = k + 4 * (k >> 8);
            v2f W[4];
#pragma unroll
            for (int r = 1; r < 4; r++) W[r] = pk(tw4096[r * k]);   // W_4096^(r k), r k < 4096
#pragma unroll
            for (int g = 0; g < G; g++) {
                const int b = b0 + g;
                v2f T[4];
#pragma unroll
                for (int r = 0; r < 4; r++) T[r] = pk(xr[g * A4_BSTR + r * A4_QS + pos]);
#pragma unroll
                for (int r = 1; r < 4; r++) T[r] = pk_cmul(T[r], W[r]);
                const v2f s02 = T[0] + T[2], d02 = T[0] - T[2], s13 = T[1] + T[3], d13 = T[1] - T[3];
                const v2f jd13 = v2f{-d13.y, d13.x};   // i (T1 - T3)
                const v2f Yo[4] = {s02 + s13, d02 - jd13, s02 - s13, d02 + jd13};
                // a block past the run: a base the launch's range (< 2^31) never reaches
                const unsigned base = b < ce ? (unsigned)b * (unsigned)(M * 8) : 0x80000000u;
#pragma unroll
                for (int sq = 0; sq < 4; sq++)
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, Yo[sq]), ry,
                                                          base + (unsigned)(k + 1024 * sq) * 8u, 0, 2);
            }
        }
        lq_lds_sync();   // the combine's reads are done before the next group's writes
    }
}

template <typename TC>
void launch_pfb_an4096(int p, const void *hsub, const void *hist, const void *x, long long nb, void *Y, long long S,
                       unsigned grid, hipStream_t st)
{
    constexpr int M = 4096;
    lq_switch<2, 4, 6, 8>(p, [&](auto P) {
        hipLaunchKernelGGL((k_pfb_an4096<P, TC>), dim3(grid), dim3(1024), 0, st, (const TC *)hsub,
                           (const float2 *)hist, (const float2 *)x, (int)(nb * M), (int)nb, (int)S, (float2 *)Y,
                           (const float2 *)lqrt_twiddles());
        LQ_CHECK_LAUNCH();
    });
}

// firpfbch analyzer, M = 64 / 128, fused as k_pfb_an_fused with Q = 256 / M
// column sets per workgroup (each on its own run of blocks; every set runs
// the same number of 16-block groups, stores past its run dropped) and the
// 16 Q forward M-point transforms of a group on R = M / 16 lanes each
// (fft_small16xR)
template <int P, typename TC, int MS>
__global__ __launch_bounds__(256, 2) void k_pfb_an_small(const TC *__restrict__ hsub, const float2 *__restrict__ hist,
                                                        const float2 *__restrict__ x, int n_in, int nb, int S,
                                                        float2 *__restrict__ Y, const float2 *__restrict__ tw4096)
{
    constexpr int M = MS, HL = (P - 1) * M, NS = 16, Q = 256 / M, R = M / 16, PS = FFTS_LDS<R>();
    __shared__ __attribute__((aligned(16))) float2 xr[Q * NS * M];
    __shared__ __attribute__((aligned(16))) float2 scr[16 * Q * PS];
    const int set = threadIdx.x / M, j = threadIdx.x % M;
    float2 *xs = xr + set * (NS * M);
    TC h[P];
#pragma unroll
    for (int n = 0; n < P; n++) h[n] = hsub[(M - 1 - j) * P + n];
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)Y, (short)0, nb * M * 8, 0x00020000);
    const float2 *zero = tw4096 + LQ_TW_N;   // lqrt_zeros(): the table's zero tail
    auto row_sample = [&](int b) -> float2 {
        const int t = b * M + j;
        return lq_load_hx(hist + HL, x, zero, t, HL, n_in);
    };
    const int tg = threadIdx.x / R, t = threadIdx.x % R;   // transform tg: set tg / 16, block tg % 16
    const int tset = tg / 16, tb16 = tg % 16;
    const int e = t * (4096 / M);
    const float2 a1 = tw4096[e & 4095], a4 = tw4096[(4 * e) & 4095];
    const int cs = ((int)blockIdx.x * Q + set) * S;
    const int tcs = ((int)blockIdx.x * Q + tset) * S;
    const int tce = tcs + S < nb ? tcs + S : nb;
    float2 w[NS], pf[NS];
#pragma unroll
    for (int u = 0; u < NS; u++) w[u] = row_sample(cs - NS + u);
#pragma unroll
    for (int u = 0; u < NS; u++) pf[u] = row_sample(cs + u);
    for (int g0 = 0; g0 < S; g0 += NS) {
        const int r0 = cs + g0;
#pragma unroll
        for (int u = 0; u < NS; u++) {
            w[u] = pf[u];
            pf[u] = row_sample(r0 + NS + u);
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int n = 0; n < P; n++) acc = pfb_mac(h[n], w[(u - n) & (NS - 1)], acc);
            xs[u * M + j] = acc;
        }
        lq_lds_sync();
        float2 v[16];
        const float2 *B = xr + tset * (NS * M) + tb16 * M;
#pragma unroll
        for (int n = 0; n < 16; n++) v[n] = B[t + R * n];
        fft_small16xR<R, +1>(v, scr + tg * PS, a1, a4, t);   // (its barriers also free xr)
        const int b = tcs + g0 + tb16;
        const unsigned base = b < tce ? (unsigned)b * (unsigned)(M * 8) : 0xFFFFF000u;
        // v[u R + q] = X[t (16/R) + u + 16 q]
#pragma unroll
        for (int u = 0; u < 16 / R; u++)
#pragma unroll
            for (int q = 0; q < R; q++)
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v[u * R + q]), ry,
                                                      base + (unsigned)(t * (16 / R) + u + 16 * q) * 8u, 0, 0);
    }
}

template <typename TC>
void launch_pfb_an_small(int M, int p, const void *hsub, const void *hist, const void *x, long long nb, void *Y,
                         long long S, unsigned grid, hipStream_t st)
{
    lq_switch<2, 4, 6, 8, 10, 12, 14, 16>(p, [&](auto P) {
        lq_switch<64, 128>(M, [&](auto MM) {
            hipLaunchKernelGGL((k_pfb_an_small<P, TC, MM>), dim3(grid), dim3(256), 0, st, (const TC *)hsub,
                               (const float2 *)hist, (const float2 *)x, (int)(nb * M), (int)nb, (int)S,
                               (float2 *)Y, (const float2 *)lqrt_twiddles());
        });
        LQ_CHECK_LAUNCH();
    });
}

// firpfbch synthesizer, M = 256 R, fused: per group of 16 blocks, 16
// inverse register transforms of X (z_b = IFFT(X_b)) into LDS, then a lane
// per column i runs y_b[i] = sum_n h[i p + n] z_{b-n}[i] from a 16-deep
// register ring.  A workgroup's run of blocks warms its ring up on the 16
// blocks before it (transformed again, outputs dropped) or, for the call's
// first run, on the object's last p-1 transforms (state); the z of the
// call's last p-1 blocks go to znew for the next call.
template <int P, typename TC, int R>
__global__ __launch_bounds__(256 * R, R == 1 ? 2 : 1) void k_pfb_syn_fused(const TC *__restrict__ hsub,
                                                                           const float2 *__restrict__ state,
                                                                           const float2 *__restrict__ X, int nb,
                                                                           int S, float2 *__restrict__ y,
                                                                           float2 *__restrict__ znew,
                                                                           const float2 *__restrict__ tw4096)
{
    constexpr int M = 256 * R, HB = P - 1, NS = 16;
    constexpr bool TIGHT = R > 1;
    constexpr int PS = FFTR16_LDS<R, TIGHT>();
    __shared__ __attribute__((aligned(16))) float2 zr[NS * M];
    __shared__ __attribute__((aligned(16))) float2 scr[16 * PS];
    const int i = threadIdx.x;
    TC h[P];
#pragma unroll
    for (int n = 0; n < P; n++) h[n] = hsub[i * P + n];
    const int g = threadIdx.x / (16 * R), t = threadIdx.x % (16 * R);
    const tw16x2 w16 = fftr16_tw<R>(tw4096, t);
    const int cs = (int)blockIdx.x * S;
    const int ce = cs + S < nb ? cs + S : nb;
    float2 w[NS];
    int r0 = cs;
    if (cs == 0) {   // z_{-16} .. z_{-1}: the state's last p-1 transforms, zeros before
#pragma unroll
        for (int u = 0; u < NS; u++) {
            const int b = u - NS;
            w[u] = (b >= -HB) ? state[(HB + b) * M + i] : make_float2(0.f, 0.f);
        }
    } else {
        r0 = cs - NS;    // warm-up group: transformed, outputs dropped
    }
    for (; r0 < ce; r0 += NS) {
        {
            const int b = r0 + g;
            float2 v[16];
            const float2 *xb = X + (long long)(b < nb ? b : nb - 1) * M;
#pragma unroll
            for (int n = 0; n < 16; n++) v[n] = xb[t + 16 * R * n];
            fft_r16x16xR<R, -1, TIGHT>(v, scr + g * PS, w16, t);
            float2 *zb = zr + g * M;
#pragma unroll
            for (int sidx = 0; sidx < 16 / R; sidx++)
#pragma unroll
                for (int q = 0; q < R; q++) {
                    const int k = t + 16 * R * sidx + 256 * q;
                    zb[k] = v[sidx * R + q];
                    if (b >= nb - HB && b < nb && b >= cs && b < ce) znew[(b - (nb - HB)) * M + k] = v[sidx * R + q];
                }
        }
        lq_lds_sync();
#pragma unroll
        for (int u = 0; u < NS; u++) {
            w[u] = zr[u * M + i];
            const int b = r0 + u;
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int n = 0; n < P; n++) acc = pfb_mac(h[n], w[(u - n) & (NS - 1)], acc);
            if (b >= cs && b < ce) y[(long long)b * M + i] = acc;
        }
        lq_lds_sync();   // zr is rewritten by the next group's transforms
    }
}

template <typename TC>
void launch_pfb_syn_fused(int M, int p, const void *hsub, const void *state, const void *X, long long nb, void *y,
                          void *znew, long long S, unsigned grid, hipStream_t st)
{
    lq_switch<2, 4, 6, 8, 10, 12, 14, 16>(p, [&](auto P) {
        lq_switch<256, 512>(M, [&](auto MM) {
            hipLaunchKernelGGL((k_pfb_syn_fused<P, TC, MM / 256>), dim3(grid), dim3(MM), 0, st, (const TC *)hsub,
                               (const float2 *)state, (const float2 *)X, (int)nb, (int)S, (float2 *)y,
                               (float2 *)znew, (const float2 *)lqrt_twiddles());
        });
        LQ_CHECK_LAUNCH();
    });
}

// firpfbch synthesizer, M = 4096 fused (the two-pass path moved 48 B per
// sample): z_b = IFFT(X_b) by quarters -- waves 0..4G-1 each load the bins
// X_b[4i + r] of one block's quarter r straight from HBM and inverse-
// transform them in registers (fft1024_wave_rt) -- then the radix-4 combine
//     z[k + 1024 s] = sum_r W_4096^-(r k) Q_r[k] i^(r s)
// leaves lane t exactly its own columns t + 1024 s, so the p-tap output
// y_b[col] = sum_n h[col p + n] z_{b-n}[col] (firpfbch.c:314-336) runs from
// a register ring (its oldest entry in LDS across the transforms) with no
// further LDS traffic.  Runs warm up on the blocks before them (transformed
// again, outputs dropped) or, for the call's first run, on the object's last
// p-1 transforms (state); the z of the call's last p-1 blocks go to znew.
// (p = 8: three-block groups spill 18 VGPRs and still beat two-block groups, 0.585 vs 0.615 ms)
template <int P, typename TC, int G = 3>
__global__ __launch_bounds__(1024, 1) void k_pfb_syn4096(const TC *__restrict__ hsub, const float2 *__restrict__ state,
                                                         const float2 *__restrict__ X, int nb, int S,
                                                         float2 *__restrict__ y, float2 *__restrict__ znew,
                                                         const float2 *__restrict__ tw4096)
{
    constexpr int M = 4096, HB = P - 1, NR = P > 2 ? P - 2 : 1;
    constexpr int NW = G * ((HB + G - 1) / G);   // warm-up blocks before a run (whole groups)
    static_assert(P >= 2, "two taps per column at least");
    __shared__ __attribute__((aligned(16))) float2 xr[G * A4_BSTR];
    __shared__ __attribute__((aligned(16))) float2 tw2[64];
    __shared__ __attribute__((aligned(16))) float2 wold[4 * 1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) {   // W_64^{-b r} (inverse transform)
        const float2 u = tw4096[(64 * (tid & 3) * (tid >> 2)) & 4095];
        tw2[tid] = make_float2(u.x, -u.y);
    }
    const float2 a1 = tw4096[(4 * lane) & 4095], a4 = tw4096[(16 * lane) & 4095];
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)y, (short)0, nb * M * 8, 0x00020000);
    const int cs = (int)blockIdx.x * S;
    const int ce = cs + S < nb ? cs + S : nb;
    // ring of column t + 1024 q before block b: wold = z_{b-P+1}, r[q][u] =
    // z_{b-P+2+u} (u < P-2)
    float2 r[4][NR];
    int b0 = cs;
    if (cs == 0) {   // the state's last p-1 transforms
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int col = tid + 1024 * q;
            wold[q * 1024 + tid] = state[col];
#pragma unroll
            for (int u = 0; u < P - 2; u++) r[q][u] = state[(1 + u) * M + col];
        }
    } else {
        b0 = cs - NW;   // warm-up groups: transformed, outputs dropped
#pragma unroll
        for (int q = 0; q < 4; q++) {
            wold[q * 1024 + tid] = make_float2(0.f, 0.f);
#pragma unroll
            for (int u = 0; u < NR; u++) r[q][u] = make_float2(0.f, 0.f);
        }
    }
    __syncthreads();   // tw2 ready
    for (; b0 < ce; b0 += G) {
        if (wave < 4 * G) {   // block b0 + wave / 4, quarter wave % 4
            const int g = wave >> 2, rq = wave & 3;
            const int b = b0 + g < nb ? b0 + g : nb - 1;
            const float2 *xb = X + (long long)b * M + rq;
            float2 v[16];
#pragma unroll
            for (int n = 0; n < 16; n++) v[n] = xb[4 * (lane + 64 * n)];
            float2 *Bq = xr + g * A4_BSTR + rq * A4_QS;
            fft1024_wave_rt<-1>(v, Bq, a1, a4, tw2, lane);   // natural order at k + 4 (k >> 8)
        }
        lq_lds_sync();
        {
            const int k = tid, pos = k + 4 * (k >> 8);
            v2f W[4];
#pragma unroll
            for (int rr = 1; rr < 4; rr++) {
                const float2 u = tw4096[rr * k];   // W_4096^(r k), r k < 4096
                W[rr] = v2f{u.x, -u.y};
            }
#pragma unroll
            for (int g = 0; g < G; g++) {
                const int b = b0 + g;
                v2f T[4];
#pragma unroll
                for (int rr = 0; rr < 4; rr++) T[rr] = pk(xr[g * A4_BSTR + rr * A4_QS + pos]);
#pragma unroll
                for (int rr = 1; rr < 4; rr++) T[rr] = pk_cmul(T[rr], W[rr]);
                const v2f s02 = T[0] + T[2], d02 = T[0] - T[2], s13 = T[1] + T[3], d13 = T[1] - T[3];
                const v2f jd13 = v2f{-d13.y, d13.x};   // i (T1 - T3)
                const v2f z[4] = {s02 + s13, d02 + jd13, s02 - s13, d02 - jd13};   // columns t + 1024 s
                const bool out = b >= cs && b < ce;
                const unsigned base = out ? (unsigned)b * (unsigned)(M * 8) : 0x80000000u;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int col = tid + 1024 * q;
                    int o = col * P;
                    asm volatile("" : "+v"(o));   // taps re-read per block (L1 / L2 hits)
                    const TC *h = hsub + o;
                    const float2 zo = wold[q * 1024 + tid];
                    float2 acc = pfb_mac(h[0], unpk(z[q]), make_float2(0.f, 0.f));
#pragma unroll
                    for (int n = 1; n < P - 1; n++) acc = pfb_mac(h[n], r[q][P - 2 - n], acc);
                    acc = pfb_mac(h[P - 1], zo, acc);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, pk(acc)), ry,
                                                          base + (unsigned)col * 8u, 0, 2);
                    if (out && b >= nb - HB) znew[(long long)(b - (nb - HB)) * M + col] = unpk(z[q]);
                    // advance the ring: z_{b-P+2} becomes the LDS-held oldest
                    if constexpr (P > 2) {
                        wold[q * 1024 + tid] = r[q][0];
#pragma unroll
                        for (int u = 0; u < P - 3; u++) r[q][u] = r[q][u + 1];
                        r[q][P - 3] = unpk(z[q]);
                    } else {
                        wold[q * 1024 + tid] = unpk(z[q]);
                    }
                }
            }
        }
        lq_lds_sync();   // the combine's reads are done before the next group's transforms
    }
}

template <typename TC>
void launch_pfb_syn4096(int p, const void *hsub, const void *state, const void *X, long long nb, void *y, void *znew,
                        long long S, unsigned grid, hipStream_t st)
{
    lq_switch<2, 4, 6, 8>(p, [&](auto P) {
        hipLaunchKernelGGL((k_pfb_syn4096<P, TC>), dim3(grid), dim3(1024), 0, st, (const TC *)hsub,
                           (const float2 *)state, (const float2 *)X, (int)nb, (int)S, (float2 *)y,
                           (float2 *)znew, (const float2 *)lqrt_twiddles());
        LQ_CHECK_LAUNCH();
    });
}

// firpfbch synthesizer, M = 64 / 128, fused as k_pfb_syn_fused with Q = 256
// / M column sets per workgroup on their own runs of blocks, the 16 Q inverse
// transforms of a group on M / 16 lanes each (fft_small16xR).  Every set runs
// the same groups g0 = -16, 0, 16, .. < S relative to its run: the first is
// the warm-up (blocks before the run transformed again, or for the call's
// first run the object's last p-1 transforms, zeros before them).
template <int P, typename TC, int MS>
__global__ __launch_bounds__(256, 2) void k_pfb_syn_small(const TC *__restrict__ hsub,
                                                         const float2 *__restrict__ state,
                                                         const float2 *__restrict__ X, int nb, int S,
                                                         float2 *__restrict__ y, float2 *__restrict__ znew,
                                                         const float2 *__restrict__ tw4096)
{
    constexpr int M = MS, HB = P - 1, NS = 16, Q = 256 / M, R = M / 16, PS = FFTS_LDS<R>();
    __shared__ __attribute__((aligned(16))) float2 zr[Q * NS * M];
    __shared__ __attribute__((aligned(16))) float2 scr[16 * Q * PS];
    const int set = threadIdx.x / M, i = threadIdx.x % M;
    TC h[P];
#pragma unroll
    for (int n = 0; n < P; n++) h[n] = hsub[i * P + n];
    const int tg = threadIdx.x / R, t = threadIdx.x % R;   // transform tg: set tg / 16, block tg % 16
    const int tset = tg / 16, tb16 = tg % 16;
    const int e = t * (4096 / M);
    const float2 a1 = tw4096[e & 4095], a4 = tw4096[(4 * e) & 4095];
    const int cs = ((int)blockIdx.x * Q + set) * S;
    const int ce = cs + S < nb ? cs + S : nb;
    const int tcs = ((int)blockIdx.x * Q + tset) * S;
    const int tce = tcs + S < nb ? tcs + S : nb;
    float2 w[NS];
    for (int g0 = -NS; g0 < S; g0 += NS) {
        {
            const int b = tcs + g0 + tb16;
            float2 v[16];
            const float2 *xb = X + (long long)(b < 0 ? 0 : (b < nb ? b : nb - 1)) * M;
#pragma unroll
            for (int n = 0; n < 16; n++) v[n] = xb[t + R * n];
            fft_small16xR<R, -1>(v, scr + tg * PS, a1, a4, t);
            float2 *zb = zr + tset * (NS * M) + tb16 * M;
#pragma unroll
            for (int u = 0; u < 16 / R; u++)
#pragma unroll
                for (int q = 0; q < R; q++) {
                    const int k = t * (16 / R) + u + 16 * q;
                    float2 z = v[u * R + q];
                    if (b < 0) z = (b >= -HB) ? state[(HB + b) * M + k] : make_float2(0.f, 0.f);
                    zb[k] = z;
                    if (b >= nb - HB && b < nb && b >= tcs && b < tce) znew[(b - (nb - HB)) * M + k] = z;
                }
        }
        lq_lds_sync();
#pragma unroll
        for (int u = 0; u < NS; u++) {
            w[u] = zr[set * (NS * M) + u * M + i];
            const int b = cs + g0 + u;
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int n = 0; n < P; n++) acc = pfb_mac(h[n], w[(u - n) & (NS - 1)], acc);
            if (b >= cs && b < ce) y[(long long)b * M + i] = acc;
        }
        lq_lds_sync();   // zr is rewritten by the next group's transforms
    }
}

template <typename TC>
void launch_pfb_syn_small(int M, int p, const void *hsub, const void *state, const void *X, long long nb, void *y,
                          void *znew, long long S, unsigned grid, hipStream_t st)
{
    lq_switch<2, 4, 6, 8, 10, 12, 14, 16>(p, [&](auto P) {
        lq_switch<64, 128>(M, [&](auto MM) {
            hipLaunchKernelGGL((k_pfb_syn_small<P, TC, MM>), dim3(grid), dim3(256), 0, st, (const TC *)hsub,
                               (const float2 *)state, (const float2 *)X, (int)nb, (int)S, (float2 *)y,
                               (float2 *)znew, (const float2 *)lqrt_twiddles());
        });
        LQ_CHECK_LAUNCH();
    });
}

// ------------------------------------------------------------------ what a launch decides
// Diagnostic switch (DESIGN.md (a) history): LQ_PFB_TWO_PASS in the
// environment routes the fused sizes through the generic two-pass path.
// Read once per process.
bool pfb_two_pass()
{
    static const bool v = getenv("LQ_PFB_TWO_PASS") != nullptr;
    return v;
}

long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// runs of S blocks, a multiple of `step' and at least `least', over about T
// workgroups (or column sets): T is lqrt_grid(N, N), N itself unless
// liquid_mi355x_set_max_workgroups has set a lower limit (tests only)
long long blocks_run(long long nb, unsigned N, long long step, long long least)
{
    const long long S = cdiv(cdiv(nb, lqrt_grid(N, N)), step) * step;
    return S < least ? least : S;
}

bool even_to(unsigned p, unsigned top) { return p >= 2 && p <= top && p % 2 == 0; }   // lq_switch<2, 4, .., top>

// The routing order behind the M = 1024 fast paths (k_pfb2_fast.hip).  The
// route of complex taps is its real one + 1.
lqk_pfb_plan pfb_an_plan(int ctaps, unsigned M, unsigned p, long long nb)
{
    const lqk_pfb_plan none = {LQK_PFB_NONE, 0, 0, 1};
    if (M < 1 || p < 1 || nb < 1) return none;
    const int c = ctaps ? 1 : 0;
    const bool fused = !pfb_two_pass() && nb * (long long)M * 8 < (1ll << 31);   // 32-bit buffer offsets
    if (fused && (M == 256 || M == 512) && even_to(p, 16)) {
        const long long S = blocks_run(nb, 1024, 16, 32);
        return {LQK_PFB_AN_FUSED + c, S, cdiv(nb, S), 1};
    }
    if (fused && M == 4096 && even_to(p, 8)) {
        // one workgroup per CU: about 256 runs of S blocks (each warms up on the p - 1 rows before it)
        const long long S = blocks_run(nb, 256, 1, 32);
        return {LQK_PFB_AN4096 + c, S, cdiv(nb, S), 1};
    }
    if (fused && (M == 64 || M == 128) && even_to(p, 16)) {
        const long long S = blocks_run(nb, 2048, 16, 32);
        return {LQK_PFB_AN_SMALL + c, S, cdiv(cdiv(nb, S), 256 / M), 1};
    }
    // X is formed in Y then transformed in place: compile-time ring depths
    // for the common shapes, else the per-element kernel
    if (p == 1 || even_to(p, 16)) return {LQK_PFB_AN_RUN_FFT + c, RUN, cdiv((long long)M * cdiv(nb, RUN), 256), 1};
    return {LQK_PFB_AN_ELEM_FFT + c, 1, cdiv(nb * M, 256), 1};
}

lqk_pfb_plan pfb_syn_plan(int ctaps, unsigned M, unsigned p, long long nb)
{
    const lqk_pfb_plan none = {LQK_PFB_NONE, 0, 0, 1};
    if (M < 1 || p < 1 || nb < 1) return none;
    const int c = ctaps ? 1 : 0;
    const bool fused = !pfb_two_pass() && nb >= (long long)p;
    if (fused && (M == 256 || M == 512) && even_to(p, 16) && nb * (long long)M < (1ll << 31)) {
        const long long S = blocks_run(nb, 1024, 16, 64);
        return {LQK_PFB_SYN_FUSED + c, S, cdiv(nb, S), 1};
    }
    if (fused && M == 4096 && even_to(p, 8) && nb * (long long)M * 8 < (1ll << 31)) {
        const long long S = blocks_run(nb, 256, 3, 33);
        return {LQK_PFB_SYN4096 + c, S, cdiv(nb, S), 1};
    }
    if (fused && (M == 64 || M == 128) && even_to(p, 16) && nb * (long long)M < (1ll << 31)) {
        const long long S = blocks_run(nb, 2048, 16, 64);
        return {LQK_PFB_SYN_SMALL + c, S, cdiv(cdiv(nb, S), 256 / M), 1};
    }
    if (p == 1 || even_to(p, 16)) return {LQK_PFB_FFT_SYN_RUN + c, RUN, cdiv((long long)M * cdiv(nb, RUN), 256), 1};
    return {LQK_PFB_FFT_SYN_ELEM + c, 1, cdiv(nb * M, 256), 1};
}

template <typename TC>
void pfb_analyzer(int M, int p, const void *hsub, const void *hist, const void *x, long long nb, void *Y,
                  hipStream_t st)
{
    const lqk_pfb_plan pl = pfb_an_plan(sizeof(TC) == sizeof(float2), M, p, nb);
    const unsigned grid = (unsigned)pl.workgroups;
    switch (pl.route - ((pl.route - LQK_PFB_AN_FUSED) & 1)) {   // the real-tap code
    case LQK_PFB_AN_FUSED: launch_pfb_an_fused<TC>(M, p, hsub, hist, x, nb, Y, pl.run, grid, st); return;
    case LQK_PFB_AN4096: launch_pfb_an4096<TC>(p, hsub, hist, x, nb, Y, pl.run, grid, st); return;
    case LQK_PFB_AN_SMALL: launch_pfb_an_small<TC>(M, p, hsub, hist, x, nb, Y, pl.run, grid, st); return;
    case LQK_PFB_AN_RUN_FFT:
        lq_switch<1, 2, 4, 6, 8, 10, 12, 14, 16>(p, [&](auto P) {
            hipLaunchKernelGGL((k_pfb_an_X_run<P, TC>), dim3(grid), dim3(256), 0, st, M, (const TC *)hsub,
                               (const float2 *)hist, (const float2 *)x, nb, (float2 *)Y);
        });
        break;
    default:
        hipLaunchKernelGGL(k_pfb_an_X<TC>, dim3(grid), dim3(256), 0, st, M, p, (const TC *)hsub,
                           (const float2 *)hist, (const float2 *)x, nb, (float2 *)Y);
    }
    LQ_CHECK_LAUNCH();
    lq_fft_batch_scaled(M, +1, Y, Y, nb, 1.f, 1.f, 0, 0, st);
}

template <typename TC>
void pfb_synthesizer(int M, int p, const void *hsub, void *state, void *zscratch, const void *X, long long nb,
                     void *y, hipStream_t st)
{
    const long long HB = (long long)p - 1;
    const size_t hbytes = HB * M * sizeof(float2);
    float2 *Z = (float2 *)zscratch;
    const lqk_pfb_plan pl = pfb_syn_plan(sizeof(TC) == sizeof(float2), M, p, nb);
    const unsigned grid = (unsigned)pl.workgroups;
    const int route = pl.route - ((pl.route - LQK_PFB_SYN_FUSED) & 1);   // the real-tap code
    // fused forms: the last p-1 transforms land in the scratch, then become
    // the state (every workgroup reads the old state first)
    if (route == LQK_PFB_SYN_FUSED || route == LQK_PFB_SYN4096 || route == LQK_PFB_SYN_SMALL) {
        if (route == LQK_PFB_SYN_FUSED)
            launch_pfb_syn_fused<TC>(M, p, hsub, state, X, nb, y, Z, pl.run, grid, st);
        else if (route == LQK_PFB_SYN4096)
            launch_pfb_syn4096<TC>(p, hsub, state, X, nb, y, Z, pl.run, grid, st);
        else
            launch_pfb_syn_small<TC>(M, p, hsub, state, X, nb, y, Z, pl.run, grid, st);
        if (HB > 0) LQ_CHECK(hipMemcpyAsync(state, Z, hbytes, hipMemcpyDeviceToDevice, st));
        return;
    }
    if (HB > 0) LQ_CHECK(hipMemcpyAsync(Z, state, hbytes, hipMemcpyDeviceToDevice, st));
    lq_fft_batch_scaled(M, -1, X, Z + HB * M, nb, 1.f, 1.f, 0, 0, st);
    if (route == LQK_PFB_FFT_SYN_RUN)
        lq_switch<1, 2, 4, 6, 8, 10, 12, 14, 16>(p, [&](auto P) {
            hipLaunchKernelGGL((k_pfb_syn_out_run<P, TC>), dim3(grid), dim3(256), 0, st, M, (const TC *)hsub,
                               (const float2 *)Z, nb, (float2 *)y);
        });
    else
        hipLaunchKernelGGL(k_pfb_syn_out<TC>, dim3(grid), dim3(256), 0, st, M, p, (const TC *)hsub,
                           (const float2 *)Z, nb, (float2 *)y);
    LQ_CHECK_LAUNCH();
    if (HB > 0) LQ_CHECK(hipMemcpyAsync(state, Z + nb * M, hbytes, hipMemcpyDeviceToDevice, st));
}

} // namespace

extern "C" lqk_pfb_plan lqk_firpfbch_plan(int analyzer, int ctaps, unsigned int M, unsigned int p,
                                          unsigned long long nblocks, int x16, int y16, int signal)
{
    const lqk_pfb_plan none = {LQK_PFB_NONE, 0, 0, 1};
    if (nblocks == 0 || nblocks > (1ull << 40) || M == 0 || M > (1u << 20) || p == 0 || p > (1u << 10)) return none;
    lqk_pfb_plan pl = lqk_pfb_fast_plan(analyzer, ctaps, M, p, nblocks, x16, y16, signal);
    // (a signalling call the few-block kernel does not take goes on as a device call)
    if (pl.route == LQK_PFB_NONE && analyzer && signal)
        pl = lqk_pfb_fast_plan(1, ctaps, M, p, nblocks, x16, y16, 0);
    if (pl.route != LQK_PFB_NONE) return pl;
    return analyzer ? pfb_an_plan(ctaps, M, p, (long long)nblocks) : pfb_syn_plan(ctaps, M, p, (long long)nblocks);
}

extern "C" void lqk_firpfbch_analyzer(int ctaps, unsigned int M, unsigned int p, const void *hsub, const void *hist,
                                      const void *x, unsigned long long nblocks, void *Y, void *stream)
{
    if (nblocks == 0) return;
    if (lqk_firpfbch_analyzer_fast(ctaps, M, p, hsub, hist, x, nblocks, Y, stream)) return;
    if (ctaps)
        pfb_analyzer<float2>((int)M, (int)p, hsub, hist, x, (long long)nblocks, Y, (hipStream_t)stream);
    else
        pfb_analyzer<float>((int)M, (int)p, hsub, hist, x, (long long)nblocks, Y, (hipStream_t)stream);
}

// state: the previous p-1 z vectors; zscratch: (p-1 + nblocks)*M
extern "C" void lqk_firpfbch_synthesizer(int ctaps, unsigned int M, unsigned int p, const void *hsub, void *state,
                                         void *zscratch, const void *X, unsigned long long nblocks, void *y,
                                         void *stream)
{
    if (nblocks == 0) return;
    if (lqk_firpfbch_synthesizer_fast(ctaps, M, p, hsub, state, X, nblocks, y, stream)) return;
    if (ctaps)
        pfb_synthesizer<float2>((int)M, (int)p, hsub, state, zscratch, X, (long long)nblocks, y, (hipStream_t)stream);
    else
        pfb_synthesizer<float>((int)M, (int)p, hsub, state, zscratch, X, (long long)nblocks, y, (hipStream_t)stream);
}
