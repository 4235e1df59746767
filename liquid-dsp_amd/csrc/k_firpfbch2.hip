// k_firpfbch2.hip -- 2x-oversampled polyphase channelizer (firpfbch2),
// analyzer and synthesizer, every size but the M = 1024 fast paths
// (k_pfb2_fast.hip).
//
// Reference semantics restated, not translated:
//  firpfbch2 analyzer  src/multichannel/src/firpfbch2.c:244-282.  The
//    reference pushes M/2 samples per call into M ring buffers and runs M
//    dot products then an M-point IFFT.  Here block b is evaluated from the
//    stream directly (closed form, SURVEY Appendix B, checked numerically):
//        off = (b&1)*M/2,  i = (j - off) mod M
//        c   = j < M/2 ? b>>1 : (b-1)>>1,  base = j < M/2 ? M/2-1-j : 3M/2-1-j
//        X_b[j] = sum_{n<2m} h[i + nM] x[(c-n)M + base]
//        Y_b    = IFFT_backward(X_b) / M
//    so any number of blocks run in parallel; the only state carried between
//    calls is the last 2mM - M/2 input samples and the block parity.
//  firpfbch2 synthesizer firpfbch2.c:287-335: z_b = IFFT(X_b)*(1/M)*(M/2);
//        y_b[i] = sum_n h[i+nM] z_{b-2n}[i+fM/2] + sum_n h[i+M/2+nM] z_{b-1-2n}[i+fM/2]
//    (f = b&1); state = the last 4m-1 z vectors.
#include "lq_device.h"
#include "lq_fft1024.h"
#include "lq_kernels.h"
#include "lq_pfb.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace {

constexpr int NT = 256;

// ------------------------------------------------------------------ firpfbch2 analyzer
// One workgroup = NB consecutive blocks; X for all NB blocks is formed in LDS,
// transformed by the LDS Stockham FFT, scaled and stored coalesced.
template <int M, int NB>
__global__ __launch_bounds__(NT) void k_pfb2_an(int m, const float *__restrict__ hsub,
                                                const float2 *__restrict__ hist, const float2 *__restrict__ x,
                                                long long nblocks, int p0, float2 *__restrict__ Y,
                                                const float2 *__restrict__ tw)
{
    __shared__ __attribute__((aligned(16))) float2 a[NB * M];
    __shared__ __attribute__((aligned(16))) float2 b[NB * M];
    constexpr int M2 = M / 2;
    const int L = 2 * m;
    const int HL = 2 * m * M - M2;
    const long long blk0 = (long long)blockIdx.x * NB;

    for (int e = threadIdx.x; e < NB * M; e += NT) {
        const int bl = e / M;
        const int j = e - bl * M;
        const long long gb = blk0 + bl;
        float2 acc = make_float2(0.f, 0.f);
        if (gb < nblocks) {
            const long long bt = p0 + gb;
            const int off = (int)(bt & 1) * M2;
            const int i = (j - off) & (M - 1);
            const long long c = (j < M2) ? (bt >> 1) : ((bt - 1) >> 1);
            const int base = (j < M2) ? (M2 - 1 - j) : (3 * M2 - 1 - j);
            const long long t0 = c * M + base - (long long)p0 * M2;
            const float *hs = hsub + i * L;
            for (int n = 0; n < L; n++) {
                const float2 v = ext_load(hist, HL, x, t0 - (long long)n * M);
                acc.x = fmaf(hs[n], v.x, acc.x);
                acc.y = fmaf(hs[n], v.y, acc.y);
            }
        }
        a[e] = acc;
    }
    __syncthreads();
    float2 *res = lds_fft<M, NB, NT>(a, b, tw, -1);
    const float inv = 1.0f / (float)M; // exact: M is a power of two
    for (int e = threadIdx.x; e < NB * M; e += NT) {
        const int bl = e / M;
        const long long gb = blk0 + bl;
        if (gb < nblocks) Y[(blk0 + bl) * M + (e - bl * M)] = cscale(res[e], inv);
    }
}

// Polyphase pass for power-of-two M >= 64 (M != 1024, which has the fused
// kernel of k_pfb2_fast.hip), followed by a batched transform over Y in
// place.  Same column view as the fused kernel: in aligned coordinates
// t' = t + p0 M/2 the stream is rows of M samples, column col feeds bin
// j = M/2-1-col (lo) or 3M/2-1-col (hi), and row c completes blocks 2c + dA
// and 2c + dA + 1 (dA = 0 lo, 1 hi) with the L = 2m taps of bin j for the
// even block and of bin j ^ M/2 for the odd one:
//     X_b[j] = sum_n h[i + nM] row[c - n][col]
// A workgroup owns a slice of min(M, 256) columns (one per lane) and a run
// of S rows; L-1 rows before the run warm its register ring up.  Rows are
// read once per slice and run (2 KB coalesced per row and workgroup), a
// group of L rows is prefetched while the previous group is evaluated, and
// X goes straight into Y (coalesced: consecutive columns are consecutive
// bins, reversed), where the batched transform then runs in place.
// Samples come through two range-checked descriptors (history: HL samples,
// x: n_in), each sample in range in at most one of them.
template <int L>
__global__ __launch_bounds__(256) void k_pfb2_poly(int M, int nsl, const float *__restrict__ hsub,
                                                  const float2 *__restrict__ hist, const float2 *__restrict__ x,
                                                  int n_in, int p0, int nb, int cmin, int cmax, int S,
                                                  float2 *__restrict__ Y, const float2 *__restrict__ zero)
{
    const int M2 = M >> 1, HL = L * M - M2;
    const int sl = (int)(blockIdx.x % (unsigned)nsl), seg = (int)(blockIdx.x / (unsigned)nsl);
    const int col = sl * (int)blockDim.x + (int)threadIdx.x;
    const bool lo = col < M2;
    const int j = lo ? (M2 - 1 - col) : (3 * M2 - 1 - col);
    const int dA = lo ? 0 : 1;
    // taps of the first (ta) and second (tb) block a row completes: lo: even
    // block 2c (bin j), odd 2c+1 (j ^ M/2); hi: odd 2c+1, even 2c+2
    float ta[L], tb[L];
    {
        const int ia = lo ? j : (j ^ M2), ib = lo ? (j ^ M2) : j;
#pragma unroll
        for (int n = 0; n < L; n++) {
            ta[n] = hsub[ia * L + n];
            tb[n] = hsub[ib * L + n];
        }
    }
    // Y: nb blocks of M; a store outside (blocks before / after the call) is dropped
    const __amdgpu_buffer_rsrc_t ry =
        __builtin_amdgcn_make_buffer_rsrc((void *)Y, (short)0, nb * M * 8, 0x00020000);
    auto row_sample = [&](int r) -> float2 {
        const int t = r * M + col - p0 * M2;              // stream sample (t < 0: history)
        return lq_load_hx(hist + HL, x, zero, t, HL, n_in);
    };
    auto put = [&](int bt, float2 v) {   // block bt of the aligned numbering, bin j
        const int gb = bt - p0;
        const unsigned off = (gb >= 0 && gb < nb) ? ((unsigned)gb * (unsigned)M + (unsigned)j) * 8u : 0xFFFFFFF0u;
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), ry, off, 0, 0);
    };
    const int cs = cmin + seg * S;
    int ce = cs + S;
    if (ce > cmax + 1) ce = cmax + 1;
    // register ring over groups of L rows: step u of a group puts row
    // r + u into w[u] (the slot of row r + u - L, no longer needed), so row
    // c - n is in w[(u - n) mod L] -- static indices, no moves.  The next
    // group's samples are loaded one per step, L loads in flight.
    float2 w[L], pf[L];
    int r = cs - (L - 1);
#pragma unroll
    for (int u = 0; u < L; u++) pf[u] = row_sample(r + u);
    for (; r < ce; r += L) {
#pragma unroll
        for (int u = 0; u < L; u++) {
            w[u] = pf[u];
            pf[u] = row_sample(r + L + u);
            const int c = r + u;
            if (c >= cs && c < ce) {
                float2 da = make_float2(0.f, 0.f), db = make_float2(0.f, 0.f);
#pragma unroll
                for (int n = 0; n < L; n++) {
                    const float2 v = w[(u - n + L) % L];
                    da.x = fmaf(ta[n], v.x, da.x);
                    da.y = fmaf(ta[n], v.y, da.y);
                    db.x = fmaf(tb[n], v.x, db.x);
                    db.y = fmaf(tb[n], v.y, db.y);
                }
                put(2 * c + dA, da);
                put(2 * c + dA + 1, db);
            }
        }
    }
}

// M = 256 analyzer fused: the polyphase pass above with all 256 columns in
// one workgroup (one per lane), a ring of 8 rows in registers (L = 2m <= 8),
// and each group of 8 rows' 16 completed blocks transformed in the same
// kernel: X goes to a 17-buffer LDS ring (block b in buffer b mod 17; the
// hi half of block 2r0+16 is written one group early), then 16 inverse
// 256-point transforms run in registers (fft_r16x16xR<1>, 16 lanes each) and
// the outputs, times 1/M, leave as consecutive 8-byte stores -- Y is written
// once and never re-read (24 B per input instead of the two-pass 56).
template <int L, int R>
__global__ __launch_bounds__(256 * R, R == 1 ? 2 : 1) void k_pfb2_an256(const float *__restrict__ hsub,
                                                       const float2 *__restrict__ hist,
                                                       const float2 *__restrict__ x, int n_in, int p0, int nb,
                                                       int cmin, int cmax, int S, float2 *__restrict__ Y,
                                                       const float2 *__restrict__ tw4096)
{
    // M = 256 R columns, one per lane; R = 2 takes the tight transform
    // scratch (17 x 4 KB ring + 16 x 4.3 KB scratch fits 160 KB)
    constexpr int M = 256 * R, M2 = M / 2, HL = L * M - M2, NS = 8, NBUF = 17;
    constexpr bool TIGHT = R > 1;
    constexpr int P = FFTR16_LDS<R, TIGHT>();
    __shared__ __attribute__((aligned(16))) float2 xr[NBUF * M];
    __shared__ __attribute__((aligned(16))) float2 scr[16 * P];
    const int col = threadIdx.x;
    const bool lo = col < M2;
    const int j = lo ? (M2 - 1 - col) : (3 * M2 - 1 - col);
    const int dA = lo ? 0 : 1;
    float ta[L], tb[L];
    {
        const int ia = lo ? j : (j ^ M2), ib = lo ? (j ^ M2) : j;
#pragma unroll
        for (int n = 0; n < L; n++) {
            ta[n] = hsub[ia * L + n];
            tb[n] = hsub[ib * L + n];
        }
    }
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)Y, (short)0, nb * M * 8, 0x00020000);
    const float2 *zero = tw4096 + LQ_TW_N;   // lqrt_zeros(): the table's zero tail
    auto row_sample = [&](int r) -> float2 {
        const int t = r * M + col - p0 * M2;
        return lq_load_hx(hist + HL, x, zero, t, HL, n_in);
    };
    auto dot = [&](const float2 (&w)[NS], int newest, const float (&h)[L]) -> float2 {
        float2 acc = make_float2(0.f, 0.f);
#pragma unroll
        for (int n = 0; n < L; n++) {
            const float2 v = w[(newest - n) & (NS - 1)];
            acc.x = fmaf(h[n], v.x, acc.x);
            acc.y = fmaf(h[n], v.y, acc.y);
        }
        return acc;
    };
    auto slot = [](int b) { return ((b % NBUF) + NBUF) % NBUF; };
    const int g = threadIdx.x / (16 * R), t = threadIdx.x % (16 * R);   // transform g (block 2 r0 + g), its lane t
    const tw16x2 w16 = fftr16_tw<R>(tw4096, t);
    const float inv = 1.0f / (float)M;

    const int cs = cmin + (int)blockIdx.x * S;
    int ce = cs + S;
    if (ce > cmax + 1) ce = cmax + 1;
    // rows cs-8 .. cs-1 fill the ring (slots r & 7); the last gives the hi
    // half of block 2cs
    float2 w[NS], pf[NS];
#pragma unroll
    for (int u = 0; u < NS; u++) w[u] = row_sample(cs - NS + u);
    if (!lo) xr[slot(2 * cs) * M + j] = dot(w, NS - 1, tb);
#pragma unroll
    for (int u = 0; u < NS; u++) pf[u] = row_sample(cs + u);
    for (int r0 = cs; r0 < ce; r0 += NS) {
#pragma unroll
        for (int u = 0; u < NS; u++) {
            w[u] = pf[u];
            pf[u] = row_sample(r0 + NS + u);
            const int c = r0 + u;
            xr[slot(2 * c + dA) * M + j] = dot(w, u, ta);
            xr[slot(2 * c + dA + 1) * M + j] = dot(w, u, tb);
        }
        lq_lds_sync();
        // blocks 2 r0 .. 2 r0 + 15 are complete: one transform per 16 lanes
        const int b = 2 * r0 + g;
        float2 v[16];
        const float2 *B = xr + slot(b) * M;
#pragma unroll
        for (int n = 0; n < 16; n++) v[n] = B[t + 16 * R * n];
        fft_r16x16xR<R, -1, TIGHT>(v, scr + g * P, w16, t);   // (its barriers also free the ring buffers)
        const int gb = b - p0;
        const bool keep = gb >= 0 && gb < nb && b < 2 * ce;
        const unsigned base = keep ? (unsigned)gb * (unsigned)(M * 8) : 0xFFFFF000u;
        // v[s R + q] = X[t + 16 R s + 256 q]
#pragma unroll
        for (int sidx = 0; sidx < 16 / R; sidx++)
#pragma unroll
            for (int q = 0; q < R; q++) {
                const float2 vv = v[sidx * R + q];
                const float2 o = make_float2(vv.x * inv, vv.y * inv);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), ry,
                                                      base + (unsigned)(t + 16 * R * sidx + 256 * q) * 8u, 0, 0);
            }
    }
}

template <int L, int R>
void launch_pfb2_an256(const void *hsub, const void *hist, const void *x, long long nb, int p0, void *Y, long long S,
                       long long nseg, hipStream_t st)
{
    constexpr int M = 256 * R;
    const long long n_in = nb * (M / 2);
    const int cmin = (p0 - 1) >> 1;
    const int cmax = (int)((p0 + nb - 1) >> 1);
    hipLaunchKernelGGL((k_pfb2_an256<L, R>), dim3((unsigned)nseg), dim3(256 * R), 0, st, (const float *)hsub,
                       (const float2 *)hist, (const float2 *)x, (int)n_in, p0, (int)nb, cmin, cmax, (int)S,
                       (float2 *)Y, (const float2 *)lqrt_twiddles());
    LQ_CHECK_LAUNCH();
}

// M = 2048 analyzer fused (the two-pass path moved 56 B per input): 1024
// lanes, lane t owning the lo column t (bin j = 1023 - t) and the hi column
// t + 1024 (bin j ^ 1024), so both columns share the lane's two tap sets
// (A: taps of bin j, B: of bin j ^ 1024):
//     lo, row c:  block 2c   += A . column,  block 2c+1 += B . column
//     hi, row c:  block 2c+1 += A . column,  block 2c+2 += B . column
// A group of 4 rows completes 8 blocks into a 9-buffer LDS ring; a block's
// buffer holds its even bins and its odd bins as two 1024-point halves.
// Each of the 16 waves then inverse-transforms one half in registers
// (fft1024_wave_rt: wave-local transposes, no workgroup barrier), and after
// one barrier the wave combines its block's halves for 512 output pairs,
//     Y[k] = E[k] + W_2048^-k O[k],  Y[k + 1024] = E[k] - W_2048^-k O[k],
// times 1/M, stored as 1 KB coalesced rows.  Three barriers per group (a
// 2048-point transform across two waves took six: 1.07 ms per 2^27 samples).
constexpr int A2_HS = 1090;            // half stride: 1088-float2 transform scratch, +2 spreads the halves' banks
constexpr int A2_BSTR = 2 * A2_HS;     // 16-byte aligned halves
template <int L>
__global__ __launch_bounds__(1024, 1) void k_pfb2_an2048(const float *__restrict__ hsub,
                                                         const float2 *__restrict__ hist,
                                                         const float2 *__restrict__ x, int n_in, int p0, int nb,
                                                         int cmin, int cmax, int S, float2 *__restrict__ Y,
                                                         const float2 *__restrict__ tw4096)
{
    constexpr int M = 2048, M2 = 1024, HL = L * M - M2, NS = 8, G = 4, NBUF = 2 * G + 1;
    static_assert(L <= NS, "ring of 8 rows");
    __shared__ __attribute__((aligned(16))) float2 xr[NBUF * A2_BSTR];
    __shared__ __attribute__((aligned(16))) float2 tw2[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) {   // W_64^{-b r} (inverse transform)
        const float2 u = tw4096[(64 * (tid & 3) * (tid >> 2)) & 4095];
        tw2[tid] = make_float2(u.x, -u.y);
    }
    const float2 a1 = tw4096[(4 * lane) & 4095], a4 = tw4096[(16 * lane) & 4095];
    const int jl = M2 - 1 - tid, jh = jl ^ M2;   // bins of the lo / hi column
    // split position of bin j in its block: half j & 1, index j >> 1
    const int pl_lo = (jl & 1) * A2_HS + (jl >> 1), pl_hi = (jh & 1) * A2_HS + (jh >> 1);
    // taps re-read (L1/L2 hits) at every group instead of held across the
    // transforms: 16 VGPRs the ring and the prefetched rows need there
    float ta[L], tb[L];
    auto load_taps = [&]() {
        int oa = jl * L, ob = jh * L;
        asm volatile("" : "+v"(oa), "+v"(ob));   // keep the reload inside the loop
#pragma unroll
        for (int n = 0; n < L; n++) {
            ta[n] = hsub[oa + n];
            tb[n] = hsub[ob + n];
        }
    };
    load_taps();
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)Y, (short)0, nb * M * 8, 0x00020000);
    const float2 *zero = tw4096 + LQ_TW_N;   // lqrt_zeros(): the table's zero tail
    auto row_sample = [&](int r, int col) -> float2 {
        const int t = r * M + col - p0 * M2;
        return lq_load_hx(hist + HL, x, zero, t, HL, n_in);
    };
    auto dot = [&](const float2 (&w)[NS], int newest, const float (&h)[L]) -> float2 {
        float2 acc = make_float2(0.f, 0.f);
#pragma unroll
        for (int n = 0; n < L; n++) {
            const float2 v = w[(newest - n) & (NS - 1)];
            acc.x = fmaf(h[n], v.x, acc.x);
            acc.y = fmaf(h[n], v.y, acc.y);
        }
        return acc;
    };
    auto slot = [](int b) { return ((b % NBUF) + NBUF) % NBUF; };
    const int hb = wave >> 1, hh = wave & 1;   // this wave's block (2 r0 + hb) and half
    const float inv = 1.0f / (float)M;
    typedef float v4f __attribute__((ext_vector_type(4)));

    const int cs = cmin + (int)blockIdx.x * S;
    int ce = cs + S;
    if (ce > cmax + 1) ce = cmax + 1;
    // rows cs-8 .. cs-1 fill the ring (slot r & 7); the last gives the hi
    // half of block 2cs
    float2 wl[NS], wh[NS], pl[G], ph[G];
#pragma unroll
    for (int u = 0; u < NS; u++) {
        wl[u] = row_sample(cs - NS + u, tid);
        wh[u] = row_sample(cs - NS + u, tid + M2);
    }
    xr[slot(2 * cs) * A2_BSTR + pl_hi] = dot(wh, NS - 1, tb);
#pragma unroll
    for (int u = 0; u < G; u++) {
        pl[u] = row_sample(cs + u, tid);
        ph[u] = row_sample(cs + u, tid + M2);
    }
    __syncthreads();   // tw2 ready
    // one group: rows r0 .. r0+3 into ring slots s0 .. s0+3 (s0 = 0 or 4),
    // then the 8 completed blocks' transforms
    auto group = [&](int r0, auto s0c) {
        constexpr int s0 = decltype(s0c)::value;
        load_taps();
#pragma unroll
        for (int u = 0; u < G; u++) {
            wl[s0 + u] = pl[u];
            wh[s0 + u] = ph[u];
            pl[u] = row_sample(r0 + G + u, tid);
            ph[u] = row_sample(r0 + G + u, tid + M2);
            const int c = r0 + u;
            xr[slot(2 * c) * A2_BSTR + pl_lo] = dot(wl, s0 + u, ta);
            xr[slot(2 * c + 1) * A2_BSTR + pl_lo] = dot(wl, s0 + u, tb);
            xr[slot(2 * c + 1) * A2_BSTR + pl_hi] = dot(wh, s0 + u, ta);
            xr[slot(2 * c + 2) * A2_BSTR + pl_hi] = dot(wh, s0 + u, tb);
        }
        lq_lds_sync();
        const int b = 2 * r0 + hb;
        float2 *Bb = xr + slot(b) * A2_BSTR;
        {
            float2 *Bh = Bb + hh * A2_HS;
            float2 v[16];
#pragma unroll
            for (int n = 0; n < 16; n++) v[n] = Bh[lane + 64 * n];
            fft1024_wave_rt<-1>(v, Bh, a1, a4, tw2, lane);   // natural order at k + 4 (k >> 8)
        }
        lq_lds_sync();   // both halves of every block transformed
        const int gb = b - p0;
        const bool keep = gb >= 0 && gb < nb && b < 2 * ce;
        // a dropped block's base: 2^31 (the launch's range is below it, and
        // base + 16 KB cannot wrap around 2^32 into it)
        const unsigned base = keep ? (unsigned)gb * (unsigned)(M * 8) : 0x80000000u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = 512 * hh + 2 * lane + 128 * i;
            const int pos = k + 4 * (k >> 8);
            // W_2048^-k, W_2048^-(k+1) (table hits in L1 / L2)
            const float2 u0 = tw4096[2 * k], u1 = tw4096[2 * k + 2];
            const float2 wk[2] = {make_float2(u0.x, -u0.y), make_float2(u1.x, -u1.y)};
            const v4f E = *reinterpret_cast<const v4f *>(Bb + pos);
            const v4f O = *reinterpret_cast<const v4f *>(Bb + A2_HS + pos);
            const v2f o0 = pk_cmul(v2f{O.x, O.y}, pk(wk[0])), o1 = pk_cmul(v2f{O.z, O.w}, pk(wk[1]));
            const v2f e0 = v2f{E.x, E.y}, e1 = v2f{E.z, E.w};
            const v2f s0v = (e0 + o0) * inv, s1v = (e1 + o1) * inv, d0 = (e0 - o0) * inv, d1 = (e1 - o1) * inv;
            __builtin_amdgcn_raw_buffer_store_b128(v4f{s0v.x, s0v.y, s1v.x, s1v.y}, ry, base + (unsigned)k * 8u, 0, 2);
            __builtin_amdgcn_raw_buffer_store_b128(v4f{d0.x, d0.y, d1.x, d1.y}, ry, base + (unsigned)(k + 1024) * 8u, 0, 2);
        }
        lq_lds_sync();   // the combine's reads are done before the next group's writes
    };
    // S is a multiple of 8 rows: the ring slot of row r0 + u is u (first
    // group) or 4 + u (second)
    for (int r0 = cs; r0 < ce; r0 += 2 * G) {
        group(r0, std::integral_constant<int, 0>{});
        if (r0 + G < ce) group(r0 + G, std::integral_constant<int, G>{});
    }
}

template <int L>
void launch_pfb2_an2048(const void *hsub, const void *hist, const void *x, long long nb, int p0, void *Y, long long S,
                        long long nseg, hipStream_t st)
{
    constexpr int M = 2048;
    const long long n_in = nb * (M / 2);
    const int cmin = (p0 - 1) >> 1;
    const int cmax = (int)((p0 + nb - 1) >> 1);
    hipLaunchKernelGGL((k_pfb2_an2048<L>), dim3((unsigned)nseg), dim3(1024), 0, st, (const float *)hsub,
                       (const float2 *)hist, (const float2 *)x, (int)n_in, p0, (int)nb, cmin, cmax, (int)S,
                       (float2 *)Y, (const float2 *)lqrt_twiddles());
    LQ_CHECK_LAUNCH();
}

// M = 4096 analyzer fused (the two-pass path moved 56 B per input; the
// same structure as k_pfb2_an2048 one size up): lane t owns four columns,
// t + 1024 q.  The lo columns (q = 0, 1: bins j0 = 2047 - t, j1 = 1023 - t)
// and the hi columns (q = 2, 3: bins j0 ^ 2048, j1 ^ 2048) share the lane's
// four tap sets A_q = taps(j_q), B_q = taps(j_q ^ 2048), q = 0, 1:
//     lo q, row c:  block 2c   += A_q . column,  block 2c+1 += B_q . column
//     hi q, row c:  block 2c+1 += A_q . column,  block 2c+2 += B_q . column
// A 32 KB block leaves room for two block buffers, so a group is one row: it
// completes blocks 2c and 2c+1, whose buffers hold the four 1024-point
// quarters of bins j = r (mod 4), and starts 2c+2, whose hi half waits in a
// compact 16 KB carry buffer that each lane copies into the block-2c buffer
// at the next row (its own positions, no barrier).  Waves 0-7
// inverse-transform one quarter each in registers (fft1024_wave_rt), and
// after a barrier all 16 waves combine their block's quarters (radix 4):
//     Y[k + 1024 s] = sum_r W_4096^-(r k) Q_r[k] i^(r s)   (W^- : e^{+2 pi i ...})
// times 1/M, stored as 16-byte rows.  The row ring is shifted in registers,
// its oldest row kept in LDS (8 VGPRs fewer, which m = 4 needs to fit a
// transform beside the ring in 128).
//   Row c+1 reaches an LDS row buffer by LDS-DMA (global_load_lds_dwordx4,
// no VGPRs) right after row c's dot phase and lands during the transforms
// and the combine.  Round 5 loaded row c+1 into registers after row c's
// transforms and crossed three __syncthreads per row (each draining vmcnt):
// one row in flight per CU, 1.106 ms per 2^27 samples; this form 0.869 ms
// (profiles/r06_ab_experiments.txt).  The barriers wait for LDS only.  LDS:
// 2 x 34.9 (blocks) + 16 (carry) + 32 (oldest ring row) + 32 (row) KB.
template <int L>
__global__ __launch_bounds__(1024, 1) void k_pfb2_an4096(const float *__restrict__ hsub,
                                                          const float2 *__restrict__ hist,
                                                          const float2 *__restrict__ x, int n_in, int p0, int nb,
                                                          int cmin, int cmax, int S, float2 *__restrict__ Y,
                                                          const float2 *__restrict__ tw4096)
{
    constexpr int M = 4096, M2 = 2048, HL = L * M - M2, NS = L;
    __shared__ __attribute__((aligned(16))) float2 xb[2 * A4_BSTR];   // blocks 2c, 2c+1
    __shared__ __attribute__((aligned(16))) float2 hc[2048];          // hi half of block 2c+2
    __shared__ __attribute__((aligned(16))) float2 wold[4 * 1024];    // each column's oldest ring row
    __shared__ __attribute__((aligned(16))) float2 rb[4096];          // row c+1 (LDS-DMA)
    __shared__ __attribute__((aligned(16))) float2 tw2[64];
    typedef float v4f __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) {   // W_64^{-b r} (inverse transform)
        const float2 u = tw4096[(64 * (tid & 3) * (tid >> 2)) & 4095];
        tw2[tid] = make_float2(u.x, -u.y);
    }
    const float2 a1 = tw4096[(4 * lane) & 4095], a4 = tw4096[(16 * lane) & 4095];
    const int j0 = M2 - 1 - tid, j1 = M2 / 2 - 1 - tid;   // lo bins; hi bins j ^ M2
    auto qpos = [](int j) { return (j & 3) * A4_QS + (j >> 2); };
    auto hpos = [](int j) { return (j & 3) * 512 + ((j >> 2) - 512); };   // hi bin j in hc
    const int pl0 = qpos(j0), pl1 = qpos(j1), ph0 = qpos(j0 ^ M2), ph1 = qpos(j1 ^ M2);
    const int hc0 = hpos(j0 ^ M2), hc1 = hpos(j1 ^ M2);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)Y, (short)0, nb * M * 8, 0x00020000);
    const float2 *zero = tw4096 + LQ_TW_N;   // lqrt_zeros(): the table's zero tail (256 B)
    auto row_sample = [&](int r, int col) -> float2 {
        const int t = r * M + col - p0 * M2;
        return lq_load_hx(hist + HL, x, zero, t, HL, n_in);
    };
    // row r into rb: lane t's 16 bytes are samples 2 (t + 1024 u) and + 1
    // (HL, n_in and the row starts are even: a pair never straddles the
    // history / x / zero boundary); wave-uniform LDS base per instruction
    auto dma_row = [&](int r) {
        int to = tid;
        asm volatile("" : "+v"(to));   // addresses recomputed per row (not hoisted into live VGPRs)
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const long long t = (long long)r * M + 2 * (to + 1024 * u) - (long long)p0 * M2;
            const bool neg = t < 0;
            const bool in = neg ? (t >= -HL) : (t < n_in);
            unsigned long long a = (unsigned long long)(uintptr_t)(neg ? hist + HL : x) + (unsigned long long)(t * 8);
            a = in ? a : (unsigned long long)(uintptr_t)zero;
            __builtin_amdgcn_global_load_lds((const void *)a,
                                             (__attribute__((address_space(3))) void *)(rb + 2 * (64 * wave + 1024 * u)),
                                             16, 0, 0);
        }
    };
    // rb[tid + 1024 q] through asm: a compiler-visible LDS read of rb would
    // wait for every outstanding vector-memory operation (the DMA's counter
    // is vmcnt) -- the explicit wait before the row's barrier covers it
    auto rb_read = [&](int q) -> float2 {
        const unsigned a = (unsigned)(uintptr_t)(rb + tid);
        v2f v;
        if (q == 0) asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(a));
        if (q == 1) asm volatile("ds_read_b64 %0, %1 offset:8192" : "=v"(v) : "v"(a));
        if (q == 2) asm volatile("ds_read_b64 %0, %1 offset:16384" : "=v"(v) : "v"(a));
        if (q == 3) asm volatile("ds_read_b64 %0, %1 offset:24576" : "=v"(v) : "v"(a));
        return make_float2(v.x, v.y);
    };
    float2 w[4][NS - 1], wo[4];
    auto dot = [&](int q, const float (&h)[NS]) -> float2 {
        float2 acc = make_float2(0.f, 0.f);
#pragma unroll
        for (int n = 0; n < NS; n++) {
            const float2 v = n < NS - 1 ? w[q][NS - 2 - n] : wo[q];
            acc.x = fmaf(h[n], v.x, acc.x);
            acc.y = fmaf(h[n], v.y, acc.y);
        }
        return acc;
    };
    // the lane's four tap sets (A0 = taps(j0), Bt0 = taps(j0 ^ M2), A1, Bt1),
    // re-read (L1 / L2 hits) one set at a time in the dot phase: 8 VGPRs of
    // taps live, not 32 (loaded before the previous row's stores instead, all
    // four sets beside the ring spilled 16 VGPRs)
    float th[NS];
    auto load_set = [&](int j) {
        int o = j * L;
        asm volatile("" : "+v"(o));   // reloaded per row, not hoisted
#pragma unroll
        for (int n = 0; n < NS; n++) th[n] = hsub[o + n];
    };
    const float inv = 1.0f / (float)M;

    const int cs = cmin + (int)blockIdx.x * S;
    int ce = cs + S;
    if (ce > cmax + 1) ce = cmax + 1;
    dma_row(cs);
    // rows cs-NS .. cs-1 fill the ring; the last gives the hi half of block 2cs
#pragma unroll
    for (int q = 0; q < 4; q++) {
        wo[q] = row_sample(cs - NS, tid + 1024 * q);
#pragma unroll
        for (int u = 0; u < NS - 1; u++) w[q][u] = row_sample(cs - NS + 1 + u, tid + 1024 * q);
    }
    load_set(j0 ^ M2);
    hc[hc0] = dot(2, th);
    load_set(j1 ^ M2);
    hc[hc1] = dot(3, th);
    if constexpr (NS > 1) {   // row cs - NS + 1: the oldest of row cs's dots
#pragma unroll
        for (int q = 0; q < 4; q++) wold[q * 1024 + tid] = w[q][0];
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();   // tw2, row cs in rb
    const int qb = wave >> 2, qq = wave & 3;   // transform phase: block 2c + qb, quarter qq (waves 0-7)
    const int cb = wave >> 3, wb = wave & 7;   // combine phase: block 2c + cb, pairs lane + 64 wb
    float2 *B0 = xb, *B1 = xb + A4_BSTR;
    for (int c = cs; c < ce; c++) {
        float2 nr[4];
#pragma unroll
        for (int q = 0; q < 4; q++) nr[q] = rb_read(q);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int q = 0; q < 4; q++) {
            wo[q] = wold[q * 1024 + tid];
            if constexpr (NS > 1) {
#pragma unroll
                for (int u = 0; u < NS - 2; u++) w[q][u] = w[q][u + 1];
                w[q][NS - 2] = nr[q];
            } else {
                wo[q] = nr[q];
            }
        }
        // block 2c's hi half, carried from row c - 1 (this lane's positions)
        B0[ph0] = hc[hc0];
        B0[ph1] = hc[hc1];
        load_set(j0);
        B0[pl0] = dot(0, th);
        B1[ph0] = dot(2, th);
        asm volatile("" ::: "memory");
        load_set(j0 ^ M2);
        B1[pl0] = dot(0, th);
        hc[hc0] = dot(2, th);
        asm volatile("" ::: "memory");
        load_set(j1);
        B0[pl1] = dot(1, th);
        B1[ph1] = dot(3, th);
        asm volatile("" ::: "memory");
        load_set(j1 ^ M2);
        B1[pl1] = dot(1, th);
        hc[hc1] = dot(3, th);
        if constexpr (NS > 1) {
#pragma unroll
            for (int q = 0; q < 4; q++) wold[q * 1024 + tid] = w[q][0];
        }
        lq_lds_sync();   // blocks complete, rb consumed by every wave
        if (c + 1 < ce) dma_row(c + 1);
        if (wave < 8) {
            float2 *Bq = (qb ? B1 : B0) + qq * A4_QS;
            float2 v[16];
#pragma unroll
            for (int n = 0; n < 16; n++) v[n] = Bq[lane + 64 * n];
            fft1024_wave_rt<-1>(v, Bq, a1, a4, tw2, lane);   // natural order at k + 4 (k >> 8)
        }
        lq_lds_sync();   // every quarter of both blocks transformed
        {
            const int b = 2 * c + cb;
            const float2 *Bb = cb ? B1 : B0;
            const int gb = b - p0;
            const bool keep = gb >= 0 && gb < nb && b < 2 * ce;
            const unsigned base = keep ? (unsigned)gb * (unsigned)(M * 8) : 0x80000000u;
            const int k = 2 * (lane + 64 * wb);
            const int pos = k + 4 * (k >> 8);
            v2f T[4][2];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const v4f E = *reinterpret_cast<const v4f *>(Bb + r * A4_QS + pos);
                T[r][0] = v2f{E.x, E.y};
                T[r][1] = v2f{E.z, E.w};
            }
#pragma unroll
            for (int e = 0; e < 2; e++)
#pragma unroll
                for (int r = 1; r < 4; r++) {
                    const float2 u = tw4096[r * (k + e)];
                    T[r][e] = pk_cmul(T[r][e], v2f{u.x, -u.y});
                }
            v2f Yo[4][2];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const v2f s02 = T[0][e] + T[2][e], d02 = T[0][e] - T[2][e];
                const v2f s13 = T[1][e] + T[3][e], d13 = T[1][e] - T[3][e];
                const v2f jd13 = v2f{-d13.y, d13.x};
                Yo[0][e] = (s02 + s13) * inv;
                Yo[1][e] = (d02 + jd13) * inv;
                Yo[2][e] = (s02 - s13) * inv;
                Yo[3][e] = (d02 - jd13) * inv;
            }
#pragma unroll
            for (int sq = 0; sq < 4; sq++)
                __builtin_amdgcn_raw_buffer_store_b128(v4f{Yo[sq][0].x, Yo[sq][0].y, Yo[sq][1].x, Yo[sq][1].y}, ry,
                                                       base + (unsigned)(k + 1024 * sq) * 8u, 0, 2);
        }
        // the DMA has landed; only the four stores may be in flight
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        lq_lds_sync();   // combine reads done; row c+1 in rb for every wave
    }
}

template <int L>
void launch_pfb2_an4096(const void *hsub, const void *hist, const void *x, long long nb, int p0, void *Y, long long S,
                        long long nseg, hipStream_t st)
{
    constexpr int M = 4096;
    const long long n_in = nb * (M / 2);
    const int cmin = (p0 - 1) >> 1;
    const int cmax = (int)((p0 + nb - 1) >> 1);
    hipLaunchKernelGGL((k_pfb2_an4096<L>), dim3((unsigned)nseg), dim3(1024), 0, st, (const float *)hsub,
                       (const float2 *)hist, (const float2 *)x, (int)n_in, p0, (int)nb, cmin, cmax, (int)S,
                       (float2 *)Y, (const float2 *)lqrt_twiddles());
    LQ_CHECK_LAUNCH();
}

// M = 64 / 128 analyzer fused (the two-pass path moved 56 B per input): as
// k_pfb2_an256, with Q = 256 / M column sets per workgroup, each a lane per
// column over its own run of rows (segment blockIdx.x Q + set), and each
// group of 8 rows' 16 blocks per set transformed in registers by R = M / 16
// lanes (fft_small16xR: 16 Q transforms of M points per workgroup, all 256
// lanes).  Every set runs the same number of groups (its stores past its
// rows are dropped), so the barriers stay uniform.
template <int L, int MS>
__global__ __launch_bounds__(256, 2) void k_pfb2_an_small(const float *__restrict__ hsub,
                                                         const float2 *__restrict__ hist,
                                                         const float2 *__restrict__ x, int n_in, int p0, int nb,
                                                         int cmin, int cmax, int S, float2 *__restrict__ Y,
                                                         const float2 *__restrict__ tw4096)
{
    constexpr int M = MS, M2 = M / 2, HL = L * M - M2, NS = 8, NBUF = 17;
    constexpr int Q = 256 / M, R = M / 16, P = FFTS_LDS<R>();
    __shared__ __attribute__((aligned(16))) float2 xr[Q * NBUF * M];
    __shared__ __attribute__((aligned(16))) float2 scr[16 * Q * P];
    const int set = threadIdx.x / M, col = threadIdx.x % M;
    float2 *xs = xr + set * (NBUF * M);
    const bool lo = col < M2;
    const int j = lo ? (M2 - 1 - col) : (3 * M2 - 1 - col);
    const int dA = lo ? 0 : 1;
    float ta[L], tb[L];
    {
        const int ia = lo ? j : (j ^ M2), ib = lo ? (j ^ M2) : j;
#pragma unroll
        for (int n = 0; n < L; n++) {
            ta[n] = hsub[ia * L + n];
            tb[n] = hsub[ib * L + n];
        }
    }
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)Y, (short)0, nb * M * 8, 0x00020000);
    const float2 *zero = tw4096 + LQ_TW_N;   // lqrt_zeros(): the table's zero tail
    auto row_sample = [&](int r) -> float2 {
        const int t = r * M + col - p0 * M2;
        return lq_load_hx(hist + HL, x, zero, t, HL, n_in);
    };
    auto dot = [&](const float2 (&w)[NS], int newest, const float (&h)[L]) -> float2 {
        float2 acc = make_float2(0.f, 0.f);
#pragma unroll
        for (int n = 0; n < L; n++) {
            const float2 v = w[(newest - n) & (NS - 1)];
            acc.x = fmaf(h[n], v.x, acc.x);
            acc.y = fmaf(h[n], v.y, acc.y);
        }
        return acc;
    };
    auto slot = [](int b) { return ((b % NBUF) + NBUF) % NBUF; };
    // transform phase: transform tg = threadIdx.x / R of set tg / 16 (its block
    // 2 r0 + tg % 16), lane t
    const int tg = threadIdx.x / R, t = threadIdx.x % R;
    const int tset = tg / 16, tb16 = tg % 16;
    const int e = t * (4096 / M);
    const float2 a1 = tw4096[e & 4095], a4 = tw4096[(4 * e) & 4095];
    const float inv = 1.0f / (float)M;

    const int seg = (int)blockIdx.x * Q + set;
    const int cs = cmin + seg * S;
    int ce = cs + S;
    if (ce > cmax + 1) ce = cmax + 1;
    // the transform lanes' set (another set's rows)
    const int tcs = cmin + ((int)blockIdx.x * Q + tset) * S;
    int tce = tcs + S;
    if (tce > cmax + 1) tce = cmax + 1;
    float2 w[NS], pf[NS];
#pragma unroll
    for (int u = 0; u < NS; u++) w[u] = row_sample(cs - NS + u);
    if (!lo) xs[slot(2 * cs) * M + j] = dot(w, NS - 1, tb);
#pragma unroll
    for (int u = 0; u < NS; u++) pf[u] = row_sample(cs + u);
    for (int g0 = 0; g0 < S; g0 += NS) {
        const int r0 = cs + g0;
#pragma unroll
        for (int u = 0; u < NS; u++) {
            w[u] = pf[u];
            pf[u] = row_sample(r0 + NS + u);
            const int c = r0 + u;
            xs[slot(2 * c + dA) * M + j] = dot(w, u, ta);
            xs[slot(2 * c + dA + 1) * M + j] = dot(w, u, tb);
        }
        lq_lds_sync();
        // blocks 2 r0 .. 2 r0 + 15 of every set are complete
        const int tr0 = tcs + g0;
        const int b = 2 * tr0 + tb16;
        float2 v[16];
        const float2 *B = xr + tset * (NBUF * M) + slot(b) * M;
#pragma unroll
        for (int n = 0; n < 16; n++) v[n] = B[t + R * n];
        fft_small16xR<R, -1>(v, scr + tg * P, a1, a4, t);   // (its barriers also free the ring buffers)
        const int gb = b - p0;
        const bool keep = gb >= 0 && gb < nb && tr0 < tce;
        const unsigned base = keep ? (unsigned)gb * (unsigned)(M * 8) : 0xFFFFF000u;
        // v[u R + q] = X[t (16/R) + u + 16 q]
#pragma unroll
        for (int u = 0; u < 16 / R; u++)
#pragma unroll
            for (int q = 0; q < R; q++) {
                const float2 vv = v[u * R + q];
                const float2 o = make_float2(vv.x * inv, vv.y * inv);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), ry,
                                                      base + (unsigned)(t * (16 / R) + u + 16 * q) * 8u, 0, 0);
            }
    }
}

template <int L, int MS>
void launch_pfb2_an_small(const void *hsub, const void *hist, const void *x, long long nb, int p0, void *Y,
                          long long S, long long nwg, hipStream_t st)
{
    constexpr int M = MS;
    const long long n_in = nb * (M / 2);
    const int cmin = (p0 - 1) >> 1;
    const int cmax = (int)((p0 + nb - 1) >> 1);
    hipLaunchKernelGGL((k_pfb2_an_small<L, MS>), dim3((unsigned)nwg), dim3(256), 0, st, (const float *)hsub,
                       (const float2 *)hist, (const float2 *)x, (int)n_in, p0, (int)nb, cmin, cmax, (int)S,
                       (float2 *)Y, (const float2 *)lqrt_twiddles());
    LQ_CHECK_LAUNCH();
}

template <int L>
void launch_pfb2_poly(int M, const void *hsub, const void *hist, const void *x, long long nb, int p0, void *Y,
                      long long S, long long nwg, hipStream_t st)
{
    const long long n_in = nb * (M / 2);
    const int cmin = (p0 - 1) >> 1;                            // floor((p0 - 1) / 2)
    const int cmax = (int)((p0 + nb - 1) >> 1);
    const int nt = M < 256 ? M : 256;
    const int nsl = M / nt;
    hipLaunchKernelGGL((k_pfb2_poly<L>), dim3((unsigned)nwg), dim3(nt), 0, st, M, nsl, (const float *)hsub,
                       (const float2 *)hist, (const float2 *)x, (int)n_in, p0, (int)nb, cmin, cmax, (int)S,
                       (float2 *)Y, (const float2 *)lqrt_zeros());
    LQ_CHECK_LAUNCH();
}

// generic even M (not a power of two): direct O(M^2) DFT, one workgroup per block
__global__ __launch_bounds__(NT) void k_pfb2_an_generic(int M, int m, const float *__restrict__ hsub,
                                                        const float2 *__restrict__ hist,
                                                        const float2 *__restrict__ x, long long nblocks, int p0,
                                                        float2 *__restrict__ Y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *X = reinterpret_cast<float2 *>(smem);
    const int M2 = M / 2, L = 2 * m, HL = 2 * m * M - M2;
    const long long gb = blockIdx.x;
    const long long bt = p0 + gb;
    for (int j = threadIdx.x; j < M; j += NT) {
        const int off = (int)(bt & 1) * M2;
        const int i = ((j - off) % M + M) % M;
        const long long c = (j < M2) ? (bt >> 1) : ((bt - 1) >> 1);
        const int base = (j < M2) ? (M2 - 1 - j) : (3 * M2 - 1 - j);
        const long long t0 = c * M + base - (long long)p0 * M2;
        float2 acc = make_float2(0.f, 0.f);
        for (int n = 0; n < L; n++) {
            const float2 v = ext_load(hist, HL, x, t0 - (long long)n * M);
            acc.x = fmaf(hsub[i * L + n], v.x, acc.x);
            acc.y = fmaf(hsub[i * L + n], v.y, acc.y);
        }
        X[j] = acc;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < M; k += NT) {
        float2 acc = make_float2(0.f, 0.f);
        for (int j = 0; j < M; j++) {
            double s, co;
            sincospi(2.0 * (double)(((long long)j * k) % M) / (double)M, &s, &co);
            acc = cadd(acc, cmul(X[j], make_float2((float)co, (float)s)));
        }
        Y[gb * M + k] = make_float2(acc.x / (float)M, acc.y / (float)M);
    }
}

// ------------------------------------------------------------------ firpfbch2 synthesizer output
// Z holds [4m-1 history z vectors | nblocks new z vectors], each M long.
__global__ void k_pfb2_syn_out(int M, int m, const float *__restrict__ hsub, const float2 *__restrict__ Z,
                               long long nblocks, int p0, float2 *__restrict__ y)
{
    const int M2 = M / 2, L = 2 * m, HB = 4 * m - 1;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nblocks * M2) return;
    const long long bl = e / M2;
    const int i = (int)(e - bl * M2);
    const int f = (int)((p0 + bl) & 1);
    const int col = i + f * M2;
    const long long zb = HB + bl; // index of z_b in Z
    float2 acc0 = make_float2(0.f, 0.f), acc1 = make_float2(0.f, 0.f);
    for (int n = 0; n < L; n++) {
        const float h0 = hsub[i * L + n];
        const float h1 = hsub[(i + M2) * L + n];
        const float2 z0 = Z[(zb - 2 * n) * M + col];
        const float2 z1 = Z[(zb - 1 - 2 * n) * M + col];
        acc0.x = fmaf(h0, z0.x, acc0.x);
        acc0.y = fmaf(h0, z0.y, acc0.y);
        acc1.x = fmaf(h1, z1.x, acc1.x);
        acc1.y = fmaf(h1, z1.y, acc1.y);
    }
    y[bl * M2 + i] = cadd(acc0, acc1);
}

// firpfbch2 synthesizer output (firpfbch2.c:287-335): block b (parity f) uses
// column c = i + f M/2: y = sum_n h0[n] z_{b-2n}[c] + h1[n] z_{b-1-2n}[c].
// The lane keeps 2L-deep histories of both of its columns.
template <int L>
__global__ __launch_bounds__(256) void k_pfb2_syn_out_run(int M, const float *__restrict__ hsub,
                                                          const float2 *__restrict__ Z, long long nblocks, int p0,
                                                          float2 *__restrict__ y)
{
    const int M2 = M / 2, HB = 2 * L - 1;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(e % M2);
    const long long b0 = (e / M2) * RUN;
    if (b0 >= nblocks) return;
    float h0[L], h1[L];
#pragma unroll
    for (int n = 0; n < L; n++) {
        h0[n] = hsub[i * L + n];
        h1[n] = hsub[(i + M2) * L + n];
    }
    float2 wa[2 * L], wb[2 * L];   // columns i and i + M/2; w[k] = z_{b-k}
#pragma unroll
    for (int k = 1; k < 2 * L; k++) {
        wa[k] = Z[(HB + b0 - k) * M + i];
        wb[k] = Z[(HB + b0 - k) * M + i + M2];
    }
    const long long be = b0 + RUN < nblocks ? b0 + RUN : nblocks;
    float2 na[RPF], nb2[RPF];   // next RPF transforms' column samples in flight
#pragma unroll
    for (int d = 0; d < RPF; d++) {
        const long long bc = b0 + d < be ? b0 + d : be - 1;
        na[d] = Z[(HB + bc) * M + i];
        nb2[d] = Z[(HB + bc) * M + i + M2];
    }
    for (long long b = b0; b < be; b += RPF) {
#pragma unroll
        for (int d = 0; d < RPF; d++) {
            if (b + d >= be) break;
            wa[0] = na[d];
            wb[0] = nb2[d];
            const long long bn = b + d + RPF < be ? b + d + RPF : be - 1;
            na[d] = Z[(HB + bn) * M + i];
            nb2[d] = Z[(HB + bn) * M + i + M2];
            const bool f = ((p0 + b + d) & 1) != 0;
            float2 acc0 = make_float2(0.f, 0.f), acc1 = make_float2(0.f, 0.f);
#pragma unroll
            for (int n = 0; n < L; n++) {
                const float2 z0 = f ? wb[2 * n] : wa[2 * n];
                const float2 z1 = f ? wb[2 * n + 1] : wa[2 * n + 1];
                acc0.x = fmaf(h0[n], z0.x, acc0.x);
                acc0.y = fmaf(h0[n], z0.y, acc0.y);
                acc1.x = fmaf(h1[n], z1.x, acc1.x);
                acc1.y = fmaf(h1[n], z1.y, acc1.y);
            }
            y[(b + d) * M2 + i] = cadd(acc0, acc1);
#pragma unroll
            for (int k = 2 * L - 1; k > 0; k--) {
                wa[k] = wa[k - 1];
                wb[k] = wb[k - 1];
            }
        }
    }
}

// firpfbch2 synthesizer, M = 256 R, m <= 4, fused the same way: 16 inverse
// transforms per group (scaled 1/M then M/2, as firpfbch2.c:303-307) into
// LDS, then lane i < M/2 keeps 16-deep rings of columns i and i + M/2 and
// emits y_b[i] = sum_n h[i + nM] z_{b-2n}[c] + h[i + M/2 + nM] z_{b-1-2n}[c],
// c = i + f M/2 (f = block parity).
template <int L, int R>
__global__ __launch_bounds__(256 * R, R == 1 ? 2 : 1) void k_pfb2_syn_fused(const float *__restrict__ hsub,
                                                                            const float2 *__restrict__ state,
                                                                            const float2 *__restrict__ X, int nb,
                                                                            int p0, int S, float2 *__restrict__ y,
                                                                            float2 *__restrict__ znew,
                                                                            const float2 *__restrict__ tw4096)
{
    constexpr int M = 256 * R, M2 = M / 2, HB = 2 * L - 1, NS = 16;
    static_assert(2 * L <= NS, "ring too small");
    constexpr bool TIGHT = R > 1;
    constexpr int PS = FFTR16_LDS<R, TIGHT>();
    __shared__ __attribute__((aligned(16))) float2 zr[NS * M];
    __shared__ __attribute__((aligned(16))) float2 scr[16 * PS];
    const int i = threadIdx.x;   // output column (lanes < M/2)
    const bool outl = i < M2;
    float h0[L], h1[L];
#pragma unroll
    for (int n = 0; n < L; n++) {
        h0[n] = outl ? hsub[i * L + n] : 0.f;
        h1[n] = outl ? hsub[(i + M2) * L + n] : 0.f;
    }
    const int g = threadIdx.x / (16 * R), t = threadIdx.x % (16 * R);
    const tw16x2 w16 = fftr16_tw<R>(tw4096, t);
    const float s1 = 1.0f / (float)M, s2 = (float)M2;
    const int cs = (int)blockIdx.x * S;
    const int ce = cs + S < nb ? cs + S : nb;
    float2 wa[NS], wb[NS];
    int r0 = cs;
    if (cs == 0) {
#pragma unroll
        for (int u = 0; u < NS; u++) {
            const int b = u - NS;
            const bool in = b >= -HB && outl;
            wa[u] = in ? state[(HB + b) * M + i] : make_float2(0.f, 0.f);
            wb[u] = in ? state[(HB + b) * M + i + M2] : make_float2(0.f, 0.f);
        }
    } else {
        r0 = cs - NS;
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
                    const float2 z = cscale(cscale(v[sidx * R + q], s1), s2);
                    zb[k] = z;
                    if (b >= nb - HB && b < nb && b >= cs && b < ce) znew[(b - (nb - HB)) * M + k] = z;
                }
        }
        lq_lds_sync();
        if (outl) {
#pragma unroll
            for (int u = 0; u < NS; u++) {
                wa[u] = zr[u * M + i];
                wb[u] = zr[u * M + i + M2];
                const int b = r0 + u;
                const bool f = ((p0 + b) & 1) != 0;
                float2 acc0 = make_float2(0.f, 0.f), acc1 = make_float2(0.f, 0.f);
#pragma unroll
                for (int n = 0; n < L; n++) {
                    const int k0 = (u - 2 * n) & (NS - 1), k1 = (u - 2 * n - 1) & (NS - 1);
                    const float2 z0 = f ? wb[k0] : wa[k0];
                    const float2 z1 = f ? wb[k1] : wa[k1];
                    acc0.x = fmaf(h0[n], z0.x, acc0.x);
                    acc0.y = fmaf(h0[n], z0.y, acc0.y);
                    acc1.x = fmaf(h1[n], z1.x, acc1.x);
                    acc1.y = fmaf(h1[n], z1.y, acc1.y);
                }
                if (b >= cs && b < ce) y[(long long)b * M2 + i] = cadd(acc0, acc1);
            }
        }
        lq_lds_sync();
    }
}

// firpfbch2 synthesizer, M = 4096 fused: the z transforms as in
// k_pfb_syn4096 (quarters of X straight from HBM, radix-4 combine into the
// lane's own columns t + 1024 s, scaled 1/M then M/2 as firpfbch2.c:303-307).
// Output i < M/2 of block b (parity f) is
//     y_b[i] = sum_n h0[n] z_{b-2n}[c] + h1[n] z_{b-1-2n}[c],  c = i + f M/2
// (h0 = h[i + nM], h1 = h[i + M/2 + nM]), so column c only ever feeds the
// outputs of blocks of one parity; a 2L-deep ring of z per column (4 columns
// x 16 x 8 B per lane at m = 4) would not fit, so each column keeps the L
// partial outputs it still feeds instead (transposed form): z_b[c] adds
// h0[j] z_b[c] to the block b + 2j output when b has c's parity (then that
// output is complete and leaves), else h1[j] z_b[c] to block b + 1 + 2j.
template <int L, int G = 3>
__global__ __launch_bounds__(1024, 1) void k_pfb2_syn4096(const float *__restrict__ hsub,
                                                          const float2 *__restrict__ state,
                                                          const float2 *__restrict__ X, int nb, int p0, int S,
                                                          float2 *__restrict__ y, float2 *__restrict__ znew,
                                                          const float2 *__restrict__ tw4096)
{
    constexpr int M = 4096, M2 = 2048, HB = 2 * L - 1;
    constexpr int NW = G * ((HB + G - 1) / G);   // warm-up blocks before a run (whole groups)
    __shared__ __attribute__((aligned(16))) float2 xr[G * A4_BSTR];
    __shared__ __attribute__((aligned(16))) float2 tw2[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) {   // W_64^{-b r} (inverse transform)
        const float2 u = tw4096[(64 * (tid & 3) * (tid >> 2)) & 4095];
        tw2[tid] = make_float2(u.x, -u.y);
    }
    const float2 a1 = tw4096[(4 * lane) & 4095], a4 = tw4096[(16 * lane) & 4095];
    const float s1 = 1.0f / (float)M, s2 = (float)M2;
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)y, (short)0, nb * M2 * 8, 0x00020000);
    const int cs = (int)blockIdx.x * S;
    const int ce = cs + S < nb ? cs + S : nb;
    // column q = t + 1024 q of this lane: q < 2 feeds even-parity blocks
    // (output i = col), q >= 2 odd ones (output i = col - M/2)
    v2f A[4][L];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int j = 0; j < L; j++) A[q][j] = v2f{0.f, 0.f};
    // one z vector (this lane's four columns) of block b into the partial outputs
    auto feed = [&](int b, const v2f (&z)[4], bool emit) {
        const int f = (p0 + b) & 1;
        const bool out = emit && b >= cs && b < ce;
        const unsigned base = out ? (unsigned)b * (unsigned)(M2 * 8) : 0x80000000u;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int fc = q >> 1, i = tid + 1024 * (q & 1);
            // taps h0 (same parity) or h1, re-read per block (L1 / L2 hits)
            int o = (f == fc ? i : i + M2) * L;
            asm volatile("" : "+v"(o));
            const float *h = hsub + o;
#pragma unroll
            for (int j = 0; j < L; j++) A[q][j] = v2f{h[j], h[j]} * z[q] + A[q][j];
            if (f == fc) {
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, A[q][0]), ry, base + (unsigned)i * 8u, 0, 2);
#pragma unroll
                for (int j = 0; j < L - 1; j++) A[q][j] = A[q][j + 1];
                A[q][L - 1] = v2f{0.f, 0.f};
            }
        }
    };
    int b0 = cs;
    if (cs == 0) {   // the state's 2L-1 transforms (blocks -HB .. -1)
        for (int b = -HB; b < 0; b++) {
            v2f z[4];
#pragma unroll
            for (int q = 0; q < 4; q++) z[q] = pk(state[(long long)(HB + b) * M + tid + 1024 * q]);
            feed(b, z, false);
        }
    } else {
        b0 = cs - NW;   // warm-up groups: transformed, outputs dropped
    }
    __syncthreads();   // tw2 ready
    for (; b0 < ce; b0 += G) {
        if (wave < 4 * G) {   // block b0 + wave / 4, quarter wave % 4
            const int g = wave >> 2, rq = wave & 3;
            int b = b0 + g < nb ? b0 + g : nb - 1;
            b = b < 0 ? 0 : b;
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
                v2f z[4] = {s02 + s13, d02 + jd13, s02 - s13, d02 - jd13};   // columns t + 1024 s
#pragma unroll
                for (int q = 0; q < 4; q++) z[q] = (z[q] * s1) * s2;
                if (b < ce && b >= 0) {
                    feed(b, z, true);
                    if (b >= cs && b >= nb - HB) {
#pragma unroll
                        for (int q = 0; q < 4; q++) znew[(long long)(b - (nb - HB)) * M + tid + 1024 * q] = unpk(z[q]);
                    }
                }
            }
        }
        lq_lds_sync();   // the combine's reads are done before the next group's transforms
    }
}

template <int M>
void launch_pfb2_an(int m, const void *hsub, const void *hist, const void *x, long long nblocks, int p0, void *Y,
                    long long grid, hipStream_t st)
{
    constexpr int NB = M >= 1024 ? 1 : 1024 / M;
    hipLaunchKernelGGL((k_pfb2_an<M, NB>), dim3((unsigned)grid), dim3(NT), 0, st, m, (const float *)hsub,
                       (const float2 *)hist, (const float2 *)x, nblocks, p0, (float2 *)Y,
                       (const float2 *)lqrt_twiddles());
    LQ_CHECK_LAUNCH();
}

int is_pow2(unsigned v) { return v && !(v & (v - 1)); }

// Diagnostic switch (DESIGN.md (a) history): LQ_PFB2_TWO_PASS in the
// environment routes the fused sizes through the generic two-pass path.
// Read once per process.
bool pfb2_two_pass()
{
    static const bool v = getenv("LQ_PFB2_TWO_PASS") != nullptr;
    return v;
}

// ------------------------------------------------------------------ what a launch decides
// The launches below and lqk_firpfbch2_plan (the route query) both call
// these.  The workgroup targets N ("about N workgroups on long calls") are
// lqrt_grid(N, N): N itself unless liquid_mi355x_set_max_workgroups has set a
// lower limit, which lengthens the runs (tests only).
long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// runs of S rows, a multiple of 8 and at least 32, over about T workgroups.
// A remainder of a few rows past T full runs goes to one short extra run
// rather than stretching every run to the next multiple of 8 (M = 2048, 2^27
// inputs: 65 537 rows, 256 x 256 + 1 instead of 249 x 264 -- 7 CUs idle)
long long rows_run8(long long rows, long long T, bool extra)
{
    long long S = cdiv(cdiv(rows, T), 8) * 8;
    const long long S8 = rows / (8 * T) * 8;
    if (extra && S8 >= 32 && rows - T * S8 <= S8 / 4) S = S8;
    return S < 32 ? 32 : S;
}

constexpr bool pfb2_direct_size(unsigned M)
{
    return M == 2 || M == 4 || M == 8 || M == 16 || M == 32 || M == 64 || M == 128 || M == 256 || M == 512 ||
           M == 1024 || M == 2048 || M == 4096;
}

// one launch (chunk) of the analyzer at a size with a polyphase form
// (M >= 64 a power of two, 2m <= 16): nb blocks from parity p0.  run is in
// blocks (two per row of the polyphase matrix).
lqk_pfb_plan pfb2_an_chunk(unsigned M, unsigned m, long long nb, int p0)
{
    const lqk_pfb_plan none = {LQK_PFB_NONE, 0, 0, 1};
    const long long n_in = nb * (M / 2);
    if (n_in * 8 >= (1ll << 31) || nb * (long long)M * 8 >= (1ll << 31)) return none;   // 32-bit buffer offsets
    const long long cmin = (p0 - 1) >> 1;                      // floor((p0 - 1) / 2)
    const long long cmax = (p0 + nb - 1) >> 1;
    const long long rows = cmax - cmin + 1;
    const int L = 2 * (int)m;
    // the fused forms (one pass, Y written once), where the size has one
    if (L <= 8 && !pfb2_two_pass()) {
        if (M == 256 || M == 512) {   // about 1024 workgroups on long calls
            const long long S = rows_run8(rows, lqrt_grid(1024, 1024), true);
            return {M == 256 ? LQK_PFB2_AN256 : LQK_PFB2_AN512, 2 * S, cdiv(rows, S), 1};
        }
        if (M == 2048) {              // one workgroup per CU: about 256 runs
            const long long S = rows_run8(rows, lqrt_grid(256, 256), true);
            return {LQK_PFB2_AN2048, 2 * S, cdiv(rows, S), 1};
        }
        if (M == 4096) {              // about 256 runs (each warms up on the 2m rows before it)
            long long S = cdiv(rows, lqrt_grid(256, 256));
            if (S < 32) S = 32;
            return {LQK_PFB2_AN4096, 2 * S, cdiv(rows, S), 1};
        }
        if (M == 64 || M == 128) {
            // runs of S rows per set: about 2048 sets on long calls (no short
            // extra run here: every set of a workgroup runs the same number
            // of groups, so an extra workgroup costs a whole run -- measured
            // 0.83 -> 1.07 ms at M = 64, r05zo)
            const long long S = rows_run8(rows, lqrt_grid(2048, 2048), false);
            return {LQK_PFB2_AN_SMALL, 2 * S, cdiv(cdiv(rows, S), 256 / M), 1};
        }
    }
    // polyphase pass, then the batched transform: runs of S rows, >= 2048
    // workgroups when the call is long, and runs of at least 4L rows so the
    // L-1 warm-up rows stay a small overhead
    const long long nsl = M / 256 ? M / 256 : 1;
    long long S = cdiv(rows * nsl, lqrt_grid(2048, 2048));
    if (S < 4 * L) S = 4 * L;
    return {LQK_PFB2_POLY_FFT, 2 * S, cdiv(rows, S) * nsl, 1};
}

bool pfb2_an_chunked(unsigned M, unsigned m) { return M >= 64 && is_pow2(M) && 2 * m <= 16 && m >= 1; }

// the first chunk's launch and the number of chunks (an even number of blocks
// whose outputs fit 1 GiB: 32-bit buffer offsets)
lqk_pfb_plan pfb2_an_plan(unsigned M, unsigned m, long long nb, int p0, long long *CB)
{
    lqk_pfb_plan pl = {LQK_PFB_NONE, 0, 0, 1};
    if (M < 2 || M % 2 || m < 1 || nb < 1) return pl;
    if (pfb2_an_chunked(M, m)) {
        *CB = lqrt_pfb_chunk((1ll << 27) / M);
        pl = pfb2_an_chunk(M, m, nb < *CB ? nb : *CB, p0);
        pl.chunks = cdiv(nb, *CB);
        return pl;
    }
    if (pfb2_direct_size(M)) {
        const long long NB = M >= 1024 ? 1 : 1024 / M;
        return {LQK_PFB2_DIRECT, NB, cdiv(nb, NB), 1};
    }
    if ((size_t)M * sizeof(float2) > 64 * 1024) return pl;
    return {LQK_PFB2_GENERIC, 1, nb, 1};
}

lqk_pfb_plan pfb2_syn_plan(unsigned M, unsigned m, long long nb)
{
    const lqk_pfb_plan none = {LQK_PFB_NONE, 0, 0, 1};
    if (M < 2 || M % 2 || m < 1 || nb < 1) return none;
    if (!pfb2_two_pass() && M == 4096 && m <= 4 && nb >= 4 * (long long)m - 1 && nb * 4096ll * 8 < (1ll << 31)) {
        long long S = cdiv(nb, lqrt_grid(256, 256));   // about 256 runs (one workgroup per CU), whole groups of three
        S = (S + 2) / 3 * 3;
        if (S < 33) S = 33;
        return {LQK_PFB2_SYN4096, S, cdiv(nb, S), 1};
    }
    if (!pfb2_two_pass() && (M == 256 || M == 512) && m <= 4 && nb >= 16 && nb * (long long)M < (1ll << 31)) {
        long long S = cdiv(cdiv(nb, lqrt_grid(1024, 1024)), 16) * 16;
        if (S < 64) S = 64;
        return {LQK_PFB2_SYN_FUSED, S, cdiv(nb, S), 1};
    }
    // batched transform, then the output filter: a lane per column and run of RUN blocks where 2m has a ring
    if (2 * m == 4 || 2 * m == 6 || 2 * m == 8)
        return {LQK_PFB2_TWO_PASS_RUN, RUN, cdiv((long long)(M / 2) * cdiv(nb, RUN), 256), 1};
    return {LQK_PFB2_TWO_PASS_ELEM, 1, cdiv(nb * (M / 2), 256), 1};
}

const char *const ROUTE_NAMES[LQK_PFB_NROUTES] = {
    "pfb2_an1024", "pfb2_an1024_unpaired", "pfb2_an1024_few", "pfb2_an1024_few_signal", "pfb2_an256", "pfb2_an512",
    "pfb2_an2048", "pfb2_an4096", "pfb2_an_small", "pfb2_poly+fft", "pfb2_direct", "pfb2_generic", "pfb2_syn1024",
    "pfb2_syn_fused", "pfb2_syn4096", "pfb2_two_pass_run", "pfb2_two_pass_elem",
    "pfb_an1024", "pfb_an1024_unpaired", "pfb_an1024_few", "pfb_an1024_few_signal", "pfb_an_fused", "pfb_an_fused_c",
    "pfb_an4096", "pfb_an4096_c", "pfb_an_small", "pfb_an_small_c", "pfb_an_run+fft", "pfb_an_run+fft_c",
    "pfb_an_elem+fft", "pfb_an_elem+fft_c", "pfb_syn1024", "pfb_syn_fused", "pfb_syn_fused_c", "pfb_syn4096",
    "pfb_syn4096_c", "pfb_syn_small", "pfb_syn_small_c", "pfb_fft+syn_run", "pfb_fft+syn_run_c", "pfb_fft+syn_elem",
    "pfb_fft+syn_elem_c"};

} // namespace

extern "C" const char *lqk_pfb_route_name(int route)
{
    return route >= 0 && route < LQK_PFB_NROUTES ? ROUTE_NAMES[route] : nullptr;
}

extern "C" lqk_pfb_plan lqk_firpfbch2_plan(int analyzer, unsigned int M, unsigned int m, unsigned long long nblocks,
                                           int p0, int x16, int y16, int signal)
{
    const lqk_pfb_plan none = {LQK_PFB_NONE, 0, 0, 1};
    if (nblocks == 0 || nblocks > (1ull << 40) || M > (1u << 20) || m > (1u << 10)) return none;
    lqk_pfb_plan pl = lqk_pfb2_fast_plan(analyzer, M, m, nblocks, p0, x16, y16, signal);
    if (pl.route != LQK_PFB_NONE) return pl;
    // (a signalling call the few-block kernel does not take goes on as a device call)
    if (analyzer && signal) pl = lqk_pfb2_fast_plan(1, M, m, nblocks, p0, x16, y16, 0);
    if (pl.route != LQK_PFB_NONE) return pl;
    long long CB = 0;
    return analyzer ? pfb2_an_plan(M, m, (long long)nblocks, p0 & 1, &CB) : pfb2_syn_plan(M, m, (long long)nblocks);
}

extern "C" void lqk_firpfbch2_analyzer(unsigned int M, unsigned int m, const void *hsub, const void *hist,
                                       const void *x, unsigned long long nblocks, int p0, void *Y, void *stream)
{
    if (nblocks == 0) return;
    hipStream_t st = (hipStream_t)stream;
    const long long nb = (long long)nblocks;
    long long CB = 0;
    const lqk_pfb_plan whole = pfb2_an_plan(M, m, nb, p0, &CB);
    if (pfb2_an_chunked(M, m)) {
        // Calls run in chunks of an even number of blocks; a later chunk's
        // history is the input just before it (a chunk spans far more than
        // 2mM samples).  The polyphase pass goes into Y, then the batched
        // inverse transform in place (each transform kernel reads its whole
        // block before writing it).
        const long long M2 = M / 2, HL = 2ll * m * M - M2;
        for (long long b0 = 0; b0 < nb; b0 += CB) {
            const long long nbc = (nb - b0) < CB ? (nb - b0) : CB;
            const float2 *xc = (const float2 *)x + b0 * M2;
            const void *hc = b0 == 0 ? hist : (const void *)(xc - HL);
            float2 *Yc = (float2 *)Y + b0 * M;
            const lqk_pfb_plan pl = pfb2_an_chunk(M, m, nbc, p0);
            const long long S = pl.run / 2, nwg = pl.workgroups;
            if (pl.route == LQK_PFB_NONE) {
                fprintf(stderr, "error: firpfbch2: polyphase pass rejected a %lld-block chunk\n", nbc);
                exit(1);
            }
            if (pl.route == LQK_PFB2_POLY_FFT) {
                lq_switch<2, 4, 6, 8, 10, 12, 14, 16>(
                    2 * m, [&](auto L) { launch_pfb2_poly<L>((int)M, hsub, hc, xc, nbc, p0, Yc, S, nwg, st); });
                lq_fft_batch_scaled(M, -1, Yc, Yc, nbc, 1.0f / (float)M, 1.0f, 1, 0, st);
                continue;
            }
            lq_switch<2, 4, 6, 8>(2 * m, [&](auto L) {
                switch (pl.route) {
                case LQK_PFB2_AN256: launch_pfb2_an256<L, 1>(hsub, hc, xc, nbc, p0, Yc, S, nwg, st); break;
                case LQK_PFB2_AN512: launch_pfb2_an256<L, 2>(hsub, hc, xc, nbc, p0, Yc, S, nwg, st); break;
                case LQK_PFB2_AN2048: launch_pfb2_an2048<L>(hsub, hc, xc, nbc, p0, Yc, S, nwg, st); break;
                case LQK_PFB2_AN4096: launch_pfb2_an4096<L>(hsub, hc, xc, nbc, p0, Yc, S, nwg, st); break;
                default:
                    lq_switch<64, 128>(M, [&](auto MM) {
                        launch_pfb2_an_small<L, MM>(hsub, hc, xc, nbc, p0, Yc, S, nwg, st);
                    });
                }
            });
        }
        return;
    }
    if (whole.route == LQK_PFB2_DIRECT) {
        lq_switch<2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096>(
            M, [&](auto MM) { launch_pfb2_an<MM>(m, hsub, hist, x, nb, p0, Y, whole.workgroups, st); });
        return;
    }
    if (whole.route != LQK_PFB2_GENERIC) {
        fprintf(stderr, "error: firpfbch2: %u channels not supported on the GPU path\n", M);
        exit(1);
    }
    const size_t lds = (size_t)M * sizeof(float2);
    hipLaunchKernelGGL(k_pfb2_an_generic, dim3((unsigned)nb), dim3(NT), lds, st, (int)M, (int)m,
                       (const float *)hsub, (const float2 *)hist, (const float2 *)x, nb, p0, (float2 *)Y);
    LQ_CHECK_LAUNCH();
}

// state: the previous 4m-1 z vectors (M each); zscratch: (4m-1 + nblocks)*M.
extern "C" void lqk_firpfbch2_synthesizer(unsigned int M, unsigned int m, const void *hsub, void *state,
                                          void *zscratch, const void *X, unsigned long long nblocks, int p0,
                                          void *Y, void *stream)
{
    if (nblocks == 0) return;
    if (lqk_firpfbch2_synthesizer_fast(M, m, hsub, state, X, nblocks, p0, Y, stream)) return;
    hipStream_t st = (hipStream_t)stream;
    const long long HB = 4 * (long long)m - 1, nb = (long long)nblocks;
    float2 *Z = (float2 *)zscratch;
    const lqk_pfb_plan pl = pfb2_syn_plan(M, m, nb);
    const unsigned grid = (unsigned)pl.workgroups;
    if (pl.route == LQK_PFB2_SYN4096 || pl.route == LQK_PFB2_SYN_FUSED) {
        // fused: the last 4m-1 transforms land in the scratch, then become the state
        lq_switch<2, 4, 6, 8>(2 * m, [&](auto L) {
            if (pl.route == LQK_PFB2_SYN4096)
                hipLaunchKernelGGL((k_pfb2_syn4096<L>), dim3(grid), dim3(1024), 0, st, (const float *)hsub,
                                   (const float2 *)state, (const float2 *)X, (int)nb, p0, (int)pl.run, (float2 *)Y,
                                   (float2 *)Z, (const float2 *)lqrt_twiddles());
            else
                lq_switch<256, 512>(M, [&](auto MM) {
                    hipLaunchKernelGGL((k_pfb2_syn_fused<L, MM / 256>), dim3(grid), dim3(MM), 0, st,
                                       (const float *)hsub, (const float2 *)state, (const float2 *)X, (int)nb, p0,
                                       (int)pl.run, (float2 *)Y, (float2 *)Z, (const float2 *)lqrt_twiddles());
                });
        });
        LQ_CHECK_LAUNCH();
        LQ_CHECK(hipMemcpyAsync(state, Z, HB * M * sizeof(float2), hipMemcpyDeviceToDevice, st));
        return;
    }
    LQ_CHECK(hipMemcpyAsync(Z, state, HB * M * sizeof(float2), hipMemcpyDeviceToDevice, st));
    lq_fft_batch_scaled(M, -1, X, Z + HB * M, nb, 1.0f / (float)M, (float)(M / 2), 1, 1, st);
    if (pl.route == LQK_PFB2_TWO_PASS_RUN)
        lq_switch<4, 6, 8>(2 * m, [&](auto L) {
            hipLaunchKernelGGL(k_pfb2_syn_out_run<L>, dim3(grid), dim3(256), 0, st, (int)M, (const float *)hsub,
                               (const float2 *)Z, nb, p0, (float2 *)Y);
        });
    else
        hipLaunchKernelGGL(k_pfb2_syn_out, dim3(grid), dim3(256), 0, st, (int)M, (int)m, (const float *)hsub,
                           (const float2 *)Z, nb, p0, (float2 *)Y);
    LQ_CHECK_LAUNCH();
    // keep the newest HB z vectors as the state for the next call
    LQ_CHECK(hipMemcpyAsync(state, Z + nb * M, HB * M * sizeof(float2), hipMemcpyDeviceToDevice, st));
}
