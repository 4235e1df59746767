// k_firdecim.hip -- firdecim: the plain kernel, the phase-layout kernels
// (one-shot and persistent) and the plan that routes a call to one of them.
//
// Reference semantics restated (not translated):
//   firdecim src/filter/src/firdecim.c:189-223 y[o] = sum_k h[k] x[o*M - k]
// Every output is independent: a workgroup stages the inputs of its tile of
// outputs in LDS once (with the hlen-1 sample history before the first tile).
#include "lq_fir.h"
#include "lq_kernels.h"

namespace {

// The plain kernel: one output per lane; LDS tile covers [o0*M - (HP-1), (o0+NT)*M)
template <int KIND>
__global__ __launch_bounds__(NT) void k_firdecim(const typename kt<KIND>::T *__restrict__ hist,
                                                 const typename kt<KIND>::T *__restrict__ x,
                                                 long long nout, int M,
                                                 typename kt<KIND>::T *__restrict__ y,
                                                 const typename kt<KIND>::TC *__restrict__ hpad,
                                                 int HP, int hlen)
{
    typedef typename kt<KIND>::T T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *tile = reinterpret_cast<T *>(smem);
    const long long o0 = (long long)blockIdx.x * NT;
    const long long s0 = o0 * M - (HP - 1);
    const int S = NT * M + HP - 1;
    const long long nin = nout * M;
    for (int u = threadIdx.x; u < S; u += NT) {
        long long s = s0 + u;
        T v;
        if (s < 0) v = hist[HP - 1 + s];
        else if (s < nin) v = x[s];
        else v = zero<T>();
        tile[u] = v;
    }
    __syncthreads();
    const long long o = o0 + threadIdx.x;
    if (o >= nout) return;
    // newest sample of output o is x[o*M] -> tile index (HP-1) + threadIdx.x*M
    const T *w = tile + (HP - 1) + threadIdx.x * M;
    T acc = zero<T>();
    for (int k = 0; k < hlen; k++) mac(acc, hpad[k], w[-k]);
    y[o] = acc;
}

// Phase-layout decimator.  With the filter padded to QC*M taps and split
// k = q*M + r, output o is
//     y[o] = sum_r sum_q hq[r*QC + q] x[(o - q)*M - r],   hq[r*QC + q] = h[q*M + r],
// i.e. M short filters, filter r running over input phase (-r mod M) at the
// output rate.  The workgroup stages its input tile in LDS de-interleaved by
// phase, P[ph][j] = tile[j*M + ph], one padded row per phase; lane t produces
// R consecutive outputs, sliding a QCT+R-1 register window along each phase
// row with the taps wave-uniform (scalar loads), so a phase costs QCT+R-1 LDS
// reads for QCT*R multiply-adds.  Row element j sits at j + (j >> 5): lanes R
// elements apart then spread over all banks.
// Tile: outputs [o0, o0+TO), TO = NT*R; tile sample u = input s0 + u with
// s0 = o0*M - QC*M + 1, u = j*M + ph for j < TO + QC - 1.
__host__ __device__ __forceinline__ int dph_pitch(int J) { return J + (J >> 5) + 1; }
__device__ __forceinline__ int dph_col(int j) { return j + (j >> 5); }

template <int KIND, int QCT, int R, int NT_>
__global__ __launch_bounds__(NT_) void k_firdecim_ph(const typename kt<KIND>::T *__restrict__ hist, int hl1,
                                                     const typename kt<KIND>::T *__restrict__ x, long long nout,
                                                     int M, int QC, typename kt<KIND>::T *__restrict__ y,
                                                     const typename kt<KIND>::TC *__restrict__ hq)
{
    typedef typename kt<KIND>::T T;
    typedef typename kt<KIND>::TC TC;
    constexpr int TO = NT_ * R;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *P = reinterpret_cast<T *>(smem);
    const int J = TO + QC - 1;
    const int pitch = dph_pitch(J);
    const long long o0 = (long long)blockIdx.x * TO;
    const long long nin = nout * M;
    // stage: aligned start s0 - 1 (o0*M and QC*M are multiples of 4), tile
    // sample u = v - 1
    const long long sa = o0 * M - (long long)QC * M;
    const int S = J * M + 1;
    constexpr int VW = 16 / (int)sizeof(T);
    const bool vec_ok = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    for (int v0 = threadIdx.x * VW; v0 < S; v0 += NT_ * VW) {
        const long long s = sa + v0;
        T e[VW];
        if (vec_ok && s >= 0 && s + VW <= nin) {
            load16<T>(x + s, e);
        } else {
#pragma unroll
            for (int i = 0; i < VW; i++) {
                const long long si = s + i;
                T val = zero<T>();
                if (si < 0) {
                    if (si >= -(long long)hl1) val = hist[hl1 + si];
                } else if (si < nin) {
                    val = x[si];
                }
                e[i] = val;
            }
        }
#pragma unroll
        for (int i = 0; i < VW; i++) {
            const int u = v0 + i - 1;
            if (u >= 0 && u < S - 1) {
                const int j = u / M, ph = u - j * M;
                P[ph * pitch + dph_col(j)] = e[i];
            }
        }
    }
    __syncthreads();
    T acc[R];
#pragma unroll
    for (int rr = 0; rr < R; rr++) acc[rr] = zero<T>();
    const int tb = threadIdx.x * R;
    for (int ph = 0; ph < M; ph++) {
        const T *row = P + ph * pitch;
        const TC *hr = hq + (M - 1 - ph) * QC;
        for (int c = 0; c < QC; c += QCT) {
            const int base = tb + QC - c - QCT; // window start of this tap chunk
            T w[QCT + R - 1];
#pragma unroll
            for (int i = 0; i < QCT + R - 1; i++) w[i] = row[dph_col(base + i)];
#pragma unroll
            for (int q = 0; q < QCT; q++) {
                const TC h = hr[c + q];
#pragma unroll
                for (int rr = 0; rr < R; rr++) mac(acc[rr], h, w[QCT - 1 + rr - q]);
            }
        }
    }
    const long long o = o0 + tb;
#pragma unroll
    for (int rr = 0; rr < R; rr++)
        if (o + rr < nout) y[o + rr] = acc[rr];
}

// Phase-layout decimator, second form: R consecutive outputs per lane (R =
// 2 as launched) and taps in chunks of four (QC a multiple of 4 instead of
// 4/8/16/32: the M = 8, m = 8 filter has 17 taps per phase, padded to 20
// rather than 32).  Each phase row is stored de-interleaved by R (column j
// at (j mod R) Q + j / R), so the window reads of a wave -- lanes R outputs
// apart -- are consecutive (conflict-free) and a lane's R + 3 window samples
// per tap chunk serve 4 R multiply-adds.  The staging issues four 16-byte
// loads per lane before any LDS store and divides by M with a float
// reciprocal and an exact integer correction.
template <int R>
__host__ __device__ __forceinline__ int dph2_q(int J) { return (J + R - 1) / R + 1; }   // 1/R-row stride (+1 pad)

constexpr int DNU = 4;   // staging loads in flight per lane (8 and 12 measured the same)

template <int KIND, int R, int NT_>
__global__ __launch_bounds__(NT_) void k_firdecim_ph2(const typename kt<KIND>::T *__restrict__ hist, int hl1,
                                                      const typename kt<KIND>::T *__restrict__ x, long long nout,
                                                      int M, int QC, typename kt<KIND>::T *__restrict__ y,
                                                      const typename kt<KIND>::TC *__restrict__ hq)
{
    typedef typename kt<KIND>::T T;
    typedef typename kt<KIND>::TC TC;
    constexpr int TO = NT_ * R;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *P = reinterpret_cast<T *>(smem);
    const int J = TO + QC - 1;
    const int QR = dph2_q<R>(J), pitch = R * QR + 1;
    const long long o0 = (long long)blockIdx.x * TO;
    const long long nin = nout * M;
    const long long sa = o0 * M - (long long)QC * M;
    const int S = J * M + 1;
    const float rM = 1.0f / (float)M;
    constexpr int VW = 16 / (int)sizeof(T);
    const bool vec_ok = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    auto put = [&](int v0, const T (&e)[VW]) {
#pragma unroll
        for (int i = 0; i < VW; i++) {
            const int u = v0 + i - 1;
            if (u >= 0 && u < S - 1) {
                int j = (int)((float)u * rM);   // u < 2^24: off by at most one
                j -= (j * M > u) ? 1 : 0;
                j += ((j + 1) * M <= u) ? 1 : 0;
                const int ph = u - j * M;
                P[ph * pitch + (j % R) * QR + j / R] = e[i];
            }
        }
    };
    if (vec_ok && nin * (long long)sizeof(T) < (1ll << 31)) {
        // four 16-byte loads per lane in flight at a time through a
        // range-checked descriptor (zeros outside x; sa is a multiple of VW,
        // so a vector never straddles x's start); the history only reaches
        // the first tile
        typedef float v4f_ __attribute__((ext_vector_type(4)));
        const __amdgpu_buffer_rsrc_t rx =
            __builtin_amdgcn_make_buffer_rsrc((void *)x, (short)0, (int)(nin * (long long)sizeof(T)), 0x00020000);
        for (int vb = threadIdx.x * VW; vb < S; vb += DNU * NT_ * VW) {
            T e[DNU][VW];
#pragma unroll
            for (int k = 0; k < DNU; k++) {
                const long long sk = sa + vb + k * NT_ * VW;
                const unsigned off = (unsigned)(sk * (long long)sizeof(T));
                unpack16(__builtin_bit_cast(v4f_, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0)), e[k]);
            }
            if (sa < 0) {   // first tile: samples before the call come from the history
#pragma unroll
                for (int k = 0; k < DNU; k++)
#pragma unroll
                    for (int i = 0; i < VW; i++) {
                        const long long si = sa + vb + k * NT_ * VW + i;
                        if (si < 0 && si >= -(long long)hl1) e[k][i] = hist[hl1 + si];
                    }
            }
#pragma unroll
            for (int k = 0; k < DNU; k++) {
                const int v0 = vb + k * NT_ * VW;
                if (v0 < S) put(v0, e[k]);
            }
        }
    } else {
        for (int v0 = threadIdx.x * VW; v0 < S; v0 += NT_ * VW) {
            const long long s = sa + v0;
            T e[VW];
#pragma unroll
            for (int i = 0; i < VW; i++) {
                const long long si = s + i;
                T val = zero<T>();
                if (si < 0) {
                    if (si >= -(long long)hl1) val = hist[hl1 + si];
                } else if (si < nin) {
                    val = x[si];
                }
                e[i] = val;
            }
            put(v0, e);
        }
    }
    __syncthreads();
    T acc[R];
#pragma unroll
    for (int rr = 0; rr < R; rr++) acc[rr] = zero<T>();
    const int tb = threadIdx.x * R;
    for (int ph = 0; ph < M; ph++) {
        const T *row = P + ph * pitch;
        const TC *hr = hq + (M - 1 - ph) * QC;
        for (int c = 0; c < QC; c += 4) {
            // window columns tb + QC - c - 4 + i, i < R + 3; the base is a
            // multiple of R, so column base + i sits at (i % R) QR + base/R + i/R
            const int bR = (tb + QC - c - 4) / R;
            T w[R + 3];
#pragma unroll
            for (int i = 0; i < R + 3; i++) w[i] = row[(i % R) * QR + bR + i / R];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const TC h = hr[c + q];
#pragma unroll
                for (int rr = 0; rr < R; rr++) mac(acc[rr], h, w[3 + rr - q]);
            }
        }
    }
    const long long o = o0 + tb;
#pragma unroll
    for (int rr = 0; rr < R; rr++)
        if (o + rr < nout) y[o + rr] = acc[rr];
}

// Persistent form of k_firdecim_ph2: each workgroup walks tiles blockIdx.x,
// + gridDim.x, ..., and the next tile's NL 16-byte vectors per lane are
// loaded into registers as soon as this tile's are in LDS, so they are in
// flight during this tile's multiply-adds and stores (the one-shot form
// stages, waits, then computes: its loads and its arithmetic never overlap
// within a workgroup).  16-byte aligned x only.
template <int KIND, int R, int NT_, int NL>
__global__ __launch_bounds__(NT_) void k_firdecim_pf(const typename kt<KIND>::T *__restrict__ hist, int hl1,
                                                     const typename kt<KIND>::T *__restrict__ x, long long nout,
                                                     int M, int QC, typename kt<KIND>::T *__restrict__ y,
                                                     const typename kt<KIND>::TC *__restrict__ hq)
{
    typedef typename kt<KIND>::T T;
    typedef typename kt<KIND>::TC TC;
    typedef float v4f_ __attribute__((ext_vector_type(4)));
    constexpr int TO = NT_ * R;
    constexpr int VW = 16 / (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *P = reinterpret_cast<T *>(smem);
    const int J = TO + QC - 1;
    const int QR = dph2_q<R>(J), pitch = R * QR + 1;
    const long long nin = nout * M;
    const int S = J * M + 1;
    const float rM = 1.0f / (float)M;
    const long long ntiles = (nout + TO - 1) / TO;
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc((void *)x, (short)0, (int)(nin * (long long)sizeof(T)), 0x00020000);
    auto load = [&](long long t, v4f_ (&e)[NL]) {
        const long long sa = t * TO * M - (long long)QC * M;
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const long long sk = sa + (threadIdx.x + k * NT_) * VW;
            const unsigned off = (t < ntiles && sk < nin) ? (unsigned)(sk * (long long)sizeof(T)) : 0xFFFFFFF0u;
            e[k] = __builtin_bit_cast(v4f_, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
        }
    };
    v4f_ e[NL];
    long long t = blockIdx.x;
    if (t >= ntiles) return;
    load(t, e);
    for (; t < ntiles; t += gridDim.x) {
        const long long o0 = t * TO;
        const long long sa = o0 * M - (long long)QC * M;
        __syncthreads();   // the previous tile's window reads are done
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const int v0 = (threadIdx.x + k * NT_) * VW;
            T ev[VW];   // by hand: unpack16 here costs the complex NL = 5 kernels 26 instructions
            if constexpr (VW == 2) {
                ev[0] = make_float2(e[k].x, e[k].y);
                ev[1] = make_float2(e[k].z, e[k].w);
            } else {
                ev[0] = e[k].x;
                ev[1] = e[k].y;
                ev[2] = e[k].z;
                ev[3] = e[k].w;
            }
            if (sa < 0) {   // first tile: samples before the call come from the history
#pragma unroll
                for (int i = 0; i < VW; i++) {
                    const long long si = sa + v0 + i;
                    if (si < 0) ev[i] = si >= -(long long)hl1 ? hist[hl1 + si] : zero<T>();
                }
            }
#pragma unroll
            for (int i = 0; i < VW; i++) {
                const int u = v0 + i - 1;
                if (u >= 0 && u < S - 1) {
                    int j = (int)((float)u * rM);   // u < 2^24: off by at most one
                    j -= (j * M > u) ? 1 : 0;
                    j += ((j + 1) * M <= u) ? 1 : 0;
                    const int ph = u - j * M;
                    P[ph * pitch + (j % R) * QR + j / R] = ev[i];
                }
            }
        }
        if (t + gridDim.x < ntiles) load(t + gridDim.x, e);
        __syncthreads();
        T acc[R];
#pragma unroll
        for (int rr = 0; rr < R; rr++) acc[rr] = zero<T>();
        const int tb = threadIdx.x * R;
        for (int ph = 0; ph < M; ph++) {
            const T *row = P + ph * pitch;
            const TC *hr = hq + (M - 1 - ph) * QC;
            for (int c = 0; c < QC; c += 4) {
                const int bR = (tb + QC - c - 4) / R;
                T w[R + 3];
#pragma unroll
                for (int i = 0; i < R + 3; i++) w[i] = row[(i % R) * QR + bR + i / R];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const TC h = hr[c + q];
#pragma unroll
                    for (int rr = 0; rr < R; rr++) mac(acc[rr], h, w[3 + rr - q]);
                }
            }
        }
        const long long o = o0 + tb;
#pragma unroll
        for (int rr = 0; rr < R; rr++)
            if (o + rr < nout) y[o + rr] = acc[rr];
    }
}

// dynamic LDS of the plain k_firdecim: NT outputs' inputs and HP taps' history
size_t decim_plain_lds(int kind, unsigned M, unsigned HP) { return ((size_t)NT * M + HP) * elem_size(kind); }

} // namespace

extern "C" void lqk_firdecim(int kind, unsigned int hlen, const void *hpad, unsigned int M, const void *hist,
                             const void *x, unsigned long long nout, void *y, void *stream)
{
    if (nout == 0) return;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = (unsigned)((nout + NT - 1) / NT);
    const size_t lds = decim_plain_lds(kind, M, hlen);
    if (lds > FIR_LDS_MAX) {
        fprintf(stderr, "error: firdecim: decimation/filter length exceeds the GPU tile limit\n");
        exit(1);
    }
    fir_kind(kind, [&](auto k) {
        typedef typename kt<k>::T T;
        typedef typename kt<k>::TC TC;
        // the taps are not padded: the history length HP is hlen
        hipLaunchKernelGGL(k_firdecim<k>, dim3(nb), dim3(NT), lds, st, (const T *)hist, (const T *)x,
                           (long long)nout, (int)M, (T *)y, (const TC *)hpad, (int)hlen, (int)hlen);
    });
    LQ_CHECK_LAUNCH();
}

extern "C" unsigned lqk_firdecim_ph_qc(unsigned M, unsigned hlen)
{
    const unsigned q0 = (hlen + M - 1) / M;
    return (q0 + 3) / 4 * 4;   // k_firdecim_ph2 runs taps in chunks of four
}

namespace {
// lanes and outputs per lane of each route's workgroup, by LQK_DECIM_*: what
// decim_decide sizes a tile by, what the launches instantiate, and what
// lqk_firdecim_route_tile reports
struct decim_geom {
    int r, nt;
};
constexpr decim_geom DECIM_GEOM[LQK_DECIM_REFUSED] = {{4, 128}, {2, 256}, {2, 256}, {1, 256}, {1, 64}, {1, NT}};
constexpr int decim_tile(int route) { return DECIM_GEOM[route].r * DECIM_GEOM[route].nt; }

// Where a call goes, and the launch arithmetic of that route: the one decision
// behind lqk_firdecim_route and lqk_firdecim_ph's launches.
struct decim_plan {
    int route;       // LQK_DECIM_*
    size_t lds;      // dynamic LDS of the launch
    int nl;          // persistent form: 16-byte vectors per lane and tile
    unsigned cap;    // persistent form: the grid cap, 256 wpc; else 0
};

// The persistent prefetching form (k_firdecim_pf) for 16-byte aligned x: R
// outputs per lane on NTD lanes, TO = R NTD outputs and (TO + QC - 1) M input
// samples per workgroup in LDS; false when the shape does not fit it
template <int ROUTE>
bool decim_pf_fits(int kind, unsigned M, unsigned QC, bool x16, unsigned long long nout, decim_plan *p)
{
    constexpr int R = DECIM_GEOM[ROUTE].r, NTD = DECIM_GEOM[ROUTE].nt;
    const int J = decim_tile(ROUTE) + (int)QC - 1;
    const size_t lds = (size_t)M * (R * dph2_q<R>(J) + 1) * elem_size(kind);
    if (!((QC % 4) == 0 && lds <= 40 * 1024 && (unsigned long long)(J) * M < (1u << 24) && x16 &&
          nout * M * elem_size(kind) < (1ull << 31)))
        return false;
    const int S = J * (int)M + 1;
    const int vw = 16 / (int)elem_size(kind);
    const int nl = (S + NTD * vw - 1) / (NTD * vw);
    if (nl > 12) return false;
    const int wpc = (int)((160 * 1024) / lds) < 8 ? (int)((160 * 1024) / lds) : 8;
    *p = decim_plan{ROUTE, lds, nl, 256u * (unsigned)wpc};
    return true;
}

decim_plan decim_decide(int kind, unsigned M, unsigned QC, unsigned hlen, bool x16, unsigned long long nout)
{
    decim_plan p{LQK_DECIM_REFUSED, 0, 0, 0};
    // the persistent form: at M = 8 (m = 8 crcf, 2^27 inputs: 0.304-0.333 ->
    // 0.283-0.286 ms against the one-shot form, r05zf) two outputs per lane
    // on 256 lanes (four per lane on 128: 0.271 -> 0.36 ms); at small M, where
    // the outputs are many and each is M (QC / 4)(R + 3) / R window reads,
    // four per lane on 128 lanes (M = 2 / 3 / 4: 0.468 / 0.337 / 0.303 ->
    // 0.333 / 0.303 / 0.266 ms, r06fd)
    if (M <= 4 ? decim_pf_fits<LQK_DECIM_PF_R4X128>(kind, M, QC, x16, nout, &p)
               : decim_pf_fits<LQK_DECIM_PF_R2X256>(kind, M, QC, x16, nout, &p))
        return p;
    {
        // one-shot form: 512 outputs per workgroup, two per lane, 256 lanes
        constexpr int R = DECIM_GEOM[LQK_DECIM_PH2].r;
        const int J = decim_tile(LQK_DECIM_PH2) + (int)QC - 1;
        const size_t lds = (size_t)M * (R * dph2_q<R>(J) + 1) * elem_size(kind);
        if ((QC % 4) == 0 && lds <= 64 * 1024 && (unsigned long long)(J) * M < (1u << 24))
            return decim_plan{LQK_DECIM_PH2, lds, 0, 0u};
    }
    // longer spans (M >= 16 at 2 M m taps): the persistent form on 256-output
    // tiles, one output per lane (M = 16 m = 8: 0.479 -> 0.308 ms; at M = 12
    // the one-shot form above is faster, 0.306 vs 0.366, r06fd)
    if (decim_pf_fits<LQK_DECIM_PF_R1X256>(kind, M, QC, x16, nout, &p)) return p;
    {
        // 64 outputs per workgroup.  (A 512-output tile of this layout,
        // M dph_pitch(511 + QC) elements, is never the choice: whenever it is
        // within 64 KB the one-shot form above, M (515 + QC) at most, is too.)
        const size_t lds = (size_t)M * dph_pitch(decim_tile(LQK_DECIM_PH_R1X64) + (int)QC - 1) * elem_size(kind);
        if ((QC % 4) == 0 && lds <= FIR_LDS_MAX) return decim_plan{LQK_DECIM_PH_R1X64, lds, 0, 0u};
    }
    // the plain kernel's tile, 256 M + hlen samples, is the smaller one only
    // past about 6000 taps per unit of M (dph_pitch pads a row by 1/32)
    const size_t lds = decim_plain_lds(kind, M, hlen);
    if (lds <= FIR_LDS_MAX) return decim_plan{LQK_DECIM_PLAIN, lds, 0, 0u};
    return p;
}
} // namespace

extern "C" int lqk_firdecim_route(int kind, unsigned int M, unsigned int hlen, int x_aligned16,
                                  unsigned long long nout)
{
    if (kind < 0 || kind > 2 || M == 0 || hlen == 0) return LQK_DECIM_REFUSED;
    return decim_decide(kind, M, lqk_firdecim_ph_qc(M, hlen), hlen, x_aligned16 != 0, nout).route;
}

extern "C" unsigned int lqk_firdecim_route_tile(int route)
{
    return route >= 0 && route < LQK_DECIM_REFUSED ? (unsigned)decim_tile(route) : 0;
}

extern "C" unsigned int lqk_firdecim_route_cap(int kind, unsigned int M, unsigned int hlen, int route)
{
    // the plan of a one-output aligned call, which is the route's persistent
    // form wherever that form fits the shape at all
    if (kind < 0 || kind > 2 || M == 0 || hlen == 0) return 0;
    const decim_plan p = decim_decide(kind, M, lqk_firdecim_ph_qc(M, hlen), hlen, true, 1);
    return p.route == route ? p.cap : 0;
}

extern "C" int lqk_firdecim_ph(int kind, unsigned int M, unsigned int QC, const void *hq, unsigned int hl1,
                               const void *hist, const void *x, unsigned long long nout, void *y, void *stream)
{
    if (nout == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const decim_plan p = decim_decide(kind, M, QC, hl1 + 1, ((uintptr_t)x & 15) == 0, nout);
    if (p.route >= LQK_DECIM_PLAIN) return -1;   // the plain kernel or none: lqk_firdecim launches or refuses
    // one workgroup per tile, or the persistent form's capped grid
    const unsigned long long nt = (nout + decim_tile(p.route) - 1) / decim_tile(p.route);
    const unsigned nb = p.cap ? lqrt_grid(nt, p.cap) : (unsigned)nt;
    // k_firdecim_pf's prefetch depth by class; k_firdecim_ph's tap chunk by QC
    // (the plan has checked QC % 4 == 0 and the LDS need)
    const int nlc = p.nl <= 5 ? 5 : p.nl <= 9 ? 9 : 12;
    const int qct = (QC == 4 || QC == 8 || QC == 16 || QC == 32) ? (int)QC : QC % 16 == 0 ? 16 : 4;
    fir_kind(kind, [&](auto k) {
        typedef typename kt<k>::T T;
        typedef typename kt<k>::TC TC;
        // the three phase-layout kernels take the same arguments
        auto go = [&](auto kernel, int lanes) {
            hipLaunchKernelGGL(kernel, dim3(nb), dim3(lanes), p.lds, st, (const T *)hist, (int)hl1, (const T *)x,
                               (long long)nout, (int)M, (int)QC, (T *)y, (const TC *)hq);
        };
        lq_switch<LQK_DECIM_PF_R4X128, LQK_DECIM_PF_R2X256, LQK_DECIM_PF_R1X256>(p.route, [&](auto r) {
            constexpr decim_geom g = DECIM_GEOM[r];
            lq_switch<5, 9, 12>(nlc, [&](auto nl) { go(k_firdecim_pf<k, g.r, g.nt, nl>, g.nt); });
        });
        constexpr decim_geom g2 = DECIM_GEOM[LQK_DECIM_PH2], g1 = DECIM_GEOM[LQK_DECIM_PH_R1X64];
        if (p.route == LQK_DECIM_PH2) go(k_firdecim_ph2<k, g2.r, g2.nt>, g2.nt);
        if (p.route == LQK_DECIM_PH_R1X64)
            lq_switch<4, 8, 16, 32>(qct, [&](auto q) { go(k_firdecim_ph<k, q, g1.r, g1.nt>, g1.nt); });
    });
    LQ_CHECK_LAUNCH();
    return 0;
}
