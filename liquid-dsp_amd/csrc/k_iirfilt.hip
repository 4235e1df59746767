// k_iirfilt.hip -- iirfilt (src/filter/src/iirfilt.c, iirfiltsos.c) over a
// block of samples: a cascade of up to 8 direct-form-II second-order sections,
// run block-parallel because the recurrence is linear.
//
// Write s for the cascade's state, P = 2 nsec values (v[1], v[2] of every
// section, section 0 first).  Over any span of samples
//     s_end = z + G s_start,
// z the end state the span reaches from zero state and G = A^len the
// homogeneous map of the span (A one sample's).  So spans run in parallel from
// zero state and only their P-vectors are combined serially:
//   lane    RUN consecutive samples, serial through all sections
//   tile    NT lanes: a scan over the lanes' z with G_R = A^RUN
//   block   LQK_IIRFILT_SCAN tiles (or chunks of tiles): the same scan over
//           per-tile vectors with G_R^NT (G_R^(NT SCAN))
// Every scan is the routine block_scan below.  The host builds the ladder
// L[k] = G_R^(2^k), k < LQK_IIRFILT_LEVELS, in float64 and stores it in
// float32; a scan whose step is G_R^(2^b) uses L[b .. b+6].  A is block lower
// triangular (section k feeds only sections after it), and so is every power.
//
// Three stages, separate launches in stream order; no workgroup ever waits
// on another:
//   1 k_iir_tile   every full tile but the last: z of the tile
//   2 k_iir_scan   the tiles' start states from the z's and the object's state
//                  (one launch up to SCAN tiles, else reduce per chunk / scan
//                  the chunk totals / scan within the chunks)
//   3 k_iir_apply  every tile again, from its true start state: writes y; the
//                  last tile's end state becomes the object's state
// Stage 3 reads x a second time: 24 B of traffic per crcf sample against 16
// algorithmic.  A call of at most one tile is stage 3 alone.
//
// Global loads and stores are 16 bytes per lane, consecutive across lanes; a
// tile goes through LDS, where lane l's run is the row l of RUN samples plus
// 16 bytes of padding: the row stride is 20 or 36 dwords, so the 16 lanes that
// one ds_read_b128 serves together land on 16 different 4-bank slots.  A tile
// is read whole before any of it is written and nothing outside the tile is
// touched, so y == x is allowed.
//
// The two rate changers (iirdecim.c, iirinterp.c: the full-rate filter with
// M-1 of every M outputs dropped, or M-1 zeros fed per input) are the same
// three stages with another tile input or output, chosen by the template
// parameter MODE of k_iir_tile and k_iir_apply:
//   DECIM   stage 3 writes only the tile's samples whose full-rate index is a
//           multiple of M, read from the LDS rows (stride M: bank conflicts
//           that depend on M) and stored by consecutive lanes to consecutive
//           outputs.  y is 1/M the size of x, so y == x is not allowed.
//   INTERP  a tile is TILE output samples; stages 1 and 3 zero the LDS rows
//           and place the inputs i with base <= i M < base + nvalid at row
//           position i M - base.  The stuffed stream is never in memory.
// A long call is cut into pieces of a multiple of M full-rate samples, so a
// piece starts on a kept sample (an input sample) and the phase within a
// piece is the full-rate index modulo M.
#include <hip/hip_runtime.h>

#include "lq_device.h"
#include "lq_kernels.h"

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int RUN = LQK_IIRFILT_RUN;
constexpr int TILE = NT * RUN;
static_assert(TILE == LQK_IIRFILT_TILE, "tile size is part of the interface (tests cut blocks at it)");
static_assert(NT == LQK_IIRFILT_SCAN, "a scan block takes one vector per lane");
static_assert(NT == 256 && RUN == 16, "ladder levels below assume 2^4 samples per lane, 2^8 lanes");
enum { PLAIN = 0, DECIM = 1, INTERP = 2 };
constexpr int LV_TILE = 0;    // step G_R: lanes of a tile
constexpr int LV_SCAN = 8;    // step G_R^256: tiles of a chunk
constexpr int LV_TOP = 16;    // step G_R^65536: chunks of a piece
static_assert(LV_TOP + 7 == LQK_IIRFILT_LEVELS, "ladder length");

template <int KIND> struct iir_t { using S = float2; using K = float; };
template <> struct iir_t<0> { using S = float; using K = float; };
template <> struct iir_t<2> { using S = float2; using K = float2; };

#define DI __device__ __forceinline__
DI float iadd(float a, float b) { return a + b; }
DI float2 iadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
DI float isub(float a, float b) { return a - b; }
DI float2 isub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
DI float imul(float k, float s) { return k * s; }
DI float2 imul(float k, float2 s) { return make_float2(k * s.x, k * s.y); }
DI float2 imul(float2 k, float2 s) { return make_float2(k.x * s.x - k.y * s.y, k.x * s.y + k.y * s.x); }
DI float ishfl_up(float v, int d) { return __shfl_up(v, d, 64); }
DI float2 ishfl_up(float2 v, int d) { return make_float2(__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64)); }
template <class S> DI S izero();
template <> DI float izero<float>() { return 0.0f; }
template <> DI float2 izero<float2>() { return make_float2(0.0f, 0.0f); }

// out = M u over the first P rows, M row-major with row stride PM and block
// lower triangular: row r has columns below 2 (r/2 + 1)
template <int PM, class S, class K>
DI void matvec(S (&out)[PM], const K *__restrict__ M, const S (&u)[PM], int P)
{
#pragma unroll
    for (int r = 0; r < PM; r++) {
        S a = izero<S>();
        if (r < P) {
#pragma unroll
            for (int c = 0; c < 2 * (r / 2 + 1); c++) a = iadd(a, imul(M[r * PM + c], u[c]));
        }
        out[r] = a;
    }
}

// The scan over the NT lanes of a workgroup.  In: v = the zero-state end
// state of the lane's span, carry = the state before lane 0's span (uniform),
// lad = L[b..]: lad[k] steps 2^k lanes.  Out: total = the state after the
// last lane's span (uniform) and, if want_start, v = the state before the
// lane's own span.  wt: NW * PM values of LDS; one barrier.
template <int PM, class S, class K>
DI void block_scan(S (&v)[PM], const S (&carry)[PM], const K *__restrict__ lad, int P, S *wt, S (&total)[PM],
                   bool want_start)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // inclusive scan within the wave: v = sum_{j <= lane} G^(lane-j) z_j
#pragma unroll
    for (int k = 0; k < 6; k++) {
        S u[PM], a[PM];
#pragma unroll
        for (int r = 0; r < PM; r++) u[r] = ishfl_up(v[r], 1 << k);
        matvec<PM>(a, lad + k * PM * PM, u, P);
        if (lane >= (1 << k)) {
#pragma unroll
            for (int r = 0; r < PM; r++) v[r] = iadd(v[r], a[r]);
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int r = 0; r < PM; r++) wt[w * PM + r] = v[r];
    }
    __syncthreads();
    // the waves in turn: s = the state before wave ww
    S s[PM], mine[PM];
#pragma unroll
    for (int r = 0; r < PM; r++) mine[r] = s[r] = carry[r];
#pragma unroll
    for (int ww = 0; ww < NW; ww++) {
        if (ww == w) {
#pragma unroll
            for (int r = 0; r < PM; r++) mine[r] = s[r];
        }
        S a[PM];
        matvec<PM>(a, lad + 6 * PM * PM, s, P);
#pragma unroll
        for (int r = 0; r < PM; r++) s[r] = iadd(wt[ww * PM + r], a[r]);
    }
#pragma unroll
    for (int r = 0; r < PM; r++) total[r] = s[r];
    if (!want_start) return;
    // h = G^lane mine, by the bits of lane
#pragma unroll
    for (int k = 0; k < 6; k++) {
        S a[PM];
        matvec<PM>(a, lad + k * PM * PM, mine, P);
        if (lane & (1 << k)) {
#pragma unroll
            for (int r = 0; r < PM; r++) mine[r] = a[r];
        }
    }
#pragma unroll
    for (int r = 0; r < PM; r++) {
        S e = ishfl_up(v[r], 1);
        if (lane == 0) e = izero<S>();
        v[r] = iadd(e, mine[r]);
    }
}

// one sample through one section (iirfiltsos.c:167-184, execute_df2); c =
// b0, b1, b2, a1, a2 and (s0, s1) = (v[1], v[2]) of the coming sample
template <class S, class K> DI S sos_step(const K (&c)[5], S x, S &s0, S &s1)
{
    const S v0 = isub(isub(x, imul(c[3], s0)), imul(c[4], s1));
    const S y = iadd(iadd(imul(c[0], v0), imul(c[1], s0)), imul(c[2], s1));
    s1 = s0;
    s0 = v0;
    return y;
}

// the lane's first cnt samples through the cascade, from state st
template <int MS, bool WRITE, class S, class K>
DI void run_lane(const K *__restrict__ coef, int nsec, S (&x)[RUN], S (&st)[2 * MS], int cnt)
{
    K c[MS][5];
#pragma unroll
    for (int k = 0; k < MS; k++) {
#pragma unroll
        for (int i = 0; i < 5; i++) c[k][i] = coef[k < nsec ? 5 * k + i : 0];
    }
#pragma unroll
    for (int j = 0; j < RUN; j++) {
        if (j < cnt) {
            S t = x[j];
#pragma unroll
            for (int k = 0; k < MS; k++) {
                if (k < nsec) t = sos_step(c[k], t, st[2 * k], st[2 * k + 1]);
            }
            if (WRITE) x[j] = t;
        }
    }
}

template <class S> struct tile_io {
    static constexpr int W = sizeof(S) / 4;     // dwords per sample
    static constexpr int RW = RUN * W;          // dwords per lane run
    static constexpr int ROW = RW + 4;          // LDS row stride
    static constexpr int IT = TILE * W / 4 / NT;   // 16-byte pieces per lane
    static constexpr int LDS = NT * ROW;

    // the tile's first nvalid samples from x into the rows (zeros beyond)
    static DI void load(const S *x, int nvalid, bool vec, float *lds)
    {
        const float *xf = reinterpret_cast<const float *>(x);
        const int nd = nvalid * W, t = threadIdx.x;
        float4 v[IT];
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const int d = 4 * (it * NT + t);
            if (vec && d + 4 <= nd) {
                v[it] = *reinterpret_cast<const float4 *>(xf + d);
            } else {
                v[it].x = d < nd ? xf[d] : 0.0f;
                v[it].y = d + 1 < nd ? xf[d + 1] : 0.0f;
                v[it].z = d + 2 < nd ? xf[d + 2] : 0.0f;
                v[it].w = d + 3 < nd ? xf[d + 3] : 0.0f;
            }
        }
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const int d = 4 * (it * NT + t);
            *reinterpret_cast<float4 *>(lds + d + (d / RW) * 4) = v[it];
        }
    }

    static DI void store(S *y, int nvalid, bool vec, const float *lds)
    {
        float *yf = reinterpret_cast<float *>(y);
        const int nd = nvalid * W, t = threadIdx.x;
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const int d = 4 * (it * NT + t);
            const float4 v = *reinterpret_cast<const float4 *>(lds + d + (d / RW) * 4);
            if (vec && d + 4 <= nd) {
                *reinterpret_cast<float4 *>(yf + d) = v;
            } else {
                if (d < nd) yf[d] = v.x;
                if (d + 1 < nd) yf[d + 1] = v.y;
                if (d + 2 < nd) yf[d + 2] = v.z;
                if (d + 3 < nd) yf[d + 3] = v.w;
            }
        }
    }

    // INTERP: the tile's first nvalid full-rate samples, base the full-rate index
    // of the first, of the input x stuffed with M - 1 zeros per sample
    static DI void load_stuffed(const S *x, long long base, int nvalid, int M, float *lds)
    {
        const int t = threadIdx.x;
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const int d = 4 * (it * NT + t);
            *reinterpret_cast<float4 *>(lds + d + (d / RW) * 4) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        __syncthreads();
        const long long i0 = (base + M - 1) / M, i1 = (base + nvalid - 1) / M;   // inputs i0 .. i1
        const int cnt = i1 >= i0 ? (int)(i1 - i0 + 1) : 0, pos0 = (int)(i0 * M - base);
        for (int k = t; k < cnt; k += NT) {
            const int d = (pos0 + k * M) * W;
            unpack(x[i0 + k], lds + d + (d / RW) * 4);
        }
    }

    // DECIM: the tile's samples at full-rate indices that are multiples of M
    // (base the index of the tile's first) to y[index / M]
    static DI void store_kept(S *y, long long base, int nvalid, int M, const float *lds)
    {
        const int j0 = (int)((M - base % M) % M);
        const int cnt = j0 < nvalid ? (nvalid - j0 - 1) / M + 1 : 0;
        S *y0 = y + (base + j0) / M;
        for (int k = threadIdx.x; k < cnt; k += NT) {
            const int d = (j0 + k * M) * W;
            y0[k] = pack(lds + d + (d / RW) * 4);
        }
    }

    static DI void get_run(const float *lds, S (&x)[RUN])
    {
        const float4 *p = reinterpret_cast<const float4 *>(lds + threadIdx.x * ROW);
        float f[RW];
#pragma unroll
        for (int i = 0; i < RW / 4; i++) {
            const float4 v = p[i];
            f[4 * i] = v.x, f[4 * i + 1] = v.y, f[4 * i + 2] = v.z, f[4 * i + 3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < RUN; j++) x[j] = pack(f + j * W);
    }

    static DI void put_run(float *lds, const S (&x)[RUN])
    {
        float4 *p = reinterpret_cast<float4 *>(lds + threadIdx.x * ROW);
        float f[RW];
#pragma unroll
        for (int j = 0; j < RUN; j++) unpack(x[j], f + j * W);
#pragma unroll
        for (int i = 0; i < RW / 4; i++) p[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
    }

    static DI S pack(const float *f)
    {
        if constexpr (W == 1) return f[0];
        else return make_float2(f[0], f[1]);
    }
    static DI void unpack(S v, float *f)
    {
        if constexpr (W == 1) f[0] = v;
        else f[0] = v.x, f[1] = v.y;
    }
};

// stage 1: z[tile] for the full tiles blockIdx.x (INTERP: x is the input
// before stuffing by M)
template <int KIND, int MS, int MODE>
__global__ __launch_bounds__(NT) void k_iir_tile(const typename iir_t<KIND>::K *__restrict__ coef, int nsec,
                                                 const typename iir_t<KIND>::K *__restrict__ lad,
                                                 const typename iir_t<KIND>::S *x, int vec,
                                                 typename iir_t<KIND>::S *__restrict__ z, int M)
{
    using S = typename iir_t<KIND>::S;
    using IO = tile_io<S>;
    constexpr int PM = 2 * MS;
    __shared__ __attribute__((aligned(16))) float lds[IO::LDS];
    __shared__ S wt[NW * PM];
    const int P = 2 * nsec;
    if constexpr (MODE == INTERP) IO::load_stuffed(x, (long long)blockIdx.x * TILE, TILE, M, lds);
    else IO::load(x + (size_t)blockIdx.x * TILE, TILE, vec != 0, lds);
    __syncthreads();
    S xr[RUN], st[PM], carry[PM], total[PM];
    IO::get_run(lds, xr);
#pragma unroll
    for (int r = 0; r < PM; r++) st[r] = carry[r] = izero<S>();
    run_lane<MS, false>(coef, nsec, xr, st, RUN);
    block_scan<PM>(st, carry, lad + LV_TILE * PM * PM, P, wt, total, false);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < PM; r++) z[(size_t)blockIdx.x * PM + r] = total[r];
    }
}

// stage 3: tile blockIdx.x of the n samples from start[tile] to y; the last
// tile leaves the state after sample n-1 in state_out (start may be state_out
// when there is one tile: every lane has read it before the barrier in
// block_scan, the writer stores after it).  n counts full-rate samples: DECIM
// writes the n / M kept ones, INTERP reads n / M inputs.
template <int KIND, int MS, int MODE>
__global__ __launch_bounds__(NT) void k_iir_apply(const typename iir_t<KIND>::K *__restrict__ coef, int nsec,
                                                  const typename iir_t<KIND>::K *__restrict__ lad,
                                                  const typename iir_t<KIND>::S *x, long long n, int vec,
                                                  const typename iir_t<KIND>::S *start, int start_stride,
                                                  typename iir_t<KIND>::S *y, typename iir_t<KIND>::S *state_out,
                                                  int M)
{
    using S = typename iir_t<KIND>::S;
    using IO = tile_io<S>;
    constexpr int PM = 2 * MS;
    __shared__ __attribute__((aligned(16))) float lds[IO::LDS];
    __shared__ S wt[NW * PM];
    const int P = 2 * nsec, t = threadIdx.x;
    const long long base = (long long)blockIdx.x * TILE;
    const int nvalid = n - base < TILE ? (int)(n - base) : TILE;
    if constexpr (MODE == INTERP) IO::load_stuffed(x, base, nvalid, M, lds);
    else IO::load(x + base, nvalid, vec != 0, lds);
    S carry[PM];
#pragma unroll
    for (int r = 0; r < PM; r++) carry[r] = r < P ? start[(size_t)blockIdx.x * start_stride + r] : izero<S>();
    __syncthreads();
    S xr[RUN], st[PM], total[PM];
    IO::get_run(lds, xr);
    int cnt = nvalid - t * RUN;
    cnt = cnt < 0 ? 0 : (cnt > RUN ? RUN : cnt);
#pragma unroll
    for (int r = 0; r < PM; r++) st[r] = izero<S>();
    run_lane<MS, false>(coef, nsec, xr, st, cnt);
    block_scan<PM>(st, carry, lad + LV_TILE * PM * PM, P, wt, total, true);
    run_lane<MS, true>(coef, nsec, xr, st, cnt);
    IO::put_run(lds, xr);
    if (base + nvalid == n && t == (nvalid - 1) / RUN) {
#pragma unroll
        for (int r = 0; r < PM; r++) {
            if (r < P) state_out[r] = st[r];
        }
    }
    __syncthreads();
    if constexpr (MODE == DECIM) IO::store_kept(y, base, nvalid, M, lds);
    else IO::store(y + base, nvalid, vec != 0, lds);
}

// stage 2: block b scans the vectors z[256 b + lane] (zero from nz on) from
// the state carry[b] (zero if null); writes the state before each of the
// first nout vectors to start (if given) and the state after the block's 256
// to total[b] (if given).  Vectors are PM apart; carry may be the object's
// state (one block).
template <int KIND, int MS>
__global__ __launch_bounds__(NT) void k_iir_scan(const typename iir_t<KIND>::K *__restrict__ lad, int nsec,
                                                 const typename iir_t<KIND>::S *__restrict__ z, long long nz,
                                                 const typename iir_t<KIND>::S *__restrict__ carry_in,
                                                 typename iir_t<KIND>::S *__restrict__ start, long long nout,
                                                 typename iir_t<KIND>::S *__restrict__ total_out)
{
    using S = typename iir_t<KIND>::S;
    constexpr int PM = 2 * MS;
    __shared__ S wt[NW * PM];
    const int P = 2 * nsec;
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    S v[PM], carry[PM], total[PM];
#pragma unroll
    for (int r = 0; r < PM; r++) {
        v[r] = (e < nz && r < P) ? z[e * PM + r] : izero<S>();
        carry[r] = (carry_in != nullptr && r < P) ? carry_in[(size_t)blockIdx.x * PM + r] : izero<S>();
    }
    block_scan<PM>(v, carry, lad, P, wt, total, start != nullptr);
    if (start != nullptr && e < nout) {
#pragma unroll
        for (int r = 0; r < PM; r++) start[e * PM + r] = v[r];
    }
    if (total_out != nullptr && threadIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < PM; r++) total_out[(size_t)blockIdx.x * PM + r] = total[r];
    }
}

constexpr unsigned long long PIECE = (unsigned long long)TILE * NT * NT;   // samples per three-stage pass

// n full-rate samples; vec: the 16-byte global accesses of the mode (DECIM
// loads, INTERP stores, PLAIN both) are aligned
template <int KIND, int MS, int MODE>
void run_piece(unsigned int nsec, const void *coef_, const void *lad_, void *state_, const void *x_,
               unsigned long long n, int M, void *y_, void *work, hipStream_t st)
{
    using S = typename iir_t<KIND>::S;
    using K = typename iir_t<KIND>::K;
    constexpr int PM = 2 * MS;
    const K *coef = (const K *)coef_, *lad = (const K *)lad_;
    S *state = (S *)state_, *y = (S *)y_;
    const S *x = (const S *)x_;
    const int vec = (((MODE == INTERP ? 0 : (uintptr_t)x_) | (MODE == DECIM ? 0 : (uintptr_t)y_)) & 15) == 0;
    const long long ntiles = (long long)((n + TILE - 1) / TILE);
    const int route = lqk_iirfilt_route(n);
    if (route == 0) {
        hipLaunchKernelGGL((k_iir_apply<KIND, MS, MODE>), dim3(1), dim3(NT), 0, st, coef, (int)nsec, lad, x,
                           (long long)n, vec, (const S *)state, 0, y, state, M);
        LQ_CHECK_LAUNCH();
        return;
    }
    const long long nch = (ntiles + NT - 1) / NT;
    S *z = (S *)work, *start = z + ntiles * PM, *ctot = start + ntiles * PM, *cstart = ctot + nch * PM;
    hipLaunchKernelGGL((k_iir_tile<KIND, MS, MODE == INTERP ? INTERP : PLAIN>), dim3((unsigned)(ntiles - 1)), dim3(NT),
                       0, st, coef, (int)nsec, lad, x, vec, z, M);
    LQ_CHECK_LAUNCH();
    if (route == 1) {
        hipLaunchKernelGGL((k_iir_scan<KIND, MS>), dim3(1), dim3(NT), 0, st, lad + LV_SCAN * PM * PM, (int)nsec,
                           (const S *)z, ntiles - 1, (const S *)state, start, ntiles, (S *)nullptr);
        LQ_CHECK_LAUNCH();
    } else {
        hipLaunchKernelGGL((k_iir_scan<KIND, MS>), dim3((unsigned)nch), dim3(NT), 0, st, lad + LV_SCAN * PM * PM,
                           (int)nsec, (const S *)z, ntiles - 1, (const S *)nullptr, (S *)nullptr, 0LL, ctot);
        LQ_CHECK_LAUNCH();
        hipLaunchKernelGGL((k_iir_scan<KIND, MS>), dim3(1), dim3(NT), 0, st, lad + LV_TOP * PM * PM, (int)nsec,
                           (const S *)ctot, nch - 1, (const S *)state, cstart, nch, (S *)nullptr);
        LQ_CHECK_LAUNCH();
        hipLaunchKernelGGL((k_iir_scan<KIND, MS>), dim3((unsigned)nch), dim3(NT), 0, st, lad + LV_SCAN * PM * PM,
                           (int)nsec, (const S *)z, ntiles - 1, (const S *)cstart, start, ntiles, (S *)nullptr);
        LQ_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL((k_iir_apply<KIND, MS, MODE>), dim3((unsigned)ntiles), dim3(NT), 0, st, coef, (int)nsec, lad,
                       x, (long long)n, vec, (const S *)start, PM, y, state, M);
    LQ_CHECK_LAUNCH();
}

// n full-rate samples in pieces of at most PIECE, a multiple of M each
template <int MODE>
void run_all(int kind, unsigned int nsec, const void *coef, const void *ladder, void *state, const void *x,
             unsigned long long n, unsigned int M, void *y, void *work, void *stream, const char *who)
{
    hipStream_t st = (hipStream_t)stream;
    const size_t esz = kind == 0 ? 4 : 8;
    if (M == 0 || M > PIECE) lq_check(hipErrorInvalidValue, who, __FILE__, __LINE__);
    const unsigned long long piece = PIECE / M * M;
    for (unsigned long long i = 0; i < n; i += piece) {
        const unsigned long long m = n - i < piece ? n - i : piece;
        const void *xi = (const char *)x + (MODE == INTERP ? i / M : i) * esz;
        void *yi = (char *)y + (MODE == DECIM ? i / M : i) * esz;
        const bool ok = lq_switch<1, 2, 4, 8>((int)lqk_iirfilt_maxsec(nsec), [&](auto ms) {
            constexpr int MS = decltype(ms)::value;
            lq_switch<0, 1, 2>(kind, [&](auto k) {
                run_piece<k, MS, MODE>(nsec, coef, ladder, state, xi, m, (int)M, yi, work, st);
            });
        });
        if (!ok) lq_check(hipErrorInvalidValue, who, __FILE__, __LINE__);
    }
}

} // namespace

extern "C" unsigned int lqk_iirfilt_maxsec(unsigned int nsec)
{
    unsigned int ms = 1;
    while (ms < nsec) ms *= 2;
    return ms;
}

// the launch structure of a piece of n full-rate samples (a longer call: of
// its full pieces): 0 k_iir_apply alone, 1 one k_iir_scan launch between the
// tile and apply stages, 2 three (reduce per chunk / scan the chunk totals /
// scan within the chunks)
extern "C" int lqk_iirfilt_route(unsigned long long n)
{
    if (n > PIECE) n = PIECE;
    const unsigned long long ntiles = (n + TILE - 1) / TILE;
    return ntiles <= 1 ? 0 : ntiles <= NT ? 1 : 2;
}

extern "C" size_t lqk_iirfilt_work_bytes(int kind, unsigned int nsec, unsigned long long n)
{
    if (n > PIECE) n = PIECE;
    const size_t ntiles = (size_t)((n + TILE - 1) / TILE), nch = (ntiles + NT - 1) / NT;
    const size_t vecb = 2 * lqk_iirfilt_maxsec(nsec) * (kind == 0 ? 4 : 8);
    return ntiles <= 1 ? 0 : 2 * (ntiles + nch) * vecb;
}

extern "C" void lqk_iirfilt(int kind, unsigned int nsec, const void *coef, const void *ladder, void *state,
                            const void *x, unsigned long long n, void *y, void *work, void *stream)
{
    run_all<PLAIN>(kind, nsec, coef, ladder, state, x, n, 1, y, work, stream, "lqk_iirfilt: more than 8 sections");
}

extern "C" void lqk_iirfilt_decim(int kind, unsigned int nsec, const void *coef, const void *ladder, void *state,
                                  const void *x, unsigned long long n_in, unsigned int M, void *y, void *work,
                                  void *stream)
{
    if (M > LQK_IIRFILT_TILE || n_in % (M ? M : 1) != 0)
        lq_check(hipErrorInvalidValue, "lqk_iirfilt_decim: M above the tile size, or n_in not a multiple of M", __FILE__,
                 __LINE__);
    run_all<DECIM>(kind, nsec, coef, ladder, state, x, n_in, M, y, work, stream,
                   "lqk_iirfilt_decim: more than 8 sections, or M = 0");
}

extern "C" void lqk_iirfilt_interp(int kind, unsigned int nsec, const void *coef, const void *ladder, void *state,
                                   const void *x, unsigned long long n_in, unsigned int M, void *y, void *work,
                                   void *stream)
{
    if (M > LQK_IIRFILT_TILE)
        lq_check(hipErrorInvalidValue, "lqk_iirfilt_interp: M above the tile size", __FILE__, __LINE__);
    run_all<INTERP>(kind, nsec, coef, ladder, state, x, n_in * M, M, y, work, stream,
                    "lqk_iirfilt_interp: more than 8 sections, or M = 0");
}
