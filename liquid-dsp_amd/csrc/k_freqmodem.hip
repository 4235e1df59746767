// k_freqmodem.hip -- freqmod / freqdem block calls (src/modem/src/freqmod.c,
// freqdem.c), both of which the reference runs as a per-sample loop.
//
// freqmod.  The state is a 16-bit phase accumulator advanced per sample by
// (int)roundf(ref * m[i]) modulo 2^16 (freqmod.c:112-113); the output is entry
// ((phase + 0x20) >> 6) & 0x3ff of a 1024-entry table.  Integer addition modulo
// 2^16 is associative, so a prefix sum gives the reference's accumulator bit for
// bit.  Three launches in stream order, no workgroup ever waits on another:
//
//   sums   one workgroup per full tile of LQK_FREQMOD_TILE samples but the
//          last: the tile's sum of increments (kept modulo 2^32);
//   scan   one workgroup walks the tile sums in passes of LQK_FREQMOD_PASS
//          tiles and leaves, in place, each tile's starting accumulator: the
//          object's accumulator plus the sums before it;
//   mod    one workgroup per tile: lane t takes the RUN = 8 consecutive samples
//          t*8 .. t*8+7 (two 16-byte loads), scans them, the wave scans the lane
//          totals with lane shifts, the four wave totals cross in LDS; the
//          table indices go through LDS (lane stride 9 words, as in k_nco.hip)
//          and the lanes change roles: lane t stores sample pairs
//          (j*256 + t)*2 with one 16-byte store each, table values read from an
//          LDS copy.  The lane that holds the call's last sample writes the new
//          accumulator.
// A call of at most one tile is `mod` alone, started from the accumulator.
//
// freqdem.  m[i] = arg(conj(r[i-M]) r[i]) * ref, M the number of interleaved
// channels (1: the reference's object); samples before the call come from the
// history of the last M samples.  Two geometries:
//
//   flat   M < LQK_FREQDEM_SWITCH: a workgroup stages its tile of
//          LQK_FREQDEM_TILE samples and the M before it in LDS (16-byte loads)
//          and every lane reads its neighbour at lag M from there;
//   cols   M >= LQK_FREQDEM_SWITCH: a workgroup takes 256 adjacent channels
//          and LQK_FREQDEM_FRAMES frames; a lane walks the frames of its own
//          channel with the previous sample in a register, so a sample is read
//          once (plus one frame of halo per walk), a wave's loads are 512
//          contiguous bytes and its stores 256.
// Both then write, grid-strided, the last M samples of (history ++ input) as
// the new history.  The product is the float32 one the host forms
// (re = a c + b d, im = a d - b c, four rounded products); its argument is
// taken in float64 and rounded once, then multiplied by ref: the device
// library's float32 atan2 is documented more loosely than the bound the tests
// hold, and the kernel is bound by memory.
#include <cstdio>
#include <cstdlib>

#include "lq_device.h"

// ref * m is one rounded multiply and the discriminator's products are
// separately rounded, as on the host (compiled with -ffp-contract=off)
#pragma clang fp contract(off)

namespace {

constexpr int NT = 256, NW = NT / 64;
constexpr unsigned TILE = LQK_FREQMOD_TILE, PASS = LQK_FREQMOD_PASS;
constexpr int RUN = TILE / NT, PRUN = PASS / NT;
static_assert(RUN == 8 && PRUN >= 1 && PASS % NT == 0, "runs of 8 samples (two 16-byte loads, the LDS padding)");

// the increment of one sample, modulo 2^32: roundf rounds halves away from
// zero; a product that is not finite or is 2^31 or more in magnitude counts
// what the x86 conversion yields, 0x80000000, whose low 16 bits are 0
__device__ __forceinline__ unsigned fm_inc(float ref, float m)
{
    const float r = roundf(ref * m);
    return fabsf(r) < 2147483648.0f ? (unsigned)(int)r : 0u;
}

// exclusive scan of one value per lane over the workgroup and the total; every
// lane of the workgroup calls it (it synchronises); wsum: NW words of LDS
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned *wsum, unsigned &total)
{
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d);
        if (lane >= (unsigned)d) inc += o;
    }
    if (lane == 63u) wsum[w] = inc;
    __syncthreads();
    unsigned woff = 0;
    total = 0;
#pragma unroll
    for (unsigned i = 0; i < (unsigned)NW; i++) {
        const unsigned s = wsum[i];
        if (i < w) woff += s;
        total += s;
    }
    __syncthreads();
    return woff + inc - v;
}

// the RUN samples of lane t of the tile at base; beyond n: 0 (no increment)
template <bool V16>
__device__ __forceinline__ void fm_load(const float *__restrict__ m, unsigned i0, unsigned n, float (&v)[RUN])
{
    if (V16 && i0 + RUN <= n) {
        const float4 a = *reinterpret_cast<const float4 *>(m + i0), b = *reinterpret_cast<const float4 *>(m + i0 + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        return;
    }
#pragma unroll
    for (int k = 0; k < RUN; k++) v[k] = i0 + k < n ? m[i0 + k] : 0.0f;
}

// sums[b] = the sum of the increments of tile b; launched for full tiles only
template <bool V16>
__global__ __launch_bounds__(NT) void k_fm_sums(float ref, const float *__restrict__ m, unsigned n,
                                                unsigned *__restrict__ sums)
{
    __shared__ unsigned wsum[NW];
    float v[RUN];
    fm_load<V16>(m, blockIdx.x * TILE + threadIdx.x * RUN, n, v);
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < RUN; k++) s += fm_inc(ref, v[k]);
    unsigned total;
    block_scan(s, wsum, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// in place: sums[b] (b < ntiles - 1 valid) -> acc + sum of sums[< b], b < ntiles
__global__ __launch_bounds__(NT) void k_fm_scan(const unsigned *__restrict__ acc, unsigned *sums, unsigned ntiles)
{
    __shared__ unsigned wsum[NW];
    unsigned carry = acc[0];
    for (unsigned p0 = 0; p0 < ntiles; p0 += PASS) {
        const unsigned i0 = p0 + threadIdx.x * PRUN;
        unsigned v[PRUN], s = 0;
#pragma unroll
        for (int k = 0; k < PRUN; k++) {
            v[k] = i0 + k + 1 < ntiles ? sums[i0 + k] : 0u;
            s += v[k];
        }
        unsigned total;
        unsigned run = carry + block_scan(s, wsum, total);
#pragma unroll
        for (int k = 0; k < PRUN; k++) {
            if (i0 + k < ntiles) sums[i0 + k] = run;
            run += v[k];
        }
        carry += total;
    }
}

__device__ __forceinline__ unsigned pad(unsigned j) { return j + (j >> 3); }

// offs[b]: the accumulator before tile b (a call of one tile: the object's own)
template <bool V16>
__global__ __launch_bounds__(NT) void k_fm_mod(float ref, const float2 *__restrict__ tab,
                                               const unsigned *__restrict__ offs, unsigned *__restrict__ acc_out,
                                               const float *__restrict__ m, float2 *__restrict__ s, unsigned n)
{
    __shared__ float2 ltab[1024];
    __shared__ unsigned ph[TILE + TILE / 8];
    __shared__ unsigned wsum[NW];
    const unsigned t = threadIdx.x, base = blockIdx.x * TILE, i0 = base + t * RUN;
    {
        const float4 *g = reinterpret_cast<const float4 *>(tab);
        float4 *l = reinterpret_cast<float4 *>(ltab);
        l[t] = g[t];
        l[t + NT] = g[t + NT];
    }
    float v[RUN];
    fm_load<V16>(m, i0, n, v);
    unsigned p[RUN], sum = 0;
#pragma unroll
    for (int k = 0; k < RUN; k++) {
        sum += fm_inc(ref, v[k]);
        p[k] = sum;
    }
    unsigned total;
    const unsigned before = offs[blockIdx.x] + block_scan(sum, wsum, total);
#pragma unroll
    for (int k = 0; k < RUN; k++) {
        const unsigned phase = (before + p[k]) & 0xffffu;
        ph[pad(t * RUN + k)] = ((phase + 0x20u) >> 6) & 0x3ffu;
        if (i0 + k + 1 == n) acc_out[0] = phase;
    }
    __syncthreads();

    if (V16) {
#pragma unroll
        for (int j = 0; j < RUN / 2; j++) {
            const unsigned li = 2 * (j * NT + t), gi = base + li;
            if (gi >= n) continue;
            const float2 a = ltab[ph[pad(li)]];
            if (gi + 1 < n) {
                const float2 b = ltab[ph[pad(li + 1)]];
                *reinterpret_cast<float4 *>(s + gi) = make_float4(a.x, a.y, b.x, b.y);
            } else {
                s[gi] = a;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < RUN; j++) {
            const unsigned li = j * NT + t, gi = base + li;
            if (gi < n) s[gi] = ltab[ph[pad(li)]];
        }
    }
}

// ---------------------------------------------------------------- freqdem

constexpr unsigned DTILE = LQK_FREQDEM_TILE, SW = LQK_FREQDEM_SWITCH;
constexpr int DRUN = DTILE / NT, FR = LQK_FREQDEM_FRAMES;
static_assert(DRUN == 8 && SW <= NT, "the flat geometry's halo is one sample per lane at most");

__device__ __forceinline__ float fd_out(float2 p, float2 r, float ref)
{
    const float re = p.x * r.x + p.y * r.y;
    const float im = p.x * r.y - p.y * r.x;
    return (float)atan2((double)im, (double)re) * ref;
}

// hout[j] = (hist ++ r)[n + j], j < M: the last M samples
__device__ __forceinline__ void fd_state(const float2 *__restrict__ hist, float2 *__restrict__ hout,
                                         const float2 *__restrict__ r, unsigned long long n, unsigned long long M)
{
    const unsigned long long step = (unsigned long long)gridDim.x * NT;
    for (unsigned long long j = (unsigned long long)blockIdx.x * NT + threadIdx.x; j < M; j += step) {
        const unsigned long long k = n + j;
        hout[j] = k < M ? hist[k] : r[k - M];
    }
}

template <bool V16>
__global__ __launch_bounds__(NT) void k_fd_flat(float ref, unsigned M, const float2 *__restrict__ hist,
                                                float2 *__restrict__ hout, const float2 *__restrict__ r,
                                                float *__restrict__ m, unsigned n)
{
    __shared__ float2 buf[DTILE + SW];   // buf[j] = sample base - M + j
    const unsigned t = threadIdx.x, base = blockIdx.x * DTILE;
    if (t < M) {
        // base - M + t < base <= n - 1: inside the input where it is not history
        buf[t] = base + t < M ? hist[base + t] : r[base + t - M];
    }
    if (V16) {
#pragma unroll
        for (int j = 0; j < DRUN / 2; j++) {
            const unsigned li = 2 * (j * NT + t), gi = base + li;
            if (gi + 1 < n) {
                const float4 v = *reinterpret_cast<const float4 *>(r + gi);
                buf[M + li] = make_float2(v.x, v.y);
                buf[M + li + 1] = make_float2(v.z, v.w);
            } else if (gi < n) {
                buf[M + li] = r[gi];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < DRUN / 2; j++) {
            const unsigned li = 2 * (j * NT + t), gi = base + li;
            if (gi >= n) continue;
            const float a = fd_out(buf[li], buf[M + li], ref);
            if (gi + 1 < n) {
                const float b = fd_out(buf[li + 1], buf[M + li + 1], ref);
                *reinterpret_cast<float2 *>(m + gi) = make_float2(a, b);
            } else {
                m[gi] = a;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < DRUN; j++) {
            const unsigned li = j * NT + t, gi = base + li;
            if (gi < n) buf[M + li] = r[gi];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < DRUN; j++) {
            const unsigned li = j * NT + t, gi = base + li;
            if (gi < n) m[gi] = fd_out(buf[li], buf[M + li], ref);
        }
    }
    fd_state(hist, hout, r, n, M);
}

// workgroup blockIdx.x = fb * colblocks + cb: channels cb*256 .. +255 of frames fb*FR .. +FR-1
__global__ __launch_bounds__(NT) void k_fd_cols(float ref, unsigned M, unsigned colblocks,
                                                const float2 *__restrict__ hist, float2 *__restrict__ hout,
                                                const float2 *__restrict__ r, float *__restrict__ m, unsigned n)
{
    const unsigned cb = blockIdx.x % colblocks, fb = blockIdx.x / colblocks;
    const unsigned long long c = (unsigned long long)cb * NT + threadIdx.x;
    if (c < M) {
        const unsigned long long f0 = (unsigned long long)fb * FR, i0 = f0 * M + c;
        if (i0 < n) {
            float2 prev = f0 == 0 ? hist[c] : r[i0 - M];
            float2 v[FR];
#pragma unroll
            for (int k = 0; k < FR; k++) {
                const unsigned long long i = i0 + (unsigned long long)k * M;
                if (i < n) v[k] = r[i];
            }
#pragma unroll
            for (int k = 0; k < FR; k++) {
                const unsigned long long i = i0 + (unsigned long long)k * M;
                if (i < n) {
                    m[i] = fd_out(prev, v[k], ref);
                    prev = v[k];
                }
            }
        }
    }
    fd_state(hist, hout, r, n, M);
}

} // namespace

extern "C" void lqk_freqmod(float ref, const void *tab, const unsigned *acc_in, unsigned *acc_out, unsigned *sums,
                            const float *m, void *s, unsigned long long n, void *stream)
{
    if (n == 0) return;
    if (n > LQK_FREQMOD_MAXN) {
        fprintf(stderr, "error: lqk_freqmod: call of %llu samples outside the kernel's range\n", n);
        exit(1);
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned nn = (unsigned)n, ntiles = (nn + TILE - 1) / TILE;
    const bool v16 = (((uintptr_t)m | (uintptr_t)s) & 15u) == 0;
    const unsigned *offs = acc_in;
    if (ntiles > 1) {
        if (v16) hipLaunchKernelGGL(k_fm_sums<true>, dim3(ntiles - 1), dim3(NT), 0, st, ref, m, nn, sums);
        else hipLaunchKernelGGL(k_fm_sums<false>, dim3(ntiles - 1), dim3(NT), 0, st, ref, m, nn, sums);
        LQ_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_fm_scan, dim3(1), dim3(NT), 0, st, acc_in, sums, ntiles);
        LQ_CHECK_LAUNCH();
        offs = sums;
    }
    if (v16)
        hipLaunchKernelGGL(k_fm_mod<true>, dim3(ntiles), dim3(NT), 0, st, ref, (const float2 *)tab, offs, acc_out, m,
                           (float2 *)s, nn);
    else
        hipLaunchKernelGGL(k_fm_mod<false>, dim3(ntiles), dim3(NT), 0, st, ref, (const float2 *)tab, offs, acc_out, m,
                           (float2 *)s, nn);
    LQ_CHECK_LAUNCH();
}

extern "C" void lqk_freqdem(float ref, unsigned M, const void *hist, void *hist_out, const void *r, float *m,
                            unsigned long long n, void *stream)
{
    if (n == 0) return;
    if (n > LQK_FREQDEM_MAXN || M == 0) {
        fprintf(stderr, "error: lqk_freqdem: call of %llu samples, %u channels outside the kernel's range\n", n, M);
        exit(1);
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned nn = (unsigned)n;
    const float2 *h = (const float2 *)hist, *x = (const float2 *)r;
    float2 *ho = (float2 *)hist_out;
    if (M < SW) {
        const unsigned grid = (nn + DTILE - 1) / DTILE;
        const bool v16 = ((uintptr_t)r & 15u) == 0 && ((uintptr_t)m & 7u) == 0;
        if (v16) hipLaunchKernelGGL(k_fd_flat<true>, dim3(grid), dim3(NT), 0, st, ref, M, h, ho, x, m, nn);
        else hipLaunchKernelGGL(k_fd_flat<false>, dim3(grid), dim3(NT), 0, st, ref, M, h, ho, x, m, nn);
    } else {
        // a call shorter than a frame has columns 0 .. n-1 only
        const unsigned long long cols = n < M ? n : M, frames = (n + M - 1) / M;
        const unsigned long long colblocks = (cols + NT - 1) / NT, grid = colblocks * ((frames + FR - 1) / FR);
        hipLaunchKernelGGL(k_fd_cols, dim3((unsigned)grid), dim3(NT), 0, st, ref, M, (unsigned)colblocks, h, ho, x, m,
                           nn);
    }
    LQ_CHECK_LAUNCH();
}
