// k_firinterp.hip -- firinterp (and firpfb's block interpolation).
//
// Reference semantics restated (not translated):
//   firinterp src/filter/src/firinterp.c:187-215 via firpfb.c:325-345
//            y[i*M+p] = sum_l h'[p + l*M] x[i - l]
// Every output is independent: a workgroup stages NT inputs and the L-1
// sample history before them in LDS once; each lane forms its input's M outputs.
#include "lq_fir.h"
#include "lq_kernels.h"

#include <cstdio>
#include <cstdlib>

namespace {

// one input sample per lane -> M outputs; hpoly[p*L + l] = h'[p + l*M]
template <int KIND>
__global__ __launch_bounds__(NT) void k_firinterp(const typename kt<KIND>::T *__restrict__ hist,
                                                  const typename kt<KIND>::T *__restrict__ x,
                                                  long long n, int M, int L,
                                                  const typename kt<KIND>::TC *__restrict__ hpoly,
                                                  float sre, float sim, typename kt<KIND>::T *__restrict__ y)
{
    typedef typename kt<KIND>::T T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *tile = reinterpret_cast<T *>(smem);
    const long long i0 = (long long)blockIdx.x * NT;
    const int S = NT + L - 1;
    for (int u = threadIdx.x; u < S; u += NT) {
        long long s = i0 - (L - 1) + u;
        T v;
        if (s < 0) v = (L > 1) ? hist[L - 1 + s] : zero<T>();
        else if (s < n) v = x[s];
        else v = zero<T>();
        tile[u] = v;
    }
    __syncthreads();
    const long long i = i0 + threadIdx.x;
    if (i >= n) return;
    const T *w = tile + threadIdx.x + (L - 1); // w[-l] = x[i-l]
    for (int p = 0; p < M; p++) {
        T acc = zero<T>();
        for (int l = 0; l < L; l++) mac(acc, hpoly[p * L + l], w[-l]);
        y[i * M + p] = oscale<KIND>(acc, sre, sim);
    }
}

// firinterp crcf/rrrf (real taps), L <= LT taps per phase, M phases: a tile of
// NT inputs in LDS, the phase taps in LDS (read as broadcasts), each lane
// keeps its input's window in registers and forms all M outputs, which go
// back through LDS so that the wave's 64*M outputs leave as contiguous 16-byte
// stores.  Window samples older than the object's L-1 history are zero.
template <int KIND, int LT>
__global__ __launch_bounds__(NT) void k_firinterp_t(const typename kt<KIND>::T *__restrict__ hist,
                                                    const typename kt<KIND>::T *__restrict__ x, long long n,
                                                    int M, int L, const float *__restrict__ hpoly, float sre,
                                                    float sim, typename kt<KIND>::T *__restrict__ y)
{
    typedef typename kt<KIND>::T T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *tp = reinterpret_cast<float *>(smem);                         // M x LT taps, zero padded
    T *tile = reinterpret_cast<T *>(smem + ((M * LT * 4 + 15) & ~15));  // NT + LT - 1 samples
    T *stage = tile + ((NT + LT - 1 + 3) & ~3);                            // NT * M outputs
    const long long i0 = (long long)blockIdx.x * NT;
    for (int e = threadIdx.x; e < M * LT; e += NT) {
        const int p = e / LT, l = e - p * LT;
        tp[e] = l < L ? hpoly[p * L + l] : 0.0f;
    }
    for (int u = threadIdx.x; u < NT + LT - 1; u += NT) {
        const long long s = i0 - (LT - 1) + u;
        T v = zero<T>();
        if (s >= 0) {
            if (s < n) v = x[s];
        } else if (s >= -(long long)(L - 1)) {
            v = hist[L - 1 + s];
        }
        tile[u] = v;
    }
    __syncthreads();
    T w[LT];   // w[l] = x[i - l]
#pragma unroll
    for (int l = 0; l < LT; l++) w[l] = tile[threadIdx.x + LT - 1 - l];
    T *st = stage + (threadIdx.x >> 6) * 64 * M;   // this wave's outputs, natural order
    const int lane = threadIdx.x & 63;
    for (int p = 0; p < M; p++) {
        const float *hp = tp + p * LT;
        T acc = zero<T>();
#pragma unroll
        for (int l = 0; l < LT; l += 4) {
            const float4 h4 = *reinterpret_cast<const float4 *>(hp + l);
            mac(acc, h4.x, w[l]);
            if (l + 1 < LT) mac(acc, h4.y, w[l + 1]);
            if (l + 2 < LT) mac(acc, h4.z, w[l + 2]);
            if (l + 3 < LT) mac(acc, h4.w, w[l + 3]);
        }
        st[lane * M + p] = oscale<KIND>(acc, sre, sim);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // the wave's outputs y[(iw) M .. (iw + 64) M), iw = its first input
    const long long iw = i0 + (threadIdx.x & ~63);
    if (iw >= n) return;
    const long long nin = (n - iw) < 64 ? (n - iw) : 64;
    const int nout = (int)(nin * M);
    constexpr int VE = vec16<T>::N;
    T *yw = y + iw * M;
    for (int e = lane * VE; e < nout; e += 64 * VE) {
        if (e + VE <= nout) {
            // non-temporal: the outputs are not read back (M = 8 m = 8 crcf,
            // 2^27 outputs: 0.270 -> 0.244-0.248 ms, M = 4: 0.314 -> 0.244-0.250,
            // r06fi)
            typedef float v4nt __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(*reinterpret_cast<const v4nt *>(st + e), reinterpret_cast<v4nt *>(yw + e));
        } else {
            for (int k = 0; k < VE && e + k < nout; k++) yw[e + k] = st[e + k];
        }
    }
}

} // namespace

// the launch's decision: 0 for the plain kernel, else the LT class of
// k_firinterp_t (real taps, L <= 32, M <= 64, a 16-byte aligned output, and
// taps + tile + staged outputs within 64 KB of LDS, *lds2)
static int firinterp_route(int kind, unsigned int M, unsigned int L, bool y_aligned16, size_t *lds2)
{
    if (kind == 2 || L > 32 || M > 64 || !y_aligned16) return 0;
    const int LT = L <= 8 ? 8 : L <= 12 ? 12 : L <= 16 ? 16 : L <= 20 ? 20 : L <= 24 ? 24 : 32;
    const size_t es = elem_size(kind);
    *lds2 = (((size_t)M * LT * 4 + 15) & ~(size_t)15) + (((size_t)NT + LT - 1 + 3) & ~(size_t)3) * es +
            (size_t)NT * M * es;
    return *lds2 <= 64 * 1024 ? LT : 0;
}

extern "C" int lqk_firinterp_route(int kind, unsigned int M, unsigned int L, int y_aligned16)
{
    size_t lds2 = 0;
    return firinterp_route(kind, M, L, y_aligned16 != 0, &lds2);
}

// the plain kernel's tile and history, (NT + L) samples, within the dynamic
// LDS budget (it has no static segment): the longest phase any shape can run
extern "C" unsigned int lqk_firinterp_max_taps(int kind) { return (unsigned int)(FIR_LDS_MAX / elem_size(kind)) - NT; }

extern "C" void lqk_firinterp(int kind, const void *hpoly, unsigned int M, unsigned int L, float sre, float sim,
                              const void *hist, const void *x, unsigned long long n, void *y, void *stream)
{
    if (n == 0) return;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = (unsigned)((n + NT - 1) / NT);
    size_t lds2 = 0;
    const int LT = firinterp_route(kind, M, L, ((uintptr_t)y & 15) == 0, &lds2);
    if (LT) {   // the register-window kernel
        lq_switch<0, 1>(kind, [&](auto k) {
            typedef typename kt<k>::T T;
            lq_switch<8, 12, 16, 20, 24, 32>(LT, [&](auto lt) {
                hipLaunchKernelGGL((k_firinterp_t<k, lt>), dim3(nb), dim3(NT), lds2, st, (const T *)hist,
                                   (const T *)x, (long long)n, (int)M, (int)L, (const float *)hpoly, sre, sim,
                                   (T *)y);
            });
        });
        LQ_CHECK_LAUNCH();
        return;
    }
    if (L > lqk_firinterp_max_taps(kind)) {   // refused at create (host/firdecim.c, host/firpfb.c)
        fprintf(stderr, "error: firinterp: %u taps per phase exceed the GPU kernel limit\n", L);
        exit(1);
    }
    const size_t lds = (size_t)(NT + L) * elem_size(kind);
    fir_kind(kind, [&](auto k) {
        typedef typename kt<k>::T T;
        typedef typename kt<k>::TC TC;
        hipLaunchKernelGGL(k_firinterp<k>, dim3(nb), dim3(NT), lds, st, (const T *)hist, (const T *)x, (long long)n,
                           (int)M, (int)L, (const TC *)hpoly, sre, sim, (T *)y);
    });
    LQ_CHECK_LAUNCH();
}
