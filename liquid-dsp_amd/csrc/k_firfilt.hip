// k_firfilt.hip -- firfilt on the VALU, the per-sample single-output path
// (firfilt_execute, firpfb_execute) and window (history) maintenance.
// firdecim: k_firdecim.hip; firinterp: k_firinterp.hip; the matrix-core
// firfilt: k_firfilt_mx.hip.
//
// Reference semantics restated (not translated):
//   firfilt  src/filter/src/firfilt.c:297-359  y[t] = scale * sum_k h[k] x[t-k]
// The reference walks a ring buffer one sample at a time; here every output is
// independent: a workgroup stages one contiguous input tile (plus the h-1
// sample halo) in LDS once, and each lane produces R consecutive outputs from
// a sliding register window, with the coefficients in scalar registers
// (uniform across the wave), so the inner loop is pure FMA.
#include "lq_fir.h"
#include "lq_kernels.h"

namespace {

constexpr int R = 16;        // consecutive outputs per lane
constexpr int TILE = NT * R; // outputs per workgroup

// Grid: one workgroup per TILE outputs.  LDS holds samples [t0-HP, t0+TILE).
// Lane tid computes outputs t0 + R*tid + r (r < R) with the R x HC tap block
// fully unrolled: coefficients are wave-uniform (scalar loads / SGPR
// operands), window samples come from LDS 16 bytes at a time, one row of 16
// samples per 16-tap group, so the inner body is pure FMA.  Outputs are
// transposed back through LDS and written with coalesced 16-byte stores.
// `win` = the previous HP samples (oldest first); ext[t<0] = win[HP + t].
template <int KIND, int HC>
__global__ __launch_bounds__(NT) void k_firfilt(const typename kt<KIND>::T *__restrict__ win,
                                                const typename kt<KIND>::T *x, long long n,
                                                typename kt<KIND>::T *y,
                                                const typename kt<KIND>::TC *__restrict__ hpad,
                                                int nchunk, float sre, float sim,
                                                const typename kt<KIND>::T *__restrict__ halo, int hexact)
{
    typedef typename kt<KIND>::T T;
    typedef typename kt<KIND>::TC TC;
    constexpr int VE = vec16<T>::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int HP = HC * nchunk;
    const long long t0 = (long long)blockIdx.x * TILE;
    const int S = TILE + HP;

    // hexact = hlen when the taps are zero padded (hlen < HP): a padded zero
    // tap times an Inf / NaN sample would put NaN into outputs the reference
    // (firfilt.c:322-338, hlen taps) keeps finite, so a tile holding a
    // non-finite sample runs the exact loop over the true taps instead
    bool bad = false;
    if (halo == nullptr && ((reinterpret_cast<uintptr_t>(x) & 15) == 0) && n * (long long)sizeof(T) < (1ll << 31)) {
        // four 16-byte loads per lane in flight through a range-checked
        // descriptor (zeros past n, and before x: the first tile then takes
        // those samples from the history) -- the branchy per-vector loop
        // below waited for one load latency per iteration
        const __amdgpu_buffer_rsrc_t rx =
            __builtin_amdgcn_make_buffer_rsrc((void *)x, (short)0, (int)(n * (long long)sizeof(T)), 0x00020000);
        constexpr int NV = 4;
        for (int e0 = threadIdx.x; e0 < S / VE; e0 += NV * NT) {
            float4 pv[NV];
#pragma unroll
            for (int k = 0; k < NV; k++) {
                const long long s = t0 - HP + (long long)(e0 + k * NT) * VE;
                pv[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                       rx, (unsigned)(s * (long long)sizeof(T)), 0, 0));
            }
#pragma unroll
            for (int k = 0; k < NV; k++) {
                const int e = e0 + k * NT;
                if (e >= S / VE) break;
                const int u = e * VE;
                const long long s = t0 - HP + u;
                if (s < 0) {
                    T o[VE];
                    load16(win + HP + s, o);
                    pv[k] = pack16(o);
                }
                if (hexact) bad |= !(isfinite(pv[k].x) && isfinite(pv[k].y) && isfinite(pv[k].z) && isfinite(pv[k].w));
                *reinterpret_cast<float4 *>(smem + lds_off<T>(u)) = pv[k];
            }
        }
    } else {
        for (int e = threadIdx.x; e < S / VE; e += NT) {
            const int u = e * VE;
            const long long s = t0 - HP + u;
            T o[VE];
            if (s < 0) {
                load16(win + HP + s, o);
            } else if (halo != nullptr && u < HP && blockIdx.x > 0) {
                load16(halo + (size_t)blockIdx.x * HP + u, o);
            } else if (s + VE <= n) {
                load16(x + s, o);
            } else {
#pragma unroll
                for (int i = 0; i < VE; i++) o[i] = (s + i < n) ? x[s + i] : zero<T>();
            }
            const float4 pv = pack16(o);
            if (hexact) bad |= !(isfinite(pv.x) && isfinite(pv.y) && isfinite(pv.z) && isfinite(pv.w));
            *reinterpret_cast<float4 *>(smem + lds_off<T>(u)) = pv;
        }
    }
    const bool exact = hexact ? __syncthreads_or(bad) : (__syncthreads(), false);

    T acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = zero<T>();

    if (exact) {
        for (int r = 0; r < R; r++) {
            const int u = HP + R * threadIdx.x + r;
            T a = zero<T>();
            for (int k = 0; k < hexact; k++) mac(a, hpad[k], *reinterpret_cast<const T *>(smem + lds_off<T>(u - k)));
            acc[r] = a;
        }
    }
    for (int c = 0; c < (exact ? 0 : nchunk); c++) {
        const TC *hc = hpad + c * HC;
        // window sample a' (0 <= a' < HC+R) of this chunk is tile sample
        // u = R*tid + HP - c*HC - HC + a'  (a row start when a' % 16 == 0)
        const int row0 = threadIdx.x + ((HP - c * HC - HC) >> 4);
        const unsigned char *rb = smem + lds_off<T>(16 * row0);
        T v[HC + R];
        // newest row first: a' in [HC, HC+16)
#pragma unroll
        for (int i = 0; i < 16 / VE; i++) {
            T o[VE];
            load16(reinterpret_cast<const T *>(rb + lds_off<T>(HC + i * VE)), o);
#pragma unroll
            for (int k = 0; k < VE; k++) v[HC + i * VE + k] = o[k];
        }
#pragma unroll
        for (int g = 0; g < HC / 16; g++) {
            // bring in the next older row: a' in [HC-16g-16, HC-16g)
#pragma unroll
            for (int i = 0; i < 16 / VE; i++) {
                const int a = HC - 16 * g - 16 + i * VE;
                T o[VE];
                load16(reinterpret_cast<const T *>(rb + lds_off<T>(a)), o);
#pragma unroll
                for (int k = 0; k < VE; k++) v[a + k] = o[k];
            }
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const TC hv = hc[16 * g + j];
#pragma unroll
                for (int r = 0; r < R; r++) mac(acc[r], hv, v[r - (16 * g + j) + HC]);
            }
        }
    }

    // transpose through LDS for coalesced stores
    __syncthreads();
#pragma unroll
    for (int i = 0; i < R / VE; i++) {
        T o[VE];
#pragma unroll
        for (int k = 0; k < VE; k++) o[k] = oscale<KIND>(acc[i * VE + k], sre, sim);
        *reinterpret_cast<float4 *>(smem + lds_off<T>(R * threadIdx.x + i * VE)) = pack16(o);
    }
    __syncthreads();
    const long long nt = n - t0 < TILE ? n - t0 : TILE;
    for (int e = threadIdx.x; e < TILE / VE; e += NT) {
        const int u = e * VE;
        if (u >= nt) break;
        const float4 val = *reinterpret_cast<const float4 *>(smem + lds_off<T>(u));
        if (u + VE <= nt) {
            *reinterpret_cast<float4 *>(y + t0 + u) = val;
        } else {
            T o[VE];
            load16(reinterpret_cast<const T *>(smem + lds_off<T>(u)), o);
            for (int k = 0; k < VE && u + k < nt; k++) y[t0 + u + k] = o[k];
        }
    }
}

template <int KIND>
__global__ void k_halo_copy(const typename kt<KIND>::T *x, long long n, int HP, long long ntiles, int tile,
                            typename kt<KIND>::T *halo)
{
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long tot = ntiles * HP;
    if (i >= tot) return;
    long long tl = i / HP;
    int u = (int)(i - tl * HP);
    if (tl == 0) return;
    long long s = tl * tile - HP + u;
    halo[i] = (s >= 0 && s < n) ? x[s] : zero<typename kt<KIND>::T>();
}

// dst = the last L samples of (src ++ x[0..n)), one thread per sample
template <typename T>
__global__ void k_window_append(lqk_hist_job j)
{
    lq_hist_job_run<T>(j);
}

// One output from a window: y = scale * sum_{k < nh} h[k] newest[-k], `newest`
// the window's last sample.  firfilt_execute (h = the padded taps' first hlen,
// window of HP samples) and firpfb_execute(i) (h = row i of hpoly, window of L).
template <int KIND>
__global__ void k_fir_single(const typename kt<KIND>::TC *__restrict__ h, int nh,
                             const typename kt<KIND>::T *__restrict__ newest, float sre, float sim,
                             typename kt<KIND>::T *y, unsigned *flag, unsigned seq)
{
    typedef typename kt<KIND>::T T;
    __shared__ T part[64];
    T acc = zero<T>();
    for (int k = threadIdx.x; k < nh; k += 64) mac(acc, h[k], newest[-k]);
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        T s = zero<T>();
        for (int i = 0; i < 64; i++) s = vadd(s, part[i]);
        y[0] = oscale<KIND>(s, sre, sim);
        lq_signal(flag, seq);
    }
}

// the kernel's static group segment (queried once per instantiation)
template <int KIND, int HC>
size_t fir_static_lds()
{
    static const size_t v = [] {
        hipFuncAttributes a;
        LQ_CHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_firfilt<KIND, HC>)));
        return (size_t)a.sharedSizeBytes;
    }();
    return v;
}

// the one rule for both the create-time limit and the launch: dynamic LDS
// within the budget and, with the static segment on top, within the CU's 160 KB
inline bool fir_lds_fits(size_t lds, size_t lds_static)
{
    return lds <= FIR_LDS_MAX && lds + lds_static <= 160 * 1024;
}

template <int KIND, int HC>
void launch_firfilt(const lqk_fir_desc *d, const void *hist, const void *x, long long n, void *y,
                    const void *halo, hipStream_t st)
{
    typedef typename kt<KIND>::T T;
    typedef typename kt<KIND>::TC TC;
    const int HP = HC * (int)d->nchunk;
    const long long ntiles = (n + TILE - 1) / TILE;
    const size_t lds = (size_t)lds_bytes<T>(TILE + HP);
    if (!fir_lds_fits(lds, fir_static_lds<KIND, HC>())) {
        fprintf(stderr, "error: firfilt: filter length %u exceeds the GPU tile limit\n", d->hlen);
        exit(1);
    }
    hipLaunchKernelGGL((k_firfilt<KIND, HC>), dim3((unsigned)ntiles), dim3(NT), lds, st, (const T *)hist,
                       (const T *)x, n, (T *)y, (const TC *)d->hpad, (int)d->nchunk, d->scale_re,
                       d->scale_im, (const T *)halo, (int)d->hlen < HP ? (int)d->hlen : 0);
    LQ_CHECK_LAUNCH();
}

} // namespace

extern "C" unsigned int lqk_firfilt_max_history(int kind)
{
    // the launch rule (fir_lds_fits) for the HC = 64 kernel, which every
    // filter past 32 taps runs; HP a multiple of 64
    unsigned int hp = 0;
    fir_kind(kind, [&](auto k) {
        while (fir_lds_fits((size_t)lds_bytes<typename kt<k>::T>(TILE + hp + 64), fir_static_lds<k, 64>())) hp += 64;
    });
    return hp;
}

extern "C" size_t lqk_firfilt_scratch_bytes(const lqk_fir_desc *d, unsigned long long n)
{
    const long long ntiles = ((long long)n + TILE - 1) / TILE;
    return (size_t)ntiles * d->hc * d->nchunk * elem_size(d->kind);
}

extern "C" void lqk_firfilt(const lqk_fir_desc *d, const void *hist, const void *x, unsigned long long n,
                            void *y, void *scratch, const lqk_hist_job *job, void *stream)
{
    if (n == 0) return;
    // LQ_FIRFILT_NO_MFMA=1 keeps crcf h<=64 on the VALU kernel (comparisons)
    static int no_mx = -1;
    if (no_mx < 0) no_mx = getenv("LQ_FIRFILT_NO_MFMA") != nullptr;
    if (!no_mx && lqk_firfilt_mx(d, hist, x, n, y, job, stream)) return;
    // the VALU kernel may run in place: the window update reads x first
    if (job && job->dst) lqk_window_append(d->kind != 0, job->src, job->L, job->x, job->n, job->dst, stream);
    hipStream_t st = (hipStream_t)stream;
    const void *halo = nullptr;
    if (x == y) {
        // in place: save each tile's halo before any workgroup overwrites it
        const int HP = (int)(d->hc * d->nchunk);
        const long long ntiles = ((long long)n + TILE - 1) / TILE;
        const long long tot = ntiles * HP;
        const unsigned nb = (unsigned)((tot + 255) / 256);
        // a copy by sample size: the real kind or either complex one
        lq_switch<0, 1>(d->kind != 0, [&](auto k) {
            typedef typename kt<k>::T T;
            hipLaunchKernelGGL(k_halo_copy<k>, dim3(nb), dim3(256), 0, st, (const T *)x, (long long)n, HP, ntiles,
                               TILE, (T *)scratch);
        });
        LQ_CHECK_LAUNCH();
        halo = scratch;
    }
    fir_kind(d->kind, [&](auto k) {
        if (!lq_switch<16, 32, 64>((int)d->hc,
                                   [&](auto hc) { launch_firfilt<k, hc>(d, hist, x, (long long)n, y, halo, st); })) {
            fprintf(stderr, "error: firfilt: invalid chunk class %u\n", d->hc);
            exit(1);
        }
    });
}

extern "C" void lqk_window_append(int is_complex, const void *src_hist, unsigned int L, const void *x,
                                  unsigned long long n, void *dst_hist, void *stream)
{
    if (L == 0) return;
    hipStream_t st = (hipStream_t)stream;
    unsigned nb = (L + 255) / 256;
    const lqk_hist_job job = {src_hist, x, n, dst_hist, L};
    lq_switch<0, 1>(is_complex != 0, [&](auto k) {
        hipLaunchKernelGGL(k_window_append<typename kt<k>::T>, dim3(nb), dim3(256), 0, st, job);
    });
    LQ_CHECK_LAUNCH();
}

namespace {
// y = scale * (h[0..nh) against the window whose last sample is win[newest])
void launch_fir_single(int kind, const void *h, size_t h0, unsigned nh, const void *win, size_t newest, float sre,
                       float sim, void *y, unsigned *flag, unsigned seq, void *stream)
{
    fir_kind(kind, [&](auto k) {
        typedef typename kt<k>::T T;
        typedef typename kt<k>::TC TC;
        hipLaunchKernelGGL(k_fir_single<k>, dim3(1), dim3(64), 0, (hipStream_t)stream, (const TC *)h + h0, (int)nh,
                           (const T *)win + newest, sre, sim, (T *)y, flag, seq);
    });
    LQ_CHECK_LAUNCH();
}
} // namespace

extern "C" void lqk_fir_single(const lqk_fir_desc *d, const void *win, void *y, unsigned *flag, unsigned seq,
                               void *stream)
{
    launch_fir_single(d->kind, d->hpad, 0, d->hlen, win, (size_t)d->hc * d->nchunk - 1, d->scale_re, d->scale_im, y,
                      flag, seq, stream);
}

// firpfb_execute(i): row i of hpoly (M x L) against the L-sample window
extern "C" void lqk_firpfb_single(int kind, const void *hpoly, unsigned int L, unsigned int i, const void *win,
                                  float sre, float sim, void *y, unsigned *flag, unsigned seq, void *stream)
{
    launch_fir_single(kind, hpoly, (size_t)i * L, L, win, L - 1, sre, sim, y, flag, seq, stream);
}
