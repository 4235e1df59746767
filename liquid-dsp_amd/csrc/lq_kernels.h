/*
 * lq_kernels.h -- the thin C-ABI between the C host objects (host/ *.c) and the
 * hand-written HIP kernels (csrc/ *.hip).  Plain pointers and sizes only.
 *
 * Device pointers are `void *` (complex samples are interleaved float pairs,
 * 8 bytes).  Every launcher enqueues on the given HIP stream and returns
 * immediately; errors abort with a message (lqrt_check).
 */
#ifndef LQ_KERNELS_H
#define LQ_KERNELS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- runtime */
void   lqrt_require_device(const char *who);    /* abort if no usable GPU */
void  *lqrt_malloc(size_t bytes);               /* device memory, zeroed   */
void   lqrt_free(void *p);
void  *lqrt_host_alloc(size_t bytes);           /* pinned host memory      */
void   lqrt_host_free(void *p);
void  *lqrt_stream_create(void);
void   lqrt_stream_destroy(void *s);
void   lqrt_h2d(void *dst, const void *src, size_t bytes, void *stream);
void   lqrt_d2h(void *dst, const void *src, size_t bytes, void *stream);
void   lqrt_d2d(void *dst, const void *src, size_t bytes, void *stream);
void   lqrt_memset(void *dst, size_t bytes, void *stream);
void   lqrt_sync(void *stream);
void   lqrt_device_sync(void);
int    lqrt_is_device_ptr(const void *p);
const float *lqrt_twiddles(void);               /* W_4096^e = exp(-2 pi i e/4096), e<4096 */
#define LQRT_ZEROS 256
const float *lqrt_zeros(void);                  /* LQRT_ZEROS bytes of zeros in device memory */
/* grid of a persistent launch: min(want, cap), and at most the limit of
 * liquid_mi355x_set_max_workgroups when one is set (tests only) */
unsigned lqrt_grid(unsigned long long want, unsigned cap);
/* small-call completion: one kernel copies `bytes` (a multiple of 4, at most
 * LQRT_COPYOUT_MAX) from device memory src to pinned host memory dst, makes
 * them visible system-wide and then stores `seq` to the pinned word *flag;
 * lqrt_wait_flag spins until it sees seq (then falls back to a stream sync,
 * which also reports a kernel fault). */
#define LQRT_COPYOUT_MAX (64u << 10)
void   lqrt_copyout_signal(const void *src, void *dst, size_t bytes, unsigned *flag, unsigned seq, void *stream);
void   lqrt_wait_flag(const unsigned *flag, unsigned seq, void *stream);

/* ---------------------------------------------------------------- dotprod
 * Y[v] = sum_i h[i] X[v*stride + i], v < nvec.  kind: 0 rrrf, 1 crcf, 2 cccf */
void lqk_dotprod_batch(int kind, const void *h, unsigned int n, const void *X,
                       unsigned long long stride, unsigned long long nvec, void *Y, void *stream);
/* the launch lqk_dotprod_batch makes for nvec rows of n samples at stride n
 * (its own decision, no GPU call): bit 4 set for k_dot_vec (n a multiple of
 * the 16-byte chunk and X 16-byte aligned), clear for k_dot_scalar; bits 0-3
 * lg G, the lanes per row; *blocks the grid and *block_cap the cap past which
 * the groups stride over the rows (either may be NULL).  -1: invalid kind */
int lqk_dotprod_route(int kind, unsigned int n, int x_aligned16, unsigned long long nvec, unsigned int *blocks,
                      unsigned int *block_cap);
/* one dot product (dotprod_*_execute): x may be pinned host memory, y is
 * pinned host memory, *flag = seq is raised once y is visible to the host */
void lqk_dotprod_single(int kind, const void *h, unsigned int n, const void *x, void *y, unsigned *flag,
                        unsigned seq, void *stream);

/* ---------------------------------------------------------------- firfilt
 * Streaming FIR: y[i] = scale * sum_{k<hlen} h[k] ext[i-k], where ext[t] = x[t]
 * for t >= 0 and win[HP+t] for t < 0 (win = the previous HP = hc*nchunk
 * inputs, oldest first, 16-byte aligned).  hpad: coefficients in natural order, zero padded to
 * nchunk*hc.  kind: 0 rrrf, 1 crcf, 2 cccf.  x == y allowed (in-place). */
typedef struct {
    int kind;
    unsigned int hlen;       /* logical length */
    unsigned int hc;         /* compile-time chunk class: 16, 32, 64 */
    unsigned int nchunk;     /* padded length = hc*nchunk */
    const void *hpad;        /* device coefficients (float or float2) */
    float scale_re, scale_im;
    int mx_ok;               /* taps finite, nonzero |h| in [2^-50, 2^50]: the matrix-core kernel's
                              * three-term bf16 split is float32-accurate (k_firfilt_mx.hip) */
} lqk_fir_desc;

/* A stream object's history update folded into its stream kernel: dst =
 * the last L samples of (src: L samples) ++ (x: n samples), what
 * lqk_window_append does as a launch of its own (~5 us per call, measured in
 * the round-6 rocprof trace).  The kernel's workgroups copy grid-strided
 * slices of it before their own work; dst == NULL: no job. */
typedef struct {
    const void *src;
    const void *x;
    unsigned long long n;
    void *dst;
    unsigned int L;
} lqk_hist_job;

/* job (NULL: none): the window update, done inside the matrix-core kernel
 * when it takes the call, else launched before the VALU kernel (which may
 * run in place) */
void lqk_firfilt(const lqk_fir_desc *d, const void *hist, const void *x, unsigned long long n,
                 void *y, void *scratch, const lqk_hist_job *job, void *stream);
/* crcf with 33..64 taps on the matrix cores (k_firfilt_mx.hip); returns 0
 * when the call does not qualify (then lqk_firfilt runs the VALU kernel) */
int lqk_firfilt_mx(const lqk_fir_desc *d, const void *hist, const void *x, unsigned long long n, void *y,
                   const lqk_hist_job *job, void *stream);
/* bytes of scratch lqk_firfilt needs for an in-place call of n samples */
size_t lqk_firfilt_scratch_bytes(const lqk_fir_desc *d, unsigned long long n);
/* longest history (padded tap count) the direct FIR kernel can hold in LDS */
unsigned int lqk_firfilt_max_history(int kind);

/* window maintenance: dst[0..L) = last L samples of (src_hist[0..L) ++ x[0..n)) */
void lqk_window_append(int is_complex, const void *src_hist, unsigned int L, const void *x,
                       unsigned long long n, void *dst_hist, void *stream);

/* one output of a dot product of hr (reversed coefficients, hlen) against
 * win (oldest first), times scale: the per-sample firfilt_execute() path.
 * With a flag, y is pinned host memory and the kernel raises *flag = seq
 * once y is visible to the host (see lqrt_wait_flag); flag may be NULL. */
void lqk_fir_single(const lqk_fir_desc *d, const void *win, void *y, unsigned *flag, unsigned seq, void *stream);

/* ---------------------------------------------------------------- firdecim / firinterp
 * decim: y[o] = sum_k h[k] ext[o*M + phase - k]  (o < nout)
 * interp: y[i*M + p] = scale * sum_{l<L} h[p + l*M] ext[i - l]  (i < n) */
void lqk_firdecim(int kind, unsigned int hlen, const void *hpad /* hlen taps, natural order */, unsigned int M,
                  const void *hist, const void *x, unsigned long long nout, void *y, void *stream);
/* phase-layout decimator: hq = M x QC phase-major padded taps,
 * hq[r*QC + q] = h[q*M + r] (0 past hlen), QC = lqk_firdecim_ph_qc(M, hlen);
 * hist = the previous hl1 = hlen-1 inputs.  Returns -1 (nothing launched)
 * when the tile does not fit in LDS. */
unsigned lqk_firdecim_ph_qc(unsigned M, unsigned hlen);
int lqk_firdecim_ph(int kind, unsigned int M, unsigned int QC, const void *hq, unsigned int hl1,
                    const void *hist, const void *x, unsigned long long nout, void *y, void *stream);
/* Which kernel a device call takes: a pure function of the shape, the one
 * lqk_firdecim_ph itself switches on (hlen -> QC by lqk_firdecim_ph_qc).
 * PLAIN and REFUSED are the cases where lqk_firdecim_ph returns -1 and
 * lqk_firdecim launches k_firdecim or exits.  _tile: outputs per workgroup
 * tile of a route; _cap: the grid cap of a persistent route for this shape
 * (0 when the shape never takes that route). */
enum {
    LQK_DECIM_PF_R4X128 = 0,   /* k_firdecim_pf, 4 outputs per lane, 128 lanes */
    LQK_DECIM_PF_R2X256 = 1,   /* k_firdecim_pf, 2 per lane, 256 lanes */
    LQK_DECIM_PH2 = 2,         /* k_firdecim_ph2, 2 per lane, 256 lanes */
    LQK_DECIM_PF_R1X256 = 3,   /* k_firdecim_pf, 1 per lane, 256 lanes */
    LQK_DECIM_PH_R1X64 = 4,    /* k_firdecim_ph, 1 per lane, 64 lanes */
    LQK_DECIM_PLAIN = 5,       /* k_firdecim */
    LQK_DECIM_REFUSED = 6
};
int lqk_firdecim_route(int kind, unsigned int M, unsigned int hlen, int x_aligned16, unsigned long long nout);
unsigned int lqk_firdecim_route_tile(int route);
unsigned int lqk_firdecim_route_cap(int kind, unsigned int M, unsigned int hlen, int route);
void lqk_firinterp(int kind, const void *hpoly /* M x L, h[p + l*M] */, unsigned int M,
                   unsigned int L, float scale_re, float scale_im, const void *hist, const void *x,
                   unsigned long long n, void *y, void *stream);
/* the kernel lqk_firinterp takes for L taps per phase (its own decision):
 * 0 the plain kernel, else the LT class of the register-window kernel */
int lqk_firinterp_route(int kind, unsigned int M, unsigned int L, int y_aligned16);
/* the longest phase (taps) lqk_firinterp can run: the plain kernel's LDS */
unsigned int lqk_firinterp_max_taps(int kind);

/* ---------------------------------------------------------------- firpfbch2 analyzer
 * nblocks consecutive analyzer blocks over x (nblocks*M/2 samples); hist holds
 * the previous 2*m*M - M/2 inputs; p0 = parity of the first block.
 * hsub: M x 2m table, hsub[i*2m + n] = h[i + n*M].  Y: nblocks x M, already
 * divided by M (firpfbch2.c:277-278). */
void lqk_firpfbch2_analyzer(unsigned int M, unsigned int m, const void *hsub, const void *hist,
                            const void *x, unsigned long long nblocks, int p0, void *Y,
                            void *stream);
/* M = 1024 (m = 2 or 4) register/LDS-streaming fast path; returns 0 if the
 * shape is not covered (caller then uses lqk_firpfbch2_analyzer).  B0 = global
 * index of the first block (only its parity matters).  hsub here is the tap
 * table already multiplied by 1/M (the kernel applies no output scale). */
/* firpfbch_crcf analyzer M = 1024, p in {4, 8}, real taps (k_pfb2_fast.hip); 0 = not handled */
int lqk_firpfbch_analyzer_fast(int ctaps, unsigned int M, unsigned int p, const void *hsub, const void *hist,
                               const void *x, unsigned long long nblocks, void *Y, void *stream);
/* firpfbch_crcf synthesizer M = 1024, p in {4, 8}, real taps, nblocks >= p-1; 0 = not handled */
int lqk_firpfbch_synthesizer_fast(int ctaps, unsigned int M, unsigned int p, const void *hsub, void *state,
                                  const void *X, unsigned long long nblocks, void *y, void *stream);
/* firpfbch2_crcf synthesizer M = 1024, m in {2, 4}, nblocks >= 4m-1; 0 = not handled */
int lqk_firpfbch2_synthesizer_fast(unsigned int M, unsigned int m, const void *hsub, void *state, const void *X,
                                   unsigned long long nblocks, int p0, void *Y, void *stream);
/* batched transforms with the two sequential output scales of lq_fft_batch_scaled (k_fft_batch.hip) */
void lqk_fft_batch_scaled(unsigned int n, int dir, const void *x, void *y, unsigned long long batch, float s1,
                          float s2, void *stream);
/* job (NULL: none) is done only when the call is handled (returns 1).
 * flag (NULL: none): Y is pinned host memory, and the kernel raises *flag =
 * seq (system scope) once Y is visible to the host -- for calls that take a
 * single workgroup (a few blocks), else 0 is returned before any launch */
int lqk_firpfbch2_analyzer_fast(unsigned int M, unsigned int m, const void *hsub, const void *hist,
                                const void *x, unsigned long long nblocks, long long B0, void *Y,
                                const lqk_hist_job *job, unsigned *flag, unsigned seq, void *stream);
/* synthesizer: nblocks x M channel inputs -> nblocks x M/2 outputs.
 * state: the previous 4m-1 IFFT vectors (M each), zscratch (4m-1+nblocks)*M;
 * see csrc/k_firpfbch2.hip */
void lqk_firpfbch2_synthesizer(unsigned int M, unsigned int m, const void *hsub_syn,
                               void *state, void *zscratch, const void *X,
                               unsigned long long nblocks, int p0, void *Y, void *stream);

/* ---------------------------------------------------------------- firpfbch (critically sampled)
 * analyzer: block b consumes x[bM .. bM+M); window i receives x[bM + M-1-i]
 * X[M-1-i] = sum_n h[i + n*M] win_i, Y = FFT_forward(X).  hsub[i*p + n] = h[i+n*M];
 * ctaps: hsub holds complex taps (cccf), else real (crcf) */
/* firpfbch analyzer M = 1024 (crcf, p in {4, 8}), calls of <= 16 blocks in
 * one workgroup, with the history job and, optionally, the completion flag
 * (Y pinned host memory; see lqk_firpfbch2_analyzer_fast); 0: not handled */
int lqk_firpfbch_analyzer_few(int ctaps, unsigned int M, unsigned int p, const void *hsub, const void *hist,
                              const void *x, unsigned long long nblocks, void *Y, const lqk_hist_job *job,
                              unsigned *flag, unsigned seq, void *stream);
void lqk_firpfbch_analyzer(int ctaps, unsigned int M, unsigned int p, const void *hsub, const void *hist,
                           const void *x, unsigned long long nblocks, void *Y, void *stream);
void lqk_firpfbch_synthesizer(int ctaps, unsigned int M, unsigned int p, const void *hsub, void *state,
                              void *zscratch, const void *X, unsigned long long nblocks, void *y,
                              void *stream);

/* ---------------------------------------------------------------- channelizer routes
 * What a firpfbch2 / firpfbch launch decides, formed by one host function per
 * ladder that the launch itself calls (k_firpfbch2.hip, k_firpfbch.hip,
 * k_pfb2_fast.hip), so a query cannot drift from the launch.  A route is one
 * kernel template family plus what a test must tell apart (paired or 8-byte
 * loads, the few-block and the signalling form, real or complex taps `_c');
 * the unrolled depth (L, P) and the size within a family are not part of it.
 * Every hipLaunchKernelGGL of the three files belongs to exactly one route
 * (DESIGN.md has the table). */
enum {
    LQK_PFB_NONE = -1,                 /* not handled here / impossible arguments */
    LQK_PFB2_AN1024 = 0,               /* k_pfb2_an1024<L, true> */
    LQK_PFB2_AN1024_UNPAIRED,          /* k_pfb2_an1024<L, false> */
    LQK_PFB2_AN1024_FEW,               /* k_pfb2_an1024_few<L> */
    LQK_PFB2_AN1024_FEW_SIGNAL,        /* the same kernel raising the host's completion flag */
    LQK_PFB2_AN256,                    /* k_pfb2_an256<L, 1> */
    LQK_PFB2_AN512,                    /* k_pfb2_an256<L, 2> */
    LQK_PFB2_AN2048,                   /* k_pfb2_an2048<L> */
    LQK_PFB2_AN4096,                   /* k_pfb2_an4096<L> */
    LQK_PFB2_AN_SMALL,                 /* k_pfb2_an_small<L, 64 | 128> */
    LQK_PFB2_POLY_FFT,                 /* k_pfb2_poly<L> + batched transform */
    LQK_PFB2_DIRECT,                   /* k_pfb2_an<M, NB> */
    LQK_PFB2_GENERIC,                  /* k_pfb2_an_generic */
    LQK_PFB2_SYN1024,                  /* k_pfb2_syn1024<L> + state transform */
    LQK_PFB2_SYN_FUSED,                /* k_pfb2_syn_fused<L, 1 | 2> */
    LQK_PFB2_SYN4096,                  /* k_pfb2_syn4096<L> */
    LQK_PFB2_TWO_PASS_RUN,             /* batched transform + k_pfb2_syn_out_run<L> */
    LQK_PFB2_TWO_PASS_ELEM,            /* batched transform + k_pfb2_syn_out */
    LQK_PFB_AN1024,                    /* k_pfb_an1024<P, PF, true> */
    LQK_PFB_AN1024_UNPAIRED,           /* k_pfb_an1024<P, PF, false> */
    LQK_PFB_AN1024_FEW,                /* k_pfb_an1024_few<P> */
    LQK_PFB_AN1024_FEW_SIGNAL,
    LQK_PFB_AN_FUSED,                  /* k_pfb_an_fused<P, float, 1 | 2> */
    LQK_PFB_AN_FUSED_C,                /* ... <P, float2, R>; the `_C' routes follow their real one by 1 */
    LQK_PFB_AN4096,
    LQK_PFB_AN4096_C,
    LQK_PFB_AN_SMALL,
    LQK_PFB_AN_SMALL_C,
    LQK_PFB_AN_RUN_FFT,                /* k_pfb_an_X_run<P, TC> + batched transform */
    LQK_PFB_AN_RUN_FFT_C,
    LQK_PFB_AN_ELEM_FFT,               /* k_pfb_an_X<TC> + batched transform */
    LQK_PFB_AN_ELEM_FFT_C,
    LQK_PFB_SYN1024,                   /* k_pfb_syn1024<P> + state transform */
    LQK_PFB_SYN_FUSED,
    LQK_PFB_SYN_FUSED_C,
    LQK_PFB_SYN4096,
    LQK_PFB_SYN4096_C,
    LQK_PFB_SYN_SMALL,
    LQK_PFB_SYN_SMALL_C,
    LQK_PFB_FFT_SYN_RUN,               /* batched transform + k_pfb_syn_out_run<P, TC> */
    LQK_PFB_FFT_SYN_RUN_C,
    LQK_PFB_FFT_SYN_ELEM,              /* batched transform + k_pfb_syn_out<TC> */
    LQK_PFB_FFT_SYN_ELEM_C,
    LQK_PFB_NROUTES
};
/* run: blocks one workgroup (or one column set of it) walks, of the first
 * chunk; workgroups: that chunk's grid (for the two-pass forms the filter
 * kernel's); chunks: launches the call is cut into */
typedef struct {
    int route;
    long long run, workgroups, chunks;
} lqk_pfb_plan;
/* the M = 1024 fast ladders (k_pfb2_fast.hip); route LQK_PFB_NONE: not theirs.
 * signal: the call comes with a completion flag (a host call whose output fits
 * LQRT_COPYOUT_MAX).  x and Y are taken as 8-byte aligned; x16 / y16: 16-byte */
lqk_pfb_plan lqk_pfb2_fast_plan(int analyzer, unsigned int M, unsigned int m, unsigned long long nblocks, int p0,
                                int x16, int y16, int signal);
lqk_pfb_plan lqk_pfb_fast_plan(int analyzer, int ctaps, unsigned int M, unsigned int p, unsigned long long nblocks,
                               int x16, int y16, int signal);
/* the whole ladder, as the host objects walk it (fast forms first) */
lqk_pfb_plan lqk_firpfbch2_plan(int analyzer, unsigned int M, unsigned int m, unsigned long long nblocks, int p0,
                                int x16, int y16, int signal);
lqk_pfb_plan lqk_firpfbch_plan(int analyzer, int ctaps, unsigned int M, unsigned int p, unsigned long long nblocks,
                               int x16, int y16, int signal);
const char *lqk_pfb_route_name(int route);
/* blocks per launch of the chunking analyzers: liquid_mi355x_set_channelizer_chunk's
 * value (tests only), or dflt when none is set */
long long lqrt_pfb_chunk(long long dflt);

/* ---------------------------------------------------------------- FFT / fftfilt */
/* batched complex FFT of power-of-two size n (2..4096): dir +1 forward, -1 backward */
void lqk_fft_batch(unsigned int n, int dir, const void *x, void *y, unsigned long long batch,
                   void *stream);
/* overlap-save fast convolution: y[t] = scale * sum_k h[k] ext[t-k], t < n;
 * nfft = lqk_fftfilt_nfft(real_io, hlen) (4096-point segments up to 2049
 * taps, 8192 for complex I/O up to 4097 taps, 0: too long);
 * H = FFT_nfft(h zero padded) (unscaled, lqk_fftfilt_make_H); scale = the
 * user scale; hist = previous hlen-1 inputs.  x must not alias y.
 * A transform's rounding error scales with the loudest sample of a segment,
 * not with the inputs each output sees: for fftfilt only (firfilt is held to
 * the direct form's per-output bound, tests/fir_bound.py). */
unsigned int lqk_fftfilt_nfft(int real_io, unsigned int hlen);
void lqk_fftfilt_run(int real_io, unsigned int hlen, unsigned int nfft, const void *H, const void *hist,
                     const void *x, unsigned long long n, void *y, float scale_re, float scale_im,
                     const lqk_hist_job *job, void *stream);
void lqk_fftfilt_make_H(const void *h_dev, unsigned int hlen, int is_complex, unsigned int nfft, void *H,
                        void *stream);

/* ---------------------------------------------------------------- resamp / firpfb
 * Timing plan: checkpoint c = the resampler's timing state before plan input
 * c*LQK_RS_CK and K = outputs emitted by the plan's inputs before it; the
 * state at any other input is the checkpoint before it stepped forward
 * (< LQK_RS_CK inputs).  Power-of-two bank counts store (tau, K) -- the rest
 * of the state is a function of tau there (host/resamp_plan.c) -- other bank
 * counts the whole state (tau, mu, b, state; bst = b*2 + (state == INTERP)).
 * Inputs g >= pre repeat with period P (Q outputs per period): state(g) =
 * state(pre + (g-pre) % P), K += Q per period; positions beyond `end` are
 * clamped to it (direct plans cover end + 1 positions). */
#define LQK_RS_CK 4   /* a checkpoint per replay lane's 4 inputs (csrc/k_resamp.hip k_resamp3) */
typedef struct {
    float tau, mu;
    int bst;
    unsigned int K;
} lqk_rs_entry;
typedef struct {
    float tau;
    unsigned int K;
} lqk_rs_entry_p2;
typedef struct {
    const void *tab;           /* device: lqk_rs_entry_p2[] (p2) or lqk_rs_entry[], checkpoint c at [c] */
    unsigned long long pre, P, Q;
    unsigned long long end;
    int p2;
} lqk_rs_plan;
/* n inputs x (plan positions g0 .. g0+n) -> the nout outputs y[K(g) - K0 ...]
 * (n <= LQK_RS_MAXN, nout * sample size < 2^31);
 * taps: npfb x L pairs (h[b + n*npfb], h[(b+1)%npfb + n*npfb]); hist = last L inputs.
 * real_io: float samples (rrrf), else interleaved complex (crcf, cccf: the taps are real for every type) */
#define LQK_RS_MAXN (1ull << 27)
void lqk_resamp(int real_io, const lqk_rs_plan *pl, unsigned long long g0, unsigned long long K0, unsigned int npfb,
                unsigned int L, float del, const void *taps, const void *taps2, const void *hist, const void *x,
                unsigned long long n, void *y, unsigned long long nout, void *stream);
/* The kernel such a launch takes (with taps2 given) and, in *tile, its inputs
 * per tile: k_resamp3 with the constant or the run-time pair-table stride
 * (tin), k_resamp (8 x 256), k_resamp_generic (256); P, pre, end: the plan's.
 * RS4_*: k_resamp4's rate classes, lqk_resamp4_route (256 outputs per tile) */
enum {
    LQK_RS_ROUTE_R3_CONST = 0, LQK_RS_ROUTE_R3_STRIDE, LQK_RS_ROUTE_RS, LQK_RS_ROUTE_GENERIC,
    LQK_RS_ROUTE_RS4_UP, LQK_RS_ROUTE_RS4_UP_R4, LQK_RS_ROUTE_RS4_DOWN, LQK_RS_ROUTE_RS4_DOWN_DN
};
int lqk_resamp_route(int real_io, unsigned long long P, unsigned long long pre, unsigned long long end,
                     unsigned int npfb, unsigned int L, float del, unsigned int *tile);
/* taps2: (npfb+1) x LP pairs, LP = (L+3) & ~1: row b < npfb (h_b[L-p], h_{b+1}[L-p]) for p = 1..L, row
 * npfb the BOUNDARY pair (h_{npfb-1}[L-1-p], h_0[L-p]); zero elsewhere (NULL: untiled kernel) */
/* Output plan of k_resamp4 (csrc/k_resamp4.hip: complex samples, power-of-two
 * npfb, 1/4 < r <= npfb with one or two outputs per input (any number past
 * r = 2), or an output every one or two (two to four below r = 1/2) inputs,
 * over the whole plan):
 * entries {tau, i} = the timing phase at which a plan output is emitted and
 * the plan input it belongs to -- tab[c] for output 4c (c < npre =
 * ceil(pre / 4)), then tab[npre + c] for output pre + 4c within one period.
 * Outputs k >= pre repeat with period QT outputs / PT inputs (QT >= 256):
 * state(k) = state(pre + (k - pre) % QT) with i += PT per period; pre = ~0:
 * no period (a direct plan; ntab entries cover the plan's outputs). */
typedef struct {
    float tau;
    unsigned int i;
} lqk_rs4_entry;
typedef struct {
    const void *tab;              /* device lqk_rs4_entry[ntab] */
    unsigned long long ntab;
    unsigned long long pre, npre, QT, PT;
} lqk_rs4_plan;
/* msresamp's interpolating chain fused into k_resamp4: the resampler's
 * outputs u feed one half-band interpolator stage (resamp2 interp mode,
 * src/filter/src/resamp2.c:330-360) in registers -- y[2k] = u[k - m],
 * y[2k+1] = sum_j h1[j] u[k+1+j-2m] -- and never reach HBM.  hist: the
 * stage's window before the call (2m samples, oldest first, both of its
 * windows hold the same pushes in interp mode); hist_new0 / hist_new1: its two
 * windows after the call (written by the kernel; nout >= 1). */
#define LQK_RS4_HB_MAXM 12
typedef struct {
    int m;                        /* semi-length: 3 .. LQK_RS4_HB_MAXM */
    float h1[2 * LQK_RS4_HB_MAXM];/* odd taps h1[j] = h[4m-1-2j] (real) */
    const void *hist;
    void *hist_new0, *hist_new1;
} lqk_rs4_hb;
int lqk_resamp4_supported(unsigned int npfb, unsigned int L);
/* the fused chain's shapes: L = 14, npfb = 64, 1 < r < 2, m in 3 .. LQK_RS4_HB_MAXM */
int lqk_resamp4_hb_supported(unsigned int npfb, unsigned int L, float del, int m);
/* the rate class an unfused launch takes (LQK_RS_ROUTE_RS4_*) and, in *tile,
 * the outputs per wave tile; hm > 0: of the fused chain (class UP), whose tiles are shorter by the stage's halo */
int lqk_resamp4_route(float del, int hm, unsigned int *tile);
/* n complex inputs x (plan inputs g0 .. g0+n) -> the nout outputs y[k - K0]
 * for plan outputs k = K0 .. K0+nout-1; taps2 and hist as lqk_resamp.  hb
 * (NULL: none): y receives the half-band stage's 2 nout outputs instead */
void lqk_resamp4(const lqk_rs4_plan *pl, unsigned long long g0, unsigned long long K0, unsigned int npfb,
                 unsigned int L, float del, const void *taps2, const void *hist, const void *x, unsigned long long n,
                 void *y, unsigned long long nout, const lqk_rs4_hb *hb, const lqk_hist_job *job, void *stream);
/* firpfb_execute(i): y = scale * sum_n hpoly[i*L + n] win[L-1-n] (win: L samples, oldest first) */
void lqk_firpfb_single(int kind, const void *hpoly, unsigned int L, unsigned int i, const void *win,
                       float scale_re, float scale_im, void *y, unsigned *flag, unsigned seq, void *stream);

/* ---------------------------------------------------------------- FFT of any size (csrc/k_fft.hip)
 * batch transforms of n points (complex, contiguous), dir +1 forward / -1
 * backward, unnormalised; x may alias y.  work: lqk_fft_work_bytes(n, batch)
 * bytes of device scratch (NULL when 0). */
size_t lqk_fft_work_bytes(unsigned int n, unsigned long long batch);
void lqk_fft_any(unsigned int n, int dir, const void *x, void *y, unsigned long long batch, void *work,
                 void *stream);
/* The kernels lqk_fft_any takes for n points read from a pointer that is or is
 * not 16-byte aligned -- the decision the launches themselves switch on
 * (lq_fft_batch_scaled, fft_four_step, lqk_fft_any).  a16: the 16-byte loads of
 * the 8192- and 16384-point kernels; N1 x N2: the two-pass split of n
 * (FOUR_STEP) or of M (BLUESTEIN_FUSED), columns k_fft2p_cols_r / k_bs_cols_r
 * <N1 / 256>, rows k_bs_rows_s<N2 / 16> when rows_s, else k_fft2p_rows_r /
 * k_bs_rows_r<N2 / 256>; M: Bluestein's padded size (its M-point transforms go
 * by lqk_fft_route(M) when not fused). */
enum {
    LQK_FFT_REFUSED = 0,          /* n = 0 or past 2^24 (2^23 when not a power of two) */
    LQK_FFT_DFT = 1,              /* k_dft_batch: n = 1 and other n <= 16 */
    LQK_FFT_BATCH = 2,            /* k_fft_batch<n>: 2, 4, 8, 16 */
    LQK_FFT_SMALL = 3,            /* k_fftsmall_batch<n / 16>: 32, 64, 128 */
    LQK_FFT_R16 = 4,              /* k_fftr16_batch<n / 256>: 256, 512, 2048 */
    LQK_FFT_1024 = 5,
    LQK_FFT_4096 = 6,
    LQK_FFT_8192 = 7,
    LQK_FFT_16384 = 8,
    LQK_FFT_FOUR_STEP = 9,        /* powers of two from 32768 */
    LQK_FFT_BLUESTEIN = 10,       /* M <= 4096: k_bs_pre, M-point transform, k_bs_mul, back, k_bs_post */
    LQK_FFT_BLUESTEIN_FUSED = 11, /* M > 4096: chirp products fused into the two-pass kernels */
};
typedef struct {
    int family, a16, rows_s;
    unsigned int N1, N2;
    unsigned long long M;
} lqk_fft_route_t;
lqk_fft_route_t lqk_fft_route(unsigned int n, int aligned16);
/* real-to-real (fft_r2r_1d.c): type codes as liquid_fft_type (10-13 DCT, 20-23 DST); x must not alias y */
enum {
    LQK_R2R_REDFT00 = 10, LQK_R2R_REDFT10 = 11, LQK_R2R_REDFT01 = 12, LQK_R2R_REDFT11 = 13,
    LQK_R2R_RODFT00 = 20, LQK_R2R_RODFT10 = 21, LQK_R2R_RODFT01 = 22, LQK_R2R_RODFT11 = 23,
};
void lqk_fft_r2r(int type, unsigned int n, const void *x, void *y, unsigned long long batch, void *stream);

/* ---------------------------------------------------------------- spgram (csrc/k_spgram.hip)
 * gather: out[t][i] = ext[ends[t]+1+i] w[i] (i < W, zero to nfft), ext = hist(W) ++ x;
 * accumulate: psd = (1-a) psd + a |X_t|^2 in t order; sum: acc[shift(k)] += sum_t |X_t[k]|^2;
 * db: mode 0 10log10(|X|^2+1e-16) shifted, 1 10log10(v) shifted, 2 10log10(v/T) */
void lqk_spgram_gather(int real_in, const void *hist, unsigned int W, const void *x, const long long *ends,
                       unsigned long long T, const float *w, unsigned int nfft, void *out, void *stream);
/* per-bin reductions over T transforms; work: lqk_spgram_work_bytes(T, nfft) bytes of device scratch */
size_t lqk_spgram_work_bytes(unsigned long long T, unsigned int nfft);
void lqk_spgram_accumulate(const void *X, unsigned long long T, unsigned int nfft, float alpha, float *psd,
                           void *work, void *stream);
void lqk_spgram_sum(const void *X, unsigned long long T, unsigned int nfft, float *acc, void *work, void *stream);
/* nfft = 1024 (W <= 1024): windows gathered from (hist | x), transformed and reduced in one pass;
 * transform t ends at e0 + t*hop (the last at elast); accum: dst = psd (exponential average),
 * else dst = acc (sum, fft-shifted); work: lqk_spgram_work_bytes(T, 1024) bytes */
void lqk_spgram_fused1024(int real_in, const void *hist, unsigned int W, const void *x, long long e0,
                          long long hop, unsigned long long T, long long elast, const float *w, int accum,
                          float alpha, float *dst, void *work, void *stream);
/* the launches' own decisions, for the tests: the path of a call of n samples (0: gather, batch
 * transform, k_spg_part; else k_spg_fused1024<S, HALF, TR> as 1 + 2 HALF + 4 TR), the transforms
 * per chunk and the chunks per first-level fold group (more chunks fold in two levels) */
int lqk_spgram_route(int real_in, unsigned int nfft, unsigned int W, unsigned long long n);
unsigned int lqk_spgram_chunk(void);
unsigned int lqk_spgram_fold_group(void);
void lqk_spgram_db(int mode, const void *X, const float *v, unsigned int nfft, float T, float *out, void *stream);

/* ---------------------------------------------------------------- resamp2 (half-band)
 * n calls of one resamp2 mode (src/filter/src/resamp2.c:273-356).  hist0/hist1 =
 * the two 2m-sample windows (oldest first); the updated windows go to
 * hist0_new/hist1_new (must not alias).  taps: the 2m odd taps h1[j] = h[4m-1-2j]
 * (float for kind 0/1, float2 for kind 2).  Outputs: filter y0[i], y1[i];
 * decim y0[i] (times scale, a power of two); analyzer/interp/synthesizer
 * y0[2i], y0[2i+1].  t0: filter-mode toggle before the first call. */
enum { LQK_R2_FILTER = 0, LQK_R2_ANALYZER, LQK_R2_SYNTHESIZER, LQK_R2_DECIM, LQK_R2_INTERP };
/* the kernel a launch of this mode, m and bytes of x takes (-1: bad arguments) and its calls per workgroup */
enum { LQK_R2_ROUTE_FILTER = 0, LQK_R2_ROUTE_TILED_B, LQK_R2_ROUTE_TILED };
int lqk_resamp2_route(int mode, unsigned int m, unsigned long long xbytes);
unsigned int lqk_resamp2_route_tile(int route);
void lqk_resamp2(int kind, int mode, unsigned int m, int t0, float scale, const void *taps, const void *hist0,
                 const void *hist1, void *hist0_new, void *hist1_new, const void *x, unsigned long long n,
                 void *y0, void *y1, void *stream);

/* ---------------------------------------------------------------- firhilbf (Hilbert transform)
 * n calls of one firhilbf mode (src/filter/src/firhilb.c:168-301).  hist0/hist1 =
 * the two windows of 2m floats (oldest first); the updated windows go to
 * hist0_new/hist1_new (must not alias).  taps: the 2m quadrature taps
 * hq[j] = h[4m-1-2j].  decim: x 2n floats, y n complex; interp: x n complex,
 * y 2n floats; r2c: x n floats, y n complex, t0 the toggle before the first
 * call.  x and y must not overlap.  LQK_FIRHILB_TILE: calls per workgroup. */
enum { LQK_FH_DECIM = 0, LQK_FH_INTERP, LQK_FH_R2C };
#define LQK_FIRHILB_TILE 1024
#define LQK_FIRHILB_MAXM 2048   /* the tile's windows and the taps in 64 KB of LDS */
void lqk_firhilb(int mode, unsigned int m, int t0, const void *taps, const void *hist0, const void *hist1,
                 void *hist0_new, void *hist1_new, const void *x, unsigned long long n, void *y, void *stream);
/* c2r: y[i] = Re x[i] */
void lqk_firhilb_c2r(const void *x, unsigned long long n, void *y, void *stream);

/* ---------------------------------------------------------------- iirfilt (recursive filters)
 * n samples through a cascade of nsec <= LQK_IIRFILT_MAXSEC direct-form-II
 * second-order sections (src/filter/src/iirfiltsos.c:167-184), block-parallel
 * (k_iirfilt.hip).  kind 0 rrrf, 1 crcf, 2 cccf; samples S = float / float2,
 * coefficients K = float (kind 0, 1) / float2.  With MS = lqk_iirfilt_maxsec(nsec)
 * (nsec rounded up to a power of two) and PM = 2 MS:
 *   coef    5 nsec K: b0, b1, b2, a1, a2 per section (a0 = 1)
 *   ladder  LQK_IIRFILT_LEVELS matrices of PM x PM K, row-major: ladder[k] =
 *           G^(2^k), G the map of the state over LQK_IIRFILT_RUN samples of
 *           zero input
 *   state   2 nsec S: v[1], v[2] of each section for the coming sample; read,
 *           and left as after sample n-1
 *   work    lqk_iirfilt_work_bytes(kind, nsec, n) bytes
 * x == y allowed.  LQK_IIRFILT_RUN: consecutive samples per lane;
 * LQK_IIRFILT_TILE: samples per workgroup; LQK_IIRFILT_SCAN: tiles per block
 * of the cross-tile scan (more tiles than that: two scan levels). */
#define LQK_IIRFILT_MAXSEC 8
#define LQK_IIRFILT_RUN 16
#define LQK_IIRFILT_TILE 4096
#define LQK_IIRFILT_SCAN 256
#define LQK_IIRFILT_LEVELS 23
unsigned int lqk_iirfilt_maxsec(unsigned int nsec);
size_t lqk_iirfilt_work_bytes(int kind, unsigned int nsec, unsigned long long n);
/* launches of a piece of n full-rate samples: 0 apply alone (at most one tile), 1 one scan launch (at
 * most LQK_IIRFILT_SCAN tiles), 2 three scan launches */
int lqk_iirfilt_route(unsigned long long n);
void lqk_iirfilt(int kind, unsigned int nsec, const void *coef, const void *ladder, void *state, const void *x,
                 unsigned long long n, void *y, void *work, void *stream);
/* The same filter as a rate changer by M, 1 <= M <= LQK_IIRFILT_TILE, with the
 * same coef / ladder / state / work contracts; work is sized by the full-rate
 * sample count (n_in for the decimator, n_in M for the interpolator).
 *   decim   x: n_in samples, n_in a multiple of M; y: n_in / M samples, the
 *           filter's outputs at the indices that are multiples of M.  x and y
 *           must not overlap.
 *   interp  x: n_in samples; y: n_in M samples, the filter's outputs for x[i]
 *           followed by M - 1 zeros each.  x and y must not overlap.
 * The state is left as after the last full-rate sample. */
void lqk_iirfilt_decim(int kind, unsigned int nsec, const void *coef, const void *ladder, void *state, const void *x,
                       unsigned long long n_in, unsigned int M, void *y, void *work, void *stream);
void lqk_iirfilt_interp(int kind, unsigned int nsec, const void *coef, const void *ladder, void *state, const void *x,
                        unsigned long long n_in, unsigned int M, void *y, void *work, void *stream);

/* ---------------------------------------------------------------- autocorr (k_autocorr.hip)
 * rxx[i] = sum_{k=i-W+1..i} s[k] conj(s[k-d]) (cx; else s[k] s[k-d]) and, when
 * e2 is not NULL, e2[i] = sum_{k=i-W+1..i} |s[k]|^2, i < n, over the stream
 * s = hist ++ x: hist holds the H = W + d samples before x, oldest first (the
 * block outputs read the last H - 1 of them; the single output below reads all).
 * Every output is the sum of its own W terms and of nothing else.  hist_new
 * receives the last H samples of s (must not alias hist).  x must not overlap
 * rxx or e2.  1 <= W <= LQK_AUTOCORR_MAXW, W + d < 2^31.
 * LQK_AUTOCORR_TILE: outputs per workgroup. */
#define LQK_AUTOCORR_TILE 2048
#define LQK_AUTOCORR_MAXW 4096
void lqk_autocorr(int cx, unsigned int W, unsigned long long d, const void *hist, const void *x,
                  unsigned long long n, void *rxx, float *e2, void *hist_new, void *stream);
/* the output at the last sample of hist: out = rxx (1 or 2 floats), then e2;
 * any W.  With a flag, out is pinned host memory and the kernel raises
 * *flag = seq once it is visible to the host; flag may be NULL. */
void lqk_autocorr_single(int cx, unsigned int W, unsigned long long d, const void *hist, float *out,
                         unsigned *flag, unsigned seq, void *stream);

/* ---------------------------------------------------------------- nco (k_nco.hip)
 * y[i] = x[i] (cos th_i +- j sin th_i), i < n <= LQK_NCO_MAXN, th_i the
 * oscillator's float32 phase before sample i, replayed from a phase plan
 * (host/nco_plan.c): tab[c] = the phase before plan position c * LQK_NCO_CK;
 * any other position is the checkpoint before it stepped forward (th += d_theta
 * in float32, one wrap by 2 pi computed in double) fewer than LQK_NCO_CK times.
 * Sample i stands at plan position p0 + i; with P > 0 positions >= pre repeat
 * with period P (position g means pre + (g - pre) % P; p0 < pre + P; th_pre =
 * the phase at pre) and tab covers [0, pre + P); with P == 0 tab covers
 * [0, p0 + n).  vco == 0: sin th = sintab[k], cos th = sintab[(k + 64) & 255],
 * k the reference's table index of th (sintab: 256 floats in device memory);
 * vco != 0: sinf / cosf of th.  down: the conjugate rotator.  x == y allowed;
 * otherwise they must not overlap.  LQK_NCO_TILE: samples per workgroup. */
#define LQK_NCO_CK 64
#define LQK_NCO_TILE 2048
#define LQK_NCO_MAXN (1ull << 30)
typedef struct {
    const float *tab;
    unsigned long long p0, pre, P;
    float d_theta, th_pre;
} lqk_nco_plan;
void lqk_nco_mix(int vco, int down, const lqk_nco_plan *pl, const float *sintab, const void *x, void *y,
                 unsigned long long n, void *stream);

/* ---------------------------------------------------------------- freqmod / freqdem (k_freqmodem.hip)
 * freqmod: phase_i = acc_in[0] + sum_{k <= i} inc(m[k]) modulo 2^16, inc(m) =
 * (int)roundf(ref * m) reduced modulo 2^16 (0 where the product is not finite
 * or reaches 2^31 in magnitude); s[i] = tab[((phase_i + 0x20) >> 6) & 0x3ff],
 * tab 1024 complex values in device memory, 16-byte aligned; acc_out[0] =
 * phase_{n-1}.  n <= LQK_FREQMOD_MAXN; sums: ceil(n / LQK_FREQMOD_TILE) words of
 * scratch; m and s must not overlap.  LQK_FREQMOD_TILE: samples per workgroup;
 * LQK_FREQMOD_PASS: tile sums per pass of the one-workgroup scan across tiles.
 * freqdem: m[i] = arg(conj(p_i) r[i]) * ref, p_i = r[i - M] or, for i < M,
 * hist[i] (hist: the M samples before the call, oldest first); hist_out: the
 * last M samples of hist ++ r (not hist itself).  M < LQK_FREQDEM_SWITCH: a
 * tile of LQK_FREQDEM_TILE samples per workgroup with the halo in LDS; else a
 * lane walks LQK_FREQDEM_FRAMES frames of its own channel. */
#define LQK_FREQMOD_TILE 2048
#define LQK_FREQMOD_PASS 1024
#define LQK_FREQMOD_MAXN (1ull << 30)
#define LQK_FREQDEM_TILE 2048
#define LQK_FREQDEM_SWITCH 128
#define LQK_FREQDEM_FRAMES 16
#define LQK_FREQDEM_MAXN (1ull << 30)
void lqk_freqmod(float ref, const void *tab, const unsigned *acc_in, unsigned *acc_out, unsigned *sums,
                 const float *m, void *s, unsigned long long n, void *stream);
void lqk_freqdem(float ref, unsigned M, const void *hist, void *hist_out, const void *r, float *m,
                 unsigned long long n, void *stream);

/* ---------------------------------------------------------------- detector (k_detector.hip)
 * The correlator bank of detector_cccf over the stream s = hist ++ x (hist:
 * the len samples before x, oldest first; hist_new receives the last len of s
 * and must not alias hist).  For sample t < n with window w = s[t-len+1 .. t]:
 *   c_k = sum_i p_k[i] w[i], E = sum_i |w[i]|^2, r_k = |c_k| / sqrt(len E)
 * (0 where E == 0), each a float32 sum of its own window, i = 0 .. len-1 in
 * order.  pt: the templates tap-major and zero padded, pt[i * m + k] = p_k[i]
 * for i < len, 0 for len <= i < LQK_DETECTOR_PADLEN(len), complex, 16-byte
 * aligned device memory.  drxy: NULL or n * m floats, row t = r_0 .. r_{m-1}.
 * With nt = ceil(n / LQK_DETECTOR_TILE) tiles, list is device memory of
 * LQK_DETECTOR_LIST_WORDS(m, nt, cap) 32-bit words: word 0 is the number of
 * marked samples (zeroed by the launch itself before the kernel); from word
 * LQK_DETECTOR_LIST_HEAD on, one word of flags per tile (bit 0 / 2: the largest
 * r_k of the tile's first / last sample exceeds thr; bit 1 / 3: that sample is
 * marked); then the first cap records of 2 + m words each, in no particular
 * order: t, E, r_0 .. r_{m-1}.  Marked: the samples whose largest r_k exceeds
 * thr, the samples next to one in the same tile, and the first and last sample
 * of the call.  edge: device memory, 2 nt records of the same form: the first
 * and the last sample of every tile.  1 <= len <= LQK_DETECTOR_MAXLEN, 2 <= m
 * <= LQK_DETECTOR_MAXM, n < 2^31. */
#define LQK_DETECTOR_TILE 2048
#define LQK_DETECTOR_MAXLEN 2048
#define LQK_DETECTOR_MAXM 16
#define LQK_DETECTOR_LIST_HEAD 4
#define LQK_DETECTOR_PADLEN(len) (((len) + 3u) & ~3u)
#define LQK_DETECTOR_LIST_WORDS(m, nt, cap) (LQK_DETECTOR_LIST_HEAD + (size_t)(nt) + (size_t)(cap) * (2u + (m)))
void lqk_detector(unsigned int len, unsigned int m, float thr, const void *pt, const void *hist, const void *x,
                  unsigned long long n, float *drxy, unsigned int *list, unsigned int cap, unsigned int *edge,
                  void *hist_new, void *stream);

/* ---------------------------------------------------------------- qdetector (k_qdetector.hip)
 * The stream a call sees is ext = carry (clen samples) ++ x.  seek: the records
 * (4 words each: peak, index, offset, energy; rec 16-byte aligned device or
 * pinned host memory) of the nw windows ext[pos + w nfft/2 .. + nfft), each a
 * function of its own nfft samples, S (FFT of the zero-padded template), range,
 * s_len and s2_sum alone.  nfft a power of two >= 2, 2 range + 1 <= nfft.
 * route: lqk_qdetector_route(nfft) -- FUSED (nfft = 512: 32 lanes per window,
 * nfft = 1024: one wave), nothing but the record leaves the CU, scratch unused
 * (a FUSED launch of any other nfft is refused); COMPOSED (any nfft):
 * gather, lqk_fft_any, shifted products for nb offsets at a time (at most
 * LQK_QD_PRODUCT_SAMPLES values, at least one offset), lqk_fft_any back, fold;
 * scratch: lqk_qdetector_scratch_bytes(nfft, range, nw, &nb) bytes. */
enum { LQK_QD_ROUTE_COMPOSED = 0, LQK_QD_ROUTE_FUSED = 1 };
#define LQK_QD_PRODUCT_SAMPLES (1ull << 23)
int lqk_qdetector_route(unsigned int nfft);
size_t lqk_qdetector_scratch_bytes(unsigned int nfft, int range, unsigned long long nw, unsigned int *nb);
void lqk_qdetector_seek(int route, unsigned int nfft, unsigned int s_len, float s2_sum, int range, const void *S,
                        const void *carry, unsigned long long clen, const void *x, unsigned long long pos,
                        unsigned long long nw, void *scratch, void *rec, void *stream);
/* S = FFT(s_padded) (nfft values each); work: lqk_fft_work_bytes(nfft, 1) */
void lqk_qdetector_spectrum(unsigned int nfft, const void *s_padded, void *S, void *work, void *stream);
/* align stage over the frame ext[pos .. pos + nfft): frame receives it; out13 =
 * (re, im) of IFFT(X conj(S shifted by offset)) at lags -1, 0, +1, the first
 * arg-max bin i0 of FFT(frame conj(s) zero padded), (re, im) of its bins i0 - 1,
 * i0, i0 + 1.  scratch: lqk_qdetector_align_bytes(nfft); its first nfft values
 * are left holding frame conj(s), which lqk_qdetector_metric sums as
 * sum_{i < s_len} . exp(-j dphi i) into out2 (fixed order) */
size_t lqk_qdetector_align_bytes(unsigned int nfft);
void lqk_qdetector_align(unsigned int nfft, unsigned int s_len, int offset, const void *S, const void *s,
                         const void *carry, unsigned long long clen, const void *x, unsigned long long pos,
                         void *frame, void *scratch, void *out13, void *stream);
void lqk_qdetector_metric(unsigned int s_len, float dphi, const void *scratch, void *out2, void *stream);

#ifdef __cplusplus
}
#endif

#endif
