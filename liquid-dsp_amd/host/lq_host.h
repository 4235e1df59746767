/*
 * lq_host.h -- internal helpers shared by the C host objects.
 *
 * The objects keep the reference's create/execute/destroy contract
 * (include/liquid.h) and its failure style (message on stderr, exit(1)).
 * All sample arithmetic happens in the HIP kernels behind csrc/lq_kernels.h;
 * the host side only designs coefficients (create time, as the reference
 * does), validates arguments, moves buffers and tracks per-object state --
 * except the opt-in small-call mode (lq_small.c: LQ_SMALL_CALLS=host), in
 * which single-sample calls compute on the host.
 */
#ifndef LQ_HOST_H
#define LQ_HOST_H

#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../csrc/lq_kernels.h"
#include "liquid_mi355x.h"

#define LQ_FAIL(...)                                                                               \
    do {                                                                                           \
        fprintf(stderr, __VA_ARGS__);                                                              \
        exit(1);                                                                                   \
    } while (0)

/* sample kinds (also the kernel `kind` codes) */
enum { LQ_RRRF = 0, LQ_CRCF = 1, LQ_CCCF = 2 };

/* bytes per sample / per coefficient, and the type suffix of a kind */
static inline size_t lq_esz(int kind) { return kind == LQ_RRRF ? 4 : 8; }
static inline size_t lq_csz(int kind) { return kind == LQ_CCCF ? 8 : 4; }
static inline const char *lq_ext(int kind) { return kind == LQ_RRRF ? "rrrf" : (kind == LQ_CRCF ? "crcf" : "cccf"); }

/* grow-on-demand device buffer */
typedef struct {
    void *p;
    size_t cap;
} lq_devbuf;

void *lq_devbuf_get(lq_devbuf *b, size_t bytes);
void lq_devbuf_free(lq_devbuf *b);

/* per-object execution context: a HIP stream (owned unless supplied) and
 * the pinned host staging of the per-call (host-pointer) API */
typedef struct {
    void *stream;
    int own;
    void *pin_in, *pin_out;   /* pinned host buffers (lazily allocated) */
    size_t in_cap, out_cap;
    unsigned *flag;           /* pinned completion word */
    unsigned seq;
    int in_busy;              /* pin_in may still be read by queued kernels */
} lq_ctx;

void lq_ctx_init(lq_ctx *c);
void lq_ctx_free(lq_ctx *c);
void lq_ctx_set_stream(lq_ctx *c, void *stream);

/* Host-pointer calls (the reference's own API, which returns with the result
 * in host memory).  lq_call_in stages x: up to LQ_PIN_IN bytes are copied
 * into pinned host memory that the kernels then read in place (no copy
 * command), larger inputs go to device buffer b by DMA; returns the pointer
 * to hand to the device path.  lq_call_out delivers a device result of up to
 * LQRT_COPYOUT_MAX bytes through one copy-out kernel + completion flag
 * (spin-wait, no stream synchronisation), larger ones by DMA + sync.
 * lq_call_done waits for a call without a result. */
#define LQ_PIN_IN (256u << 10)
const void *lq_call_in(lq_ctx *c, lq_devbuf *b, const void *x, size_t bytes);
void lq_call_out(lq_ctx *c, void *y, const void *dy, size_t bytes);
void lq_call_done(lq_ctx *c);
/* single results (firfilt/firpfb/dotprod execute) whose kernel writes the
 * pinned result itself and raises the flag: lq_sig_out returns the pinned
 * destination, the flag word and the sequence number to hand to the kernel;
 * lq_sig_wait spins for it and copies the result to y */
void *lq_sig_out(lq_ctx *c, size_t bytes, unsigned **flag, unsigned *seq);
void lq_sig_wait(lq_ctx *c, void *y, size_t bytes, unsigned seq);

/* opt-in host path for single-sample calls (host/lq_small.c) */
int lq_small_host(void);
void lq_host_dot(int kind, const float *h, const void *x, unsigned int n, void *y);
float *lq_host_taps(int kind, const float *h, unsigned int n, int rev);
void lq_host_tdot(int kind, const float *g, const void *x, unsigned int n, void *y);
/* y *= scale: a real scale per component (rrrf, crcf; firfilt.c:337), a
 * complex one (cccf) */
static inline void lq_host_scale(int kind, float sre, float sim, float *y)
{
    if (kind == LQ_CCCF) {
        const float a = y[0], b = y[1];
        y[0] = a * sre - b * sim;
        y[1] = a * sim + b * sre;
        return;
    }
    y[0] *= sre;
    if (kind == LQ_CRCF) y[1] *= sre;
}
/* real design taps in a kind's coefficient layout: hf itself, or for cccf
 * its (h, 0) pairs with hf freed; the caller frees the result */
float *lq_taps_from_real(int kind, float *hf, unsigned int n);

/* host copy of a device-resident history of n samples; pinned: the buffer is
 * pinned host memory, which a kernel may read in place */
typedef struct {
    unsigned char *buf;
    size_t n, esz, cap, off;   /* history = n samples at buf + off*esz */
    int pinned;
    int host_valid, dev_valid;
} lq_mirror;
void lq_mirror_init(lq_mirror *m, size_t n, size_t esz, int pinned);
void lq_mirror_free(lq_mirror *m);
void lq_mirror_zero(lq_mirror *m);
void lq_mirror_need_host(lq_mirror *m, const void *dev_hist, void *stream);
void lq_mirror_need_dev(lq_mirror *m, void *dev_hist, void *stream);
void lq_mirror_append(lq_mirror *m, const void *x, size_t k);
/* after an append of k samples: keep the last n */
static inline void lq_mirror_commit(lq_mirror *m, size_t k) { m->off += k; }
static inline unsigned char *lq_mirror_ptr(lq_mirror *m) { return m->buf + m->off * m->esz; }

/* The streaming history of an object (host/lq_hist.c): the last n samples,
 * oldest first, in two device buffers used ping-pong -- a block call reads
 * the current one, its kernel (or lqk_window_append) writes the other, and
 * lq_hist_flip makes that one current -- plus, by mode, a host mirror for
 * the calls that compute on the host (MIRROR), in pinned memory where the
 * single-output kernels read the window in place (PINNED).  Whichever side
 * ran last is authoritative; the other is refreshed on demand.  n may be 0. */
enum { LQ_HIST_DEV = 0, LQ_HIST_MIRROR = 1, LQ_HIST_PINNED = 2 };
typedef struct {
    void *d[2];
    int cur, mode;
    lq_mirror m;
} lq_hist;
void lq_hist_init(lq_hist *h, size_t n, size_t esz, int mode);
/* an object whose per-sample calls need no GPU: MIRROR mode with the host side
 * only (no runtime call); lq_hist_attach, before the first device use, adds
 * the device pair (once; the mirror stays authoritative) */
void lq_hist_init_host(lq_hist *h, size_t n, size_t esz);
void lq_hist_attach(lq_hist *h);
void lq_hist_free(lq_hist *h);
void lq_hist_zero(lq_hist *h, void *stream);   /* both sides zero and in step; waits for the stream */
void *lq_hist_dev(lq_hist *h, void *stream);   /* the current device buffer, brought up to date */
const void *lq_hist_read(lq_hist *h);          /* the window where it is authoritative: the device
                                                  buffer, or (PINNED) the host window after appends */
static inline void *lq_hist_next(lq_hist *h) { return h->d[h->cur ^ 1]; }
/* after the launch that wrote lq_hist_next: it is current, the host copy stale */
static inline void lq_hist_flip(lq_hist *h)
{
    h->cur ^= 1;
    h->m.host_valid = 0;
}
/* host side: the window of n samples, up to date (after a device block this
 * waits for the device) */
static inline unsigned char *lq_hist_host(lq_hist *h, void *stream)
{
    if (!h->m.host_valid) lq_mirror_need_host(&h->m, h->d[h->cur], stream);
    return lq_mirror_ptr(&h->m);
}
/* ... with k samples appended: n + k samples, newest last; lq_hist_commit
 * then keeps the last n */
static inline unsigned char *lq_hist_append(lq_hist *h, const void *x, size_t k, void *stream)
{
    lq_hist_host(h, stream);
    lq_mirror_append(&h->m, x, k);
    return lq_mirror_ptr(&h->m);
}
static inline void lq_hist_commit(lq_hist *h, size_t k) { lq_mirror_commit(&h->m, k); }

void *lq_xmalloc(size_t bytes);
unsigned int lq_msb_index(unsigned int x);
int lq_is_pow2(unsigned int x);

/* host-side design routines (create time only; src/filter/src/firdes.c) */
float lq_kaiser_beta_As(float As);
void lq_firdes_kaiser(unsigned int n, float fc, float As, float mu, float *h);
float lq_sincf(float x);                                                   /* math.c:128-139 */
float lq_kaiser_window(unsigned int n, unsigned int N, float beta, float mu); /* math.c:289-312 */

/* generic firfilt engine used by the three typed front ends */
typedef struct lq_firfilt_s lq_firfilt;
lq_firfilt *lq_firfilt_create(int kind, const float *h, unsigned int n, const char *who);
lq_firfilt *lq_firfilt_recreate(lq_firfilt *q, const float *h, unsigned int n);
void lq_firfilt_destroy(lq_firfilt *q);
void lq_firfilt_reset(lq_firfilt *q);
void lq_firfilt_print(lq_firfilt *q);
void lq_firfilt_set_scale(lq_firfilt *q, float re, float im);
void lq_firfilt_push(lq_firfilt *q, const void *x);
void lq_firfilt_execute(lq_firfilt *q, void *y);
void lq_firfilt_execute_block(lq_firfilt *q, const void *x, unsigned long long n, void *y);
void lq_firfilt_execute_block_dev(lq_firfilt *q, const void *dx, unsigned long long n, void *dy);
unsigned int lq_firfilt_get_length(lq_firfilt *q);
lq_ctx *lq_firfilt_ctx(lq_firfilt *q);

/* recursive filter engine (host/iirfilt.c) as the rate changers use it
 * (host/iirdecim.c).  mode 1: decimate by M (n M samples in, n out, the first
 * output of each group of M); mode 2: interpolate by M (n in, n M out, M - 1
 * zeros fed after each input).  small: the call is a single execute, which
 * follows the small-call rule.  rate_eligible: block calls run on the GPU. */
typedef struct lq_iir_s lq_iir;
lq_iir *lq_iir_create(int kind, const void *b, unsigned int nb, const void *a, unsigned int na);
lq_iir *lq_iir_create_prototype(int kind, liquid_iirdes_filtertype ftype, liquid_iirdes_bandtype btype,
                                liquid_iirdes_format format, unsigned int order, float fc, float f0, float Ap,
                                float As);
void lq_iir_destroy(lq_iir *q);
void lq_iir_print(lq_iir *q);
void lq_iir_reset(lq_iir *q);
float lq_iir_groupdelay(lq_iir *q, float fc);
int lq_iir_rate_eligible(lq_iir *q, unsigned int M);
lq_ctx *lq_iir_ctx(lq_iir *q);
void lq_iir_run_rate(lq_iir *q, int mode, unsigned int M, const void *x, unsigned long long n, void *y, int small);
void lq_iir_run_rate_dev(lq_iir *q, int mode, unsigned int M, const void *dx, unsigned long long n, void *dy);

/* ---- the resampler's timing plan (host/resamp_plan.c): float32 timing
 * arithmetic only -- no runtime call, no kernel launch, libc and libm alone */
enum { RS_BOUNDARY = 0, RS_INTERP = 1 };
enum { RS_D3 = 3, RS_D4 = 4 };        /* device table: input checkpoints (k_resamp3) / output plan (k_resamp4) */

typedef struct {
    float tau, mu;
    int b, st;
} rs_state;

static const rs_state rs_initial = {0.0f, 0.0f, 0, RS_INTERP};   /* resamp.c:181-195 */

static inline int rs_eq(const rs_state *a, const rs_state *b)
{
    return memcmp(&a->tau, &b->tau, 4) == 0 && memcmp(&a->mu, &b->mu, 4) == 0 && a->b == b->b && a->st == b->st;
}

/* One input of resamp.c:245-311 with the data path removed, in the three
 * pieces every user composes; float32 arithmetic exactly as the reference
 * (the library is compiled with -ffp-contract=off).
 *
 * rs_due: is an output due at this state?  resamp.c:254 compares int b with
 * unsigned npfb: the comparison is unsigned, so a negative b (a BOUNDARY
 * update that leaves tau < 0, only when del < 1/npfb) ends the input, and
 * rs_end_input's decrement (unsigned arithmetic there too) keeps b negative
 * until it wraps modulo 2^32.  An INTERP state at the last bank turns
 * BOUNDARY and waits for the next input (resamp.c:280-285). */
static inline int rs_due(rs_state *s, unsigned int npfb)
{
    if ((unsigned int)s->b >= npfb) return 0;
    if (s->st == RS_INTERP && s->b == (int)npfb - 1) {
        s->st = RS_BOUNDARY;
        s->b = (int)npfb;
        return 0;
    }
    return 1;
}

/* advance after an output (resamp.c:352-363) */
static inline void rs_advance(rs_state *s, float del, unsigned int npfb)
{
    s->tau += del;
    const float bf = s->tau * (float)npfb;
    s->b = (int)floorf(bf);
    s->mu = bf - (float)s->b;
    s->st = RS_INTERP;
}

/* end the input (resamp.c:305-307) */
static inline void rs_end_input(rs_state *s, unsigned int npfb)
{
    s->tau -= 1.0f;
    s->b = (int)((unsigned int)s->b - npfb);
}

/* the whole input; returns its number of outputs */
static inline unsigned int rs_step(rs_state *s, float del, unsigned int npfb)
{
    unsigned int n = 0;
    while (rs_due(s, npfb)) {
        n++;
        rs_advance(s, del, npfb);
    }
    rs_end_input(s, npfb);
    return n;
}

/* the tau-only form of the timing (resamp_plan.c) holds at this rate */
int rs_tau_only(float del, unsigned int npfb);
/* outputs of the next nx inputs from state s */
unsigned long long rs_count_outputs(rs_state s, float del, unsigned int npfb, unsigned long long nx);

/* A plan: position g counts inputs from `origin`; rs_plan_at gives the state
 * before input g and K = outputs of the inputs before it.  Periodic plans
 * cover every g (inputs >= pre repeat every P inputs / Q outputs), direct
 * plans g <= end.  The device table is dn entries of desz bytes at dtab
 * (lqk_rs_entry_p2 when p2, else lqk_rs_entry, for dk == RS_D3; lqk_rs4_entry
 * for RS_D4, whose outputs >= opre repeat every QT outputs / PT inputs,
 * entries [npre, ..) theirs). */
typedef struct {
    float del;
    unsigned int npfb;
    int p2;                       /* tau-only timing (rs_tau_only) */
    int valid, periodic;
    rs_state origin;
    lqk_rs_entry *tab;            /* host: state at plan position c * RS_HCK (K lookups) */
    size_t nck, cap;
    unsigned long long pre, P, Q, end;
    int dk;                       /* device table kind (RS_D3 / RS_D4) */
    unsigned char *dtab;          /* the table, until rs_plan_drop_table */
    size_t dn, desz;
    unsigned long long opre, npre, QT, PT;
} rs_plan;

void rs_plan_init(rs_plan *pl);
void rs_plan_free(rs_plan *pl);
void rs_plan_drop_table(rs_plan *pl);   /* the device table's host copy (once uploaded) */
/* want_d4: record an output plan where the timing allows, else (and as the
 * fall-back) input checkpoints.  periodic: 1, or 0 if the orbit has no
 * period within the search limit (nothing is left allocated); direct: the
 * next nx inputs: 1, 0 if their outputs do not fit 32 bits, -1 if no table
 * could be made (nothing is left allocated either way) */
int rs_plan_build_periodic(rs_plan *pl, float del, unsigned int npfb, rs_state origin, int want_d4);
int rs_plan_build_direct(rs_plan *pl, float del, unsigned int npfb, rs_state origin, unsigned long long nx,
                         int want_d4);
rs_state rs_plan_at(const rs_plan *pl, unsigned long long g, unsigned long long *K);

/* arbitrary-rate resampler engine (host/resamp.c), used by msresamp */
typedef struct lq_rs_s lq_rs;
lq_rs *lq_rs_create(int kind, float rate, unsigned int m, float fc, float As, unsigned int npfb);
void lq_rs_destroy(lq_rs *q);
void lq_rs_reset(lq_rs *q);
unsigned long long lq_rs_num_output(lq_rs *q, unsigned long long nx);
void lq_rs_block_dev(lq_rs *q, const void *dx, unsigned long long nx, void *dy, unsigned long long *ny);
/* msresamp's interpolating chain: the resampler followed by one half-band
 * interpolator stage (resamp2 interp mode), fused into k_resamp4 where the
 * plan allows (lqk_resamp4_hb_supported) and run as two kernels otherwise */
typedef struct {
    int m;                        /* the stage's semi-length */
    float h1[LQK_RS4_HB_MAXM * 2];/* its odd taps (real) */
    void *w[2][2];                /* its ping-pong windows [buffer][window] */
    int *cur;                     /* its current buffer, flipped per fused launch */
    void (*run)(void *ctx, const void *u, unsigned long long n, void *y);   /* the stage alone: n -> 2n */
    void *ctx;
} lq_rs_hb;
void lq_rs_block_dev_hb(lq_rs *q, const void *dx, unsigned long long nx, void *dy, unsigned long long *ny,
                        const lq_rs_hb *hb);
lq_ctx *lq_rs_ctx(lq_rs *q);
/* Host only: the kernel (LQK_RS_ROUTE_*) and tile of the first block call of
 * nx inputs on a fresh engine, by the plan policy and launch decision the
 * calls use; hm > 0: with a half-band stage of that semi-length behind it,
 * *fused whether the launch takes the stage along.  -1: bad arguments */
int lq_rs_route(int kind, float rate, unsigned int m, unsigned int npfb, unsigned long long nx, int hm,
                unsigned int *tile, int *fused);

/* ---- the oscillator's phase plan (host/nco_plan.c): float32 phase
 * arithmetic only -- no runtime call, no kernel launch, libc and libm alone */
#define NCO_PI 3.14159265358979323846

/* one step of nco.c:134-138 + 355-361: a float32 add, comparisons against the
 * double pi, one wrap by 2 pi computed in double and rounded once */
static inline float nco_step_theta(float th, float d)
{
    th += d;
    if (th > NCO_PI) th -= 2 * NCO_PI;
    else if (th < -NCO_PI) th += 2 * NCO_PI;
    return th;
}

/* the sine table's index of a phase (nco.c:372): three separately rounded
 * float32 operations (the library is compiled with -ffp-contract=off) */
static inline unsigned int nco_table_index(float th)
{
    return ((unsigned int)(th * 40.743665f + 512.0f + 0.5f)) & 0xff;
}

static inline int nco_same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

/* A plan belongs to one orbit: the phases theta0, step(theta0), ... at
 * positions 0, 1, ...; tab[c] = the phase at position c * LQK_NCO_CK.  A
 * direct plan covers positions 0 .. end; a periodic one every position:
 * positions >= pre repeat every P (the phase at g is the phase at
 * pre + (g - pre) % P), tab covers [0, pre + P) and th_pre is the phase at pre. */
typedef struct {
    float theta0, d_theta;
    int valid, periodic;
    float *tab;
    size_t ntab, cap;
    unsigned long long pre, P, end;
    float th_pre;
} nco_plan;

void nco_plan_init(nco_plan *pl);
void nco_plan_free(nco_plan *pl);
/* the next n positions from theta0; 1, or 0 when out of memory (nothing is left allocated) */
int nco_plan_build_direct(nco_plan *pl, float theta0, float d_theta, unsigned long long n);
/* pre-period and period by cycle detection; 0 when pre + P would exceed cap
 * positions (nothing is left allocated) */
int nco_plan_build_periodic(nco_plan *pl, float theta0, float d_theta, unsigned long long cap);
/* the table position that serves position g (g itself below pre + P) */
unsigned long long nco_plan_reduce(const nco_plan *pl, unsigned long long g);
/* the phase at position g: the checkpoint before it stepped forward */
float nco_plan_at(const nco_plan *pl, unsigned long long g);

/* ---- qdetector's walk (host/qdetector_walk.c): the decisions over window
 * records, the realignment arithmetic and the closed-form estimates -- no
 * runtime call, no kernel launch, libc and libm alone.
 *
 * A call sees the stream ext = (the `counter` samples carried from earlier
 * calls) ++ (its n new samples), `total` long.  `base` is the ext position of
 * the seek grid's origin (SEEK: windows start at base + w nfft/2) or of the
 * frame being aligned (ALIGN).  qdw_next names the next piece of device work;
 * qdw_seek takes the records of windows base, base + nfft/2, ... in order and
 * stops at the first detection; qdw_align_fit / qdw_align_finish take the
 * align stage's scalars and restart the grid half a buffer into the frame;
 * qdw_end leaves ext[base .. total) as the next call's carried samples. */
enum { QDW_SEEK = 0, QDW_ALIGN = 1 };
enum { QDW_DO_SEEK = 0, QDW_DO_ALIGN = 1, QDW_DO_END = 2 };
typedef struct {
    unsigned int nfft, s_len;
    float s2_sum, threshold;
    int range;
    /* carried between calls */
    int state;
    unsigned int counter;             /* samples held: SEEK [nfft/2, nfft), ALIGN (s_len, nfft) */
    int offset;                       /* coarse carrier offset of the frame being aligned */
    float tau_hat, gamma_hat, dphi_hat, phi_hat;
    /* within a call */
    unsigned long long total, base, c0;
} qd_walk;

void qdw_init(qd_walk *w, unsigned int nfft, unsigned int s_len, float s2_sum);
void qdw_reset(qd_walk *w);           /* the state after create; threshold and range stay */
int qdw_set_threshold(qd_walk *w, float threshold);   /* 0: out of range, ignored */
int qdw_set_range(qd_walk *w, float dphi_max);
void qdw_begin(qd_walk *w, unsigned long long n);
/* DO_SEEK: *count whole windows from ext position *pos; DO_ALIGN: the frame's
 * nfft samples start at *pos; DO_END: *count samples from *pos are carried */
int qdw_next(const qd_walk *w, unsigned long long *pos, unsigned long long *count);
/* records of the nrec windows from base; returns how many of them the seek
 * stage completed (the detecting one is the last) */
unsigned long long qdw_seek(qd_walk *w, const qdetector_cccf_record *rec, unsigned long long nrec);
int qdw_detects(const qd_walk *w, const qdetector_cccf_record *rec);
/* rxy: (re, im) of the lags -1, 0, +1 at the coarse offset, unscaled; i0: the
 * arg-max bin of FFT(x conj s); v: (re, im) of the bins i0 - 1, i0, i0 + 1 */
void qdw_align_fit(qd_walk *w, const float rxy[6], unsigned int i0, const float v[6]);
/* metric: the de-rotation sum; returns the index within this call of the
 * sample that completed the frame.  After qdw_begin(w, 0) on a full buffer
 * (execute(): the completing sample arrived before the call) there is no such
 * sample and ~0ull is returned */
unsigned long long qdw_align_finish(qd_walk *w, float mre, float mim);
void qdw_end(qd_walk *w);
/* the closed forms (qdetector_cccf.c:504-514, 553-562) */
void qdw_fit_tau_gamma(float aneg, float a0, float apos, unsigned int nfft, float s2_sum, float *tau, float *gamma);
float qdw_fit_dphi(unsigned int i0, float vneg, float v0, float vpos, unsigned int nfft);

/* generic dotprod engine */
typedef struct lq_dotprod_s lq_dotprod;
lq_dotprod *lq_dotprod_create(int kind, const float *h, unsigned int n);
lq_dotprod *lq_dotprod_recreate(lq_dotprod *q, const float *h, unsigned int n);
void lq_dotprod_destroy(lq_dotprod *q);
void lq_dotprod_print(lq_dotprod *q);
void lq_dotprod_execute_batch(lq_dotprod *q, const void *X, unsigned long long nvec, void *Y);
void lq_dotprod_execute_batch_dev(lq_dotprod *q, const void *dX, unsigned long long nvec, void *dY);
void lq_dotprod_run(int kind, const float *h, const void *x, unsigned int n, void *y);
lq_ctx *lq_dotprod_ctx(lq_dotprod *q);

#endif
