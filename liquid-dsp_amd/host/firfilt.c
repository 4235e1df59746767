/*
 * firfilt.c -- firfilt_{rrrf,crcf,cccf} on the MI355X.
 *
 * API and semantics: include/liquid.h:1985-2090, src/filter/src/firfilt.c:62-404
 *   y[t] = scale * sum_{k<h} h[k] x[t-k], zero initial history;
 *   push() appends one sample, execute() reads the current window without
 *   pushing, execute_block() = push+execute per sample (in place allowed).
 *
 * State model.  The filter state is the window of the last HP samples
 * (HP = length padded to the kernel's chunk class), oldest first, kept on
 * the device with a pinned host mirror for the per-sample push() path
 * (lq_hist, PINNED).  Exactly one copy is authoritative at a time; the other
 * is refreshed lazily.  Outside the small-call mode every output sample,
 * including the per-sample execute(), is computed by a HIP kernel.
 */
#include <complex.h>
#include <math.h>

#include "lq_host.h"

struct lq_firfilt_s {
    int kind;
    unsigned int hlen, HP;
    size_t esz;        /* sample size: 4 (rrrf) or 8 */
    size_t csz;        /* coefficient size: 4 or 8 (cccf) */
    float *h;          /* natural-order coefficients (host copy) */
    float *hg;         /* reversed, expanded for the host path (lq_host_taps) */
    void *d_hpad;      /* device, zero padded to HP */
    lqk_fir_desc d;
    lq_hist win;       /* the window, HP samples; pinned: the per-sample execute() reads it in place */
    lq_ctx ctx;
    lq_devbuf xbuf, ybuf, scratch, one;
    const char *who;   /* the public object name, for error messages */
};

static void lq_firfilt_layout(lq_firfilt *q, unsigned int n)
{
    q->hlen = n;
    if (n <= 16) {
        q->d.hc = 16;
        q->d.nchunk = 1;
    } else if (n <= 32) {
        q->d.hc = 32;
        q->d.nchunk = 1;
    } else {
        q->d.hc = 64;
        q->d.nchunk = (n + 63) / 64;
    }
    q->HP = q->d.hc * q->d.nchunk;
    q->d.hlen = n;
    /* the direct kernel holds a tile plus the HP-sample history in LDS:
       refuse at create time what no launch could run (fftfilt's long-filter
       path lands here too) */
    if (q->HP > lqk_firfilt_max_history(q->d.kind))
        LQ_FAIL("error: %s_create(), filter length %u exceeds the GPU kernel limit of %u taps\n", q->who, n,
                lqk_firfilt_max_history(q->d.kind));
}

static void lq_firfilt_alloc_state(lq_firfilt *q)
{
    q->d_hpad = lqrt_malloc((size_t)q->HP * q->csz);
    lq_hist_init(&q->win, q->HP, q->esz, LQ_HIST_PINNED);
}

static void lq_firfilt_free_state(lq_firfilt *q)
{
    lqrt_free(q->d_hpad);
    lq_hist_free(&q->win);
}

static void lq_firfilt_upload_coefs(lq_firfilt *q)
{
    size_t bytes = (size_t)q->HP * q->csz;
    unsigned char *pad = (unsigned char *)lq_xmalloc(bytes);
    memcpy(pad, q->h, (size_t)q->hlen * q->csz);
    lqrt_h2d(q->d_hpad, pad, bytes, q->ctx.stream);
    lqrt_sync(q->ctx.stream);
    free(pad);
    q->d.hpad = q->d_hpad;
    /* the matrix-core kernel splits taps into three bf16 terms; outside
     * [2^-50, 2^50] (or non-finite) the split would lose float32 accuracy or
     * the reference's Inf/NaN propagation, so such filters stay on the VALU
     * kernel */
    const unsigned int nv = q->hlen * (unsigned int)(q->csz / sizeof(float));
    q->d.mx_ok = 1;
    for (unsigned int i = 0; i < nv; i++) {
        const float a = fabsf(q->h[i]);
        if (!(a <= 0x1p50f) || (a != 0.0f && a < 0x1p-50f)) q->d.mx_ok = 0;
    }
}

lq_firfilt *lq_firfilt_create(int kind, const float *h, unsigned int n, const char *who)
{
    if (n == 0) LQ_FAIL("error: %s_create(), filter length must be greater than zero\n", who);
    lqrt_require_device(who);
    lq_firfilt *q = (lq_firfilt *)lq_xmalloc(sizeof(*q));
    q->kind = kind;
    q->esz = lq_esz(kind);
    q->csz = lq_csz(kind);
    q->d.kind = kind;
    q->d.scale_re = 1.0f;
    q->d.scale_im = 0.0f;
    q->who = who;
    lq_firfilt_layout(q, n);
    q->h = (float *)lq_xmalloc((size_t)n * q->csz);
    memcpy(q->h, h, (size_t)n * q->csz);
    q->hg = lq_host_taps(kind, q->h, n, 1);
    lq_ctx_init(&q->ctx);
    lq_firfilt_alloc_state(q);
    lq_firfilt_upload_coefs(q);
    return q;
}

/* src/filter/src/firfilt.c:201-237: new taps; a length change restarts the
 * buffer (the reference leaves it uninitialised; here it is cleared) */
lq_firfilt *lq_firfilt_recreate(lq_firfilt *q, const float *h, unsigned int n)
{
    if (n == 0) LQ_FAIL("error: firfilt_recreate(), filter length must be greater than zero\n");
    lqrt_sync(q->ctx.stream);
    if (n != q->hlen) {
        lq_firfilt_free_state(q);
        lq_firfilt_layout(q, n);
        free(q->h);
        q->h = (float *)lq_xmalloc((size_t)n * q->csz);
        lq_firfilt_alloc_state(q);
    }
    memcpy(q->h, h, (size_t)n * q->csz);
    free(q->hg);
    q->hg = lq_host_taps(q->kind, q->h, n, 1);
    lq_firfilt_upload_coefs(q);
    return q;
}

void lq_firfilt_destroy(lq_firfilt *q)
{
    lqrt_sync(q->ctx.stream);
    lq_firfilt_free_state(q);
    lq_devbuf_free(&q->xbuf);
    lq_devbuf_free(&q->ybuf);
    lq_devbuf_free(&q->scratch);
    lq_devbuf_free(&q->one);
    lq_ctx_free(&q->ctx);
    free(q->h);
    free(q->hg);
    free(q);
}

void lq_firfilt_reset(lq_firfilt *q) { lq_hist_zero(&q->win, q->ctx.stream); }

void lq_firfilt_print(lq_firfilt *q)
{
    printf("firfilt_%s:\n", lq_ext(q->kind));
    for (unsigned int i = 0; i < q->hlen; i++) {
        if (q->kind == LQ_CCCF)
            printf("  h(%3u) = %12.8f + j*%12.8f\n", i + 1, q->h[2 * i], q->h[2 * i + 1]);
        else
            printf("  h(%3u) = %12.8f\n", i + 1, q->h[i]);
    }
    if (q->kind == LQ_CCCF)
        printf("  scale = %12.8f + j*%12.8f\n", q->d.scale_re, q->d.scale_im);
    else
        printf("  scale = %12.8f\n", q->d.scale_re);
}

void lq_firfilt_set_scale(lq_firfilt *q, float re, float im)
{
    q->d.scale_re = re;
    q->d.scale_im = im;
}

/* the window moves up one sample in the host mirror (the reference's window.c
 * likewise appends and only moves the window back when its buffer is full) */
void lq_firfilt_push(lq_firfilt *q, const void *x)
{
    lq_hist_append(&q->win, x, 1, q->ctx.stream);
    lq_hist_commit(&q->win, 1);
}

/* one output from the current window: the kernel reads the window where it
 * is authoritative -- in place from the pinned host mirror after push()es,
 * or the device copy after a device block -- and writes the result to
 * pinned host memory and raises the completion flag itself (one launch, no
 * stream sync) */
void lq_firfilt_execute(lq_firfilt *q, void *y)
{
    if (lq_small_host()) {   /* the host path (lq_small.c) */
        /* the last hlen window samples, oldest first, against the reversed taps */
        const unsigned char *w = lq_hist_host(&q->win, q->ctx.stream) + (size_t)(q->HP - q->hlen) * q->esz;
        lq_host_tdot(q->kind, q->hg, w, q->hlen, y);
        lq_host_scale(q->kind, q->d.scale_re, q->d.scale_im, (float *)y);
        return;
    }
    unsigned *flag, seq;
    void *py = lq_sig_out(&q->ctx, q->esz, &flag, &seq);
    lqk_fir_single(&q->d, lq_hist_read(&q->win), py, flag, seq, q->ctx.stream);
    lq_sig_wait(&q->ctx, y, q->esz, seq);
}

/* device-resident block: window update first (reads x before an in-place
 * overwrite), then the filter kernel on the old window's last HP-1 samples.
 * Every filter length and block size runs the direct kernels: each output is
 * one float32 sum over its own hlen inputs, as in the reference
 * (firfilt.c:322-338), so its error is proportional to the inputs it sees and
 * does not depend on how the caller cuts the stream
 * (tests/test_gpu_fir_bound.py).  An overlap-save transform form for long
 * complex filters was withdrawn: its rounding error scales with the loudest
 * sample of a whole 4096- or 8192-point segment.  fftfilt,
 * transform-based in the reference too, keeps it. */
void lq_firfilt_execute_block_dev(lq_firfilt *q, const void *dx, unsigned long long n, void *dy)
{
    if (n == 0) return;
    void *wold = lq_hist_dev(&q->win, q->ctx.stream), *wnew = lq_hist_next(&q->win);
    void *scr = NULL;
    if (dx == dy) scr = lq_devbuf_get(&q->scratch, lqk_firfilt_scratch_bytes(&q->d, n));
    /* the window update: inside the matrix-core kernel, else launched first */
    const lqk_hist_job job = {wold, dx, n, wnew, q->HP};
    lqk_firfilt(&q->d, wold, dx, n, dy, scr, &job, q->ctx.stream);
    lq_hist_flip(&q->win);
}

void lq_firfilt_execute_block(lq_firfilt *q, const void *x, unsigned long long n, void *y)
{
    if (n == 0) return;
    size_t bytes = (size_t)n * q->esz;
    const void *dx = lq_call_in(&q->ctx, &q->xbuf, x, bytes);
    void *dy = lq_devbuf_get(&q->ybuf, bytes);
    lq_firfilt_execute_block_dev(q, dx, n, dy);
    lq_call_out(&q->ctx, y, dy, bytes);
}

unsigned int lq_firfilt_get_length(lq_firfilt *q) { return q->hlen; }

/* firfilt.c:371-387: H = scale * sum_i hr[i] e^{j 2 pi fc i}, hr = the
 * reference's internally reversed taps (host arithmetic, as the reference) */
static void lq_firfilt_freqresponse(lq_firfilt *q, float fc, liquid_float_complex *H)
{
    float complex acc = 0.0f;
    const unsigned int n = q->hlen;
    for (unsigned int i = 0; i < n; i++) {
        const unsigned int k = n - 1 - i;
        const float complex hk = q->kind == LQ_CCCF ? q->h[2 * k] + _Complex_I * q->h[2 * k + 1] : q->h[k];
        acc += hk * cexpf(_Complex_I * 2 * M_PI * fc * i);
    }
    acc *= q->d.scale_re + _Complex_I * q->d.scale_im;
    *H = acc;
}

/* firfilt.c:393-404 and group_delay.c:34-56 (real parts of the taps) */
static float lq_firfilt_groupdelay(lq_firfilt *q, float fc)
{
    const unsigned int n = q->hlen;
    if (fc < -0.5 || fc > 0.5) LQ_FAIL("error: fir_group_delay(), _fc must be in [-0.5,0.5]\n");
    float complex t0 = 0.0f, t1 = 0.0f;
    for (unsigned int i = 0; i < n; i++) {
        const float hi = q->kind == LQ_CCCF ? q->h[2 * i] : q->h[i];
        t0 += hi * cexpf(_Complex_I * 2 * M_PI * fc * i) * i;
        t1 += hi * cexpf(_Complex_I * 2 * M_PI * fc * i);
    }
    return crealf(t0 / t1);
}
lq_ctx *lq_firfilt_ctx(lq_firfilt *q) { return &q->ctx; }

/* ----------------------------------------------------------------- typed front ends */

/* from real design taps hf (taken over) */
static lq_firfilt *lq_firfilt_create_real(int kind, float *hf, unsigned int n, const char *who)
{
    float *h = lq_taps_from_real(kind, hf, n);
    lq_firfilt *f = lq_firfilt_create(kind, h, n, who);
    free(h);
    return f;
}

#define LQ_FIRFILT_FRONT(NAME, KIND, TO, TC, TI, SCALE_RE, SCALE_IM)                                \
    struct NAME##_s {                                                                               \
        lq_firfilt *f;                                                                              \
    };                                                                                              \
    static NAME NAME##_wrap(lq_firfilt *f)                                                          \
    {                                                                                               \
        NAME q = (NAME)lq_xmalloc(sizeof(*q));                                                      \
        q->f = f;                                                                                   \
        return q;                                                                                   \
    }                                                                                               \
    NAME NAME##_create(TC *_h, unsigned int _n)                                                     \
    {                                                                                               \
        return NAME##_wrap(lq_firfilt_create(KIND, (const float *)_h, _n, #NAME));                  \
    }                                                                                               \
    NAME NAME##_create_kaiser(unsigned int _n, float _fc, float _As, float _mu)                     \
    {                                                                                               \
        if (_n == 0) LQ_FAIL("error: " #NAME "_create_kaiser(), filter length must be greater than zero\n"); \
        float *hf = (float *)lq_xmalloc(_n * sizeof(float));                                        \
        lq_firdes_kaiser(_n, _fc, _As, _mu, hf);                                                    \
        return NAME##_wrap(lq_firfilt_create_real(KIND, hf, _n, #NAME));                            \
    }                                                                                               \
    NAME NAME##_create_rect(unsigned int _n)                                                        \
    {                                                                                               \
        if (_n == 0 || _n > 1024) LQ_FAIL("error: " #NAME "_create_rect(), filter length must be in [1,1024]\n"); \
        float *hf = (float *)lq_xmalloc(_n * sizeof(float));                                        \
        for (unsigned int i = 0; i < _n; i++) hf[i] = 1.0f;                                         \
        return NAME##_wrap(lq_firfilt_create_real(KIND, hf, _n, #NAME));                            \
    }                                                                                               \
    /* firfilt.c:140-171: 2km+1 taps from liquid_firdes_prototype */                                \
    NAME NAME##_create_rnyquist(int _type, unsigned int _k, unsigned int _m, float _beta, float _mu)\
    {                                                                                               \
        if (_k < 2) LQ_FAIL("error: " #NAME "_create_rnyquist(), filter samples/symbol must be greater than 1\n");\
        if (_m == 0) LQ_FAIL("error: " #NAME "_create_rnyquist(), filter delay must be greater than 0\n");\
        if (_beta < 0.0f || _beta > 1.0f)                                                           \
            LQ_FAIL("error: " #NAME "_create_rnyquist(), filter excess bandwidth factor must be in [0,1]\n");\
        const unsigned int n = 2 * _k * _m + 1;                                                     \
        float *hf = (float *)lq_xmalloc(n * sizeof(float));                                         \
        liquid_firdes_prototype((liquid_firfilt_type)_type, _k, _m, _beta, _mu, hf);                \
        return NAME##_wrap(lq_firfilt_create_real(KIND, hf, n, #NAME));                             \
    }                                                                                               \
    NAME NAME##_recreate(NAME _q, TC *_h, unsigned int _n)                                          \
    {                                                                                               \
        _q->f = lq_firfilt_recreate(_q->f, (const float *)_h, _n);                                  \
        return _q;                                                                                  \
    }                                                                                               \
    void NAME##_destroy(NAME _q)                                                                    \
    {                                                                                               \
        lq_firfilt_destroy(_q->f);                                                                  \
        free(_q);                                                                                   \
    }                                                                                               \
    void NAME##_reset(NAME _q) { lq_firfilt_reset(_q->f); }                                         \
    void NAME##_print(NAME _q) { lq_firfilt_print(_q->f); }                                         \
    void NAME##_set_scale(NAME _q, TC _scale) { lq_firfilt_set_scale(_q->f, SCALE_RE, SCALE_IM); }  \
    void NAME##_push(NAME _q, TI _x) { lq_firfilt_push(_q->f, &_x); }                               \
    void NAME##_execute(NAME _q, TO *_y) { lq_firfilt_execute(_q->f, _y); }                         \
    void NAME##_execute_block(NAME _q, TI *_x, unsigned int _n, TO *_y)                             \
    {                                                                                               \
        lq_firfilt_execute_block(_q->f, _x, _n, _y);                                                \
    }                                                                                               \
    unsigned int NAME##_get_length(NAME _q) { return lq_firfilt_get_length(_q->f); }                \
    void NAME##_freqresponse(NAME _q, float _fc, liquid_float_complex *_H)                          \
    {                                                                                               \
        lq_firfilt_freqresponse(_q->f, _fc, _H);                                                    \
    }                                                                                               \
    float NAME##_groupdelay(NAME _q, float _fc) { return lq_firfilt_groupdelay(_q->f, _fc); }        \
    void NAME##_execute_block_dev(NAME _q, const TI *_dx, unsigned long long _n, TO *_dy)           \
    {                                                                                               \
        lq_firfilt_execute_block_dev(_q->f, _dx, _n, _dy);                                          \
    }                                                                                               \
    void NAME##_set_stream(NAME _q, void *_s) { lq_ctx_set_stream(lq_firfilt_ctx(_q->f), _s); }     \
    void *NAME##_get_stream(NAME _q) { return lq_firfilt_ctx(_q->f)->stream; }                      \
    void NAME##_synchronize(NAME _q) { lqrt_sync(lq_firfilt_ctx(_q->f)->stream); }

LQ_FIRFILT_FRONT(firfilt_rrrf, LQ_RRRF, float, float, float, _scale, 0.0f)
LQ_FIRFILT_FRONT(firfilt_crcf, LQ_CRCF, liquid_float_complex, float, liquid_float_complex, _scale, 0.0f)
LQ_FIRFILT_FRONT(firfilt_cccf, LQ_CCCF, liquid_float_complex, liquid_float_complex, liquid_float_complex,
                 crealf(_scale), cimagf(_scale))
