/*
 * autocorr.c -- autocorr_{cccf,rrrf} on the MI355X.
 *
 * API and semantics: include/liquid.h:1908-1970, src/filter/src/autocorr.c:41-172
 *   push() appends one sample; execute() returns
 *     rxx = sum_{k=n-W+1..n} x[k] conj(x[k-d])     (n the last sample pushed)
 *   without pushing; execute_block() = push + execute per sample (in place
 *   allowed); samples before the last reset are zero.
 *
 * State model.  The object's state is the last H = W + d samples, oldest
 * first -- what the reference keeps in its delayed window -- as one lq_hist in
 * mirror mode: on the device for the block kernel (k_autocorr.hip), with a
 * host mirror for push() and the single calls.  (A block call reads only the
 * last H - 1 of them; execute() after a push needs x[n-W+1-d], the H-th.)
 *
 * get_energy() is the float32 sum of |x|^2 over the last W samples of the
 * history, computed when asked.  The reference keeps a running sum instead
 * (autocorr.c:123-127: add the newest, subtract the oldest), whose rounding
 * error grows over the life of the stream; that accumulator is not replayed.
 *
 * A window longer than the kernel takes (LQK_AUTOCORR_MAXW) runs block calls
 * in a host loop over the mirror, one lq_host_dot per output.
 */
#include <complex.h>

#include "lq_host.h"

typedef struct {
    int kind;                 /* LQ_CCCF or LQ_RRRF */
    unsigned int W;
    unsigned long long d, H;
    size_t esz;
    int eligible;             /* block calls run on the GPU */
    lq_hist hist;             /* the last H samples */
    lq_ctx ctx;
    lq_devbuf xbuf, ybuf;
    float *ext, *cj;          /* host loop: hist ++ x and its conjugate (grown on demand) */
    size_t ext_cap;
    const char *who;
} lq_autocorr;

static lq_autocorr *lq_autocorr_create(int kind, unsigned int W, unsigned int d, const char *who)
{
    /* the reference fails in its window object (window.c:47-52) */
    if (W == 0) LQ_FAIL("error: %s_create(), window size must be greater than zero\n", who);
    lqrt_require_device(who);
    lq_autocorr *q = (lq_autocorr *)lq_xmalloc(sizeof(*q));
    memset(q, 0, sizeof(*q));
    q->kind = kind;
    q->W = W;
    q->d = d;
    q->H = (unsigned long long)W + d;
    if (q->H > 0x7fffffffull) LQ_FAIL("error: %s_create(), window size + delay must be less than 2^31\n", who);
    q->esz = lq_esz(kind);
    q->eligible = W <= LQK_AUTOCORR_MAXW;
    q->who = who;
    lq_ctx_init(&q->ctx);
    lq_hist_init(&q->hist, (size_t)q->H, q->esz, LQ_HIST_MIRROR);
    return q;
}

static void lq_autocorr_destroy(lq_autocorr *q)
{
    lqrt_sync(q->ctx.stream);
    lq_hist_free(&q->hist);
    lq_devbuf_free(&q->xbuf);
    lq_devbuf_free(&q->ybuf);
    lq_ctx_free(&q->ctx);
    free(q->ext);
    free(q->cj);
    free(q);
}

static void lq_autocorr_reset(lq_autocorr *q) { lq_hist_zero(&q->hist, q->ctx.stream); }

static void lq_autocorr_print(lq_autocorr *q)
{
    printf("autocorr [%u window, %u delay]\n", q->W, (unsigned int)q->d);
}

static void lq_autocorr_push(lq_autocorr *q, const void *x)
{
    lq_hist_append(&q->hist, x, 1, q->ctx.stream);
    lq_hist_commit(&q->hist, 1);
}

/* host scratch for nf floats in q->ext (and q->cj for complex samples) */
static void lq_autocorr_scratch(lq_autocorr *q, size_t nf)
{
    if (nf <= q->ext_cap) return;
    free(q->ext);
    free(q->cj);
    q->ext_cap = nf;
    q->ext = (float *)lq_xmalloc(nf * sizeof(float));
    q->cj = q->kind == LQ_CCCF ? (float *)lq_xmalloc(nf * sizeof(float)) : NULL;
}

/* rxx of the W samples at w against the W samples at wd (d samples earlier),
 * on the host: lq_host_dot multiplies without conjugating, so complex samples
 * go through a conjugated copy of the delayed window (cj: W samples) */
static void lq_autocorr_host_dot(const lq_autocorr *q, const float *w, const float *wd, float *cj, void *y)
{
    if (q->kind == LQ_RRRF) {
        lq_host_dot(LQ_RRRF, wd, w, q->W, y);
        return;
    }
    for (unsigned int i = 0; i < q->W; i++) {
        cj[2 * i] = wd[2 * i];
        cj[2 * i + 1] = -wd[2 * i + 1];
    }
    lq_host_dot(LQ_CCCF, cj, w, q->W, y);
}

/* sum |x|^2 of the W samples at w */
static float lq_autocorr_host_energy(const lq_autocorr *q, const float *w)
{
    float e;
    lq_host_dot(LQ_RRRF, w, w, q->W * (unsigned int)(q->esz / sizeof(float)), &e);
    return e;
}

/* the single outputs (small-call rule, lq_small.c): on the host over the
 * mirror, or one launch over the history; out = rxx (1 or 2 floats), e2 */
static void lq_autocorr_single(lq_autocorr *q, float *out)
{
    const size_t nf = q->esz / sizeof(float);
    if (lq_small_host()) {
        const float *h = (const float *)lq_hist_host(&q->hist, q->ctx.stream);
        const float *w = h + (size_t)q->d * nf;
        lq_autocorr_scratch(q, (size_t)q->W * nf);
        lq_autocorr_host_dot(q, w, h, q->cj, out);
        out[nf] = lq_autocorr_host_energy(q, w);
        return;
    }
    unsigned *flag, seq;
    const size_t bytes = (nf + 1) * sizeof(float);
    float *po = (float *)lq_sig_out(&q->ctx, bytes, &flag, &seq);
    lqk_autocorr_single(q->kind == LQ_CCCF, q->W, q->d, lq_hist_dev(&q->hist, q->ctx.stream), po, flag, seq,
                        q->ctx.stream);
    lq_sig_wait(&q->ctx, out, bytes, seq);
}

static void lq_autocorr_execute(lq_autocorr *q, void *rxx)
{
    float out[3];
    lq_autocorr_single(q, out);
    memcpy(rxx, out, q->esz);
}

static float lq_autocorr_get_energy(lq_autocorr *q)
{
    float out[3];
    lq_autocorr_single(q, out);
    return out[q->esz / sizeof(float)];
}

/* the host loop (W above the kernel's limit): host pointers, e2 may be NULL,
 * rxx == x allowed (the outputs are formed from the copy in ext) */
static void lq_autocorr_block_host(lq_autocorr *q, const void *x, unsigned long long n, void *rxx, float *e2)
{
    const size_t nf = q->esz / sizeof(float), H = (size_t)q->H;
    lq_autocorr_scratch(q, (H + (size_t)n) * nf);
    memcpy(q->ext, lq_hist_host(&q->hist, q->ctx.stream), H * q->esz);
    memcpy(q->ext + H * nf, x, (size_t)n * q->esz);
    lq_hist_append(&q->hist, x, (size_t)n, q->ctx.stream);
    lq_hist_commit(&q->hist, (size_t)n);
    if (q->kind == LQ_CCCF)
        for (size_t i = 0; i < H + (size_t)n; i++) {
            q->cj[2 * i] = q->ext[2 * i];
            q->cj[2 * i + 1] = -q->ext[2 * i + 1];
        }
    /* sample k of the call is ext[H + k]: output i reads the window from
     * ext[H + i - W + 1] and the delayed one from ext[i + 1] */
    for (size_t i = 0; i < (size_t)n; i++) {
        const float *w = q->ext + (H + i + 1 - q->W) * nf;
        if (q->kind == LQ_CCCF)
            lq_host_dot(LQ_CCCF, q->cj + (i + 1) * nf, w, q->W, (float *)rxx + i * nf);
        else
            lq_host_dot(LQ_RRRF, q->ext + (i + 1), w, q->W, (float *)rxx + i);
        if (e2) e2[i] = lq_autocorr_host_energy(q, w);
    }
}

static void lq_autocorr_execute_block_dev(lq_autocorr *q, const void *dx, unsigned long long n, void *drxx, float *de2)
{
    if (n == 0) return;
    if (q->eligible) {
        void *hold = lq_hist_dev(&q->hist, q->ctx.stream), *hnew = lq_hist_next(&q->hist);
        lqk_autocorr(q->kind == LQ_CCCF, q->W, q->d, hold, dx, n, drxx, de2, hnew, q->ctx.stream);
        lq_hist_flip(&q->hist);
        return;
    }
    /* device pointers on an object the kernel does not take: through the host loop */
    const size_t bytes = (size_t)n * q->esz;
    unsigned char *hx = (unsigned char *)lq_xmalloc(bytes);
    float *he = de2 ? (float *)lq_xmalloc((size_t)n * sizeof(float)) : NULL;
    lqrt_d2h(hx, dx, bytes, q->ctx.stream);
    lqrt_sync(q->ctx.stream);
    lq_autocorr_block_host(q, hx, n, hx, he);
    lqrt_h2d(drxx, hx, bytes, q->ctx.stream);
    if (de2) lqrt_h2d(de2, he, (size_t)n * sizeof(float), q->ctx.stream);
    lqrt_sync(q->ctx.stream);
    free(hx);
    free(he);
}

static void lq_autocorr_execute_block(lq_autocorr *q, const void *x, unsigned long long n, void *rxx)
{
    if (n == 0) return;
    if (!q->eligible) {
        lq_autocorr_block_host(q, x, n, rxx, NULL);
        return;
    }
    const size_t bytes = (size_t)n * q->esz;
    const void *dx = lq_call_in(&q->ctx, &q->xbuf, x, bytes);
    void *dy = lq_devbuf_get(&q->ybuf, bytes);
    lq_autocorr_execute_block_dev(q, dx, n, dy, NULL);
    lq_call_out(&q->ctx, rxx, dy, bytes);
}

/* ----------------------------------------------------------------- typed front ends */

#define LQ_AUTOCORR_FRONT(NAME, KIND, T)                                                            \
    struct NAME##_s {                                                                               \
        lq_autocorr *f;                                                                             \
    };                                                                                              \
    NAME NAME##_create(unsigned int _window_size, unsigned int _delay)                              \
    {                                                                                               \
        lq_autocorr *f = lq_autocorr_create(KIND, _window_size, _delay, #NAME);                     \
        NAME q = (NAME)lq_xmalloc(sizeof(*q));                                                      \
        q->f = f;                                                                                   \
        return q;                                                                                   \
    }                                                                                               \
    void NAME##_destroy(NAME _q)                                                                    \
    {                                                                                               \
        lq_autocorr_destroy(_q->f);                                                                 \
        free(_q);                                                                                   \
    }                                                                                               \
    void NAME##_reset(NAME _q) { lq_autocorr_reset(_q->f); }                                        \
    void NAME##_print(NAME _q) { lq_autocorr_print(_q->f); }                                        \
    void NAME##_push(NAME _q, T _x) { lq_autocorr_push(_q->f, &_x); }                               \
    void NAME##_execute(NAME _q, T *_rxx) { lq_autocorr_execute(_q->f, _rxx); }                     \
    void NAME##_execute_block(NAME _q, T *_x, unsigned int _n, T *_rxx)                             \
    {                                                                                               \
        lq_autocorr_execute_block(_q->f, _x, _n, _rxx);                                             \
    }                                                                                               \
    float NAME##_get_energy(NAME _q) { return lq_autocorr_get_energy(_q->f); }                      \
    void NAME##_execute_block_dev(NAME _q, const T *_dx, unsigned long long _n, T *_drxx, float *_de2) \
    {                                                                                               \
        lq_autocorr_execute_block_dev(_q->f, _dx, _n, _drxx, _de2);                                 \
    }                                                                                               \
    int NAME##_device_eligible(NAME _q) { return _q->f->eligible; }                                 \
    void NAME##_set_stream(NAME _q, void *_s) { lq_ctx_set_stream(&_q->f->ctx, _s); }               \
    void NAME##_synchronize(NAME _q) { lqrt_sync(_q->f->ctx.stream); }

LQ_AUTOCORR_FRONT(autocorr_cccf, LQ_CCCF, liquid_float_complex)
LQ_AUTOCORR_FRONT(autocorr_rrrf, LQ_RRRF, float)

unsigned int liquid_mi355x_autocorr_tile(void) { return LQK_AUTOCORR_TILE; }
unsigned int liquid_mi355x_autocorr_max_window(void) { return LQK_AUTOCORR_MAXW; }
