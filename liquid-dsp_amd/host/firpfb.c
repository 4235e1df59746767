/*
 * firpfb.c -- firpfb_{rrrf,crcf,cccf} polyphase filter bank.
 *
 * include/liquid.h:2392-2486, src/filter/src/firpfb.c:46-345.
 *   Bank i = h[i + n*M], n < L = floor(h_len/M) (:73-84); push() appends one
 *   sample; execute(i) = scale * sum_n h[i + n*M] x[t-n] (:325-345, index
 *   check :330-334); create_kaiser designs 2Mm+1 taps at fc/M (:105-138);
 *   recreate with a new shape re-creates the object (:250-258).
 * Extension: execute_block pushes each input and evaluates every bank after
 * it (y[t*M + i]) -- the interpolator kernel's contraction.
 */
#include <complex.h>

#include <math.h>

#include "lq_host.h"

typedef struct {
    int kind;
    size_t esz, csz;
    unsigned int M, hlen, L;
    float sre, sim;
    float *hpoly;                 /* M x L coefficients, hpoly[i*L + n] = h[i + n*M] */
    void *d_hpoly;
    lq_hist win;                  /* last L inputs, oldest first; pinned: execute() reads it in place */
    lq_ctx ctx;
    lq_devbuf xbuf, ybuf, one;
} lq_pfb;

static void lq_pfb_load(lq_pfb *q, const float *h)
{
    const size_t cf = q->csz / 4;
    for (unsigned int i = 0; i < q->M; i++)
        for (unsigned int n = 0; n < q->L; n++) memcpy(q->hpoly + cf * (i * q->L + n), h + cf * (i + n * q->M), q->csz);
}

static lq_pfb *lq_pfb_create(int kind, unsigned int M, const float *h, unsigned int hlen)
{
    if (M == 0) LQ_FAIL("error: firpfb_%s_create(), number of filters must be greater than zero\n", lq_ext(kind));
    if (hlen == 0) LQ_FAIL("error: firpfb_%s_create(), filter length must be greater than zero\n", lq_ext(kind));
    if (hlen < M)
        LQ_FAIL("error: firpfb_%s_create(), filter length must be at least the number of filters\n", lq_ext(kind));
    if (hlen / M > lqk_firinterp_max_taps(kind))
        LQ_FAIL("error: firpfb_%s_create(), filter length (%u taps per filter) exceeds the GPU kernel limit (%u)\n",
                lq_ext(kind), hlen / M, lqk_firinterp_max_taps(kind));
    lqrt_require_device("firpfb_create");
    lq_pfb *q = (lq_pfb *)lq_xmalloc(sizeof(*q));
    q->kind = kind;
    q->esz = lq_esz(kind);
    q->csz = lq_csz(kind);
    q->M = M;
    q->hlen = hlen;
    q->L = hlen / M;
    q->sre = 1.0f;
    q->sim = 0.0f;
    q->hpoly = (float *)lq_xmalloc((size_t)M * q->L * q->csz);
    lq_pfb_load(q, h);
    lq_ctx_init(&q->ctx);
    q->d_hpoly = lqrt_malloc((size_t)M * q->L * q->csz);
    lqrt_h2d(q->d_hpoly, q->hpoly, (size_t)M * q->L * q->csz, q->ctx.stream);
    lq_hist_init(&q->win, q->L, q->esz, LQ_HIST_PINNED);
    lqrt_sync(q->ctx.stream);
    return q;
}

/* from real design taps hf (taken over) */
static lq_pfb *lq_pfb_create_real(int kind, unsigned int M, float *hf, unsigned int n)
{
    float *h = lq_taps_from_real(kind, hf, n);
    lq_pfb *q = lq_pfb_create(kind, M, h, n);
    free(h);
    return q;
}

static float *lq_pfb_kaiser(const char *who, unsigned int M, unsigned int m, float fc, float As, unsigned int *n)
{
    if (M == 0) LQ_FAIL("error: %s_create_kaiser(), number of filters must be greater than zero\n", who);
    if (m == 0) LQ_FAIL("error: %s_create_kaiser(), filter delay must be greater than 0\n", who);
    if (fc < 0.0f || fc > 0.5f) LQ_FAIL("error: %s_create_kaiser(), filter cut-off frequence must be in (0,0.5)\n", who);
    if (As < 0.0f) LQ_FAIL("error: %s_create_kaiser(), filter excess bandwidth factor must be in [0,1]\n", who);
    *n = 2 * M * m + 1;
    float *hf = (float *)lq_xmalloc(*n * sizeof(float));
    lq_firdes_kaiser(*n, fc / (float)M, As, 0.0f, hf);
    return hf;
}

/* firpfb.c:146-240: prototype of 2*M*k*m+1 taps at M*k samples/symbol; the
 * derivative bank is the central difference (circular at the ends) scaled so
 * that max |h dh| = 0.06 */
static float *lq_pfb_rnyquist(const char *who, const char *fn, int deriv, int type, unsigned int M, unsigned int k,
                              unsigned int m, float beta, unsigned int *n)
{
    if (M == 0) LQ_FAIL("error: %s%s(), number of filters must be greater than zero\n", who, fn);
    if (k < 2) LQ_FAIL("error: %s%s(), filter samples/symbol must be greater than 1\n", who, fn);
    if (m == 0) LQ_FAIL("error: %s%s(), filter delay must be greater than 0\n", who, fn);
    if (beta < 0.0f || beta > 1.0f) LQ_FAIL("error: %s%s(), filter excess bandwidth factor must be in [0,1]\n", who, fn);
    const unsigned int N = 2 * M * k * m + 1;
    *n = N;
    float *H = (float *)lq_xmalloc(N * sizeof(float));
    liquid_firdes_prototype((liquid_firfilt_type)type, M * k, m, beta, 0, H);
    if (!deriv) return H;
    float *dH = (float *)lq_xmalloc(N * sizeof(float));
    float mx = 0.0f;
    for (unsigned int i = 0; i < N; i++) {
        dH[i] = H[i == N - 1 ? 0 : i + 1] - H[i == 0 ? N - 1 : i - 1];
        if (fabsf(H[i] * dH[i]) > mx) mx = fabsf(H[i] * dH[i]);
    }
    for (unsigned int i = 0; i < N; i++) dH[i] = dH[i] * 0.06f / mx;
    free(H);
    return dH;
}

static void lq_pfb_destroy(lq_pfb *q)
{
    lqrt_sync(q->ctx.stream);
    lqrt_free(q->d_hpoly);
    lq_hist_free(&q->win);
    lq_devbuf_free(&q->xbuf);
    lq_devbuf_free(&q->ybuf);
    lq_devbuf_free(&q->one);
    lq_ctx_free(&q->ctx);
    free(q->hpoly);
    free(q);
}

static void lq_pfb_recoef(lq_pfb *q, const float *h)
{
    lq_pfb_load(q, h);
    lqrt_sync(q->ctx.stream);
    lqrt_h2d(q->d_hpoly, q->hpoly, (size_t)q->M * q->L * q->csz, q->ctx.stream);
    lqrt_sync(q->ctx.stream);
}

static void lq_pfb_print(lq_pfb *q)
{
    printf("fir polyphase filterbank [%u] :\n", q->M);
    for (unsigned int i = 0; i < q->M; i++) printf("  bank %3u: \n", i);
}

static void lq_pfb_reset(lq_pfb *q) { lq_hist_zero(&q->win, q->ctx.stream); }

static void lq_pfb_push(lq_pfb *q, const void *x)
{
    lq_hist_append(&q->win, x, 1, q->ctx.stream);
    lq_hist_commit(&q->win, 1);
}

/* the kernel reads the window where it is authoritative: in place from the
 * pinned host mirror after push()es, or the device copy after a block */
static void lq_pfb_execute(lq_pfb *q, unsigned int i, void *y)
{
    if (i >= q->M) LQ_FAIL("error: firpfb_execute(), filterbank index (%u) exceeds maximum (%u)\n", i, q->M);
    unsigned *flag, seq;
    void *py = lq_sig_out(&q->ctx, q->esz, &flag, &seq);
    lqk_firpfb_single(q->kind, q->d_hpoly, q->L, i, lq_hist_read(&q->win), q->sre, q->sim, py, flag, seq,
                      q->ctx.stream);
    lq_sig_wait(&q->ctx, y, q->esz, seq);
}

static void lq_pfb_block_dev(lq_pfb *q, const void *dx, unsigned long long n, void *dy)
{
    if (n == 0) return;
    void *wold = lq_hist_dev(&q->win, q->ctx.stream), *wnew = lq_hist_next(&q->win);
    /* bank outputs after each push: the interpolator kernel (y[t*M+i]) with
     * the window's last L-1 samples as history */
    lqk_firinterp(q->kind, q->d_hpoly, q->M, q->L, q->sre, q->sim, (const char *)wold + q->esz, dx, n, dy,
                  q->ctx.stream);
    lqk_window_append(q->kind != LQ_RRRF, wold, q->L, dx, n, wnew, q->ctx.stream);
    lq_hist_flip(&q->win);
}

static void lq_pfb_block(lq_pfb *q, const void *x, unsigned long long n, void *y)
{
    if (n == 0) return;
    size_t nin = (size_t)n * q->esz, nout = nin * q->M;
    const void *dx = lq_call_in(&q->ctx, &q->xbuf, x, nin);
    void *dy = lq_devbuf_get(&q->ybuf, nout);
    lq_pfb_block_dev(q, dx, n, dy);
    lq_call_out(&q->ctx, y, dy, nout);
}

#define LQ_FIRPFB_FRONT(NAME, KIND, TO, TC, TI, SRE, SIM)                                           \
    struct NAME##_s {                                                                               \
        lq_pfb *e;                                                                                  \
    };                                                                                              \
    static NAME NAME##_wrap(lq_pfb *e)                                                              \
    {                                                                                               \
        NAME q = (NAME)lq_xmalloc(sizeof(*q));                                                      \
        q->e = e;                                                                                   \
        return q;                                                                                   \
    }                                                                                               \
    NAME NAME##_create(unsigned int _M, TC *_h, unsigned int _h_len)                                \
    {                                                                                               \
        return NAME##_wrap(lq_pfb_create(KIND, _M, (const float *)_h, _h_len));                     \
    }                                                                                               \
    NAME NAME##_create_kaiser(unsigned int _M, unsigned int _m, float _fc, float _As)               \
    {                                                                                               \
        unsigned int n;                                                                             \
        float *hf = lq_pfb_kaiser(#NAME, _M, _m, _fc, _As, &n);                                     \
        return NAME##_wrap(lq_pfb_create_real(KIND, _M, hf, n));                                    \
    }                                                                                               \
    /* firpfb.c:146-180 (d = 0) and :188-240 (d = 1: derivative bank) */                            \
    NAME NAME##_create_rnyquist(int _type, unsigned int _M, unsigned int _k, unsigned int _m, float _beta)\
    {                                                                                               \
        unsigned int n;                                                                             \
        float *hf = lq_pfb_rnyquist(#NAME, "_create_rnyquist", 0, _type, _M, _k, _m, _beta, &n);    \
        return NAME##_wrap(lq_pfb_create_real(KIND, _M, hf, n));                                    \
    }                                                                                               \
    NAME NAME##_create_drnyquist(int _type, unsigned int _M, unsigned int _k, unsigned int _m, float _beta)\
    {                                                                                               \
        unsigned int n;                                                                             \
        float *hf = lq_pfb_rnyquist(#NAME, "_create_drnyquist", 1, _type, _M, _k, _m, _beta, &n);   \
        return NAME##_wrap(lq_pfb_create_real(KIND, _M, hf, n));                                    \
    }                                                                                               \
    void NAME##_destroy(NAME _q)                                                                    \
    {                                                                                               \
        lq_pfb_destroy(_q->e);                                                                      \
        free(_q);                                                                                   \
    }                                                                                               \
    NAME NAME##_recreate(NAME _q, unsigned int _M, TC *_h, unsigned int _h_len)                     \
    {                                                                                               \
        if (_h_len != _q->e->hlen || _M != _q->e->M) {                                              \
            NAME##_destroy(_q);                                                                     \
            return NAME##_create(_M, _h, _h_len);                                                   \
        }                                                                                           \
        lq_pfb_recoef(_q->e, (const float *)_h);                                                    \
        return _q;                                                                                  \
    }                                                                                               \
    void NAME##_print(NAME _q) { lq_pfb_print(_q->e); }                                             \
    void NAME##_set_scale(NAME _q, TC _g)                                                           \
    {                                                                                               \
        _q->e->sre = SRE;                                                                           \
        _q->e->sim = SIM;                                                                           \
    }                                                                                               \
    void NAME##_reset(NAME _q) { lq_pfb_reset(_q->e); }                                             \
    void NAME##_push(NAME _q, TI _x) { lq_pfb_push(_q->e, &_x); }                                   \
    void NAME##_execute(NAME _q, unsigned int _i, TO *_y) { lq_pfb_execute(_q->e, _i, _y); }         \
    void NAME##_execute_block(NAME _q, TI *_x, unsigned long long _n, TO *_y)                       \
    {                                                                                               \
        lq_pfb_block(_q->e, _x, _n, _y);                                                            \
    }                                                                                               \
    void NAME##_execute_block_dev(NAME _q, const TI *_dx, unsigned long long _n, TO *_dy)           \
    {                                                                                               \
        lq_pfb_block_dev(_q->e, _dx, _n, _dy);                                                      \
    }                                                                                               \
    void NAME##_set_stream(NAME _q, void *_s) { lq_ctx_set_stream(&_q->e->ctx, _s); }

LQ_FIRPFB_FRONT(firpfb_rrrf, LQ_RRRF, float, float, float, _g, 0.0f)
LQ_FIRPFB_FRONT(firpfb_crcf, LQ_CRCF, liquid_float_complex, float, liquid_float_complex, _g, 0.0f)
LQ_FIRPFB_FRONT(firpfb_cccf, LQ_CCCF, liquid_float_complex, liquid_float_complex, liquid_float_complex, crealf(_g),
                cimagf(_g))
