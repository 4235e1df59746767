/*
 * firdecim.c -- firdecim_{rrrf,crcf,cccf} and firinterp_{rrrf,crcf,cccf}.
 *
 * firdecim: include/liquid.h:2664-2735, src/filter/src/firdecim.c:47-223.
 *   y[o] = sum_{k<h} h[k] x[o*M - k]: the output is formed right after the
 *   first of each group of M pushes (:195-204); execute_block's _n counts
 *   outputs (:208-223); create_kaiser designs 2Mm+1 taps at fc = 0.5/M and
 *   uses the first 2Mm (:88-122).  No output scale.
 * firinterp: include/liquid.h:2496-2565, src/filter/src/firinterp.c:43-215.
 *   L = ceil(h/M), h' = h zero-padded to M*L, y[i*M + p] =
 *   sum_{l<L} h'[p + l*M] x[i - l]; create needs M >= 2 and h_len >= M.
 *
 * One generic engine per object (sample kind rrrf / crcf / cccf chooses the
 * kernel instantiation and element sizes); the typed front ends at the end
 * only forward.
 */
#include <complex.h>

#include "lq_host.h"

/* the designs behind both objects' create_kaiser (firdecim.c:88-122: 2Mm+1
 * Kaiser taps at fc = 0.5/M, of which the first 2Mm are used) and
 * create_prototype (firdecim.c:126-160, firinterp.c:124-158: 2Mm+1 taps from
 * liquid_firdes_prototype); `what` is the factor's name in the messages */
static float *lq_mrate_kaiser(const char *who, const char *what, unsigned int M, unsigned int m, float As,
                              unsigned int *n)
{
    if (M < 2) LQ_FAIL("error: %s_create_kaiser(), %s factor must be greater than 1\n", who, what);
    if (m == 0) LQ_FAIL("error: %s_create_kaiser(), filter delay must be greater than 0\n", who);
    if (As < 0.0f) LQ_FAIL("error: %s_create_kaiser(), stop-band attenuation must be positive\n", who);
    *n = 2 * M * m + 1;
    float *hf = (float *)lq_xmalloc(*n * sizeof(float));
    lq_firdes_kaiser(*n, 0.5f / (float)M, As, 0.0f, hf);
    return hf;
}

static float *lq_mrate_prototype(const char *who, const char *what, int type, unsigned int M, unsigned int m,
                                 float beta, float dt, unsigned int *n)
{
    if (M < 2) LQ_FAIL("error: %s_create_prototype(), %s factor must be greater than 1\n", who, what);
    if (m == 0) LQ_FAIL("error: %s_create_prototype(), filter delay must be greater than 0\n", who);
    if (beta < 0.0f || beta > 1.0f)
        LQ_FAIL("error: %s_create_prototype(), filter excess bandwidth factor must be in [0,1]\n", who);
    if (dt < -1.0f || dt > 1.0f)
        LQ_FAIL("error: %s_create_prototype(), filter fractional sample delay must be in [-1,1]\n", who);
    *n = 2 * M * m + 1;
    float *hf = (float *)lq_xmalloc(*n * sizeof(float));
    liquid_firdes_prototype((liquid_firfilt_type)type, M, m, beta, dt, hf);
    return hf;
}

/* ================================================================ firdecim */

typedef struct {
    int kind;
    size_t esz, csz;
    unsigned int M, hlen;
    float *h;          /* host copy, hlen coefficients of csz bytes */
    float *hg;         /* reversed, expanded for the host path (lq_host_taps) */
    void *d_hpad;
    void *d_hq;        /* M x QC phase-major taps for the phase-layout kernel */
    unsigned int QC;
    lq_hist hist;      /* last hlen-1 inputs; mirrored for the small-call mode */
    lq_ctx ctx;
    lq_devbuf xbuf, ybuf;
} lq_decim;

static lq_decim *lq_decim_create(int kind, unsigned int M, const float *h, unsigned int hlen)
{
    if (hlen == 0) LQ_FAIL("error: decim_%s_create(), filter length must be greater than zero\n", lq_ext(kind));
    if (M == 0) LQ_FAIL("error: decim_%s_create(), decimation factor must be greater than zero\n", lq_ext(kind));
    lqrt_require_device("firdecim_create");
    lq_decim *q = (lq_decim *)lq_xmalloc(sizeof(*q));
    q->kind = kind;
    q->esz = lq_esz(kind);
    q->csz = lq_csz(kind);
    q->M = M;
    q->hlen = hlen;
    q->h = (float *)lq_xmalloc(hlen * q->csz);
    memcpy(q->h, h, hlen * q->csz);
    q->hg = lq_host_taps(kind, q->h, hlen, 1);
    lq_ctx_init(&q->ctx);
    q->d_hpad = lqrt_malloc(hlen * q->csz);
    lqrt_h2d(q->d_hpad, q->h, hlen * q->csz, q->ctx.stream);
    /* k = qM + r -> hq[r*QC + q] (zero past hlen) */
    q->QC = lqk_firdecim_ph_qc(M, hlen);
    const size_t nq = (size_t)M * q->QC, cf = q->csz / sizeof(float);
    float *hq = (float *)lq_xmalloc(nq * q->csz);
    memset(hq, 0, nq * q->csz);
    for (unsigned int k = 0; k < hlen; k++)
        memcpy(hq + ((size_t)(k % M) * q->QC + k / M) * cf, q->h + (size_t)k * cf, q->csz);
    q->d_hq = lqrt_malloc(nq * q->csz);
    lqrt_h2d(q->d_hq, hq, nq * q->csz, q->ctx.stream);
    lq_hist_init(&q->hist, hlen - 1, q->esz, LQ_HIST_MIRROR);
    lqrt_sync(q->ctx.stream);
    free(hq);
    return q;
}

static void lq_decim_destroy(lq_decim *q)
{
    lqrt_sync(q->ctx.stream);
    lqrt_free(q->d_hpad);
    lqrt_free(q->d_hq);
    lq_hist_free(&q->hist);
    lq_devbuf_free(&q->xbuf);
    lq_devbuf_free(&q->ybuf);
    lq_ctx_free(&q->ctx);
    free(q->h);
    free(q->hg);
    free(q);
}

static void lq_decim_print(lq_decim *q)
{
    printf("FIRDECIM() [%u] :\n", q->M);
    for (unsigned int i = 0; i < q->hlen; i++) {
        if (q->kind == LQ_CCCF) printf("  h(%3u) = %12.8f + j*%12.8f\n", i + 1, q->h[2 * i], q->h[2 * i + 1]);
        else printf("  h(%3u) = %12.8f\n", i + 1, q->h[i]);
    }
}

static void lq_decim_clear(lq_decim *q) { lq_hist_zero(&q->hist, q->ctx.stream); }

static void lq_decim_block_dev(lq_decim *q, const void *dx, unsigned long long nout, void *dy)
{
    if (nout == 0) return;
    void *hold = lq_hist_dev(&q->hist, q->ctx.stream), *hnew = lq_hist_next(&q->hist);
    if (lqk_firdecim_ph(q->kind, q->M, q->QC, q->d_hq, q->hlen - 1, hold, dx, nout, dy, q->ctx.stream) != 0)
        lqk_firdecim(q->kind, q->hlen, q->d_hpad, q->M, hold, dx, nout, dy, q->ctx.stream);
    if (q->hlen > 1) lqk_window_append(q->kind != LQ_RRRF, hold, q->hlen - 1, dx, nout * q->M, hnew, q->ctx.stream);
    lq_hist_flip(&q->hist);
}

/* small-call mode: one output on the host (firdecim.c:189-205: the dot
 * product right after the first of the M pushes) */
static void lq_decim_exec1_host(lq_decim *q, const void *x, void *y)
{
    const unsigned char *w = lq_hist_append(&q->hist, x, q->M, q->ctx.stream);
    lq_host_tdot(q->kind, q->hg, w, q->hlen, y);   /* the hlen-sample window, oldest first */
    lq_hist_commit(&q->hist, q->M);
}

/* single: the call is firdecim_*_execute; execute_block always runs on the GPU */
static void lq_decim_block(lq_decim *q, const void *x, unsigned long long nout, void *y, int single)
{
    if (nout == 0) return;
    if (single && lq_small_host()) {
        lq_decim_exec1_host(q, x, y);
        return;
    }
    size_t nin = (size_t)nout * q->M * q->esz, nb = (size_t)nout * q->esz;
    const void *dx = lq_call_in(&q->ctx, &q->xbuf, x, nin);
    void *dy = lq_devbuf_get(&q->ybuf, nb);
    lq_decim_block_dev(q, dx, nout, dy);
    lq_call_out(&q->ctx, y, dy, nb);
}

#define LQ_FIRDECIM_FRONT(NAME, KIND, TO, TC, TI)                                                   \
    struct NAME##_s {                                                                               \
        lq_decim *e;                                                                                \
    };                                                                                              \
    NAME NAME##_create(unsigned int _M, TC *_h, unsigned int _h_len)                                \
    {                                                                                               \
        NAME q = (NAME)lq_xmalloc(sizeof(*q));                                                      \
        q->e = lq_decim_create(KIND, _M, (const float *)_h, _h_len);                                \
        return q;                                                                                   \
    }                                                                                               \
    NAME NAME##_create_kaiser(unsigned int _M, unsigned int _m, float _As)                          \
    {                                                                                               \
        unsigned int n;                                                                             \
        float *h = lq_mrate_kaiser(#NAME, "decim", _M, _m, _As, &n);                                \
        h = lq_taps_from_real(KIND, h, n);                                                          \
        NAME q = NAME##_create(_M, (TC *)h, n - 1);                                                 \
        free(h);                                                                                    \
        return q;                                                                                   \
    }                                                                                               \
    NAME NAME##_create_prototype(int _type, unsigned int _M, unsigned int _m, float _beta, float _dt) \
    {                                                                                               \
        unsigned int n;                                                                             \
        float *h = lq_mrate_prototype(#NAME, "decimation", _type, _M, _m, _beta, _dt, &n);          \
        h = lq_taps_from_real(KIND, h, n);                                                          \
        NAME q = NAME##_create(_M, (TC *)h, n);                                                     \
        free(h);                                                                                    \
        return q;                                                                                   \
    }                                                                                               \
    void NAME##_destroy(NAME _q)                                                                    \
    {                                                                                               \
        lq_decim_destroy(_q->e);                                                                    \
        free(_q);                                                                                   \
    }                                                                                               \
    void NAME##_print(NAME _q) { lq_decim_print(_q->e); }                                           \
    void NAME##_clear(NAME _q) { lq_decim_clear(_q->e); }                                           \
    void NAME##_execute(NAME _q, TI *_x, TO *_y) { lq_decim_block(_q->e, _x, 1, _y, 1); }           \
    void NAME##_execute_block(NAME _q, TI *_x, unsigned int _n, TO *_y)                             \
    {                                                                                               \
        lq_decim_block(_q->e, _x, _n, _y, 0);                                                       \
    }                                                                                               \
    void NAME##_execute_block_dev(NAME _q, const TI *_dx, unsigned long long _n, TO *_dy)           \
    {                                                                                               \
        lq_decim_block_dev(_q->e, _dx, _n, _dy);                                                    \
    }                                                                                               \
    void NAME##_set_stream(NAME _q, void *_s) { lq_ctx_set_stream(&_q->e->ctx, _s); }

/* the route query of include/liquid_mi355x.h: the kernels' own decision */
_Static_assert((int)LIQUID_MI355X_FIRDECIM_PF_R4X128 == (int)LQK_DECIM_PF_R4X128 &&
               (int)LIQUID_MI355X_FIRDECIM_PF_R2X256 == (int)LQK_DECIM_PF_R2X256 &&
               (int)LIQUID_MI355X_FIRDECIM_PH2 == (int)LQK_DECIM_PH2 &&
               (int)LIQUID_MI355X_FIRDECIM_PF_R1X256 == (int)LQK_DECIM_PF_R1X256 &&
               (int)LIQUID_MI355X_FIRDECIM_PH_R1X64 == (int)LQK_DECIM_PH_R1X64 &&
               (int)LIQUID_MI355X_FIRDECIM_PLAIN == (int)LQK_DECIM_PLAIN &&
               (int)LIQUID_MI355X_FIRDECIM_REFUSED == (int)LQK_DECIM_REFUSED, "route codes");

int liquid_mi355x_firdecim_route(int _kind, unsigned int _M, unsigned int _h_len, int _x_aligned16,
                                 unsigned long long _nout)
{
    return lqk_firdecim_route(_kind, _M, _h_len, _x_aligned16, _nout);
}

unsigned int liquid_mi355x_firdecim_tile(int _route) { return lqk_firdecim_route_tile(_route); }

unsigned int liquid_mi355x_firdecim_grid_cap(int _kind, unsigned int _M, unsigned int _h_len, int _route)
{
    return lqk_firdecim_route_cap(_kind, _M, _h_len, _route);
}

LQ_FIRDECIM_FRONT(firdecim_rrrf, LQ_RRRF, float, float, float)
LQ_FIRDECIM_FRONT(firdecim_crcf, LQ_CRCF, liquid_float_complex, float, liquid_float_complex)
LQ_FIRDECIM_FRONT(firdecim_cccf, LQ_CCCF, liquid_float_complex, liquid_float_complex, liquid_float_complex)

/* =============================================================== firinterp */

typedef struct {
    int kind;
    size_t esz, csz;
    unsigned int M, L, hlen;
    float *h;          /* padded prototype, M*L coefficients of csz bytes */
    void *d_hpoly;     /* M x L: hpoly[p*L + l] = h'[p + l*M] */
    lq_hist hist;      /* last L-1 inputs; mirrored for the small-call mode */
    float *hpoly;      /* host copy of the M x L phase taps */
    float *hgp;        /* the phases reversed and expanded for the host path, hgs floats apart */
    size_t hgs;
    lq_ctx ctx;
    lq_devbuf xbuf, ybuf;
} lq_interp;

static lq_interp *lq_interp_create(int kind, unsigned int M, const float *h, unsigned int hlen)
{
    if (M < 2) LQ_FAIL("error: firinterp_%s_create(), interp factor must be greater than 1\n", lq_ext(kind));
    if (hlen < M)
        LQ_FAIL("error: firinterp_%s_create(), filter length cannot be less than interp factor\n", lq_ext(kind));
    if ((hlen + M - 1) / M > lqk_firinterp_max_taps(kind))
        LQ_FAIL("error: firinterp_%s_create(), filter length (%u taps per phase) exceeds the GPU kernel limit (%u)\n",
                lq_ext(kind), (hlen + M - 1) / M, lqk_firinterp_max_taps(kind));
    lqrt_require_device("firinterp_create");
    lq_interp *q = (lq_interp *)lq_xmalloc(sizeof(*q));
    q->kind = kind;
    q->esz = lq_esz(kind);
    q->csz = lq_csz(kind);
    const size_t cf = q->csz / 4;       /* floats per coefficient */
    q->M = M;
    q->L = 0;
    while (M * q->L < hlen) q->L++;
    q->hlen = M * q->L;
    q->h = (float *)lq_xmalloc(q->hlen * q->csz);  /* tail zero (firinterp.c:68-73) */
    memcpy(q->h, h, hlen * q->csz);
    float *hp = (float *)lq_xmalloc(q->hlen * q->csz);
    for (unsigned int p = 0; p < M; p++)
        for (unsigned int l = 0; l < q->L; l++)
            memcpy(hp + cf * (p * q->L + l), q->h + cf * (p + l * M), q->csz);
    lq_ctx_init(&q->ctx);
    q->d_hpoly = lqrt_malloc(q->hlen * q->csz);
    lqrt_h2d(q->d_hpoly, hp, q->hlen * q->csz, q->ctx.stream);
    lq_hist_init(&q->hist, q->L - 1, q->esz, LQ_HIST_MIRROR);
    lqrt_sync(q->ctx.stream);
    q->hpoly = hp;
    q->hgs = (size_t)q->L * (kind == LQ_RRRF ? 1 : (kind == LQ_CRCF ? 2 : 4));
    q->hgp = (float *)lq_xmalloc((size_t)M * q->hgs * sizeof(float));
    for (unsigned int p = 0; p < M; p++) {
        float *g = lq_host_taps(kind, hp + cf * p * q->L, q->L, 1);
        memcpy(q->hgp + p * q->hgs, g, q->hgs * sizeof(float));
        free(g);
    }
    return q;
}

static void lq_interp_destroy(lq_interp *q)
{
    lqrt_sync(q->ctx.stream);
    lqrt_free(q->d_hpoly);
    lq_hist_free(&q->hist);
    lq_devbuf_free(&q->xbuf);
    lq_devbuf_free(&q->ybuf);
    lq_ctx_free(&q->ctx);
    free(q->hpoly);
    free(q->hgp);
    free(q->h);
    free(q);
}

static void lq_interp_print(lq_interp *q)
{
    printf("interp():\n");
    printf("    M       :   %u\n", q->M);
    printf("    h_len   :   %u\n", q->hlen);
}

static void lq_interp_reset(lq_interp *q) { lq_hist_zero(&q->hist, q->ctx.stream); }

static void lq_interp_block_dev(lq_interp *q, const void *dx, unsigned long long n, void *dy)
{
    if (n == 0) return;
    void *hold = lq_hist_dev(&q->hist, q->ctx.stream), *hnew = lq_hist_next(&q->hist);
    lqk_firinterp(q->kind, q->d_hpoly, q->M, q->L, 1.0f, 0.0f, hold, dx, n, dy, q->ctx.stream);
    if (q->L > 1) lqk_window_append(q->kind != LQ_RRRF, hold, q->L - 1, dx, n, hnew, q->ctx.stream);
    lq_hist_flip(&q->hist);
}

/* small-call mode: the M outputs of one input on the host (firinterp.c:187-198:
 * bank p of the polyphase filter over the last L inputs) */
static void lq_interp_exec1_host(lq_interp *q, const void *x, void *y)
{
    const unsigned char *w = lq_hist_append(&q->hist, x, 1, q->ctx.stream);
    for (unsigned int p = 0; p < q->M; p++)   /* bank p over the L-sample window, oldest first */
        lq_host_tdot(q->kind, q->hgp + p * q->hgs, w, q->L, (unsigned char *)y + p * q->esz);
    lq_hist_commit(&q->hist, 1);
}

/* single: the call is firinterp_*_execute; execute_block always runs on the GPU */
static void lq_interp_block(lq_interp *q, const void *x, unsigned long long n, void *y, int single)
{
    if (n == 0) return;
    if (single && lq_small_host()) {
        lq_interp_exec1_host(q, x, y);
        return;
    }
    size_t nin = (size_t)n * q->esz, nout = (size_t)n * q->M * q->esz;
    const void *dx = lq_call_in(&q->ctx, &q->xbuf, x, nin);
    void *dy = lq_devbuf_get(&q->ybuf, nout);
    lq_interp_block_dev(q, dx, n, dy);
    lq_call_out(&q->ctx, y, dy, nout);
}

#define LQ_FIRINTERP_FRONT(NAME, KIND, TO, TC, TI)                                                  \
    struct NAME##_s {                                                                               \
        lq_interp *e;                                                                               \
    };                                                                                              \
    NAME NAME##_create(unsigned int _M, TC *_h, unsigned int _h_len)                                \
    {                                                                                               \
        NAME q = (NAME)lq_xmalloc(sizeof(*q));                                                      \
        q->e = lq_interp_create(KIND, _M, (const float *)_h, _h_len);                               \
        return q;                                                                                   \
    }                                                                                               \
    NAME NAME##_create_kaiser(unsigned int _M, unsigned int _m, float _As)                          \
    {                                                                                               \
        unsigned int n;                                                                             \
        float *h = lq_mrate_kaiser(#NAME, "interp", _M, _m, _As, &n);                               \
        h = lq_taps_from_real(KIND, h, n);                                                          \
        NAME q = NAME##_create(_M, (TC *)h, n - 1);                                                 \
        free(h);                                                                                    \
        return q;                                                                                   \
    }                                                                                               \
    NAME NAME##_create_prototype(int _type, unsigned int _M, unsigned int _m, float _beta, float _dt) \
    {                                                                                               \
        unsigned int n;                                                                             \
        float *h = lq_mrate_prototype(#NAME, "interp", _type, _M, _m, _beta, _dt, &n);              \
        h = lq_taps_from_real(KIND, h, n);                                                          \
        NAME q = NAME##_create(_M, (TC *)h, n);                                                     \
        free(h);                                                                                    \
        return q;                                                                                   \
    }                                                                                               \
    void NAME##_destroy(NAME _q)                                                                    \
    {                                                                                               \
        lq_interp_destroy(_q->e);                                                                   \
        free(_q);                                                                                   \
    }                                                                                               \
    void NAME##_print(NAME _q) { lq_interp_print(_q->e); }                                          \
    void NAME##_reset(NAME _q) { lq_interp_reset(_q->e); }                                          \
    void NAME##_execute(NAME _q, TI _x, TO *_y) { lq_interp_block(_q->e, &_x, 1, _y, 1); }          \
    void NAME##_execute_block(NAME _q, TI *_x, unsigned int _n, TO *_y)                             \
    {                                                                                               \
        lq_interp_block(_q->e, _x, _n, _y, 0);                                                      \
    }                                                                                               \
    void NAME##_execute_block_dev(NAME _q, const TI *_dx, unsigned long long _n, TO *_dy)           \
    {                                                                                               \
        lq_interp_block_dev(_q->e, _dx, _n, _dy);                                                   \
    }                                                                                               \
    void NAME##_set_stream(NAME _q, void *_s) { lq_ctx_set_stream(&_q->e->ctx, _s); }

/* the route and limit queries of include/liquid_mi355x.h: the kernels' own decision */
int liquid_mi355x_firinterp_route(int _kind, unsigned int _M, unsigned int _L, int _y_aligned16)
{
    return lqk_firinterp_route(_kind, _M, _L, _y_aligned16);
}

unsigned int liquid_mi355x_firinterp_max_taps(int _kind) { return lqk_firinterp_max_taps(_kind); }

LQ_FIRINTERP_FRONT(firinterp_rrrf, LQ_RRRF, float, float, float)
LQ_FIRINTERP_FRONT(firinterp_crcf, LQ_CRCF, liquid_float_complex, float, liquid_float_complex)
LQ_FIRINTERP_FRONT(firinterp_cccf, LQ_CCCF, liquid_float_complex, liquid_float_complex, liquid_float_complex)
