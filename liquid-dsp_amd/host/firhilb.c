/*
 * firhilb.c -- firhilbf: Hilbert transform filter, 2:1 decimator (real ->
 * complex) and interpolator (complex -> real).
 *
 * include/liquid.h:2097-2176, src/filter/src/firhilb.c:64-301.
 *   h = kaiser(4m+1, fc 0.25, As) sin(pi/2 (i - 2m)), quadrature taps
 *   hq[j] = h[4m-1-2j] (2m of them, antisymmetric); two windows w0, w1 of 2m
 *   real samples shared by every mode, and a toggle for r2c:
 *     decim  w1 <- x[0], yq = hq . w1;  w0 <- x[1], yi = w0[m-1]
 *     interp w0 <- Im x, y[0] = w0[m-1];  w1 <- Re x, y[1] = hq . w1
 *     r2c    p = toggle: w_p <- x, yi = w_p[m-1], yq = hq . w_{1-p}; toggle ^= 1
 *     c2r    y = Re x
 *   (w[m-1], oldest first, is the sample pushed m pushes before the newest).
 * Block extensions (new names): *_execute_block[_dev] run n consecutive
 * calls on the GPU (csrc/k_firhilb.hip).  Single calls follow the small-call
 * rule (lq_small.c): on the host through mirrors of the two windows unless
 * LQ_SMALL_CALLS=gpu; c2r_execute is host arithmetic always.
 */
#include <complex.h>
#include <math.h>

#include "lq_host.h"

typedef struct {
    unsigned int m, h_len;
    float As;
    float *h, *hc, *hq;   /* h_len, 2 h_len (re, im), 2m */
    void *d_taps;         /* hq */
    void *d_w[2][2];      /* [ping-pong][window] */
    int cur, toggle;
    lq_mirror wm[2];      /* host copies of the windows (small-call mode) */
    lq_ctx ctx;
    lq_devbuf xbuf, ybuf;
} lq_fh;

struct firhilbf_s {
    lq_fh e;
};

firhilbf firhilbf_create(unsigned int _m, float _As)
{
    if (_m < 2) LQ_FAIL("error: firhilb_create(), filter semi-length (m) must be at least 2\n");
    if (_m > LQK_FIRHILB_MAXM)
        LQ_FAIL("error: firhilb_create(), filter semi-length (m) above %d is not supported\n", LQK_FIRHILB_MAXM);
    lqrt_require_device("firhilbf_create");
    firhilbf o = (firhilbf)lq_xmalloc(sizeof(*o));
    lq_fh *q = &o->e;
    memset(q, 0, sizeof(*q));
    q->m = _m;
    q->As = fabsf(_As);
    q->h_len = 4 * _m + 1;
    q->h = (float *)lq_xmalloc(q->h_len * sizeof(float));
    q->hc = (float *)lq_xmalloc(2 * q->h_len * sizeof(float));
    q->hq = (float *)lq_xmalloc(2 * _m * sizeof(float));
    lq_firdes_kaiser(q->h_len, 0.25f, q->As, 0.0f, q->h);
    for (unsigned int i = 0; i < q->h_len; i++) {   /* firhilb.c:95-99: the angle formed in double, used as float */
        const float th = (float)(0.5 * M_PI * ((double)i - 2.0 * (double)_m));
        q->hc[2 * i] = q->h[i] * cosf(th);
        q->hc[2 * i + 1] = q->h[i] * sinf(th);
        q->h[i] = q->hc[2 * i + 1];
    }
    for (unsigned int j = 0; j < 2 * _m; j++) q->hq[j] = q->h[4 * _m - 1 - 2 * j];
    lq_ctx_init(&q->ctx);
    q->d_taps = lqrt_malloc(2 * _m * sizeof(float));
    for (int b = 0; b < 2; b++)
        for (int w = 0; w < 2; w++) q->d_w[b][w] = lqrt_malloc(2 * _m * sizeof(float));   /* zeroed */
    lqrt_h2d(q->d_taps, q->hq, 2 * _m * sizeof(float), q->ctx.stream);
    lqrt_sync(q->ctx.stream);
    for (int w = 0; w < 2; w++) lq_mirror_init(&q->wm[w], 2 * _m, sizeof(float), 0);
    return o;
}

void firhilbf_destroy(firhilbf _q)
{
    lq_fh *q = &_q->e;
    lqrt_sync(q->ctx.stream);
    lqrt_free(q->d_taps);
    for (int b = 0; b < 2; b++)
        for (int w = 0; w < 2; w++) lqrt_free(q->d_w[b][w]);
    lq_devbuf_free(&q->xbuf);
    lq_devbuf_free(&q->ybuf);
    lq_ctx_free(&q->ctx);
    for (int w = 0; w < 2; w++) lq_mirror_free(&q->wm[w]);
    free(q->h);
    free(q->hc);
    free(q->hq);
    free(_q);
}

void firhilbf_print(firhilbf _q)   /* firhilb.c:140-155 */
{
    lq_fh *q = &_q->e;
    printf("fir hilbert transform: [%u]\n", q->h_len);
    for (unsigned int i = 0; i < q->h_len; i++)
        printf("  hc(%4u) = %8.4f + j*%8.4f;\n", i + 1, q->hc[2 * i], q->hc[2 * i + 1]);
    printf("---\n");
    for (unsigned int i = 0; i < q->h_len; i++) printf("  h(%4u) = %8.4f;\n", i + 1, q->h[i]);
    printf("---\n");
    for (unsigned int i = 0; i < 2 * q->m; i++) printf("  hq(%4u) = %8.4f;\n", i + 1, q->hq[i]);
}

void firhilbf_reset(firhilbf _q)
{
    lq_fh *q = &_q->e;
    for (int w = 0; w < 2; w++) lqrt_memset(q->d_w[q->cur][w], 2 * q->m * sizeof(float), q->ctx.stream);
    lqrt_sync(q->ctx.stream);
    for (int w = 0; w < 2; w++) lq_mirror_zero(&q->wm[w]);
    q->toggle = 0;
}

static void lq_fh_run_dev(lq_fh *q, int mode, const void *dx, unsigned long long n, void *dy)
{
    if (n == 0) return;
    for (int w = 0; w < 2; w++) {
        lq_mirror_need_dev(&q->wm[w], q->d_w[q->cur][w], q->ctx.stream);
        q->wm[w].host_valid = 0;
    }
    const int nx = q->cur ^ 1;
    lqk_firhilb(mode, q->m, q->toggle, q->d_taps, q->d_w[q->cur][0], q->d_w[q->cur][1], q->d_w[nx][0],
                q->d_w[nx][1], dx, n, dy, q->ctx.stream);
    q->cur = nx;
    if (mode == LQK_FH_R2C) q->toggle ^= (int)(n & 1);
}

/* host pointers: every mode moves 8 bytes per call each way but r2c, which
 * reads 4 */
static void lq_fh_run(lq_fh *q, int mode, const void *x, unsigned long long n, void *y)
{
    if (n == 0) return;
    const size_t bx = (size_t)n * (mode == LQK_FH_R2C ? 4 : 8), by = (size_t)n * 8;
    const void *dx = lq_call_in(&q->ctx, &q->xbuf, x, bx);
    void *dy = lq_devbuf_get(&q->ybuf, by);
    lq_fh_run_dev(q, mode, dx, n, dy);
    lq_call_out(&q->ctx, y, dy, by);
}

/* small-call mode: push v into window w on the host; the 2m-sample window
 * after the push (oldest first) is returned and stays valid until the next
 * push into w */
static const float *lq_fh_push_host(lq_fh *q, int w, float v)
{
    lq_mirror_append(&q->wm[w], &v, 1);
    lq_mirror_commit(&q->wm[w], 1);
    return (const float *)lq_mirror_ptr(&q->wm[w]);
}

static void lq_fh_need_host(lq_fh *q)
{
    for (int w = 0; w < 2; w++) lq_mirror_need_host(&q->wm[w], q->d_w[q->cur][w], q->ctx.stream);
}

void firhilbf_r2c_execute(firhilbf _q, float _x, liquid_float_complex *_y)
{
    lq_fh *q = &_q->e;
    if (!lq_small_host()) {
        lq_fh_run(q, LQK_FH_R2C, &_x, 1, _y);
        return;
    }
    lq_fh_need_host(q);
    const int p = q->toggle;
    const float yi = lq_fh_push_host(q, p, _x)[q->m - 1];
    float yq;
    lq_host_tdot(LQ_RRRF, q->hq, lq_mirror_ptr(&q->wm[1 - p]), 2 * q->m, &yq);
    q->toggle ^= 1;
    ((float *)_y)[0] = yi;
    ((float *)_y)[1] = yq;
}

void firhilbf_c2r_execute(firhilbf _q, liquid_float_complex _x, float *_y) { *_y = ((float *)&_x)[0]; }

void firhilbf_decim_execute(firhilbf _q, float *_x, liquid_float_complex *_y)
{
    lq_fh *q = &_q->e;
    if (!lq_small_host()) {
        lq_fh_run(q, LQK_FH_DECIM, _x, 1, _y);
        return;
    }
    lq_fh_need_host(q);
    float yq;
    lq_host_tdot(LQ_RRRF, q->hq, lq_fh_push_host(q, 1, _x[0]), 2 * q->m, &yq);
    const float yi = lq_fh_push_host(q, 0, _x[1])[q->m - 1];
    ((float *)_y)[0] = yi;
    ((float *)_y)[1] = yq;
}

void firhilbf_interp_execute(firhilbf _q, liquid_float_complex _x, float *_y)
{
    lq_fh *q = &_q->e;
    if (!lq_small_host()) {
        lq_fh_run(q, LQK_FH_INTERP, &_x, 1, _y);
        return;
    }
    lq_fh_need_host(q);
    const float re = ((float *)&_x)[0], im = ((float *)&_x)[1];
    _y[0] = lq_fh_push_host(q, 0, im)[q->m - 1];
    lq_host_tdot(LQ_RRRF, q->hq, lq_fh_push_host(q, 1, re), 2 * q->m, &_y[1]);
}

void firhilbf_decim_execute_block(firhilbf _q, float *_x, unsigned int _n, liquid_float_complex *_y)
{
    lq_fh_run(&_q->e, LQK_FH_DECIM, _x, _n, _y);
}

void firhilbf_interp_execute_block(firhilbf _q, liquid_float_complex *_x, unsigned int _n, float *_y)
{
    lq_fh_run(&_q->e, LQK_FH_INTERP, _x, _n, _y);
}

void firhilbf_r2c_execute_block(firhilbf _q, float *_x, unsigned long long _n, liquid_float_complex *_y)
{
    lq_fh_run(&_q->e, LQK_FH_R2C, _x, _n, _y);
}

void firhilbf_c2r_execute_block(firhilbf _q, liquid_float_complex *_x, unsigned long long _n, float *_y)
{
    lq_fh *q = &_q->e;
    if (_n == 0) return;
    const void *dx = lq_call_in(&q->ctx, &q->xbuf, _x, (size_t)_n * 8);
    void *dy = lq_devbuf_get(&q->ybuf, (size_t)_n * 4);
    lqk_firhilb_c2r(dx, _n, dy, q->ctx.stream);
    lq_call_out(&q->ctx, _y, dy, (size_t)_n * 4);
}

void firhilbf_decim_execute_block_dev(firhilbf _q, const float *_dx, unsigned long long _n,
                                      liquid_float_complex *_dy)
{
    lq_fh_run_dev(&_q->e, LQK_FH_DECIM, _dx, _n, _dy);
}

void firhilbf_interp_execute_block_dev(firhilbf _q, const liquid_float_complex *_dx, unsigned long long _n,
                                       float *_dy)
{
    lq_fh_run_dev(&_q->e, LQK_FH_INTERP, _dx, _n, _dy);
}

void firhilbf_r2c_execute_block_dev(firhilbf _q, const float *_dx, unsigned long long _n, liquid_float_complex *_dy)
{
    lq_fh_run_dev(&_q->e, LQK_FH_R2C, _dx, _n, _dy);
}

void firhilbf_c2r_execute_block_dev(firhilbf _q, const liquid_float_complex *_dx, unsigned long long _n, float *_dy)
{
    lqk_firhilb_c2r(_dx, _n, _dy, _q->e.ctx.stream);
}

void firhilbf_set_stream(firhilbf _q, void *_s) { lq_ctx_set_stream(&_q->e.ctx, _s); }
void firhilbf_synchronize(firhilbf _q) { lqrt_sync(_q->e.ctx.stream); }
