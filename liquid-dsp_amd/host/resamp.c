/*
 * resamp.c -- resamp_{rrrf,crcf,cccf} on the MI355X.
 *
 * resamp: include/liquid.h:2938-3015, src/filter/src/resamp.c:79-363.
 *   Prototype 2*m*npfb+1 Kaiser taps at fc/npfb scaled by npfb/sum(h); bank
 *   from the first 2*m*npfb taps (L = 2m); per input the float32 timing
 *   state machine emits (1-mu) y0 + mu y1 outputs.
 *
 * The timing state evolves independently of the data, so the host tabulates
 * it -- a "plan", host/resamp_plan.c -- and the GPU replays it.  This file
 * is the object: taps and banks, the policy of which plan to build when
 * (calls of >= RS_PERIODIC_MIN inputs find the rate's period once and reuse
 * the plan for every later call; short calls, and rates whose period is out
 * of reach, get a plan covering just that call), the upload of its table
 * and the launches.  Every output sample is computed on the GPU
 * (csrc/k_resamp.hip).  The taps are real for every type (resamp.c:117-132
 * designs them with liquid_firdes_kaiser), so cccf runs the crcf kernel and
 * rrrf its real-sample instantiation.
 */
#include "lq_host.h"

/* ================================================================== resamp */

#define RS_PERIODIC_MIN (1ull << 16)   /* calls at least this long use (and build) a periodic plan */
#define RS_DIRECT_CHUNK (1ull << 24)   /* direct plans cover at most this many inputs */
#define RS_DIRECT_AHEAD (1ull << 14)   /* ... and at least this many (built ahead for short calls) */

struct lq_rs_s {
    int kind;
    size_t esz;                   /* bytes per sample */
    float rate, del, fc, As;
    unsigned int m, npfb, L;
    void *d_taps;                 /* npfb x L float pairs (bank b, bank b+1) */
    void *d_taps2;                /* (npfb+1) x LP interpolation pairs on one window (lq_kernels.h) */
    rs_plan pl;
    lq_devbuf d_tab;              /* the plan's table on the device */
    unsigned long long d_n;       /* its entries */
    int periodic_failed;          /* no period within the search limit at this rate */
    int rate_changed;             /* set_rate / adjust_rate since the last plan */
    unsigned long long gpos;      /* inputs consumed since the plan origin */
    rs_state now;                 /* timing state at gpos whenever a call returns (inside a block call
                                     it lags until rs_sync_now); the small-call path steps it in place */
    lq_hist hist;                 /* last L inputs; mirrored for the small-call mode */
    float *hbank;                 /* host bank taps h[b + n*npfb], n < L, reversed and expanded (lq_host_taps), hbs floats per bank */
    size_t hbs;
    lq_ctx ctx;
    lq_devbuf xbuf, ybuf, ubuf;   /* ubuf: resampler outputs of an unfused chain chunk */
};

/* whether an output plan (k_resamp4) is wanted: complex samples, tau-only
 * timing, r > 1/4 (del < 4; tau-only timing needs del npfb >= 1, r <= npfb);
 * the plan's walk then confirms the shape of the outputs (rs_rec4_shape).
 * Read when a plan is built */
static int rs_want_d4(int kind, float del, unsigned int npfb, unsigned int L)
{
    const char *e = getenv("LQ_RESAMP_INPUT_PLAN");   /* 1: always the input-checkpoint kernel (k_resamp3) */
    if (e && strcmp(e, "1") == 0) return 0;
    return kind != LQ_RRRF && rs_tau_only(del, npfb) && del < 4.0f && lqk_resamp4_supported(npfb, L);
}

/* a direct plan or the end of the process, with the message of the step that failed */
static void rs_build_direct(rs_plan *pl, int kind, float del, unsigned int npfb, rs_state origin,
                            unsigned long long nx, int want_d4)
{
    const int r = rs_plan_build_direct(pl, del, npfb, origin, nx, want_d4);
    if (r == 0) LQ_FAIL("error: resamp_%s: too many outputs for one call\n", lq_ext(kind));
    if (r < 0) LQ_FAIL("error: resamp_%s: timing plan\n", lq_ext(kind));
}

/* the timing state at the stream position */
static rs_state rs_here(const lq_rs *q)
{
    unsigned long long K;
    return q->pl.valid ? rs_plan_at(&q->pl, q->gpos, &K) : q->now;
}

static unsigned long long rs_K(lq_rs *q, unsigned long long g)
{
    unsigned long long K;
    rs_plan_at(&q->pl, g, &K);
    return K;
}

static void rs_sync_now(lq_rs *q) { q->now = rs_here(q); }

static void rs_plan_upload(lq_rs *q)
{
    const size_t bytes = q->pl.dn * q->pl.desz;
    void *d = lq_devbuf_get(&q->d_tab, bytes ? bytes : 8);
    if (bytes) lqrt_h2d(d, q->pl.dtab, bytes, q->ctx.stream);
    lqrt_sync(q->ctx.stream);
    q->d_n = q->pl.dn;
    rs_plan_drop_table(&q->pl);
}

static void rs_check_rate(lq_rs *q)
{
    if (!(q->del > 0.0f) || isinf(q->del) || isnan(q->del))
        LQ_FAIL("error: resamp_%s_execute(), invalid resampling rate (%f)\n", lq_ext(q->kind), q->rate);
}

/* The plan a call of nx inputs builds from `origin` (host only): which kind,
 * and with it which kernel -- the one policy behind rs_ensure_plan and
 * liquid_mi355x_resamp_route.  Returns how many of the inputs it covers. */
static unsigned long long rs_new_plan(rs_plan *pl, int kind, float del, unsigned int npfb, unsigned int L,
                                      rs_state origin, unsigned long long nx, int *periodic_failed, int *rate_changed)
{
    const int d4 = rs_want_d4(kind, del, npfb, L);
    if (!*periodic_failed && nx >= RS_PERIODIC_MIN) {
        if (rs_plan_build_periodic(pl, del, npfb, origin, d4)) return nx;
        *periodic_failed = 1;
    }
    /* a direct plan covers this call and, for short calls, the next
     * RS_DIRECT_AHEAD inputs too: the schedule does not depend on the data,
     * so per-sample execute() calls reuse one plan instead of building and
     * uploading one each (two stream synchronisations per call) */
    unsigned long long c = nx < RS_DIRECT_CHUNK ? nx : RS_DIRECT_CHUNK;
    /* right after a rate change the plan covers just this call: a loop that
     * steers the rate before every call (symsync-style) would otherwise build
     * RS_DIRECT_AHEAD inputs of schedule per call and use a fraction */
    rs_build_direct(pl, kind, del, npfb, origin, (c > RS_DIRECT_AHEAD || *rate_changed) ? c : RS_DIRECT_AHEAD, d4);
    *rate_changed = 0;
    return c;
}

/* make the plan cover inputs [gpos, gpos + nx); returns how many of them it covers */
static unsigned long long rs_ensure_plan(lq_rs *q, unsigned long long nx)
{
    rs_check_rate(q);
    if (q->pl.valid && q->pl.periodic) return nx;
    if (q->pl.valid && q->gpos + nx <= q->pl.end) return nx;
    lqrt_sync(q->ctx.stream);                /* the old table may still be in use */
    rs_sync_now(q);                          /* the new plan starts where the old one's coverage ends */
    q->pl.valid = 0;
    q->gpos = 0;
    const unsigned long long c = rs_new_plan(&q->pl, q->kind, q->del, q->npfb, q->L, q->now, nx, &q->periodic_failed,
                                             &q->rate_changed);
    rs_plan_upload(q);
    return c;
}

lq_rs *lq_rs_create(int kind, float _rate, unsigned int _m, float _fc, float _As, unsigned int _npfb)
{
    if (_rate <= 0) LQ_FAIL("error: resamp_%s_create(), resampling rate must be greater than zero\n", lq_ext(kind));
    if (_m == 0) LQ_FAIL("error: resamp_%s_create(), filter semi-length must be greater than zero\n", lq_ext(kind));
    if (_npfb == 0) LQ_FAIL("error: resamp_%s_create(), number of filter banks must be greater than zero\n", lq_ext(kind));
    if (_fc <= 0.0f || _fc >= 0.5f) LQ_FAIL("error: resamp_%s_create(), filter cutoff must be in (0,0.5)\n", lq_ext(kind));
    if (_As <= 0.0f)
        LQ_FAIL("error: resamp_%s_create(), filter stop-band suppression must be greater than zero\n", lq_ext(kind));
    lqrt_require_device("resamp_create");
    lq_rs *q = (lq_rs *)lq_xmalloc(sizeof(*q));
    q->kind = kind;
    q->esz = lq_esz(kind);
    q->rate = _rate;
    q->del = 1.0f / _rate;
    q->m = _m;
    q->fc = _fc;
    q->As = _As;
    q->npfb = _npfb;
    q->L = 2 * _m;
    /* resamp.c:117-132: design, DC normalisation, bank from the first n-1 taps */
    unsigned int n = 2 * _m * _npfb + 1;
    float *hf = (float *)lq_xmalloc(n * sizeof(float));
    lq_firdes_kaiser(n, _fc / ((float)_npfb), _As, 0.0f, hf);
    float gain = 0.0f;
    for (unsigned int i = 0; i < n; i++) gain += hf[i];
    gain = (_npfb) / (gain);
    for (unsigned int i = 0; i < n; i++) hf[i] = hf[i] * gain;
    size_t ntap = (size_t)_npfb * q->L;
    float *tp = (float *)lq_xmalloc(ntap * 2 * sizeof(float));
    for (unsigned int b = 0; b < _npfb; b++)
        for (unsigned int k = 0; k < q->L; k++) {
            tp[2 * (b * q->L + k)] = hf[b + k * _npfb];
            tp[2 * (b * q->L + k) + 1] = hf[(b + 1) % _npfb + k * _npfb];
        }
    /* window form: y = sum_p c[p] x[i-L+p], p <= L */
    const unsigned int L = q->L, LP = (L + 3) & ~1u;
    size_t ntap2 = (size_t)(_npfb + 1) * LP;
    float *tp2 = (float *)lq_xmalloc(ntap2 * 2 * sizeof(float));
    for (unsigned int b = 0; b < _npfb; b++)
        for (unsigned int p = 1; p <= L; p++) {
            tp2[2 * (b * LP + p)] = hf[b + (L - p) * _npfb];
            tp2[2 * (b * LP + p) + 1] = (b + 1 < _npfb) ? hf[b + 1 + (L - p) * _npfb] : 0.0f;
        }
    for (unsigned int p = 0; p <= L; p++) {
        tp2[2 * (_npfb * LP + p)] = p < L ? hf[_npfb - 1 + (L - 1 - p) * _npfb] : 0.0f;
        tp2[2 * (_npfb * LP + p) + 1] = p >= 1 ? hf[(L - p) * _npfb] : 0.0f;
    }
    lq_ctx_init(&q->ctx);
    q->d_taps = lqrt_malloc(ntap * 2 * sizeof(float));
    lqrt_h2d(q->d_taps, tp, ntap * 2 * sizeof(float), q->ctx.stream);
    q->d_taps2 = lqrt_malloc(ntap2 * 2 * sizeof(float));
    lqrt_h2d(q->d_taps2, tp2, ntap2 * 2 * sizeof(float), q->ctx.stream);
    lq_hist_init(&q->hist, q->L, q->esz, LQ_HIST_MIRROR);
    lqrt_sync(q->ctx.stream);
    {
        const int ck = q->kind == LQ_RRRF ? LQ_RRRF : LQ_CRCF;   /* real taps for every type */
        float *hb = (float *)lq_xmalloc((size_t)q->L * sizeof(float));
        q->hbs = (size_t)q->L * (ck == LQ_RRRF ? 1 : 2);
        q->hbank = (float *)lq_xmalloc((size_t)_npfb * q->hbs * sizeof(float));
        for (unsigned int b = 0; b < _npfb; b++) {
            for (unsigned int k = 0; k < q->L; k++) hb[k] = hf[b + k * _npfb];
            float *g = lq_host_taps(ck, hb, q->L, 1);
            memcpy(q->hbank + b * q->hbs, g, q->hbs * sizeof(float));
            free(g);
        }
        free(hb);
    }
    free(tp);
    free(tp2);
    free(hf);
    rs_plan_init(&q->pl);
    q->now = rs_initial;
    q->gpos = 0;
    return q;
}

void lq_rs_destroy(lq_rs *_q)
{
    lqrt_sync(_q->ctx.stream);
    lqrt_free(_q->d_taps);
    lqrt_free(_q->d_taps2);
    lq_hist_free(&_q->hist);
    lq_devbuf_free(&_q->d_tab);
    lq_devbuf_free(&_q->xbuf);
    lq_devbuf_free(&_q->ybuf);
    lq_devbuf_free(&_q->ubuf);
    lq_ctx_free(&_q->ctx);
    free(_q->hbank);
    rs_plan_free(&_q->pl);
    free(_q);
}

static void lq_rs_print(lq_rs *_q)
{
    printf("resampler [rate: %f]\n", _q->rate);
    printf("fir polyphase filterbank [%u] :\n", _q->npfb);
    for (unsigned int i = 0; i < _q->npfb; i++) printf("  bank %3u: \n", i);
}

void lq_rs_reset(lq_rs *_q)
{
    lq_hist_zero(&_q->hist, _q->ctx.stream);
    _q->now = rs_initial;
    _q->gpos = 0;
    /* a periodic plan that starts from the initial state stays usable */
    if (!(_q->pl.valid && _q->pl.periodic && rs_eq(&_q->pl.origin, &rs_initial))) _q->pl.valid = 0;
}


static void rs_new_del(lq_rs *q, float del)
{
    if (memcmp(&del, &q->del, 4) == 0) return;
    lqrt_sync(q->ctx.stream);
    rs_sync_now(q);
    q->del = del;
    q->pl.valid = 0;
    q->periodic_failed = 0;
    q->rate_changed = 1;
}

static void lq_rs_set_rate(lq_rs *_q, float _rate)
{
    if (_rate <= 0) LQ_FAIL("error: resamp_%s_set_rate(), resampling rate must be greater than zero\n", lq_ext(_q->kind));
    _q->rate = _rate;
    rs_new_del(_q, 1.0f / _q->rate);
}

/* resamp.c:222-239, including its clipping of the rate to [-0.5, 0.5] */
static void lq_rs_adjust_rate(lq_rs *_q, float _delta)
{
    if (_delta > 0.1f || _delta < -0.1f)
        LQ_FAIL("error: resamp_%s_adjust_rate(), resampling rate must be in [-0.1,0.1]\n", lq_ext(_q->kind));
    _q->rate += _delta;
    if (_q->rate > 0.5f) _q->rate = 0.5f;
    if (_q->rate < -0.5f) _q->rate = -0.5f;
    rs_new_del(_q, 1.0f / _q->rate);
}

unsigned long long lq_rs_num_output(lq_rs *_q, unsigned long long _nx)
{
    if (_nx == 0) return 0;
    /* periodic plans answer directly; otherwise simulate on a copy of the state */
    if (!(_q->pl.valid && _q->pl.periodic) && _nx >= RS_PERIODIC_MIN) rs_ensure_plan(_q, _nx);
    if (_q->pl.valid && (_q->pl.periodic || _q->gpos + _nx <= _q->pl.end))
        return rs_K(_q, _q->gpos + _nx) - rs_K(_q, _q->gpos);
    rs_check_rate(_q);
    return rs_count_outputs(rs_here(_q), _q->del, _q->npfb, _nx);
}

/* whether a launch on this plan takes a half-band stage of semi-length hm with it (k_resamp4's fused form) */
static int rs_fuses(const rs_plan *pl, unsigned int npfb, unsigned int L, float del, int hm)
{
    return pl->dk == RS_D4 && lqk_resamp4_hb_supported(npfb, L, del, hm);
}

void lq_rs_block_dev(lq_rs *_q, const void *_dxv, unsigned long long _nx, void *_dyv, unsigned long long *_ny)
{
    lq_rs_block_dev_hb(_q, _dxv, _nx, _dyv, _ny, NULL);
}

void lq_rs_block_dev_hb(lq_rs *_q, const void *_dxv, unsigned long long _nx, void *_dyv, unsigned long long *_ny,
                        const lq_rs_hb *hb)
{
    const char *_dx = (const char *)_dxv;
    char *_dy = (char *)_dyv;
    unsigned long long total = 0;
    /* launches of at most LQK_RS_MAXN inputs and 2^27 outputs (32-bit
     * buffer offsets in the kernel) */
    const double r = _q->rate > 1.0f ? (double)_q->rate : 1.0;
    const unsigned long long cmax = (unsigned long long)((double)LQK_RS_MAXN / (r + 1.0)) + 1;
    while (_nx > 0) {
        unsigned long long c = rs_ensure_plan(_q, _nx < cmax ? _nx : cmax);
        unsigned long long K0 = rs_K(_q, _q->gpos), K1 = rs_K(_q, _q->gpos + c);
        void *hold = lq_hist_dev(&_q->hist, _q->ctx.stream), *hnew = lq_hist_next(&_q->hist);
        const unsigned long long nk = K1 - K0;
        const int fuse = hb && nk > 0 && rs_fuses(&_q->pl, _q->npfb, _q->L, _q->del, hb->m);
        /* an unfused chain chunk: the resampler's outputs through ubuf */
        char *uy = hb && !fuse ? (char *)lq_devbuf_get(&_q->ubuf, (size_t)(nk ? nk : 1) * _q->esz) : _dy;
        if (_q->pl.dk == RS_D4) {
            lqk_rs4_plan kp = {_q->d_tab.p, _q->d_n, _q->pl.opre, _q->pl.npre, _q->pl.QT, _q->pl.PT};
            lqk_rs4_hb kh;
            if (fuse) {
                const int c0 = *hb->cur;
                kh.m = hb->m;
                memcpy(kh.h1, hb->h1, sizeof(kh.h1));
                kh.hist = hb->w[c0][0];
                kh.hist_new0 = hb->w[c0 ^ 1][0];
                kh.hist_new1 = hb->w[c0 ^ 1][1];
                *hb->cur = c0 ^ 1;
            }
            /* the kernel also writes the next history (no launch of its own) */
            const lqk_hist_job job = {hold, _dx, c, hnew, _q->L};
            lqk_resamp4(&kp, _q->gpos, K0, _q->npfb, _q->L, _q->del, _q->d_taps2, hold, _dx, c, uy, nk,
                        fuse ? &kh : NULL, &job, _q->ctx.stream);
        } else {
            lqk_rs_plan kp = {_q->d_tab.p, _q->pl.pre, _q->pl.P, _q->pl.Q, _q->pl.end, _q->pl.p2};
            lqk_resamp(_q->kind == LQ_RRRF, &kp, _q->gpos, K0, _q->npfb, _q->L, _q->del, _q->d_taps, _q->d_taps2,
                       hold, _dx, c, uy, nk, _q->ctx.stream);
        }
        if (hb && !fuse && nk > 0) hb->run(hb->ctx, uy, nk, _dy);
        if (_q->pl.dk != RS_D4) lqk_window_append(_q->kind != LQ_RRRF, hold, _q->L, _dx, c, hnew, _q->ctx.stream);
        lq_hist_flip(&_q->hist);
        _q->gpos += c;
        _dx += c * _q->esz;
        _dy += (hb ? 2 : 1) * nk * _q->esz;
        total += (hb ? 2 : 1) * nk;
        _nx -= c;
    }
    rs_sync_now(_q);
    if (_ny) *_ny = total;
}

/* small-call mode: one input on the host, resamp.c:245-311 as written (the
 * BOUNDARY state's y0 -- bank npfb-1 of the previous input, which the
 * reference stored -- is recomputed on the window one input older) */
static void lq_rs_exec1_host(lq_rs *q, const void *x, void *y, unsigned int *ny)
{
    rs_check_rate(q);
    const unsigned char *w = lq_hist_append(&q->hist, x, 1, q->ctx.stream);   /* L + 1 samples, x last */
    const int ck = q->kind == LQ_RRRF ? LQ_RRRF : LQ_CRCF;   /* real taps for every type */
    const unsigned int L = q->L, npfb = q->npfb;
    rs_state *s = &q->now;   /* the state at gpos (struct lq_rs_s) */
    unsigned int n = 0;
    while (rs_due(s, npfb)) {
        float y0[2] = {0.f, 0.f}, y1[2] = {0.f, 0.f};
        if (s->st == RS_BOUNDARY) {
            /* bank npfb-1 on the window one input older, bank 0 on the newest */
            lq_host_tdot(ck, q->hbank + (size_t)(npfb - 1) * q->hbs, w, L, y0);
            lq_host_tdot(ck, q->hbank, w + q->esz, L, y1);
        } else {
            lq_host_tdot(ck, q->hbank + (size_t)s->b * q->hbs, w + q->esz, L, y0);
            lq_host_tdot(ck, q->hbank + (size_t)(s->b + 1) * q->hbs, w + q->esz, L, y1);
        }
        const float a = 1.0f - s->mu;
        float *yo = (float *)((unsigned char *)y + (size_t)n * q->esz);
        yo[0] = a * y0[0] + s->mu * y1[0];
        if (q->kind != LQ_RRRF) yo[1] = a * y0[1] + s->mu * y1[1];
        n++;
        rs_advance(s, q->del, npfb);
    }
    rs_end_input(s, npfb);
    lq_hist_commit(&q->hist, 1);
    /* the device path continues from here: its plan position, or its state */
    if (q->pl.valid && (q->pl.periodic || q->gpos + 1 <= q->pl.end)) q->gpos += 1;
    else q->pl.valid = 0;
    *ny = n;
}

/* single: the call is resamp_*_execute (one input); execute_block always runs on the GPU */
static void lq_rs_block(lq_rs *_q, const void *_x, unsigned int _nx, void *_y, unsigned int *_ny, int single)
{
    if (_nx == 0) {
        *_ny = 0;
        return;
    }
    if (single && lq_small_host()) {
        lq_rs_exec1_host(_q, _x, _y, _ny);
        return;
    }
    unsigned long long nout = lq_rs_num_output(_q, _nx);
    const void *dx = lq_call_in(&_q->ctx, &_q->xbuf, _x, (size_t)_nx * _q->esz);
    void *dy = lq_devbuf_get(&_q->ybuf, (size_t)(nout ? nout : 1) * _q->esz);
    unsigned long long ny = 0;
    lq_rs_block_dev(_q, dx, _nx, dy, &ny);
    lq_call_out(&_q->ctx, _y, dy, (size_t)ny * _q->esz);
    *_ny = (unsigned int)ny;
}

lq_ctx *lq_rs_ctx(lq_rs *q) { return &q->ctx; }

#define LQ_RESAMP_FRONT(NAME, KIND, T)                                                                  \
    struct NAME##_s {                                                                               \
        lq_rs *e;                                                                                   \
    };                                                                                              \
    NAME NAME##_create(float _rate, unsigned int _m, float _fc, float _As, unsigned int _npfb)      \
    {                                                                                               \
        lq_rs *e = lq_rs_create(KIND, _rate, _m, _fc, _As, _npfb);                                  \
        NAME q = (NAME)lq_xmalloc(sizeof(*q));                                                      \
        q->e = e;                                                                                   \
        return q;                                                                                   \
    }                                                                                               \
    /* resamp.c:150-169: m = 7, fc = 0.25, As = 60, npfb = 64 */                                    \
    NAME NAME##_create_default(float _rate)                                                         \
    {                                                                                               \
        if (_rate <= 0)                                                                             \
            LQ_FAIL("error: " #NAME "_create_default(), resampling rate must be greater than zero\n"); \
        return NAME##_create(_rate, 7, 0.25f, 60.0f, 64);                                           \
    }                                                                                               \
    void NAME##_destroy(NAME _q)                                                                    \
    {                                                                                               \
        lq_rs_destroy(_q->e);                                                                       \
        free(_q);                                                                                   \
    }                                                                                               \
    void NAME##_print(NAME _q) { lq_rs_print(_q->e); }                                              \
    void NAME##_reset(NAME _q) { lq_rs_reset(_q->e); }                                              \
    unsigned int NAME##_get_delay(NAME _q) { return _q->e->m; }                                     \
    void NAME##_set_rate(NAME _q, float _rate) { lq_rs_set_rate(_q->e, _rate); }                     \
    void NAME##_adjust_rate(NAME _q, float _delta) { lq_rs_adjust_rate(_q->e, _delta); }             \
    unsigned long long NAME##_num_output(NAME _q, unsigned long long _nx)                           \
    {                                                                                               \
        return lq_rs_num_output(_q->e, _nx);                                                        \
    }                                                                                               \
    void NAME##_execute_block_dev(NAME _q, const T *_dx, unsigned long long _nx, T *_dy,            \
                                  unsigned long long *_ny)                                          \
    {                                                                                               \
        lq_rs_block_dev(_q->e, _dx, _nx, _dy, _ny);                                                 \
    }                                                                                               \
    void NAME##_execute_block(NAME _q, T *_x, unsigned int _nx, T *_y, unsigned int *_ny)           \
    {                                                                                               \
        lq_rs_block(_q->e, _x, _nx, _y, _ny, 0);                                                    \
    }                                                                                               \
    void NAME##_execute(NAME _q, T _x, T *_y, unsigned int *_num_written)                           \
    {                                                                                               \
        lq_rs_block(_q->e, &_x, 1, _y, _num_written, 1);                                            \
    }                                                                                               \
    void NAME##_set_stream(NAME _q, void *_s) { lq_ctx_set_stream(&_q->e->ctx, _s); }               \
    void NAME##_synchronize(NAME _q) { lqrt_sync(_q->e->ctx.stream); }

LQ_RESAMP_FRONT(resamp_rrrf, LQ_RRRF, float)
LQ_RESAMP_FRONT(resamp_crcf, LQ_CRCF, liquid_float_complex)
LQ_RESAMP_FRONT(resamp_cccf, LQ_CCCF, liquid_float_complex)

/* ---------------------------------------------------------------- test hooks
 * Host-only (no GPU): the plan of a fresh object at this rate from the
 * initial state -- periodic if `periodic`, else direct over nx inputs; with
 * d4, of a complex resampler with 2m = 14 taps per bank (which may use an
 * output plan), else of a real one.  0: no periodic plan within the search
 * limit (nothing is left allocated). */
static int rs_hook_plan(rs_plan *pl, float rate, unsigned int npfb, int periodic, unsigned long long nx, int d4)
{
    const float del = 1.0f / rate;
    const int kind = d4 ? LQ_CRCF : LQ_RRRF, want = rs_want_d4(kind, del, npfb, 14);
    rs_plan_init(pl);
    if (periodic) return rs_plan_build_periodic(pl, del, npfb, rs_initial, want);
    rs_build_direct(pl, kind, del, npfb, rs_initial, nx, want);
    return 1;
}

/* The kernel the first block call of nx inputs on a fresh object takes
 * (LQK_RS_ROUTE_*, lq_kernels.h) and, in *_tile, its tile: inputs for the
 * input-plan kernels, outputs for k_resamp4.  Host only: the plan that call
 * would build (rs_new_plan) and the launch's own decision on it.  -1: bad
 * arguments */
_Static_assert((int)LIQUID_MI355X_RESAMP3_CONST == (int)LQK_RS_ROUTE_R3_CONST &&
               (int)LIQUID_MI355X_RESAMP3_STRIDE == (int)LQK_RS_ROUTE_R3_STRIDE &&
               (int)LIQUID_MI355X_RESAMP == (int)LQK_RS_ROUTE_RS &&
               (int)LIQUID_MI355X_RESAMP_GENERIC == (int)LQK_RS_ROUTE_GENERIC &&
               (int)LIQUID_MI355X_RESAMP4_UP == (int)LQK_RS_ROUTE_RS4_UP &&
               (int)LIQUID_MI355X_RESAMP4_UP_R4 == (int)LQK_RS_ROUTE_RS4_UP_R4 &&
               (int)LIQUID_MI355X_RESAMP4_DOWN == (int)LQK_RS_ROUTE_RS4_DOWN &&
               (int)LIQUID_MI355X_RESAMP4_DOWN_DN == (int)LQK_RS_ROUTE_RS4_DOWN_DN, "route codes");

int lq_rs_route(int kind, float rate, unsigned int m, unsigned int npfb, unsigned long long nx, int hm,
                unsigned int *tile, int *fused)
{
    if (fused) *fused = 0;
    if (kind < LQ_RRRF || kind > LQ_CCCF || !(rate > 0.0f) || m == 0 || npfb == 0 || nx == 0) return -1;
    const float del = 1.0f / rate;
    const unsigned int L = 2 * m;
    rs_plan pl;
    int periodic_failed = 0, rate_changed = 0;
    rs_plan_init(&pl);
    rs_new_plan(&pl, kind, del, npfb, L, rs_initial, nx, &periodic_failed, &rate_changed);
    const int fuse = hm > 0 && rs_fuses(&pl, npfb, L, del, hm);
    const int route = pl.dk == RS_D4 ? lqk_resamp4_route(del, fuse ? hm : 0, tile)
                                     : lqk_resamp_route(kind == LQ_RRRF, pl.P, pl.pre, pl.end, npfb, L, del, tile);
    if (fused) *fused = fuse;
    rs_plan_free(&pl);
    return route;
}

int liquid_mi355x_resamp_route(int _kind, float _rate, unsigned int _m, unsigned int _npfb, unsigned long long _nx,
                               unsigned int *_tile)
{
    return lq_rs_route(_kind, _rate, _m, _npfb, _nx, 0, _tile, NULL);
}

/* Plan memory: the periodic plan's host checkpoint table allocation and the
 * device table's size (what the first call would upload).  Returns 1
 * (periodic plan), 0 (none). */
int liquid_mi355x_resamp_plan_bytes(float _rate, unsigned int _npfb, unsigned long long *_host,
                                    unsigned long long *_dev, unsigned long long *_period)
{
    rs_plan pl;
    const int ok = rs_hook_plan(&pl, _rate, _npfb, 1, 0, 1);
    *_host = (unsigned long long)pl.cap * sizeof(lqk_rs_entry);
    *_dev = ok ? (unsigned long long)pl.dn * pl.desz : 0;
    *_period = ok ? pl.P : 0;
    rs_plan_free(&pl);
    return ok;
}

/* The timing plan, expanded exactly as k_resamp replays it, recording for
 * every output the bank index (-1 for a BOUNDARY output), mu and input index
 * -- the format of the oracle's orc_resamp_schedule().  Returns the number
 * of outputs, or -1 if no periodic plan exists within the search limit. */
long long liquid_mi355x_resamp_schedule(float _rate, unsigned int _npfb, unsigned long long _nx, int _periodic,
                                        int *_b, float *_mu, unsigned int *_idx, unsigned long long _cap,
                                        unsigned long long *_pre, unsigned long long *_period)
{
    rs_plan pl;
    if (!rs_hook_plan(&pl, _rate, _npfb, _periodic, _nx, 0)) return -1;
    if (_pre) *_pre = pl.pre;
    if (_period) *_period = pl.P;
    long long k = 0;
    for (unsigned long long g = 0; g < _nx && k >= 0; g++) {
        unsigned long long K;
        rs_state s = rs_plan_at(&pl, g, &K);
        if (K != (unsigned long long)k) {
            k = -2;                          /* plan's output count disagrees with the replay */
            break;
        }
        for (; rs_due(&s, _npfb); rs_advance(&s, pl.del, _npfb), k++)
            if ((unsigned long long)k < _cap) {
                _b[k] = s.st == RS_INTERP ? s.b : -1;
                _mu[k] = s.mu;
                _idx[k] = (unsigned int)g;
            }
    }
    rs_plan_free(&pl);
    return k;
}

/* The output plan: when the plan is one (k_resamp4), every output expanded
 * exactly as k_resamp4 does: the entry at or before output k (periods
 * unwrapped), up to three steps, then bank (-1: BOUNDARY), mu and input
 * index.  Returns the number of outputs of the first nx inputs, -1 if no
 * plan, -3 if the plan is not an output plan. */
long long liquid_mi355x_resamp_schedule4(float _rate, unsigned int _npfb, unsigned long long _nx, int _periodic,
                                         int *_b, float *_mu, unsigned int *_idx, unsigned long long _cap,
                                         unsigned long long *_pre, unsigned long long *_period)
{
    rs_plan pl;
    if (!rs_hook_plan(&pl, _rate, _npfb, _periodic, _nx, 1)) return -1;
    if (pl.dk != RS_D4) {
        rs_plan_free(&pl);
        return -3;
    }
    if (_pre) *_pre = pl.opre;
    if (_period) *_period = pl.QT;
    unsigned long long Kn;
    rs_plan_at(&pl, _nx, &Kn);
    const lqk_rs4_entry *t = (const lqk_rs4_entry *)pl.dtab;
    const float del = pl.del, z = 1.0f - 1.0f / (float)_npfb, fn = (float)_npfb;
    long long ret = (long long)Kn;
    for (unsigned long long k = 0; k < Kn && k < _cap; k++) {
        unsigned long long idx = k >> 2, add = 0, skip = k & 3;
        if (k >= pl.opre) {
            const unsigned long long dt = k - pl.opre, c = dt / pl.QT, r = dt - c * pl.QT;
            idx = pl.npre + (r >> 2);
            skip = r & 3;
            add = c * pl.PT;
        }
        if (idx >= pl.dn) {
            ret = -2;
            break;
        }
        float tau = t[idx].tau;
        unsigned long long i = t[idx].i + add;
        for (unsigned s = 0; s < (unsigned)skip; s++) {   /* the kernel's step (k_resamp4.hip) */
            tau = tau + del;
            if (del > 1.0f) {
                tau = tau - 1.0f;
                i++;
            }
            if (!(tau < z)) {
                tau = tau - 1.0f;
                i++;
            }
            for (int e = 0; e < 2 && del >= 2.0f; e++)   /* 2 <= del < 4: up to two more silent inputs */
                if (!(tau < z)) {
                    tau = tau - 1.0f;
                    i++;
                }
        }
        const float bf = tau * fn, fb = floorf(bf);
        _b[k] = tau < 0.0f ? -1 : (int)fb;
        _mu[k] = bf - fb;
        _idx[k] = (unsigned int)i;
    }
    rs_plan_free(&pl);
    return ret;
}
