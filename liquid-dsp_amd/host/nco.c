/*
 * nco.c -- nco_crcf on the MI355X: oscillator, PLL and block mixer.
 *
 * API and semantics: include/liquid.h:5919-5999, src/nco/src/nco.c,
 * src/nco/src/nco.utilities.c.  The per-sample interface (phase, frequency,
 * step, sin / cos, the PLL, mix_up / mix_down) is the reference's state
 * machine restated, bit for bit, on the host; mix_block_up / mix_block_down
 * run on the GPU (csrc/k_nco.hip).
 *
 * Unlike every other object, create() does NOT require a device: a PLL
 * program calls only the per-sample interface and must run on a host without
 * a GPU.  The object takes its stream, buffers and device tables at the first
 * block call (or set_stream), which is where a missing device is fatal.
 *
 * Block calls.  The phase recurrence does not depend on the data, so the
 * host tabulates it as a plan of checkpoints (host/nco_plan.c) and the kernel
 * replays from them.  A plan belongs to one orbit -- the bits of d_theta and
 * of the phase it started from -- and the object stands at position `pos` of
 * it.  set_frequency, adjust_frequency, set_phase, adjust_phase, pll_step and
 * reset leave the orbit; step() moves one position along it (mix_up and
 * mix_down do not step).  Off the orbit the next block call builds a new plan
 * from the current phase, unless the current phase and frequency are the
 * origin of the plan at hand, which is then taken again from position 0.
 *   direct plan    the next max(n, NCO_DIRECT_MIN) positions: one host walk
 *                  of the recurrence, about as long as the reference's own
 *                  loop over those samples without the arithmetic;
 *   periodic plan  pre-period + period positions, found once by cycle
 *                  detection, serving the orbit for good.  Built once direct
 *                  plans have walked NCO_AUTO_PERIODIC positions of one orbit;
 *                  an orbit whose pre-period + period exceeds NCO_PERIOD_CAP
 *                  stays on direct plans.
 * LQ_NCO_PLAN=direct / =periodic, read at create, forces the form (tests).
 * The phase after a block is a plan lookup on the host: get_phase() does not
 * wait for the device.
 *
 * |d_theta| > 2 pi (or a phase beyond 2 pi, or a non-finite one) can leave
 * [-pi, pi] for good -- there is one wrap per step -- and the reference's
 * index conversion is then undefined: such objects run block calls in the
 * host loop (device_eligible() == 0).
 */
#include <complex.h>

#include "lq_host.h"

#define NCO_DIRECT_MIN 4096ull
#define NCO_AUTO_PERIODIC (1ull << 22)
#define NCO_PERIOD_CAP (1ull << 27)

enum { NCO_PLAN_AUTO = 0, NCO_PLAN_DIRECT = 1, NCO_PLAN_PERIODIC = 2 };

struct nco_crcf_s {
    liquid_ncotype type;
    float theta, d_theta;
    float sintab[256];
    float alpha, beta;        /* PLL: frequency and phase proportion */
    /* block calls */
    int dev_ready;
    lq_ctx ctx;
    lq_devbuf xbuf, ybuf, tabbuf;
    float *dsintab;
    int force;
    nco_plan plan;
    int on_plan;              /* theta is the plan's phase at pos */
    unsigned long long pos;
    unsigned long long walked;/* positions of this orbit walked by direct plans */
    int aperiodic;            /* no period within NCO_PERIOD_CAP on this orbit */
};

static void nco_sincos(nco_crcf q, float *s, float *c)
{
    if (q->type == LIQUID_NCO) {
        const unsigned int k = nco_table_index(q->theta);
        *s = q->sintab[k];
        *c = q->sintab[(k + 64) & 0xff];
    } else {
        *s = sinf(q->theta);
        *c = cosf(q->theta);
    }
}

static void nco_constrain(nco_crcf q)
{
    if (q->theta > NCO_PI) q->theta -= 2 * NCO_PI;
    else if (q->theta < -NCO_PI) q->theta += 2 * NCO_PI;
}

nco_crcf nco_crcf_create(liquid_ncotype _type)
{
    if (_type != LIQUID_NCO && _type != LIQUID_VCO) LQ_FAIL("error: nco_crcf_create(), unknown type : %u\n", _type);
    nco_crcf q = (nco_crcf)lq_xmalloc(sizeof(*q));
    q->type = _type;
    for (unsigned int i = 0; i < 256; i++) q->sintab[i] = sinf(2.0f * NCO_PI * (float)(i) / 256.0f);
    nco_crcf_pll_set_bandwidth(q, 0.1);
    const char *e = getenv("LQ_NCO_PLAN");
    q->force = !e ? NCO_PLAN_AUTO : !strcmp(e, "direct") ? NCO_PLAN_DIRECT : !strcmp(e, "periodic") ? NCO_PLAN_PERIODIC
                                                                                                    : NCO_PLAN_AUTO;
    nco_plan_init(&q->plan);
    nco_crcf_reset(q);
    return q;
}

void nco_crcf_destroy(nco_crcf _q)
{
    if (_q->dev_ready) {
        lqrt_sync(_q->ctx.stream);
        lq_devbuf_free(&_q->xbuf);
        lq_devbuf_free(&_q->ybuf);
        lq_devbuf_free(&_q->tabbuf);
        lqrt_free(_q->dsintab);
        lq_ctx_free(&_q->ctx);
    }
    nco_plan_free(&_q->plan);
    free(_q);
}

void nco_crcf_print(nco_crcf _q)
{
    printf("nco [type: %s, phase: %12.8f, frequency: %12.8f]\n", _q->type == LIQUID_NCO ? "nco" : "vco", _q->theta,
           _q->d_theta);
}

void nco_crcf_reset(nco_crcf _q)
{
    _q->theta = 0;
    _q->d_theta = 0;
    _q->on_plan = 0;
}

float nco_crcf_get_frequency(nco_crcf _q) { return _q->d_theta; }
float nco_crcf_get_phase(nco_crcf _q) { return _q->theta; }

void nco_crcf_set_frequency(nco_crcf _q, float _f)
{
    _q->d_theta = _f;
    _q->on_plan = 0;
}

void nco_crcf_adjust_frequency(nco_crcf _q, float _df)
{
    _q->d_theta += _df;
    _q->on_plan = 0;
}

void nco_crcf_set_phase(nco_crcf _q, float _phi)
{
    _q->theta = _phi;
    nco_constrain(_q);
    _q->on_plan = 0;
}

void nco_crcf_adjust_phase(nco_crcf _q, float _dphi)
{
    _q->theta += _dphi;
    nco_constrain(_q);
    _q->on_plan = 0;
}

void nco_crcf_step(nco_crcf _q)
{
    _q->theta = nco_step_theta(_q->theta, _q->d_theta);
    if (!_q->on_plan) return;
    /* one step from plan position pos is plan position pos + 1 */
    _q->pos++;
    if (_q->plan.periodic) _q->pos = nco_plan_reduce(&_q->plan, _q->pos);
    else if (_q->pos > _q->plan.end) _q->on_plan = 0;
}

float nco_crcf_sin(nco_crcf _q)
{
    float s, c;
    nco_sincos(_q, &s, &c);
    return s;
}

float nco_crcf_cos(nco_crcf _q)
{
    float s, c;
    nco_sincos(_q, &s, &c);
    return c;
}

void nco_crcf_sincos(nco_crcf _q, float *_s, float *_c) { nco_sincos(_q, _s, _c); }

void nco_crcf_cexpf(nco_crcf _q, liquid_float_complex *_y)
{
    float s, c;
    nco_sincos(_q, &s, &c);
    *_y = c + _Complex_I * s;
}

void nco_crcf_pll_set_bandwidth(nco_crcf _q, float _bandwidth)
{
    if (_bandwidth < 0.0f) LQ_FAIL("error: nco_pll_set_bandwidth(), bandwidth must be positive\n");
    _q->alpha = _bandwidth;
    _q->beta = sqrtf(_q->alpha);
}

void nco_crcf_pll_step(nco_crcf _q, float _dphi)
{
    nco_crcf_adjust_frequency(_q, _dphi * _q->alpha);
    nco_crcf_adjust_phase(_q, _dphi * _q->beta);
}

void nco_crcf_mix_up(nco_crcf _q, liquid_float_complex _x, liquid_float_complex *_y)
{
    float s, c;
    nco_sincos(_q, &s, &c);
    *_y = _x * (c + _Complex_I * s);
}

void nco_crcf_mix_down(nco_crcf _q, liquid_float_complex _x, liquid_float_complex *_y)
{
    float s, c;
    nco_sincos(_q, &s, &c);
    *_y = _x * (c - _Complex_I * s);
}

/* ----------------------------------------------------------------- block calls */

int nco_crcf_device_eligible(nco_crcf _q)
{
    const float lim = 6.2831855f;   /* (float)(2 pi) */
    return isfinite(_q->theta) && isfinite(_q->d_theta) && fabsf(_q->theta) <= lim && fabsf(_q->d_theta) <= lim;
}

/* the reference's loop (nco.c:294-300, 331-337), host pointers, y == x allowed */
static void nco_block_host(nco_crcf q, const liquid_float_complex *x, liquid_float_complex *y, unsigned long long n,
                           int down)
{
    for (unsigned long long i = 0; i < n; i++) {
        if (down) nco_crcf_mix_down(q, x[i], &y[i]);
        else nco_crcf_mix_up(q, x[i], &y[i]);
        nco_crcf_step(q);
    }
}

static void nco_device(nco_crcf q)
{
    if (q->dev_ready) return;
    lqrt_require_device("nco_crcf_mix_block");
    lq_ctx_init(&q->ctx);
    q->dsintab = (float *)lqrt_malloc(sizeof(q->sintab));
    lqrt_h2d(q->dsintab, q->sintab, sizeof(q->sintab), q->ctx.stream);
    lqrt_sync(q->ctx.stream);
    q->dev_ready = 1;
}

/* a plan that serves the next n positions from the current state, uploaded */
static void nco_plan_for(nco_crcf q, unsigned long long n)
{
    nco_plan *pl = &q->plan;
    if (q->on_plan && pl->valid && (pl->periodic || q->pos + n <= pl->end)) return;
    if (!q->on_plan) {
        q->walked = 0;
        q->aperiodic = 0;
        /* back at the origin of the plan at hand (a reset and the same settings, say) */
        if (pl->valid && nco_same_bits(pl->d_theta, q->d_theta) && nco_same_bits(pl->theta0, q->theta) &&
            (pl->periodic || n <= pl->end)) {
            q->pos = 0;
            q->on_plan = 1;
            return;
        }
    }
    int periodic = q->force == NCO_PLAN_PERIODIC ||
                   (q->force == NCO_PLAN_AUTO && !q->aperiodic && q->walked >= NCO_AUTO_PERIODIC);
    if (periodic && !nco_plan_build_periodic(pl, q->theta, q->d_theta, NCO_PERIOD_CAP)) {
        q->aperiodic = 1;
        periodic = 0;
    }
    if (!periodic) {
        const unsigned long long len = n > NCO_DIRECT_MIN ? n : NCO_DIRECT_MIN;
        if (!nco_plan_build_direct(pl, q->theta, q->d_theta, len)) LQ_FAIL("error: nco_crcf: out of host memory\n");
        q->walked += len;
    }
    q->pos = 0;
    q->on_plan = 1;
    /* the copy reads the host table: it has ended before the table can change */
    const size_t bytes = pl->ntab * sizeof(float);
    lqrt_h2d(lq_devbuf_get(&q->tabbuf, bytes), pl->tab, bytes, q->ctx.stream);
    lqrt_sync(q->ctx.stream);
}

static void nco_block_dev(nco_crcf q, const liquid_float_complex *dx, liquid_float_complex *dy, unsigned long long n,
                          int down)
{
    if (n == 0) return;
    nco_device(q);
    if (!nco_crcf_device_eligible(q)) {
        /* device pointers on an object the kernel does not take: through the host loop */
        const size_t bytes = (size_t)n * sizeof(liquid_float_complex);
        liquid_float_complex *h = (liquid_float_complex *)lq_xmalloc(bytes);
        lqrt_d2h(h, dx, bytes, q->ctx.stream);
        lqrt_sync(q->ctx.stream);
        nco_block_host(q, h, h, n, down);
        lqrt_h2d(dy, h, bytes, q->ctx.stream);
        lqrt_sync(q->ctx.stream);
        free(h);
        return;
    }
    while (n) {
        const unsigned long long m = n < LQK_NCO_MAXN ? n : LQK_NCO_MAXN;
        nco_plan_for(q, m);
        const nco_plan *pl = &q->plan;
        const lqk_nco_plan kp = {(const float *)q->tabbuf.p, q->pos,       pl->periodic ? pl->pre : 0,
                                 pl->periodic ? pl->P : 0,   pl->d_theta, pl->th_pre};
        lqk_nco_mix(q->type == LIQUID_VCO, down, &kp, q->dsintab, dx, dy, m, q->ctx.stream);
        q->pos = nco_plan_reduce(pl, q->pos + m);
        q->theta = nco_plan_at(pl, q->pos);
        dx += m;
        dy += m;
        n -= m;
    }
}

static void nco_block(nco_crcf q, liquid_float_complex *x, liquid_float_complex *y, unsigned long long n, int down)
{
    if (n == 0) return;
    if (!nco_crcf_device_eligible(q)) {
        nco_block_host(q, x, y, n, down);
        return;
    }
    nco_device(q);
    const size_t bytes = (size_t)n * sizeof(liquid_float_complex);
    const liquid_float_complex *dx = (const liquid_float_complex *)lq_call_in(&q->ctx, &q->xbuf, x, bytes);
    liquid_float_complex *dy = (liquid_float_complex *)lq_devbuf_get(&q->ybuf, bytes);
    nco_block_dev(q, dx, dy, n, down);
    lq_call_out(&q->ctx, y, dy, bytes);
}

void nco_crcf_mix_block_up(nco_crcf _q, liquid_float_complex *_x, liquid_float_complex *_y, unsigned int _N)
{
    nco_block(_q, _x, _y, _N, 0);
}

void nco_crcf_mix_block_down(nco_crcf _q, liquid_float_complex *_x, liquid_float_complex *_y, unsigned int _N)
{
    nco_block(_q, _x, _y, _N, 1);
}

void nco_crcf_mix_block_up_dev(nco_crcf _q, const liquid_float_complex *_dx, liquid_float_complex *_dy,
                               unsigned long long _n)
{
    nco_block_dev(_q, _dx, _dy, _n, 0);
}

void nco_crcf_mix_block_down_dev(nco_crcf _q, const liquid_float_complex *_dx, liquid_float_complex *_dy,
                                 unsigned long long _n)
{
    nco_block_dev(_q, _dx, _dy, _n, 1);
}

void nco_crcf_set_stream(nco_crcf _q, void *_s)
{
    nco_device(_q);
    lq_ctx_set_stream(&_q->ctx, _s);
}

void nco_crcf_synchronize(nco_crcf _q)
{
    if (_q->dev_ready) lqrt_sync(_q->ctx.stream);
}

unsigned int liquid_mi355x_nco_tile(void) { return LQK_NCO_TILE; }
unsigned int liquid_mi355x_nco_checkpoint(void) { return LQK_NCO_CK; }

/* The phases a plan serves for positions 0 .. n-1 -- each the checkpoint
 * before it stepped forward, as the kernel replays it, periods unwrapped --
 * and for the NCO type their table indices (_index may be NULL, as may _theta).
 * periodic: the periodic form, else the direct form for n positions.  Returns
 * n, or -1 when no plan could be made (no period within the search limit).
 * No GPU call. */
long long liquid_mi355x_nco_walk(liquid_ncotype _type, float _theta0, float _d_theta, unsigned long long _n,
                                 int _periodic, float *_theta, unsigned int *_index, unsigned long long *_pre,
                                 unsigned long long *_period)
{
    nco_plan pl;
    nco_plan_init(&pl);
    const int ok = _periodic ? nco_plan_build_periodic(&pl, _theta0, _d_theta, NCO_PERIOD_CAP)
                             : nco_plan_build_direct(&pl, _theta0, _d_theta, _n);
    if (!ok) return -1;
    if (_pre) *_pre = pl.periodic ? pl.pre : 0;
    if (_period) *_period = pl.periodic ? pl.P : 0;
    for (unsigned long long g = 0; g < _n; g++) {
        const float th = nco_plan_at(&pl, g);
        if (_theta) _theta[g] = th;
        if (_index) _index[g] = _type == LIQUID_NCO ? nco_table_index(th) : 0;
    }
    nco_plan_free(&pl);
    return (long long)_n;
}

/* ----------------------------------------------------------------- nco.utilities.c */

void liquid_unwrap_phase(float *_theta, unsigned int _n)
{
    for (unsigned int i = 1; i < _n; i++) {
        while ((_theta[i] - _theta[i - 1]) > NCO_PI) _theta[i] -= 2 * NCO_PI;
        while ((_theta[i] - _theta[i - 1]) < -NCO_PI) _theta[i] += 2 * NCO_PI;
    }
}

void liquid_unwrap_phase2(float *_theta, unsigned int _n)
{
    fprintf(stderr, "warning: liquid_unwrap_phase2() has not yet been tested!\n");
    float dphi = 0.0f;
    for (unsigned int i = 1; i < _n; i++) dphi += _theta[i] - _theta[i - 1];
    dphi /= (float)(_n - 1);
    for (unsigned int i = 1; i < _n; i++) {
        while ((_theta[i] - _theta[i - 1]) > NCO_PI + dphi) _theta[i] -= 2 * NCO_PI;
        while ((_theta[i] - _theta[i - 1]) < -NCO_PI + dphi) _theta[i] += 2 * NCO_PI;
    }
}
