/*
 * iirdecim.c -- iirdecim_{rrrf,crcf,cccf} and iirinterp_{rrrf,crcf,cccf}:
 * the recursive decimator and interpolator by an integer factor M.
 *
 * include/liquid.h:2570-2650, 2738-2820, src/filter/src/iirdecim.c,
 * iirinterp.c.  Each object is M and one recursive filter running at the full
 * rate (the lq_iir engine of iirfilt.c, which owns the state and its mirror):
 *   iirdecim   execute reads M samples, runs the filter over all of them and
 *              returns its output for the first; execute_block(x, n, y) reads
 *              n M samples and writes n
 *   iirinterp  execute feeds x and then M - 1 zeros and returns all M outputs
 *              (no gain compensation); execute_block(x, n, y) reads n samples
 *              and writes n M.  groupdelay is the filter's divided by M.
 * Block calls run on the GPU, fused (lqk_iirfilt_decim / lqk_iirfilt_interp:
 * the dropped outputs and the fed zeros never reach memory), when the filter
 * is device-eligible and M <= LQK_IIRFILT_TILE; otherwise in the host loop.
 * execute follows the small-call rule.  The messages of the M < 2 checks are
 * the reference's (both objects name iirinterp there).
 */
#include "lq_host.h"

typedef struct {
    unsigned int M;
    int mode;   /* 1 decimator, 2 interpolator */
    lq_iir *f;
} lq_iirrate;

static lq_iirrate *rate_new(int mode, unsigned int M, lq_iir *f)
{
    lq_iirrate *q = (lq_iirrate *)lq_xmalloc(sizeof(*q));
    q->M = M;
    q->mode = mode;
    q->f = f;
    return q;
}

static lq_iirrate *rate_create(int mode, int kind, unsigned int M, const void *b, unsigned int nb, const void *a,
                               unsigned int na)
{
    if (M < 2) LQ_FAIL("error: iirinterp_%s_create(), interp factor must be greater than 1\n", lq_ext(kind));
    return rate_new(mode, M, lq_iir_create(kind, b, nb, a, na));
}

static lq_iirrate *rate_create_prototype(int mode, int kind, unsigned int M, liquid_iirdes_filtertype ftype,
                                         liquid_iirdes_bandtype btype, liquid_iirdes_format format,
                                         unsigned int order, float fc, float f0, float Ap, float As)
{
    if (M < 2)
        LQ_FAIL("error: iirinterp_%s_create_prototype(), interp factor must be greater than 1\n", lq_ext(kind));
    return rate_new(mode, M, lq_iir_create_prototype(kind, ftype, btype, format, order, fc, f0, Ap, As));
}

static lq_iirrate *rate_create_default(int mode, int kind, unsigned int M, unsigned int order)
{
    return rate_create_prototype(mode, kind, M, LIQUID_IIRDES_BUTTER, LIQUID_IIRDES_LOWPASS, LIQUID_IIRDES_SOS, order,
                                 0.5f / (float)M, 0.0f, 0.1f, 60.0f);
}

static void rate_destroy(lq_iirrate *q)
{
    lq_iir_destroy(q->f);
    free(q);
}

static void rate_print(lq_iirrate *q)
{
    printf("interp():\n");
    printf("    M       :   %u\n", q->M);
    lq_iir_print(q->f);
}

static float rate_groupdelay(lq_iirrate *q, float fc)
{
    const float g = lq_iir_groupdelay(q->f, fc);
    return q->mode == 2 ? g / (float)q->M : g;
}

/* ------------------------------------------------------------------ typed front ends */
#define LQ_IIRRATE_COMMON(OBJ, MODE, KIND, TO, TC, TI)                                                         \
    struct OBJ##_s {                                                                                           \
        lq_iirrate e;                                                                                          \
    };                                                                                                         \
    OBJ OBJ##_create(unsigned int _M, TC *_b, unsigned int _nb, TC *_a, unsigned int _na)                      \
    {                                                                                                          \
        return (OBJ)rate_create(MODE, KIND, _M, _b, _nb, _a, _na);                                             \
    }                                                                                                          \
    OBJ OBJ##_create_default(unsigned int _M, unsigned int _order)                                             \
    {                                                                                                          \
        return (OBJ)rate_create_default(MODE, KIND, _M, _order);                                               \
    }                                                                                                          \
    OBJ OBJ##_create_prototype(unsigned int _M, liquid_iirdes_filtertype _ftype, liquid_iirdes_bandtype _btype, \
                               liquid_iirdes_format _format, unsigned int _order, float _fc, float _f0,        \
                               float _Ap, float _As)                                                           \
    {                                                                                                          \
        return (OBJ)rate_create_prototype(MODE, KIND, _M, _ftype, _btype, _format, _order, _fc, _f0, _Ap, _As); \
    }                                                                                                          \
    void OBJ##_destroy(OBJ _q) { rate_destroy(&_q->e); }                                                       \
    void OBJ##_print(OBJ _q) { rate_print(&_q->e); }                                                           \
    void OBJ##_reset(OBJ _q) { lq_iir_reset(_q->e.f); }                                                        \
    void OBJ##_execute_block(OBJ _q, TI *_x, unsigned int _n, TO *_y)                                          \
    {                                                                                                          \
        lq_iir_run_rate(_q->e.f, MODE, _q->e.M, _x, _n, _y, 0);                                                \
    }                                                                                                          \
    void OBJ##_execute_block_dev(OBJ _q, const TI *_dx, unsigned long long _n, TO *_dy)                        \
    {                                                                                                          \
        lq_iir_run_rate_dev(_q->e.f, MODE, _q->e.M, _dx, _n, _dy);                                             \
    }                                                                                                          \
    float OBJ##_groupdelay(OBJ _q, float _fc) { return rate_groupdelay(&_q->e, _fc); }                         \
    int OBJ##_device_eligible(OBJ _q) { return lq_iir_rate_eligible(_q->e.f, _q->e.M); }                       \
    void OBJ##_set_stream(OBJ _q, void *_s) { lq_ctx_set_stream(lq_iir_ctx(_q->e.f), _s); }                    \
    void OBJ##_synchronize(OBJ _q) { lqrt_sync(lq_iir_ctx(_q->e.f)->stream); }

#define LQ_IIRDECIM_DEFINE(OBJ, KIND, TO, TC, TI)                                                              \
    LQ_IIRRATE_COMMON(OBJ, 1, KIND, TO, TC, TI)                                                                \
    void OBJ##_execute(OBJ _q, TI *_x, TO *_y) { lq_iir_run_rate(_q->e.f, 1, _q->e.M, _x, 1, _y, 1); }

#define LQ_IIRINTERP_DEFINE(OBJ, KIND, TO, TC, TI)                                                             \
    LQ_IIRRATE_COMMON(OBJ, 2, KIND, TO, TC, TI)                                                                \
    void OBJ##_execute(OBJ _q, TI _x, TO *_y) { lq_iir_run_rate(_q->e.f, 2, _q->e.M, &_x, 1, _y, 1); }

LQ_IIRDECIM_DEFINE(iirdecim_rrrf, LQ_RRRF, float, float, float)
LQ_IIRDECIM_DEFINE(iirdecim_crcf, LQ_CRCF, liquid_float_complex, float, liquid_float_complex)
LQ_IIRDECIM_DEFINE(iirdecim_cccf, LQ_CCCF, liquid_float_complex, liquid_float_complex, liquid_float_complex)
LQ_IIRINTERP_DEFINE(iirinterp_rrrf, LQ_RRRF, float, float, float)
LQ_IIRINTERP_DEFINE(iirinterp_crcf, LQ_CRCF, liquid_float_complex, float, liquid_float_complex)
LQ_IIRINTERP_DEFINE(iirinterp_cccf, LQ_CCCF, liquid_float_complex, liquid_float_complex, liquid_float_complex)
