/*
 * iirfilt.c -- iirfilt_{rrrf,crcf,cccf}: recursive (infinite impulse
 * response) filters, the engine behind them (lq_iir in lq_host.h, which
 * iirdecim.c runs as a decimator or an interpolator), and the PLL and
 * group-delay helpers.  The filter designs are in iirdes.c.
 *
 * include/liquid.h:2247-2378, src/filter/src/iirfilt.c, iirfiltsos.c,
 * iirdes.pll.c, group_delay.c:64-117.
 *   NORM form (create): coefficients divided by a[0]; direct form II over
 *     n = max(nb, na) states v[0..n-1]:
 *       v[i] <- v[i-1];  v[0] = x - sum_{i>=1} a[i] v[i];  y = sum b[i] v[i]
 *   SOS form (create_sos, _pll, _integrator, _differentiator): a cascade of
 *     direct-form-II sections, each normalised by its own a[0]:
 *       v2 <- v1 <- v0;  v0 = x - a1 v1 - a2 v2;  y = b0 v0 + b1 v1 + b2 v2
 * The state kept between calls is what the next sample will see as v[1],
 * v[2] per section (SOS) or v[1..n-1] (NORM); the device and the host loop
 * share that layout through one mirror.
 *
 * Where a call runs.  An object is device-eligible when its recurrence can be
 * cut into spans without losing accuracy (csrc/k_iirfilt.hip; DESIGN.md,
 * "iirfilt: block-parallel recurrence"): SOS form with nsos <= 8, or NORM
 * form with n <= 3 (run as one section), every coefficient finite and every
 * pole of every section inside or on the unit circle, decided once at create
 * in float64 from the stored float32 coefficients.  execute_block and
 * execute_block_dev of an eligible object run on the GPU.  Any other object
 * runs the host loop below (device pointers: copy, loop, copy back): for an
 * unstable or badly conditioned filter the split into zero-state and
 * homogeneous parts cancels catastrophically.  execute (one sample) follows
 * the small-call rule (lq_small.c): the host loop unless LQ_SMALL_CALLS=gpu.
 * The host loop is the reference's statement order in float32.
 *
 * iirfilt_*_create_prototype and _create_lowpass stay undeclared and are not
 * exported (tests/test_iirfilt_model.py holds the library to that): a caller
 * designs with liquid_iirdes (iirdes.c) and passes the result to create_sos
 * or create.  The engine's own lq_iir_create_prototype does exactly that for
 * iirdecim and iirinterp.
 *
 * Rate changing (lq_iir_run_rate; iirdecim.c:121-145, iirinterp.c:120-141):
 * the same filter at the full rate with M - 1 of every M outputs dropped
 * (the first of each group of M is kept), or with M - 1 zeros fed after each
 * input.  On the device neither the dropped outputs nor the zeros are ever in
 * memory (lqk_iirfilt_decim, lqk_iirfilt_interp); M above LQK_IIRFILT_TILE,
 * like an object that is not eligible, runs the host loop with the stride.
 */
#include <complex.h>
#include <math.h>

#include "lq_host.h"

static const char *const kind_name[3] = {"rrrf", "crcf", "cccf"};

struct lq_iir_s {
    int kind, sos;
    unsigned int nb, na, n, nsos;
    int cw, sw;               /* floats per coefficient / per sample */
    float *b, *a;             /* as the reference keeps them: NORM normalised, SOS as given (3 per section) */
    float *sb, *sa;           /* SOS: the sections' normalised coefficients */
    int dev_ok;
    unsigned int nsec;        /* sections of the device form */
    void *d_coef, *d_lad, *d_state;
    lq_mirror sm;             /* the state (host side; device side d_state) */
    lq_ctx ctx;
    lq_devbuf xbuf, ybuf, work;
};

/* ------------------------------------------------------------------ float32 arithmetic of one kind */
#define LQ_INL static inline __attribute__((always_inline))

/* o = k s: real x real, real x complex (per component), complex x complex */
LQ_INL void kmul(int kind, const float *k, const float *s, float *o)
{
    if (kind == LQ_RRRF) {
        o[0] = k[0] * s[0];
    } else if (kind == LQ_CRCF) {
        o[0] = k[0] * s[0];
        o[1] = k[0] * s[1];
    } else {
        const float re = k[0] * s[0] - k[1] * s[1], im = k[0] * s[1] + k[1] * s[0];
        o[0] = re;
        o[1] = im;
    }
}

/* iirfilt.c:488-522 (execute_norm) on v[0..n-1] */
LQ_INL void norm_step(int kind, const lq_iir *q, float *v, const float *x, float *y)
{
    const int sw = kind == LQ_RRRF ? 1 : 2, cw = kind == LQ_CCCF ? 2 : 1;
    float t[2], v0[2] = {0, 0}, y0[2] = {0, 0};
    for (unsigned int i = q->n - 1; i > 0; i--)
        for (int c = 0; c < sw; c++) v[sw * i + c] = v[sw * (i - 1) + c];
    for (int c = 0; c < sw; c++) v0[c] = x[c];
    for (unsigned int i = 1; i < q->na; i++) {
        kmul(kind, q->a + cw * i, v + sw * i, t);
        for (int c = 0; c < sw; c++) v0[c] -= t[c];
    }
    for (int c = 0; c < sw; c++) v[c] = v0[c];
    for (unsigned int i = 0; i < q->nb; i++) {
        kmul(kind, q->b + cw * i, v + sw * i, t);
        for (int c = 0; c < sw; c++) y0[c] += t[c];
    }
    for (int c = 0; c < sw; c++) y[c] = y0[c];
}

/* iirfilt.c:528-543 over iirfiltsos.c:167-184 (execute_df2); s = (v1, v2) per section */
LQ_INL void sos_step(int kind, const lq_iir *q, float *s, const float *x, float *y)
{
    const int sw = kind == LQ_RRRF ? 1 : 2, cw = kind == LQ_CCCF ? 2 : 1;
    float t0[2] = {x[0], sw == 2 ? x[1] : 0.0f}, t1[2] = {0, 0};
    for (unsigned int k = 0; k < q->nsos; k++) {
        const float *b = q->sb + 3 * cw * k, *a = q->sa + 3 * cw * k;
        float *v1 = s + 2 * sw * k, *v2 = v1 + sw, p[2], r[2], v0[2];
        kmul(kind, a + cw, v1, p);
        kmul(kind, a + 2 * cw, v2, r);
        for (int c = 0; c < sw; c++) v0[c] = t0[c] - p[c] - r[c];
        float u0[2], u1[2], u2[2];
        kmul(kind, b, v0, u0);
        kmul(kind, b + cw, v1, u1);
        kmul(kind, b + 2 * cw, v2, u2);
        for (int c = 0; c < sw; c++) {
            t1[c] = u0[c] + u1[c] + u2[c];
            v2[c] = v1[c];
            v1[c] = v0[c];
            t0[c] = t1[c];
        }
    }
    for (int c = 0; c < sw; c++) y[c] = t1[c];
}

LQ_INL void host_loop_k(int kind, const lq_iir *q, float *s, const float *x, unsigned long long n, float *y)
{
    const int sw = kind == LQ_RRRF ? 1 : 2;
    float t[2];
    for (unsigned long long i = 0; i < n; i++) {   /* y may be x: read first */
        if (q->sos)
            sos_step(kind, q, s, x + sw * i, t);
        else
            norm_step(kind, q, s, x + sw * i, t);
        for (int c = 0; c < sw; c++) y[sw * i + c] = t[c];
    }
}

static void host_loop(lq_iir *q, const void *x, unsigned long long n, void *y)
{
    if (n == 0) return;
    lq_mirror_need_host(&q->sm, q->d_state, q->ctx.stream);
    float *s = (float *)lq_mirror_ptr(&q->sm);
    if (q->kind == LQ_RRRF)
        host_loop_k(LQ_RRRF, q, s, (const float *)x, n, (float *)y);
    else if (q->kind == LQ_CRCF)
        host_loop_k(LQ_CRCF, q, s, (const float *)x, n, (float *)y);
    else
        host_loop_k(LQ_CCCF, q, s, (const float *)x, n, (float *)y);
    q->sm.dev_valid = 0;
}

/* nf full-rate samples: mode 1 reads them all and keeps the outputs at the
 * multiples of M (y may be x: output i / M is written after input i is read),
 * mode 2 reads x[i / M] at the multiples of M and zero elsewhere */
LQ_INL void host_rate_k(int kind, const lq_iir *q, float *s, int mode, unsigned int M, const float *x,
                        unsigned long long nf, float *y)
{
    const int sw = kind == LQ_RRRF ? 1 : 2;
    const float zero[2] = {0.0f, 0.0f};
    float t[2];
    unsigned int ph = 0;   /* i mod M */
    for (unsigned long long i = 0, k = 0; i < nf; i++) {
        const float *in = mode == 1 ? x + sw * i : (ph == 0 ? x + sw * k : zero);
        if (q->sos)
            sos_step(kind, q, s, in, t);
        else
            norm_step(kind, q, s, in, t);
        float *out = mode == 1 ? y + sw * k : y + sw * i;
        if (mode == 2 || ph == 0)
            for (int c = 0; c < sw; c++) out[c] = t[c];
        if (ph == 0 && mode == 1) k++;
        if (++ph == M) {
            ph = 0;
            if (mode == 2) k++;
        }
    }
}

static void host_rate(lq_iir *q, int mode, unsigned int M, const void *x, unsigned long long nf, void *y)
{
    if (nf == 0) return;
    lq_mirror_need_host(&q->sm, q->d_state, q->ctx.stream);
    float *s = (float *)lq_mirror_ptr(&q->sm);
    if (q->kind == LQ_RRRF)
        host_rate_k(LQ_RRRF, q, s, mode, M, (const float *)x, nf, (float *)y);
    else if (q->kind == LQ_CRCF)
        host_rate_k(LQ_CRCF, q, s, mode, M, (const float *)x, nf, (float *)y);
    else
        host_rate_k(LQ_CCCF, q, s, mode, M, (const float *)x, nf, (float *)y);
    q->sm.dev_valid = 0;
}

/* ------------------------------------------------------------------ the device form */
/* one sample of zero input through the nsec sections c (b0 b1 b2 a1 a2 each) */
static void zero_input_step(unsigned int nsec, const double complex *c, double complex *s)
{
    double complex t = 0.0;
    for (unsigned int k = 0; k < nsec; k++) {
        const double complex *ck = c + 5 * k;
        const double complex v0 = t - ck[3] * s[2 * k] - ck[4] * s[2 * k + 1];
        t = ck[0] * v0 + ck[1] * s[2 * k] + ck[2] * s[2 * k + 1];
        s[2 * k + 1] = s[2 * k];
        s[2 * k] = v0;
    }
}

static void mat_square(unsigned int P, const double complex *A, double complex *B)
{
    for (unsigned int r = 0; r < P; r++)
        for (unsigned int c = 0; c < P; c++) {
            double complex acc = 0.0;
            for (unsigned int k = 0; k < P; k++) acc += A[r * P + k] * A[k * P + c];
            B[r * P + c] = acc;
        }
}

/* Both roots of z^2 + a1 z + a2 inside or on the unit circle.  Real
 * coefficients: the stability triangle |a2| <= 1, |a1| <= 1 + a2, which is
 * that condition in closed form and exact on the boundary (an integrator's
 * pole at 1 qualifies).  Complex coefficients: the roots themselves, with
 * 1e-12 for the rounding of the square root. */
static int poles_inside(double complex a1, double complex a2, int real_coef)
{
    if (real_coef) return fabs(creal(a2)) <= 1.0 && fabs(creal(a1)) <= 1.0 + creal(a2);
    const double complex d = csqrt(a1 * a1 - 4.0 * a2);
    return cabs((-a1 + d) / 2.0) <= 1.0 + 1e-12 && cabs((-a1 - d) / 2.0) <= 1.0 + 1e-12;
}

/* decide eligibility; if eligible, build the coefficient table and the
 * ladder G^(2^k) (G = the state's map over LQK_IIRFILT_RUN samples of zero
 * input) in float64 and load them, rounded to float32 */
static void device_form(lq_iir *q)
{
    const int cw = q->cw;
    q->dev_ok = 0;
    q->nsec = q->sos ? q->nsos : 1;
    if (q->sos ? q->nsos > LQK_IIRFILT_MAXSEC : q->n > 3) return;
    double complex c[5 * LQK_IIRFILT_MAXSEC];
    for (unsigned int k = 0; k < q->nsec; k++)
        for (int i = 0; i < 5; i++) {   /* b0 b1 b2 a1 a2 */
            const unsigned int j = i < 3 ? (unsigned int)i : (unsigned int)i - 2;
            const float *src = i < 3 ? (q->sos ? q->sb + 3 * cw * k : q->b) : (q->sos ? q->sa + 3 * cw * k : q->a);
            const int have = q->sos || j < (i < 3 ? q->nb : q->na);
            const double re = have ? src[cw * j] : 0.0, im = (have && cw == 2) ? src[cw * j + 1] : 0.0;
            if (!isfinite(re) || !isfinite(im)) return;
            c[5 * k + i] = re + im * I;
        }
    for (unsigned int k = 0; k < q->nsec; k++)
        if (!poles_inside(c[5 * k + 3], c[5 * k + 4], cw == 1)) return;
    q->dev_ok = 1;

    const unsigned int P = 2 * q->nsec, PM = 2 * lqk_iirfilt_maxsec(q->nsec);
    double complex A[4 * LQK_IIRFILT_MAXSEC * LQK_IIRFILT_MAXSEC], B[4 * LQK_IIRFILT_MAXSEC * LQK_IIRFILT_MAXSEC];
    for (unsigned int j = 0; j < P; j++) {   /* column j: one step from the unit state e_j */
        double complex s[2 * LQK_IIRFILT_MAXSEC] = {0};
        s[j] = 1.0;
        zero_input_step(q->nsec, c, s);
        for (unsigned int r = 0; r < P; r++) A[r * P + j] = s[r];
    }
    for (unsigned int r = 1; r < LQK_IIRFILT_RUN; r *= 2) {   /* A^RUN, RUN a power of two */
        mat_square(P, A, B);
        memcpy(A, B, sizeof(A));
    }
    float *coef = (float *)lq_xmalloc(5 * q->nsec * cw * sizeof(float));
    for (unsigned int i = 0; i < 5 * q->nsec; i++) {
        coef[cw * i] = (float)creal(c[i]);
        if (cw == 2) coef[cw * i + 1] = (float)cimag(c[i]);
    }
    const size_t lsz = (size_t)LQK_IIRFILT_LEVELS * PM * PM * cw;
    float *lad = (float *)lq_xmalloc(lsz * sizeof(float));
    memset(lad, 0, lsz * sizeof(float));
    for (unsigned int l = 0; l < LQK_IIRFILT_LEVELS; l++) {
        for (unsigned int r = 0; r < P; r++)
            for (unsigned int cc = 0; cc < P; cc++) {
                float *d = lad + (((size_t)l * PM + r) * PM + cc) * cw;
                d[0] = (float)creal(A[r * P + cc]);
                if (cw == 2) d[1] = (float)cimag(A[r * P + cc]);
            }
        mat_square(P, A, B);
        memcpy(A, B, sizeof(A));
    }
    q->d_coef = lqrt_malloc(5 * q->nsec * cw * sizeof(float));
    q->d_lad = lqrt_malloc(lsz * sizeof(float));
    lqrt_h2d(q->d_coef, coef, 5 * q->nsec * cw * sizeof(float), q->ctx.stream);
    lqrt_h2d(q->d_lad, lad, lsz * sizeof(float), q->ctx.stream);
    lqrt_sync(q->ctx.stream);
    free(coef);
    free(lad);
}

static lq_iir *iir_new(int kind, const char *who)
{
    lqrt_require_device(who);
    lq_iir *q = (lq_iir *)lq_xmalloc(sizeof(*q));
    memset(q, 0, sizeof(*q));
    q->kind = kind;
    q->cw = kind == LQ_CCCF ? 2 : 1;
    q->sw = kind == LQ_RRRF ? 1 : 2;
    lq_ctx_init(&q->ctx);
    return q;
}

/* after the coefficients are in place: state, device form */
static void iir_finish(lq_iir *q)
{
    const size_t ns = q->sos ? 2 * (size_t)q->nsos : (q->n > 2 ? q->n : 2);
    lq_mirror_init(&q->sm, ns, q->sw * sizeof(float), 0);
    device_form(q);
    if (q->dev_ok) q->d_state = lqrt_malloc((ns > 2 * q->nsec ? ns : 2 * q->nsec) * q->sw * sizeof(float));   /* zeroed */
}

/* x / a0 in the coefficient type */
static void kdiv(int cw, const float *x, const float *a0, float *o)
{
    if (cw == 1) {
        o[0] = x[0] / a0[0];
    } else {
        /* the complex quotient written out (Smith's form, in float32, as the
         * C runtime the reference is built with forms it), so that the stored
         * coefficients do not depend on which runtime this library links */
        const float a = x[0], b = x[1], c = a0[0], d = a0[1];
        if (fabsf(c) < fabsf(d)) {
            const float ratio = c / d, denom = c * ratio + d;
            o[0] = (a * ratio + b) / denom;
            o[1] = (b * ratio - a) / denom;
        } else {
            const float ratio = d / c, denom = d * ratio + c;
            o[0] = (b * ratio + a) / denom;
            o[1] = (b - a * ratio) / denom;
        }
    }
}

static lq_iir *iir_create(int kind, const void *_b, unsigned int _nb, const void *_a, unsigned int _na)
{
    if (_nb == 0) LQ_FAIL("error: iirfilt_%s_create(), numerator length cannot be zero\n", kind_name[kind]);
    if (_na == 0) LQ_FAIL("error: iirfilt_%s_create(), denominator length cannot be zero\n", kind_name[kind]);
    lq_iir *q = iir_new(kind, "iirfilt_create");
    const int cw = q->cw;
    q->nb = _nb;
    q->na = _na;
    q->n = _na > _nb ? _na : _nb;
    q->b = (float *)lq_xmalloc((size_t)_nb * cw * sizeof(float));
    q->a = (float *)lq_xmalloc((size_t)_na * cw * sizeof(float));
    const float *a0 = (const float *)_a;
    for (unsigned int i = 0; i < _nb; i++) kdiv(cw, (const float *)_b + cw * i, a0, q->b + cw * i);
    for (unsigned int i = 0; i < _na; i++) kdiv(cw, (const float *)_a + cw * i, a0, q->a + cw * i);
    iir_finish(q);
    return q;
}

static lq_iir *iir_create_sos(int kind, const void *_B, const void *_A, unsigned int _nsos)
{
    if (_nsos == 0)
        LQ_FAIL("error: iirfilt_%s_create_sos(), filter must have at least one 2nd-order section\n", kind_name[kind]);
    lq_iir *q = iir_new(kind, "iirfilt_create_sos");
    const int cw = q->cw;
    const size_t nc = 3 * (size_t)_nsos * cw;
    q->sos = 1;
    q->nsos = _nsos;
    q->n = 2 * _nsos;
    q->b = (float *)lq_xmalloc(nc * sizeof(float));
    q->a = (float *)lq_xmalloc(nc * sizeof(float));
    q->sb = (float *)lq_xmalloc(nc * sizeof(float));
    q->sa = (float *)lq_xmalloc(nc * sizeof(float));
    memcpy(q->b, _B, nc * sizeof(float));
    memcpy(q->a, _A, nc * sizeof(float));
    for (unsigned int k = 0; k < _nsos; k++) {   /* iirfiltsos.c:61-77 */
        const float *a0 = q->a + 3 * cw * k;
        for (int i = 0; i < 3; i++) {
            kdiv(cw, q->b + (3 * k + i) * cw, a0, q->sb + (3 * k + i) * cw);
            kdiv(cw, q->a + (3 * k + i) * cw, a0, q->sa + (3 * k + i) * cw);
        }
    }
    iir_finish(q);
    return q;
}

/* real design coefficients as the kind's coefficient type */
static lq_iir *iir_from_real(int kind, int sos, const float *b, unsigned int nb, const float *a, unsigned int na)
{
    const int cw = kind == LQ_CCCF ? 2 : 1;
    float *cb = (float *)lq_xmalloc((size_t)(nb + na) * cw * sizeof(float)), *ca = cb + (size_t)nb * cw;
    for (unsigned int i = 0; i < nb; i++) {
        cb[cw * i] = b[i];
        if (cw == 2) cb[2 * i + 1] = 0.0f;
    }
    for (unsigned int i = 0; i < na; i++) {
        ca[cw * i] = a[i];
        if (cw == 2) ca[2 * i + 1] = 0.0f;
    }
    lq_iir *q = sos ? iir_create_sos(kind, cb, ca, nb / 3) : iir_create(kind, cb, nb, ca, na);
    free(cb);
    return q;
}

/* iirfilt.c:196-241: the design's length follows its order, doubled by the
 * band-pass and band-stop transforms */
static lq_iir *iir_create_prototype(int kind, liquid_iirdes_filtertype ftype, liquid_iirdes_bandtype btype,
                                    liquid_iirdes_format format, unsigned int order, float fc, float f0, float Ap,
                                    float As)
{
    unsigned int N = order;
    if (btype == LIQUID_IIRDES_BANDPASS || btype == LIQUID_IIRDES_BANDSTOP) N *= 2;
    const unsigned int r = N % 2, L = (N - r) / 2;
    const unsigned int h_len = format == LIQUID_IIRDES_SOS ? 3 * (L + r) : N + 1;
    float *B = (float *)lq_xmalloc(2 * (size_t)h_len * sizeof(float)), *A = B + h_len;
    liquid_iirdes(ftype, btype, format, order, fc, f0, Ap, As, B, A);
    lq_iir *q = iir_from_real(kind, format == LIQUID_IIRDES_SOS, B, h_len, A, h_len);
    free(B);
    return q;
}

/* [Pintelon:1990] R. Pintelon and J. Schoukens, "Real-time integration and
 * differentiation of analog signals by means of digital filtering," IEEE
 * Trans. Instrum. Meas. 39 (6), 1990: the 8th-order designs of Tables II
 * (integrator) and IV (differentiator) as magnitude and angle [degrees] of
 * the digital zeros and poles, and the gain.  iirfilt.c:264-359 forms the
 * integrator's zeros in double precision and everything else in float32. */
typedef struct {
    double zmag[8], zdeg[8], pmag[8], pdeg[8], gain;
    int zeros_double;
} lq_pintelon;
static const lq_pintelon pintelon_int = {
    {1.175839, 3.371020, 3.371020, 4.549710, 4.549710, 5.223966, 5.223966, 5.443743},
    {180.0, -125.1125, 125.1125, -80.96404, 80.96404, -40.09347, 40.09347, 0.0},
    {0.5805235, 0.2332021, 0.2332021, 0.1814755, 0.1814755, 0.1641457, 0.1641457, 1.0},
    {180.0, -114.0968, 114.0968, -66.33969, 66.33969, -21.89539, 21.89539, 0.0},
    -1.89213380759321e-05, 1};
static const lq_pintelon pintelon_diff = {
    {1.702575, 5.877385, 5.877385, 4.197421, 4.197421, 5.350284, 5.350284, 1.0},
    {180.0, -221.4063, 221.4063, -144.5972, 144.5972, -66.88802, 66.88802, 0.0},
    {0.8476936, 0.2990781, 0.2990781, 0.2232427, 0.2232427, 0.1958670, 0.1958670, 0.1886088},
    {180.0, -125.5188, 125.5188, -81.52326, 81.52326, -40.51510, 40.51510, 0.0},
    2.09049284907492e-05, 0};

/* mag e^{j deg}: the real roots (0 and 180 degrees) are +-mag exactly; the
 * others take the angle to float32 radians through double, as the reference's
 * constant expressions do */
static float complex polar_root(double mag, double deg, int in_double)
{
    if (deg == 0.0) return (float)mag;
    if (deg == 180.0) return in_double ? (float)(mag * -1.0) : (float)mag * -1.0f;
    const float complex e = cexpf(_Complex_I * M_PI / 180.0f * (float)deg);
    if (in_double) return (float complex)(mag * (double complex)e);
    return (float)mag * e;
}

static lq_iir *iir_create_pintelon(int kind, const lq_pintelon *d)
{
    float complex z[8], p[8];
    for (int i = 0; i < 8; i++) {
        z[i] = polar_root(d->zmag[i], d->zdeg[i], d->zeros_double);
        p[i] = polar_root(d->pmag[i], d->pdeg[i], 0);
    }
    float B[12], A[12];
    iirdes_dzpk2sosf(z, p, 8, (float)d->gain, B, A);
    return iir_from_real(kind, 1, B, 12, A, 12);
}

static lq_iir *iir_create_dc_blocker(int kind, float alpha)
{
    const float b[2] = {1.0f, -1.0f}, a[2] = {1.0f, -1.0f + alpha};
    return iir_from_real(kind, 0, b, 2, a, 2);
}

static lq_iir *iir_create_pll(int kind, float w, float zeta, float K)
{
    if (w <= 0.0f || w >= 1.0f) LQ_FAIL("error: iirfilt_%s_create_pll(), bandwidth must be in (0,1)\n", kind_name[kind]);
    if (zeta <= 0.0f || zeta >= 1.0f)
        LQ_FAIL("error: iirfilt_%s_create_pll(), damping factor must be in (0,1)\n", kind_name[kind]);
    if (K <= 0.0f) LQ_FAIL("error: iirfilt_%s_create_pll(), loop gain must be greater than zero\n", kind_name[kind]);
    float b[3], a[3];
    iirdes_pll_active_lag(w, zeta, K, b, a);
    return iir_from_real(kind, 1, b, 3, a, 3);
}

static void iir_destroy(lq_iir *q)
{
    lqrt_sync(q->ctx.stream);
    if (q->d_coef) lqrt_free(q->d_coef);
    if (q->d_lad) lqrt_free(q->d_lad);
    if (q->d_state) lqrt_free(q->d_state);
    lq_devbuf_free(&q->xbuf);
    lq_devbuf_free(&q->ybuf);
    lq_devbuf_free(&q->work);
    lq_ctx_free(&q->ctx);
    lq_mirror_free(&q->sm);
    free(q->b);
    free(q->a);
    free(q->sb);
    free(q->sa);
    free(q);
}

static void print_coef(const lq_iir *q, const float *c)
{
    if (q->cw == 1)
        printf("%12.8f", c[0]);
    else
        printf("%12.8f+j*%12.8f", c[0], c[1]);
}

static void iir_print(const lq_iir *q)   /* iirfilt.c:437-464, iirfiltsos.c:86-99 */
{
    printf("iir filter [%s]:\n", q->sos ? "sos" : "normal");
    if (q->sos) {
        for (unsigned int k = 0; k < q->nsos; k++) {
            printf("iir filter | sos:\n");
            for (int ab = 0; ab < 2; ab++) {
                const float *c = (ab ? q->sa : q->sb) + 3 * q->cw * k;
                printf(ab ? "  a : " : "  b : ");
                print_coef(q, c);
                printf(",");
                print_coef(q, c + q->cw);
                printf(",");
                print_coef(q, c + 2 * q->cw);
                printf("\n");
            }
        }
        return;
    }
    printf("  b :");
    for (unsigned int i = 0; i < q->nb; i++) print_coef(q, q->b + q->cw * i);
    printf("\n  a :");
    for (unsigned int i = 0; i < q->na; i++) print_coef(q, q->a + q->cw * i);
    printf("\n");
}

static void iir_reset(lq_iir *q)
{
    if (q->d_state) {
        lqrt_memset(q->d_state, q->sm.n * q->sm.esz, q->ctx.stream);
        lqrt_sync(q->ctx.stream);
    }
    lq_mirror_zero(&q->sm);
}

static void iir_run_dev(lq_iir *q, const void *dx, unsigned long long n, void *dy)
{
    if (n == 0) return;
    if (!q->dev_ok) {   /* device pointers, host loop: copy, run, copy back */
        const size_t bytes = (size_t)n * q->sw * sizeof(float);
        void *h = lq_xmalloc(bytes);
        lqrt_d2h(h, dx, bytes, q->ctx.stream);
        lqrt_sync(q->ctx.stream);
        host_loop(q, h, n, h);
        lqrt_h2d(dy, h, bytes, q->ctx.stream);
        lqrt_sync(q->ctx.stream);
        free(h);
        return;
    }
    lq_mirror_need_dev(&q->sm, q->d_state, q->ctx.stream);
    q->sm.host_valid = 0;
    const size_t wb = lqk_iirfilt_work_bytes(q->kind, q->nsec, n);
    void *work = wb ? lq_devbuf_get(&q->work, wb) : NULL;
    lqk_iirfilt(q->kind, q->nsec, q->d_coef, q->d_lad, q->d_state, dx, n, dy, work, q->ctx.stream);
}

static void iir_run(lq_iir *q, const void *x, unsigned long long n, void *y)
{
    if (n == 0) return;
    if (!q->dev_ok) {
        host_loop(q, x, n, y);
        return;
    }
    const size_t bytes = (size_t)n * q->sw * sizeof(float);
    const void *dx = lq_call_in(&q->ctx, &q->xbuf, x, bytes);
    void *dy = lq_devbuf_get(&q->ybuf, bytes);
    iir_run_dev(q, dx, n, dy);
    lq_call_out(&q->ctx, y, dy, bytes);
}

static void iir_execute(lq_iir *q, const void *x, void *y)
{
    if (lq_small_host() || !q->dev_ok)
        host_loop(q, x, 1, y);
    else
        iir_run(q, x, 1, y);
}

/* ------------------------------------------------------------------ as a rate changer */
static int rate_dev_ok(const lq_iir *q, unsigned int M) { return q->dev_ok && M <= LQK_IIRFILT_TILE; }

/* n calls' worth: mode 1 n M samples in, n out; mode 2 n in, n M out */
static void iir_rate_dev(lq_iir *q, int mode, unsigned int M, const void *dx, unsigned long long n, void *dy)
{
    if (n == 0) return;
    const unsigned long long nf = n * M, nin = mode == 1 ? nf : n, nout = mode == 1 ? n : nf;
    if (!rate_dev_ok(q, M)) {   /* device pointers, host loop: copy, run, copy back */
        const size_t esz = q->sw * sizeof(float);
        void *hx = lq_xmalloc((size_t)nin * esz), *hy = lq_xmalloc((size_t)nout * esz);
        lqrt_d2h(hx, dx, (size_t)nin * esz, q->ctx.stream);
        lqrt_sync(q->ctx.stream);
        host_rate(q, mode, M, hx, nf, hy);
        lqrt_h2d(dy, hy, (size_t)nout * esz, q->ctx.stream);
        lqrt_sync(q->ctx.stream);
        free(hx);
        free(hy);
        return;
    }
    lq_mirror_need_dev(&q->sm, q->d_state, q->ctx.stream);
    q->sm.host_valid = 0;
    const size_t wb = lqk_iirfilt_work_bytes(q->kind, q->nsec, nf);
    void *work = wb ? lq_devbuf_get(&q->work, wb) : NULL;
    if (mode == 1)
        lqk_iirfilt_decim(q->kind, q->nsec, q->d_coef, q->d_lad, q->d_state, dx, nf, M, dy, work, q->ctx.stream);
    else
        lqk_iirfilt_interp(q->kind, q->nsec, q->d_coef, q->d_lad, q->d_state, dx, n, M, dy, work, q->ctx.stream);
}

static void iir_rate(lq_iir *q, int mode, unsigned int M, const void *x, unsigned long long n, void *y, int small)
{
    if (n == 0) return;
    const unsigned long long nf = n * M;
    if (!rate_dev_ok(q, M) || (small && lq_small_host())) {
        host_rate(q, mode, M, x, nf, y);
        return;
    }
    const size_t esz = q->sw * sizeof(float);
    const size_t bin = (size_t)(mode == 1 ? nf : n) * esz, bout = (size_t)(mode == 1 ? n : nf) * esz;
    const void *dx = lq_call_in(&q->ctx, &q->xbuf, x, bin);   /* staged: y may be x */
    void *dy = lq_devbuf_get(&q->ybuf, bout);
    iir_rate_dev(q, mode, M, dx, n, dy);
    lq_call_out(&q->ctx, y, dy, bout);
}

static void iir_freqresponse(const lq_iir *q, float fc, liquid_float_complex *H)   /* iirfilt.c:587-628 */
{
    const int cw = q->cw;
#define LQ_COEF(p, i) ((p)[cw * (i)] + (cw == 2 ? (p)[cw * (i) + 1] : 0.0f) * _Complex_I)
    float complex h;
    if (!q->sos) {
        float complex Ha = 0.0f, Hb = 0.0f;
        for (unsigned int i = 0; i < q->nb; i++) Hb += LQ_COEF(q->b, i) * cexpf(_Complex_I * 2 * M_PI * fc * i);
        for (unsigned int i = 0; i < q->na; i++) Ha += LQ_COEF(q->a, i) * cexpf(_Complex_I * 2 * M_PI * fc * i);
        h = Hb / Ha;
    } else {
        h = 1.0f;
        for (unsigned int k = 0; k < q->nsos; k++) {
            float complex Ha = 0.0f, Hb = 0.0f;
            for (unsigned int i = 0; i < 3; i++) {
                Hb += LQ_COEF(q->b, 3 * k + i) * cexpf(_Complex_I * 2 * M_PI * fc * i);
                Ha += LQ_COEF(q->a, 3 * k + i) * cexpf(_Complex_I * 2 * M_PI * fc * i);
            }
            h *= Hb / Ha;
        }
    }
#undef LQ_COEF
    memcpy(H, &h, sizeof(h));
}

static float iir_groupdelay(const lq_iir *q, float fc)   /* iirfilt.c:633-655, iirfiltsos.c:189-201 */
{
    const int cw = q->cw;
    if (!q->sos) {
        float *b = (float *)lq_xmalloc(q->nb * sizeof(float)), *a = (float *)lq_xmalloc(q->na * sizeof(float));
        for (unsigned int i = 0; i < q->nb; i++) b[i] = q->b[cw * i];
        for (unsigned int i = 0; i < q->na; i++) a[i] = q->a[cw * i];
        const float g = iir_group_delay(b, q->nb, a, q->na, fc);
        free(b);
        free(a);
        return g;
    }
    float g = 0;
    for (unsigned int k = 0; k < q->nsos; k++) {
        float b[3], a[3];
        for (int i = 0; i < 3; i++) {
            b[i] = q->sb[(3 * k + i) * cw];
            a[i] = q->sa[(3 * k + i) * cw];
        }
        g += (float)(iir_group_delay(b, 3, a, 3, fc) + 2.0) - 2;
    }
    return g;
}

/* ------------------------------------------------------------------ design helpers */
/* iirdes.pll.c:47-76: active lag, F(s) = (1 + t2 s) / (1 + t1 s) */
void iirdes_pll_active_lag(float _w, float _zeta, float _K, float *_b, float *_a)
{
    if (_w <= 0.0f) LQ_FAIL("error: iirdes_pll_active_lag(), bandwidth must be greater than 0\n");
    if (_zeta <= 0.0f) LQ_FAIL("error: iirdes_pll_active_lag(), damping factor must be greater than 0\n");
    if (_K <= 0.0f) LQ_FAIL("error: iirdes_pll_active_lag(), gain must be greater than 0\n");
    const float t1 = _K / (_w * _w), t2 = 2 * _zeta / _w - 1 / _K;
    _b[0] = (float)(2 * _K * (1.0 + t2 / 2.0f));   /* the sums and products with 1. and 2. are double */
    _b[1] = (float)(2 * _K * 2.0);
    _b[2] = (float)(2 * _K * (1.0 - t2 / 2.0f));
    _a[0] = 1 + t1 / 2.0f;
    _a[1] = -t1;
    _a[2] = -1 + t1 / 2.0f;
}

/* iirdes.pll.c:88-118: active PI, F(s) = (1 + t2 s) / (t1 s) (the messages name active_lag there too) */
void iirdes_pll_active_PI(float _w, float _zeta, float _K, float *_b, float *_a)
{
    if (_w <= 0.0f) LQ_FAIL("error: iirdes_pll_active_lag(), bandwidth must be greater than 0\n");
    if (_zeta <= 0.0f) LQ_FAIL("error: iirdes_pll_active_lag(), damping factor must be greater than 0\n");
    if (_K <= 0.0f) LQ_FAIL("error: iirdes_pll_active_lag(), gain must be greater than 0\n");
    const float t1 = _K / (_w * _w), t2 = 2 * _zeta / _w;
    _b[0] = (float)(2 * _K * (1.0 + t2 / 2.0f));
    _b[1] = (float)(2 * _K * 2.0);
    _b[2] = (float)(2 * _K * (1.0 - t2 / 2.0f));
    _a[0] = t1 / 2.0f;
    _a[1] = -t1;
    _a[2] = t1 / 2.0f;
}

/* group_delay.c:64-117 */
float iir_group_delay(float *_b, unsigned int _nb, float *_a, unsigned int _na, float _fc)
{
    if (_nb == 0) LQ_FAIL("error: iir_group_delay(), numerator length must be greater than zero\n");
    if (_na == 0) LQ_FAIL("error: iir_group_delay(), denominator length must be greater than zero\n");
    if (_fc < -0.5 || _fc > 0.5) LQ_FAIL("error: iir_group_delay(), _fc must be in [-0.5,0.5]\n");
    const unsigned int nc = _na + _nb - 1;   /* c = conv(b, reversed a) */
    float *c = (float *)lq_xmalloc(nc * sizeof(float));
    for (unsigned int i = 0; i < nc; i++) c[i] = 0.0f;
    for (unsigned int i = 0; i < _na; i++)
        for (unsigned int j = 0; j < _nb; j++) c[i + j] += _a[_na - i - 1] * _b[j];
    float complex t0 = 0.0f, t1 = 0.0f;
    for (unsigned int i = 0; i < nc; i++) {
        const float complex c0 = c[i] * cexpf(_Complex_I * 2 * M_PI * _fc * i);
        t0 += c0 * i;
        t1 += c0;
    }
    free(c);
    if (cabsf(t1) < 1e-5f) return 0.0f;
    return crealf(t0 / t1) - (_na - 1);
}

/* the engine as iirdecim.c sees it (lq_host.h) */
lq_iir *lq_iir_create(int kind, const void *b, unsigned int nb, const void *a, unsigned int na)
{
    return iir_create(kind, b, nb, a, na);
}
lq_iir *lq_iir_create_prototype(int kind, liquid_iirdes_filtertype ftype, liquid_iirdes_bandtype btype,
                                liquid_iirdes_format format, unsigned int order, float fc, float f0, float Ap,
                                float As)
{
    return iir_create_prototype(kind, ftype, btype, format, order, fc, f0, Ap, As);
}
void lq_iir_destroy(lq_iir *q) { iir_destroy(q); }
void lq_iir_print(lq_iir *q) { iir_print(q); }
void lq_iir_reset(lq_iir *q) { iir_reset(q); }
float lq_iir_groupdelay(lq_iir *q, float fc) { return iir_groupdelay(q, fc); }
int lq_iir_rate_eligible(lq_iir *q, unsigned int M) { return rate_dev_ok(q, M); }
lq_ctx *lq_iir_ctx(lq_iir *q) { return &q->ctx; }
void lq_iir_run_rate(lq_iir *q, int mode, unsigned int M, const void *x, unsigned long long n, void *y, int small)
{
    iir_rate(q, mode, M, x, n, y, small);
}
void lq_iir_run_rate_dev(lq_iir *q, int mode, unsigned int M, const void *dx, unsigned long long n, void *dy)
{
    iir_rate_dev(q, mode, M, dx, n, dy);
}

/* block geometry of the device path (tests cut streams at these) and the
 * launch structure a call of n full-rate samples takes (lqk_iirfilt_route) */
unsigned int liquid_mi355x_iirfilt_run(void) { return LQK_IIRFILT_RUN; }
unsigned int liquid_mi355x_iirfilt_tile(void) { return LQK_IIRFILT_TILE; }
unsigned int liquid_mi355x_iirfilt_scan(void) { return LQK_IIRFILT_SCAN; }
int liquid_mi355x_iirfilt_route(unsigned long long _n) { return lqk_iirfilt_route(_n); }

/* ------------------------------------------------------------------ typed front ends */
#define LQ_IIRFILT_DEFINE(IIRFILT, KIND, TO, TC, TI)                                                          \
    struct IIRFILT##_s {                                                                                      \
        struct lq_iir_s e;                                                                                    \
    };                                                                                                        \
    IIRFILT IIRFILT##_create(TC *_b, unsigned int _nb, TC *_a, unsigned int _na)                              \
    {                                                                                                         \
        return (IIRFILT)iir_create(KIND, _b, _nb, _a, _na);                                                   \
    }                                                                                                         \
    IIRFILT IIRFILT##_create_sos(TC *_B, TC *_A, unsigned int _nsos)                                          \
    {                                                                                                         \
        return (IIRFILT)iir_create_sos(KIND, _B, _A, _nsos);                                                  \
    }                                                                                                         \
    IIRFILT IIRFILT##_create_integrator(void) { return (IIRFILT)iir_create_pintelon(KIND, &pintelon_int); }   \
    IIRFILT IIRFILT##_create_differentiator(void) { return (IIRFILT)iir_create_pintelon(KIND, &pintelon_diff); } \
    IIRFILT IIRFILT##_create_dc_blocker(float _alpha) { return (IIRFILT)iir_create_dc_blocker(KIND, _alpha); } \
    IIRFILT IIRFILT##_create_pll(float _w, float _zeta, float _K)                                             \
    {                                                                                                         \
        return (IIRFILT)iir_create_pll(KIND, _w, _zeta, _K);                                                  \
    }                                                                                                         \
    void IIRFILT##_destroy(IIRFILT _q) { iir_destroy(&_q->e); }                                               \
    void IIRFILT##_print(IIRFILT _q) { iir_print(&_q->e); }                                                   \
    void IIRFILT##_reset(IIRFILT _q) { iir_reset(&_q->e); }                                                   \
    void IIRFILT##_execute(IIRFILT _q, TI _x, TO *_y) { iir_execute(&_q->e, &_x, _y); }                       \
    void IIRFILT##_execute_block(IIRFILT _q, TI *_x, unsigned int _n, TO *_y) { iir_run(&_q->e, _x, _n, _y); } \
    void IIRFILT##_execute_block_dev(IIRFILT _q, const TI *_dx, unsigned long long _n, TO *_dy)               \
    {                                                                                                         \
        iir_run_dev(&_q->e, _dx, _n, _dy);                                                                    \
    }                                                                                                         \
    unsigned int IIRFILT##_get_length(IIRFILT _q) { return _q->e.n; }                                         \
    void IIRFILT##_freqresponse(IIRFILT _q, float _fc, liquid_float_complex *_H)                              \
    {                                                                                                         \
        iir_freqresponse(&_q->e, _fc, _H);                                                                    \
    }                                                                                                         \
    float IIRFILT##_groupdelay(IIRFILT _q, float _fc) { return iir_groupdelay(&_q->e, _fc); }                 \
    int IIRFILT##_device_eligible(IIRFILT _q) { return _q->e.dev_ok; }                                        \
    void IIRFILT##_set_stream(IIRFILT _q, void *_s) { lq_ctx_set_stream(&_q->e.ctx, _s); }                    \
    void IIRFILT##_synchronize(IIRFILT _q) { lqrt_sync(_q->e.ctx.stream); }

LQ_IIRFILT_DEFINE(iirfilt_rrrf, LQ_RRRF, float, float, float)
LQ_IIRFILT_DEFINE(iirfilt_crcf, LQ_CRCF, liquid_float_complex, float, liquid_float_complex)
LQ_IIRFILT_DEFINE(iirfilt_cccf, LQ_CCCF, liquid_float_complex, liquid_float_complex, liquid_float_complex)
