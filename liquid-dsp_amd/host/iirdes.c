/*
 * iirdes.c -- recursive filter design: the analog prototypes (Butterworth,
 * Chebyshev I and II, elliptic, Bessel), the bilinear transform, the band
 * transforms, the zero/pole/gain conversions and liquid_iirdes itself.
 *
 * include/liquid.h:1688-1880, src/filter/src/iirdes.c, butter.c, cheby1.c,
 * cheby2.c, ellip.c, bessel.c.  Host code, create time only; nothing here
 * touches the GPU.  The arithmetic is the reference's statement order in
 * float32, with its promotions to double where a double constant (M_PI, 1.0,
 * 2.0) takes part, so that a design agrees with the reference's to the last
 * few bits of its coefficients ("iirdes, iirdecim, iirinterp").
 * Complex products and quotients are the C runtime's.
 *
 * Not the reference's method: iirdes_isstable decides by the Schur-Cohn
 * recursion in float64 instead of finding the roots by Bairstow's iteration.
 */
#include <complex.h>
#include <math.h>

#include "lq_host.h"

typedef float complex cf;
typedef double complex cd;

/* ------------------------------------------------------------------ pairing (iirdes.c:60-184) */
/* the n values of z with the conjugate pairs first (negative imaginary part
 * first, pairs by increasing real part, made exact conjugates) and the real
 * values after them in increasing order */
void liquid_cplxpair(liquid_float_complex *_z, unsigned int _n, float _tol, liquid_float_complex *_p)
{
    if (_tol < 0) LQ_FAIL("error: liquid_cplxpair(), tolerance must be positive\n");
    const cf *z = (const cf *)_z;
    cf *p = (cf *)_p;
    const unsigned int n = _n;
    const float tol = _tol;
    unsigned char *used = (unsigned char *)lq_xmalloc(n ? n : 1);
    memset(used, 0, n ? n : 1);
    unsigned int k = 0, npairs = 0;
    for (unsigned int i = 0; i < n; i++) {
        if (used[i] || fabsf(cimagf(z[i])) < tol) continue;
        for (unsigned int j = 0; j < n; j++) {
            if (j == i || used[j] || fabsf(cimagf(z[j])) < tol) continue;
            if (fabsf(cimagf(z[i]) + cimagf(z[j])) < tol && fabsf(crealf(z[i]) - crealf(z[j])) < tol) {
                p[k++] = z[i];
                p[k++] = z[j];
                used[i] = used[j] = 1;
                npairs++;
                break;
            }
        }
    }
    for (unsigned int i = 0; i < n; i++) {
        if (used[i]) continue;
        if (cimagf(z[i]) > tol) {
            fprintf(stderr, "warning, liquid_cplxpair(), complex numbers cannot be paired\n");
        } else {
            p[k++] = z[i];
            used[i] = 1;
        }
    }
    free(used);
    liquid_cplxpair_cleanup(_p, _n, npairs);
}

void liquid_cplxpair_cleanup(liquid_float_complex *_p, unsigned int _n, unsigned int _num_pairs)
{
    cf *p = (cf *)_p;
    const unsigned int n = _n, npairs = _num_pairs;
    for (unsigned int i = 0; i < npairs; i++) {
        if (!(cimagf(p[2 * i]) < 0)) p[2 * i] = conjf(p[2 * i]);
        p[2 * i + 1] = conjf(p[2 * i]);
    }
    for (unsigned int i = 0; i < npairs; i++)          /* bubble sort, pairs by real part */
        for (unsigned int j = npairs - 1; j > i; j--)
            if (crealf(p[2 * (j - 1)]) > crealf(p[2 * j]))
                for (int c = 0; c < 2; c++) {
                    const cf t = p[2 * (j - 1) + c];
                    p[2 * (j - 1) + c] = p[2 * j + c];
                    p[2 * j + c] = t;
                }
    for (unsigned int i = 2 * npairs; i < n; i++)      /* the real values */
        for (unsigned int j = n - 1; j > i; j--)
            if (crealf(p[j - 1]) > crealf(p[j])) {
                const cf t = p[j - 1];
                p[j - 1] = p[j];
                p[j] = t;
            }
}

/* iirdes.c:320-406: zeros, poles and gain to L + r second-order sections
 * (n = 2L + r), the gain spread evenly over the numerators */
void iirdes_dzpk2sosf(liquid_float_complex *_zd, liquid_float_complex *_pd, unsigned int _n,
                      liquid_float_complex _kd, float *_B, float *_A)
{
    cf *zp = (cf *)lq_xmalloc((_n ? _n : 1) * sizeof(cf));
    cf *pp = (cf *)lq_xmalloc((_n ? _n : 1) * sizeof(cf));
    liquid_cplxpair(_zd, _n, 1e-6f, (liquid_float_complex *)zp);
    liquid_cplxpair(_pd, _n, 1e-6f, (liquid_float_complex *)pp);
    const unsigned int r = _n % 2, L = (_n - r) / 2;
    for (unsigned int i = 0; i < L; i++) {
        const cf p0 = -pp[2 * i], p1 = -pp[2 * i + 1], z0 = -zp[2 * i], z1 = -zp[2 * i + 1];
        _A[3 * i] = 1.0f;
        _A[3 * i + 1] = crealf(p0 + p1);
        _A[3 * i + 2] = crealf(p0 * p1);
        _B[3 * i] = 1.0f;
        _B[3 * i + 1] = crealf(z0 + z1);
        _B[3 * i + 2] = crealf(z0 * z1);
    }
    if (r) {
        _A[3 * L] = 1.0f;
        _A[3 * L + 1] = crealf(-pp[_n - 1]);
        _A[3 * L + 2] = 0.0f;
        _B[3 * L] = 1.0f;
        _B[3 * L + 1] = crealf(-zp[_n - 1]);
        _B[3 * L + 2] = 0.0f;
    }
    cf kd;
    memcpy(&kd, &_kd, sizeof(kd));
    const float k = powf(crealf(kd), 1.0f / (float)(L + r));
    for (unsigned int i = 0; i < 3 * (L + r); i++) _B[i] *= k;
    free(zp);
    free(pp);
}

/* ------------------------------------------------------------------ small helpers */
/* math.complex.c:34-45, 58-61, 70-84: the reference's own square root,
 * logarithm and arc cosine (not the C runtime's: the branch choices differ) */
static cf lq_csqrtf(cf z)
{
    const float r = cabsf(z), a = crealf(z);
    const float re = sqrtf(0.5f * (r + a)), im = sqrtf(0.5f * (r - a));
    return cimagf(z) > 0 ? re + _Complex_I * im : re - _Complex_I * im;
}

static cf lq_clogf(cf z) { return logf(cabsf(z)) + _Complex_I * cargf(z); }

static cf lq_cacosf(cf z)
{
    const int si = crealf(z) > 0, sq = cimagf(z) > 0;
    if (si == sq) return -_Complex_I * lq_clogf(z + lq_csqrtf(z * z - 1.0f));
    return -_Complex_I * lq_clogf(z - lq_csqrtf(z * z - 1.0f));
}

/* poly.expand.c:146-170: c[0..n] of prod (x - a[i]), lowest power first */
static void expand_roots(const cf *a, unsigned int n, cf *c)
{
    if (n == 0) {
        c[0] = 0.0f;
        return;
    }
    for (unsigned int i = 0; i <= n; i++) c[i] = i == 0 ? 1.0f : 0.0f;
    for (unsigned int i = 0; i < n; i++) {
        for (unsigned int j = i + 1; j > 0; j--) c[j] = -a[i] * c[j] + c[j - 1];
        c[0] *= -a[i];
    }
}

/* ------------------------------------------------------------------ analog prototypes */
/* butter.c: n poles on the unit circle's left half, no zeros, unit gain */
void butter_azpkf(unsigned int _n, liquid_float_complex *_za, liquid_float_complex *_pa, liquid_float_complex *_ka)
{
    cf *pa = (cf *)_pa;
    const unsigned int r = _n % 2, L = (_n - r) / 2;
    unsigned int k = 0;
    for (unsigned int i = 0; i < L; i++) {
        const float theta = (float)((float)(2 * (i + 1) + _n - 1) * M_PI / (float)(2 * _n));
        pa[k++] = cexpf(_Complex_I * theta);
        pa[k++] = cexpf(-_Complex_I * theta);
    }
    if (r) pa[k++] = -1.0f;
    *(cf *)_ka = 1.0f;
}

/* the ellipse of the Chebyshev poles for ripple parameter e: minor axis a, major axis b */
static void cheby_axes(unsigned int n, float e, float *a, float *b)
{
    const float t0 = (float)sqrt(1.0 + 1.0 / (e * e));
    const float tp = powf((float)(t0 + 1.0 / e), (float)(1.0 / (float)n));
    const float tm = powf((float)(t0 - 1.0 / e), (float)(1.0 / (float)n));
    *b = (float)(0.5 * (tp + tm));
    *a = (float)(0.5 * (tp - tm));
}

/* cheby1.c: poles on the ellipse, no zeros; the gain makes |H(0)| = 1 (odd n) or 1/sqrt(1 + ep^2) */
void cheby1_azpkf(unsigned int _n, float _ep, liquid_float_complex *_za, liquid_float_complex *_pa,
                  liquid_float_complex *_ka)
{
    cf *pa = (cf *)_pa, ka;
    float a, b;
    cheby_axes(_n, _ep, &a, &b);
    const unsigned int r = _n % 2, L = (_n - r) / 2;
    unsigned int k = 0;
    for (unsigned int i = 0; i < L; i++) {
        const float theta = (float)((float)(2 * (i + 1) + _n - 1) * M_PI / (float)(2 * _n));
        pa[k++] = a * cosf(theta) - _Complex_I * b * sinf(theta);
        pa[k++] = a * cosf(theta) + _Complex_I * b * sinf(theta);
    }
    if (r) pa[k++] = -a;
    ka = r ? 1.0f : 1.0f / sqrtf(1.0f + _ep * _ep);
    for (unsigned int i = 0; i < _n; i++) ka *= pa[i];
    *(cf *)_ka = ka;
}

/* cheby2.c: the reciprocals of those poles, 2L zeros on the imaginary axis */
void cheby2_azpkf(unsigned int _n, float _es, liquid_float_complex *_za, liquid_float_complex *_pa,
                  liquid_float_complex *_ka)
{
    cf *pa = (cf *)_pa, *za = (cf *)_za, ka;
    float a, b;
    cheby_axes(_n, _es, &a, &b);
    const unsigned int r = _n % 2, L = (_n - r) / 2;
    unsigned int k = 0;
    for (unsigned int i = 0; i < L; i++) {
        const float theta = (float)((float)(2 * (i + 1) + _n - 1) * M_PI / (float)(2 * _n));
        pa[k++] = 1.0f / (a * cosf(theta) - _Complex_I * b * sinf(theta));
        pa[k++] = 1.0f / (a * cosf(theta) + _Complex_I * b * sinf(theta));
    }
    if (r) pa[k++] = -1.0f / a;
    k = 0;
    for (unsigned int i = 0; i < L; i++) {
        const float theta = (float)(0.5f * M_PI * (2 * (i + 1) - 1) / (float)_n);
        za[k++] = -1.0f / (_Complex_I * cosf(theta));
        za[k++] = 1.0f / (_Complex_I * cosf(theta));
    }
    ka = 1.0f;
    for (unsigned int i = 0; i < _n; i++) ka *= pa[i];
    for (unsigned int i = 0; i < 2 * L; i++) ka /= za[i];
    *(cf *)_ka = ka;
}

/* ---- elliptic functions (ellip.c:49-257; [Orfanidis:2006] S. J. Orfanidis,
 * "Lecture Notes on Elliptic Filter Design") */
/* the Landen sequence k -> ((1 - k') / (1 + k')), k' = sqrt(1 - k^2), n times */
static void landenf(float _k, unsigned int _n, float *_v)
{
    float k = _k;
    for (unsigned int i = 0; i < _n; i++) {
        const float kp = sqrtf(1 - k * k);
        k = (1 - kp) / (1 + kp);
        _v[i] = k;
    }
}

/* one complete elliptic integral: the product over the Landen sequence, or the
 * logarithmic approximation where k is too near 1 for float32 */
static float ellipk_one(float k, float kc, int near_one, unsigned int n)
{
    if (near_one) {
        const float L = -logf(0.25f * kc);
        return L + 0.25f * (L - 1) * kc * kc;
    }
    float *v = (float *)lq_xmalloc((n ? n : 1) * sizeof(float));
    landenf(k, n, v);
    float K = (float)(M_PI * 0.5f);
    for (unsigned int i = 0; i < n; i++) K *= (1 + v[i]);
    free(v);
    return K;
}

/* K(k) and K(k'), n Landen steps */
static void ellipkf(float _k, unsigned int _n, float *_K, float *_Kp)
{
    const float kmin = 4e-4f, kmax = sqrtf(1 - kmin * kmin);
    const float kp = sqrtf(1 - _k * _k);
    *_K = ellipk_one(_k, kp, _k > kmax, _n);
    *_Kp = ellipk_one(kp, _k, _k < kmin, _n);
}

/* the modulus k with K'/K = N K1'/K1 (the degree equation), by the nome */
static float ellipdegf(float _N, float _k1, unsigned int _n)
{
    float K1, K1p;
    ellipkf(_k1, _n, &K1, &K1p);
    const float q1 = expf((float)(-M_PI * K1p / K1));
    const float q = powf(q1, 1.0f / _N);
    float b = 0.0f, a = 0.0f;
    for (unsigned int m = 0; m < _n; m++) b += powf(q, (float)(m * (m + 1)));
    for (unsigned int m = 1; m < _n; m++) a += powf(q, (float)(m * m));
    const float g = b / (1.0f + 2.0f * a);
    return 4.0f * sqrtf(q) * g * g;
}

/* w up the Landen sequence (descending transformation backwards) */
static cf landen_ascend(cf wn, float k, unsigned int n)
{
    float *v = (float *)lq_xmalloc((n ? n : 1) * sizeof(float));
    landenf(k, n, v);
    for (unsigned int i = n; i > 0; i--) wn = (1 + v[i - 1]) * wn / (1 + v[i - 1] * wn * wn);
    free(v);
    return wn;
}

static cf ellip_cd(cf u, float k, unsigned int n) { return landen_ascend(ccosf((cf)((cd)u * M_PI * 0.5f)), k, n); }
static cf ellip_sn(cf u, float k, unsigned int n) { return landen_ascend(csinf((cf)((cd)u * M_PI * 0.5f)), k, n); }

static cf ellip_acd(cf _w, float k, unsigned int n)
{
    float *v = (float *)lq_xmalloc((n ? n : 1) * sizeof(float));
    landenf(k, n, v);
    cf w = _w;
    for (unsigned int i = 0; i < n; i++) {
        const float v1 = i == 0 ? k : v[i - 1];
        w = (cf)((cd)(w / (1 + lq_csqrtf(1 - w * w * v1 * v1))) * 2.0 / (double)(1 + v[i]));
    }
    free(v);
    return (cf)((cd)lq_cacosf(w) * 2.0 / M_PI);
}

static cf ellip_asn(cf w, float k, unsigned int n) { return (cf)(1.0 - (cd)ellip_acd(w, k, n)); }

/* ellip.c:271-398: pass band to 1 rad/s, 7 Landen steps; 2L zeros on the
 * imaginary axis, the poles from cd(u_i - j v0), the real pole of an odd order last */
void ellip_azpkf(unsigned int _n, float _ep, float _es, liquid_float_complex *_za, liquid_float_complex *_pa,
                 liquid_float_complex *_ka)
{
    cf *pa_out = (cf *)_pa, *za_out = (cf *)_za;
    const float fp = (float)(1.0f / (2.0f * M_PI));
    const unsigned int n = 7;
    const float Wp = (float)(2 * M_PI * fp);
    const float k1 = _ep / _es;
    const float N = (float)_n;
    const float k = ellipdegf(N, k1, n);
    const unsigned int L = (unsigned int)floorf(N / 2.0f), r = _n % 2;
    const cf v0 = -_Complex_I * ellip_asn(_Complex_I / _ep, k1, n) / N;
    unsigned int t = 0;
    for (unsigned int i = 0; i < L; i++) {
        const float u = (2.0f * ((float)i + 1.0f) - 1.0f) / N;
        const cf zeta = ellip_cd(u, k, n);
        const cf za = _Complex_I * Wp / (k * zeta);
        const cf pa = Wp * _Complex_I * ellip_cd(u - _Complex_I * v0, k, n);
        pa_out[t] = pa;
        za_out[t++] = za;
        pa_out[t] = conjf(pa);
        za_out[t++] = conjf(za);
    }
    if (r) pa_out[t++] = Wp * _Complex_I * ellip_sn(_Complex_I * v0, k, n);
    cf ka = r ? 1.0f : 1.0f / sqrtf(1.0f + _ep * _ep);
    for (unsigned int i = 0; i < _n; i++) ka *= pa_out[i];
    for (unsigned int i = 0; i < 2 * L; i++) ka /= za_out[i];
    *(cf *)_ka = ka;
}

/* ---- Bessel (bessel.c; [Orchard:1965] H. J. Orchard, "The Roots of the
 * Maximally Flat-Delay Polynomials", IEEE Trans. Circuit Theory, 1965) */
typedef long double complex cl;

/* The order-m polynomial by its recurrence w_i = (2i - 1) w_(i-1) + s^2 w_(i-2),
 * w_0 = 1, w_1 = 1 + s, and its derivative w_m' = w_m - s w_(m-1): 50 Newton
 * steps s -= w_m / w_m' from s, in long double (m >= 2) */
static cf bessel_newton(unsigned int m, cf start)
{
    cl s = start;
    for (unsigned int it = 0; it < 50; it++) {
        cl before = 1.0L, last = 1.0L + s;
        const cl s2 = s * s;
        for (unsigned int i = 2; i < m; i++) {
            const cl next = (long double)(2 * i - 1) * last + s2 * before;
            before = last;
            last = next;
        }
        const cl w = (long double)(2 * m - 1) * last + s2 * before, dw = w - s * last;
        if (creall(dw) == 0.0L && cimagl(dw) == 0.0L) break;
        s -= w / dw;
    }
    return (float)creall(s) + _Complex_I * (float)cimagl(s);
}

/* The upper-half-plane roots of the polynomials of order 1 .. n, one row of
 * the table per order: row m holds ceil(m / 2) roots by increasing imaginary
 * part, the real root of an odd order first.  Orders 1 and 2 are known; each
 * later root starts from the straight line through its neighbours in the two
 * rows before (the real root from the real parts alone, the lowest root of an
 * even order from the row before and the mirror image of the one before
 * that) and is then refined.  Returns row n. */
static void bessel_upper_roots(unsigned int n, cf *out)
{
    const unsigned int w = (n + 1) / 2 + 1;   /* row length */
    cf *tab = (cf *)lq_xmalloc((size_t)(n + 1) * w * sizeof(cf));
#define ROW(m) (tab + (size_t)(m) * w)
    ROW(1)[0] = -1.0f;
    if (n >= 2) ROW(2)[0] = -1.5f + _Complex_I * 0.5f * sqrtf(3.0f);
    for (unsigned int m = 3; m <= n; m++) {
        const unsigned int odd = m % 2, cnt = (m + 1) / 2;
        const cf *r1 = ROW(m - 1), *r2 = ROW(m - 2);
        cf *r = ROW(m);
        for (unsigned int j = 0; j < cnt; j++) {
            cf guess;
            if (j == 0)
                guess = odd ? 2 * crealf(r1[0]) - crealf(r2[0]) : 2 * r1[0] - conjf(r2[0]);
            else
                guess = 2 * r1[j - odd] - r2[j - 1];
            r[j] = bessel_newton(m, guess);
        }
    }
    memcpy(out, ROW(n), ((n + 1) / 2) * sizeof(cf));
#undef ROW
    free(tab);
}

/* bessel.c:67-90: the n roots scaled by the approximate 3 dB frequency
 * sqrt((2n - 1) ln 2), the conjugate pairs from the outermost inwards and the
 * real pole of an odd order last; no zeros.  (The reference asks its root
 * routine for n + 1 values, one past _pa; the extra one repeats a root and is
 * not formed here.) */
void bessel_azpkf(unsigned int _n, liquid_float_complex *_za, liquid_float_complex *_pa, liquid_float_complex *_ka)
{
    cf *pa = (cf *)_pa;
    if (_n == 0) {
        *(cf *)_ka = 1.0f;
        return;
    }
    const unsigned int odd = _n % 2, cnt = (_n + 1) / 2;
    cf *up = (cf *)lq_xmalloc(cnt * sizeof(cf));
    bessel_upper_roots(_n, up);
    const float w3dB = sqrtf((2 * _n - 1) * logf(2.0f));
    unsigned int k = 0;
    for (unsigned int j = cnt; j-- > odd;) {
        pa[k++] = up[j] / w3dB;
        pa[k++] = conjf(up[j]) / w3dB;
    }
    if (odd) pa[k++] = up[0] / w3dB;
    free(up);
    cf ka = 1.0f;
    for (unsigned int i = 0; i < _n; i++) ka *= pa[i];
    *(cf *)_ka = ka;
}

/* ------------------------------------------------------------------ transforms */
/* iirdes.c:195-216 ([Constantinides:1967] A. G. Constantinides, "Frequency
 * Transformations for Digital Filters", Electronics Letters 3 (11), 1967) */
float iirdes_freqprewarp(liquid_iirdes_bandtype _btype, float _fc, float _f0)
{
    float m = 0.0f;
    if (_btype == LIQUID_IIRDES_LOWPASS)
        m = tanf((float)(M_PI * _fc));
    else if (_btype == LIQUID_IIRDES_HIGHPASS)
        m = -cosf((float)(M_PI * _fc)) / sinf((float)(M_PI * _fc));
    else if (_btype == LIQUID_IIRDES_BANDPASS)
        m = (cosf((float)(2 * M_PI * _fc)) - cosf((float)(2 * M_PI * _f0))) / sinf((float)(2 * M_PI * _fc));
    else if (_btype == LIQUID_IIRDES_BANDSTOP)
        m = sinf((float)(2 * M_PI * _fc)) / (cosf((float)(2 * M_PI * _fc)) - cosf((float)(2 * M_PI * _f0)));
    return fabsf(m);
}

/* iirdes.c:232-276: z -> (1 + m s) / (1 - m s); npa digital zeros (-1 where
 * the analog filter has none) and poles; the quotients are formed in double */
void bilinear_zpkf(liquid_float_complex *_za, unsigned int _nza, liquid_float_complex *_pa, unsigned int _npa,
                   liquid_float_complex _ka, float _m, liquid_float_complex *_zd, liquid_float_complex *_pd,
                   liquid_float_complex *_kd)
{
    const cf *za = (const cf *)_za, *pa = (const cf *)_pa;
    cf *zd = (cf *)_zd, *pd = (cf *)_pd, G;
    memcpy(&G, &_ka, sizeof(G));
    for (unsigned int i = 0; i < _npa; i++) {
        if (i < _nza) {
            const cf zm = za[i] * _m;
            zd[i] = (cf)((1.0 + zm) / (1.0 - zm));
        } else {
            zd[i] = -1.0f;
        }
        const cf pm = pa[i] * _m;
        pd[i] = (cf)((1.0 + pm) / (1.0 - pm));
        G = (cf)(G * ((1.0 - pd[i]) / (1.0 - zd[i])));
    }
    memcpy(_kd, &G, sizeof(G));
}

/* iirdes.c:414-425 */
void iirdes_dzpk_lp2hp(liquid_float_complex *_zd, liquid_float_complex *_pd, unsigned int _n,
                       liquid_float_complex *_zdt, liquid_float_complex *_pdt)
{
    for (unsigned int i = 0; i < _n; i++) {
        ((cf *)_zdt)[i] = -((cf *)_zd)[i];
        ((cf *)_pdt)[i] = -((cf *)_pd)[i];
    }
}

/* iirdes.c:435-457: each root r becomes the two roots of z^2 - c0 (1 + r) z + r, c0 = cos(2 pi f0) */
void iirdes_dzpk_lp2bp(liquid_float_complex *_zd, liquid_float_complex *_pd, unsigned int _n, float _f0,
                       liquid_float_complex *_zdt, liquid_float_complex *_pdt)
{
    const float c0 = cosf((float)(2 * M_PI * _f0));
    for (int which = 0; which < 2; which++) {
        const cf *src = (const cf *)(which ? _pd : _zd);
        cf *dst = (cf *)(which ? _pdt : _zdt);
        for (unsigned int i = 0; i < _n; i++) {
            const cf t0 = 1 + src[i];
            dst[2 * i] = 0.5f * (c0 * t0 + csqrtf(c0 * c0 * t0 * t0 - 4 * src[i]));
            dst[2 * i + 1] = 0.5f * (c0 * t0 - csqrtf(c0 * c0 * t0 * t0 - 4 * src[i]));
        }
    }
}

/* iirdes.c:285-304: b, a of n + 1 coefficients, highest power of z first */
void iirdes_dzpk2tff(liquid_float_complex *_zd, liquid_float_complex *_pd, unsigned int _n, liquid_float_complex _kd,
                     float *_b, float *_a)
{
    cf *q = (cf *)lq_xmalloc(((size_t)_n + 1) * sizeof(cf)), k;
    memcpy(&k, &_kd, sizeof(k));
    expand_roots((const cf *)_pd, _n, q);
    for (unsigned int i = 0; i <= _n; i++) _a[i] = crealf(q[_n - i]);
    expand_roots((const cf *)_zd, _n, q);
    for (unsigned int i = 0; i <= _n; i++) _b[i] = crealf(q[_n - i] * k);
    free(q);
}

/* ------------------------------------------------------------------ liquid_iirdes (iirdes.c:470-663) */
void liquid_iirdes(liquid_iirdes_filtertype _ftype, liquid_iirdes_bandtype _btype, liquid_iirdes_format _format,
                   unsigned int _n, float _fc, float _f0, float _Ap, float _As, float *_B, float *_A)
{
    if (_fc <= 0 || _fc >= 0.5) LQ_FAIL("error: liquid_iirdes(), cutoff frequency out of range\n");
    if (_f0 < 0 || _f0 > 0.5) LQ_FAIL("error: liquid_iirdes(), center frequency out of range\n");
    if (_Ap <= 0) LQ_FAIL("error: liquid_iirdes(), pass-band ripple out of range\n");
    if (_As <= 0) LQ_FAIL("error: liquid_iirdes(), stop-band ripple out of range\n");
    if (_n == 0) LQ_FAIL("error: liquid_iirdes(), filter order must be > 0\n");

    unsigned int n = _n, nza = 0;
    const unsigned int r = n % 2, L = (n - r) / 2;
    /* analog zeros and poles; digital ones at twice the order for the band-pass and band-stop cases */
    cf *pa = (cf *)lq_xmalloc(10 * (size_t)n * sizeof(cf)), *za = pa + n, *zd = za + n, *pd = zd + 2 * n;
    cf *zd1 = pd + 2 * n, *pd1 = zd1 + 2 * n, ka, k0 = 1.0f;
    liquid_float_complex *lza = (liquid_float_complex *)za, *lpa = (liquid_float_complex *)pa;
    liquid_float_complex *lka = (liquid_float_complex *)&ka, lk0, lkd;
    float epsilon;

    switch (_ftype) {
    case LIQUID_IIRDES_BUTTER:
        butter_azpkf(n, lza, lpa, lka);
        break;
    case LIQUID_IIRDES_CHEBY1:
        epsilon = sqrtf(powf(10.0f, _Ap / 10.0f) - 1.0f);
        k0 = r ? 1.0f : (float)(1.0f / sqrt(1.0f + epsilon * epsilon));
        cheby1_azpkf(n, epsilon, lza, lpa, lka);
        break;
    case LIQUID_IIRDES_CHEBY2:
        nza = 2 * L;
        epsilon = powf(10.0f, -_As / 20.0f);
        cheby2_azpkf(n, epsilon, lza, lpa, lka);
        break;
    case LIQUID_IIRDES_ELLIP: {
        nza = 2 * L;
        const float Gp = powf(10.0f, -_Ap / 20.0f), Gs = powf(10.0f, -_As / 20.0f);
        const float ep = sqrtf(1.0f / (Gp * Gp) - 1.0f), es = sqrtf(1.0f / (Gs * Gs) - 1.0f);
        k0 = r ? 1.0f : (float)(1.0f / sqrt(1.0f + ep * ep));
        ellip_azpkf(n, ep, es, lza, lpa, lka);
        break;
    }
    case LIQUID_IIRDES_BESSEL:
        bessel_azpkf(n, lza, lpa, lka);
        break;
    default:
        LQ_FAIL("error: liquid_iirdes(), unknown filter type\n");
    }

    /* the digital gain starts from the nominal k0, not from the analog gain */
    const float m = iirdes_freqprewarp(_btype, _fc, _f0);
    memcpy(&lk0, &k0, sizeof(lk0));
    bilinear_zpkf(lza, nza, lpa, n, lk0, m, (liquid_float_complex *)zd, (liquid_float_complex *)pd, &lkd);

    if (_btype == LIQUID_IIRDES_HIGHPASS || _btype == LIQUID_IIRDES_BANDSTOP)
        iirdes_dzpk_lp2hp((liquid_float_complex *)zd, (liquid_float_complex *)pd, n, (liquid_float_complex *)zd,
                          (liquid_float_complex *)pd);
    if (_btype == LIQUID_IIRDES_BANDPASS || _btype == LIQUID_IIRDES_BANDSTOP) {
        iirdes_dzpk_lp2bp((liquid_float_complex *)zd, (liquid_float_complex *)pd, n, _f0, (liquid_float_complex *)zd1,
                          (liquid_float_complex *)pd1);
        memcpy(zd, zd1, 2 * (size_t)n * sizeof(cf));
        memcpy(pd, pd1, 2 * (size_t)n * sizeof(cf));
        n = 2 * n;
    }
    if (_format == LIQUID_IIRDES_TF)
        iirdes_dzpk2tff((liquid_float_complex *)zd, (liquid_float_complex *)pd, n, lkd, _B, _A);
    else
        iirdes_dzpk2sosf((liquid_float_complex *)zd, (liquid_float_complex *)pd, n, lkd, _B, _A);
    free(pa);
}

/* iirdes.c:669-703 says: stable unless a root of the denominator has a
 * magnitude above 1.  Here by the Schur-Cohn (Jury) recursion in float64 on
 * p(z) = a[0] z^m + ... + a[m].  With k = a[m] / a[0]:
 *   |k| > 1  the product of the roots exceeds 1 in magnitude: a root outside
 *   |k| < 1  p - k p* (p* the reversed polynomial), of order m - 1, has as
 *            many roots outside the circle as p: go on with it
 *   |k| = 1  the product of the root magnitudes is 1.  Either p = k p*
 *            (self-inversive: its roots lie on the circle or in pairs r,
 *            1 / conj(r)), and then all of them are on the circle, which the
 *            reference calls stable, exactly when the derivative has none
 *            outside (Cohn's theorem): go on with p'.  Or it is not, so not
 *            all roots are on the circle and one of them is outside.
 * |k| = 1 is met only when it holds exactly in float64 (an integrator's
 * 1 - z^-1, for instance); agreement with the reference's answers has been
 * established on the fixture's cases only (tests/test_iirdes.py checks the
 * rule itself against float64 roots).
 * a: m + 1 coefficients, t: as many of scratch */
static int schur_cohn(double *a, double *t, unsigned int m)
{
    while (m >= 1) {
        while (m >= 1 && a[0] == 0.0) {   /* leading zeros: a lower order */
            memmove(a, a + 1, m * sizeof(double));
            m--;
        }
        if (m == 0) return 1;
        const double k = a[m] / a[0];
        if (fabs(k) > 1.0) return 0;
        if (fabs(k) == 1.0) {
            for (unsigned int i = 0; i <= m; i++)
                if (a[i] != k * a[m - i]) return 0;
            for (unsigned int i = 0; i < m; i++) a[i] = a[i] * (double)(m - i);   /* the derivative */
        } else {
            for (unsigned int i = 0; i < m; i++) t[i] = a[i] - k * a[m - i];
            memcpy(a, t, m * sizeof(double));
        }
        m--;
    }
    return 1;
}

int iirdes_isstable(float *_b, float *_a, unsigned int _n)
{
    if (_n < 2) LQ_FAIL("error: iirdes_isstable(), filter order too low\n");
    double *a = (double *)lq_xmalloc(2 * (size_t)_n * sizeof(double));
    for (unsigned int i = 0; i < _n; i++) a[i] = _a[i];
    const int stable = schur_cohn(a, a + _n, _n - 1);
    free(a);
    return stable;
}
