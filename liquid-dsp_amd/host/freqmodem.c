/*
 * freqmodem.c -- freqmod and freqdem on the MI355X: analog FM modulator and
 * demodulator.
 *
 * API and semantics: include/liquid.h:5329-5372 and 5548-5591,
 * src/modem/src/freqmod.c, freqdem.c.  The per-sample calls are the
 * reference's arithmetic on the host; the block calls, which the reference
 * runs as a per-sample loop, run on the GPU (csrc/k_freqmodem.hip).
 *
 * As with nco_crcf, create() does not require a device: the object takes its
 * stream and buffers at the first block call (or set_stream), which is where a
 * missing device is fatal.
 *
 * freqmod.  The state is a phase accumulator modulo 2^16, advanced per sample
 * by (int)roundf(ref * m), ref = kf 2^16; the output is entry
 * ((phase + 0x20) >> 6) & 0x3ff of a 1024-entry table.  The increment is kept
 * in unsigned arithmetic: the roundf result converted to a 32-bit integer and
 * reduced modulo 2^16; a product that is not finite, or 2^31 or more in
 * magnitude, contributes what the x86 conversion yields, 0x80000000, whose low
 * 16 bits are 0.  Integer addition modulo 2^16 is associative, so the kernel's
 * prefix sum gives the per-sample loop's accumulator bit for bit.
 *
 * freqdem.  m[n] = arg(conj(r[n-M]) r[n]) * ref, ref = 1 / (2 pi kf); M = 1 is
 * the reference's object, M > 1 (create_channels) demodulates M interleaved
 * channels, such as a channelizer's frame-major output.  The product is formed
 * in float32 as re = a c + b d, im = a d - b c (four rounded products, what
 * conjf(p) * r compiles to), then atan2f and one multiply.
 *
 * State.  The accumulator (one 32-bit word) and the last M samples live in a
 * streaming history (lq_hist, with its host mirror): a device call leaves its
 * end state on the device and a later host call fetches it; a host-pointer
 * freqdem call of M samples or more takes its end state from the tail of its
 * input without waiting.  Until the device is taken the state is a plain host
 * window.
 */
#include <complex.h>

#include "lq_host.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

/* ----------------------------------------------------------------- state */

typedef struct {
    size_t n, esz;
    int dev_ready;
    lq_mirror pre;   /* the window before the device is taken */
    lq_hist h;       /* ... and after */
    lq_ctx ctx;
} fm_state;

static void st_init(fm_state *s, size_t n, size_t esz)
{
    memset(s, 0, sizeof(*s));
    s->n = n;
    s->esz = esz;
    lq_mirror_init(&s->pre, n, esz, 0);
}

static lq_mirror *st_mirror(fm_state *s) { return s->dev_ready ? &s->h.m : &s->pre; }

/* the window of n elements, oldest first, up to date on the host */
static unsigned char *st_host(fm_state *s)
{
    return s->dev_ready ? lq_hist_host(&s->h, s->ctx.stream) : lq_mirror_ptr(&s->pre);
}

/* k elements more; the window is then the last n */
static void st_push(fm_state *s, const void *x, size_t k)
{
    st_host(s);
    lq_mirror_append(st_mirror(s), x, k);
    lq_mirror_commit(st_mirror(s), k);
}

/* zero, without waiting for the device: its copy becomes the stale one */
static void st_reset(fm_state *s)
{
    lq_mirror_zero(st_mirror(s));
    if (s->dev_ready) s->h.m.dev_valid = 0;
}

static void st_device(fm_state *s, const char *who)
{
    if (s->dev_ready) return;
    lqrt_require_device(who);
    lq_ctx_init(&s->ctx);
    lq_hist_init(&s->h, s->n, s->esz, LQ_HIST_MIRROR);
    lq_mirror_append(&s->h.m, lq_mirror_ptr(&s->pre), s->n);
    lq_mirror_commit(&s->h.m, s->n);
    lq_mirror_free(&s->pre);
    s->dev_ready = 1;
}

/* the current device buffer, up to date; an upload reads the host window,
 * which the caller may change next: it has ended on return */
static const void *st_dev(fm_state *s)
{
    const int upload = !s->h.m.dev_valid;
    void *d = lq_hist_dev(&s->h, s->ctx.stream);
    if (upload) lqrt_sync(s->ctx.stream);
    return d;
}

static void st_free(fm_state *s)
{
    if (s->dev_ready) {
        lqrt_sync(s->ctx.stream);
        lq_hist_free(&s->h);
        lq_ctx_free(&s->ctx);
    } else {
        lq_mirror_free(&s->pre);
    }
}

static void st_set_stream(fm_state *s, void *stream, const char *who)
{
    st_device(s, who);
    lq_ctx_set_stream(&s->ctx, stream);
}

/* ----------------------------------------------------------------- freqmod */

#define FREQMOD_TABLE 1024

struct freqmod_s {
    float kf, ref;
    liquid_float_complex tab[FREQMOD_TABLE];
    fm_state st;              /* the accumulator, one 32-bit word */
    lq_devbuf mbuf, sbuf, sums;
    void *dtab;
};

freqmod freqmod_create(float _kf)
{
    if (_kf <= 0.0f || _kf > 1.0)
        LQ_FAIL("error: freqmod_create(), modulation factor %12.4e out of range [0,1]\n", _kf);
    freqmod q = (freqmod)lq_xmalloc(sizeof(*q));
    q->kf = _kf;
    q->ref = q->kf * (1 << 16);
    /* freqmod.c:66-68: the angle in double from M_PI, rounded to float, then cexpf */
    for (unsigned int i = 0; i < FREQMOD_TABLE; i++)
        q->tab[i] = cexpf(_Complex_I * 2 * M_PI * (float)i / (float)FREQMOD_TABLE);
    st_init(&q->st, 1, sizeof(unsigned int));
    return q;
}

void freqmod_destroy(freqmod _q)
{
    if (_q->st.dev_ready) {
        lqrt_sync(_q->st.ctx.stream);
        lq_devbuf_free(&_q->mbuf);
        lq_devbuf_free(&_q->sbuf);
        lq_devbuf_free(&_q->sums);
        lqrt_free(_q->dtab);
    }
    st_free(&_q->st);
    free(_q);
}

void freqmod_print(freqmod _q)
{
    printf("freqmod:\n");
    printf("    mod. factor         :   %8.4f\n", _q->kf);
    printf("    sincos table len    :   %u\n", FREQMOD_TABLE);
}

void freqmod_reset(freqmod _q) { st_reset(&_q->st); }

unsigned int freqmod_get_phase(freqmod _q)
{
    unsigned int p;
    memcpy(&p, st_host(&_q->st), sizeof(p));
    return p & 0xffff;
}

void freqmod_get_table(freqmod _q, liquid_float_complex *_tab) { memcpy(_tab, _q->tab, sizeof(_q->tab)); }

static unsigned int fm_increment(float ref, float m)
{
    const float r = roundf(ref * m);
    return fabsf(r) < 2147483648.0f ? (unsigned int)(int)r : 0u;
}

void freqmod_modulate(freqmod _q, float _m, liquid_float_complex *_s)
{
    const unsigned int phase = (freqmod_get_phase(_q) + fm_increment(_q->ref, _m)) & 0xffff;
    st_push(&_q->st, &phase, 1);
    *_s = _q->tab[((phase + 0x0020) >> 6) & 0x03ff];
}

static void fm_device(freqmod q)
{
    if (q->st.dev_ready) return;
    st_device(&q->st, "freqmod_modulate_block");
    q->dtab = lqrt_malloc(sizeof(q->tab));
    lqrt_h2d(q->dtab, q->tab, sizeof(q->tab), q->st.ctx.stream);
    lqrt_sync(q->st.ctx.stream);
}

void freqmod_modulate_block_dev(freqmod _q, const float *_dm, unsigned long long _n, liquid_float_complex *_ds)
{
    if (_n == 0) return;
    fm_device(_q);
    while (_n) {
        const unsigned long long c = _n < LQK_FREQMOD_MAXN ? _n : LQK_FREQMOD_MAXN;
        const size_t tiles = (size_t)((c + LQK_FREQMOD_TILE - 1) / LQK_FREQMOD_TILE);
        unsigned *sums = (unsigned *)lq_devbuf_get(&_q->sums, tiles * sizeof(unsigned));
        const unsigned *acc = (const unsigned *)st_dev(&_q->st);
        lqk_freqmod(_q->ref, _q->dtab, acc, (unsigned *)lq_hist_next(&_q->st.h), sums, _dm, _ds, c, _q->st.ctx.stream);
        lq_hist_flip(&_q->st.h);
        _dm += c;
        _ds += c;
        _n -= c;
    }
}

void freqmod_modulate_block(freqmod _q, float *_m, unsigned int _n, liquid_float_complex *_s)
{
    if (_n == 0) return;
    fm_device(_q);
    const float *dm = (const float *)lq_call_in(&_q->st.ctx, &_q->mbuf, _m, (size_t)_n * sizeof(float));
    const size_t bytes = (size_t)_n * sizeof(liquid_float_complex);
    liquid_float_complex *ds = (liquid_float_complex *)lq_devbuf_get(&_q->sbuf, bytes);
    freqmod_modulate_block_dev(_q, dm, _n, ds);
    lq_call_out(&_q->st.ctx, _s, ds, bytes);
}

void freqmod_set_stream(freqmod _q, void *_s)
{
    fm_device(_q);
    st_set_stream(&_q->st, _s, "freqmod_set_stream");
}

void freqmod_synchronize(freqmod _q)
{
    if (_q->st.dev_ready) lqrt_sync(_q->st.ctx.stream);
}

unsigned int liquid_mi355x_freqmod_tile(void) { return LQK_FREQMOD_TILE; }
unsigned int liquid_mi355x_freqmod_scan_pass(void) { return LQK_FREQMOD_PASS; }

/* ----------------------------------------------------------------- freqdem */

struct freqdem_s {
    float kf, ref;
    unsigned int M;
    fm_state st;              /* the last M samples */
    lq_devbuf rbuf, mbuf;
};

freqdem freqdem_create_channels(float _kf, unsigned int _M)
{
    if (_kf <= 0.0f || _kf > 1.0)
        LQ_FAIL("error: freqdem_create(), modulation factor %12.4e out of range [0,1]\n", _kf);
    if (_M == 0) LQ_FAIL("error: freqdem_create_channels(), number of channels must be greater than zero\n");
    freqdem q = (freqdem)lq_xmalloc(sizeof(*q));
    q->kf = _kf;
    q->ref = 1.0f / (2 * M_PI * q->kf);
    q->M = _M;
    st_init(&q->st, _M, sizeof(liquid_float_complex));
    return q;
}

freqdem freqdem_create(float _kf) { return freqdem_create_channels(_kf, 1); }

void freqdem_destroy(freqdem _q)
{
    if (_q->st.dev_ready) {
        lqrt_sync(_q->st.ctx.stream);
        lq_devbuf_free(&_q->rbuf);
        lq_devbuf_free(&_q->mbuf);
    }
    st_free(&_q->st);
    free(_q);
}

void freqdem_print(freqdem _q)
{
    printf("freqdem:\n");
    printf("    mod. factor :   %8.4f\n", _q->kf);
    if (_q->M > 1) printf("    channels    :   %u\n", _q->M);
}

void freqdem_reset(freqdem _q) { st_reset(&_q->st); }

unsigned int freqdem_get_channels(freqdem _q) { return _q->M; }

void freqdem_demodulate(freqdem _q, liquid_float_complex _r, float *_m)
{
    float p[2];
    memcpy(p, st_host(&_q->st), sizeof(p));   /* the oldest of the last M samples */
    const float c = crealf(_r), d = cimagf(_r);
    const float re = p[0] * c + p[1] * d;
    const float im = p[0] * d - p[1] * c;
    *_m = atan2f(im, re) * _q->ref;
    st_push(&_q->st, &_r, 1);
}

void freqdem_demodulate_block_dev(freqdem _q, const liquid_float_complex *_dr, unsigned long long _n, float *_dm)
{
    if (_n == 0) return;
    st_device(&_q->st, "freqdem_demodulate_block");
    while (_n) {
        const unsigned long long c = _n < LQK_FREQDEM_MAXN ? _n : LQK_FREQDEM_MAXN;
        const void *hist = st_dev(&_q->st);
        lqk_freqdem(_q->ref, _q->M, hist, lq_hist_next(&_q->st.h), _dr, _dm, c, _q->st.ctx.stream);
        lq_hist_flip(&_q->st.h);
        _dr += c;
        _dm += c;
        _n -= c;
    }
}

void freqdem_demodulate_block(freqdem _q, liquid_float_complex *_r, unsigned int _n, float *_m)
{
    if (_n == 0) return;
    fm_state *s = &_q->st;
    st_device(s, "freqdem_demodulate_block");
    /* a call shorter than M keeps some of the old state: have it on the host
     * before the device moves on */
    if (_n < _q->M) st_host(s);
    const size_t bytes = (size_t)_n * sizeof(liquid_float_complex);
    const liquid_float_complex *dr = (const liquid_float_complex *)lq_call_in(&s->ctx, &_q->rbuf, _r, bytes);
    float *dm = (float *)lq_devbuf_get(&_q->mbuf, (size_t)_n * sizeof(float));
    freqdem_demodulate_block_dev(_q, dr, _n, dm);
    /* the end state is the tail of the input: both sides hold it */
    lq_mirror *m = &s->h.m;
    if (_n >= _q->M) {
        m->off = 0;
        memcpy(m->buf, _r + (_n - _q->M), (size_t)_q->M * sizeof(liquid_float_complex));
    } else {
        lq_mirror_append(m, _r, _n);
        lq_mirror_commit(m, _n);
    }
    m->host_valid = m->dev_valid = 1;
    lq_call_out(&s->ctx, _m, dm, (size_t)_n * sizeof(float));
}

void freqdem_set_stream(freqdem _q, void *_s) { st_set_stream(&_q->st, _s, "freqdem_set_stream"); }

void freqdem_synchronize(freqdem _q)
{
    if (_q->st.dev_ready) lqrt_sync(_q->st.ctx.stream);
}

unsigned int liquid_mi355x_freqdem_tile(void) { return LQK_FREQDEM_TILE; }
unsigned int liquid_mi355x_freqdem_switch(void) { return LQK_FREQDEM_SWITCH; }
unsigned int liquid_mi355x_freqdem_frames(void) { return LQK_FREQDEM_FRAMES; }
