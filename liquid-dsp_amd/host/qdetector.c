/*
 * qdetector.c -- qdetector_cccf on the MI355X: the FFT preamble detector.
 *
 * API and semantics: include/liquid.h "qdetector_cccf",
 * src/framing/src/qdetector_cccf.c; the departures are listed in
 * include/liquid_mi355x.h.
 *
 * The object holds the template s, S = FFT(s zero padded) (made once on the
 * device at create), s2_sum, and the carried state: the last nfft samples of
 * the stream in one lq_hist -- the reference's buf_time_0[0 .. counter) is
 * always the newest `counter` of them -- and the walk's variables (counter,
 * SEEK / ALIGN, coarse offset, estimates; host/qdetector_walk.c, which makes
 * every decision and needs no GPU).
 *
 * A call sees ext = (those counter samples) ++ (its n samples).  It asks the
 * walk what comes next: seek windows on the current grid, computed ahead of
 * any decision in chunks of qd_chunk(nfft) windows (so at most one chunk's
 * windows are thrown away per detection); the walk stops at the first
 * detection, the align stage runs on the frame once its nfft samples are
 * there, and seek relaunches from the new grid origin.  Only a chunk's
 * records (16 bytes a window) and, per detection, 15 scalars come back.
 * At the end the history takes the call's samples (lqk_window_append) and the
 * walk keeps how many of them are still pending.
 *
 * execute() appends to the history's host mirror; once per nfft/2 samples,
 * when the buffer fills, the same path runs with no new samples.
 */
#include <complex.h>

#include "lq_host.h"

#define QD_CHUNK_SAMPLES (1u << 21)   /* a chunk's forward transforms: 16 MB */
#define QD_CHUNK_MIN 16u
#define QD_CHUNK_MAX 4096u

static unsigned int g_chunk = 0;      /* tests: liquid_mi355x_qdetector_set_chunk */
static int g_route = -1;              /* measurements: liquid_mi355x_qdetector_set_route */

static int qd_route(unsigned int nfft)
{
    return g_route == LIQUID_MI355X_QDETECTOR_COMPOSED ? LQK_QD_ROUTE_COMPOSED : lqk_qdetector_route(nfft);
}

struct qdetector_cccf_s {
    unsigned int s_len, nfft;
    float complex *s;
    qd_walk w;
    lq_hist hist;                 /* the last nfft samples */
    lq_ctx ctx;
    lq_devbuf xbuf, sbuf;         /* staged input, the composed path's scratch */
    void *ds, *dS;                /* template and its spectrum */
    void *dframe, *dalign;        /* the aligned frame, the align stage's scratch */
    void *drec;                   /* a chunk's records */
    unsigned int rec_cap;
    qdetector_cccf_record *hrec;  /* ... on the host (pinned) */
    unsigned int *hout, *dout;    /* the align stage's 13 + 2 scalars */
    float complex *frame;         /* host copy handed out by execute() */
};

typedef struct {
    unsigned int max_det, count;
    unsigned long long *idx;
    float *tau, *gamma, *dphi, *phi;
    void *frames;
    int frames_dev;
    void *records;
    int records_dev;
    unsigned long long nrec;
} qd_out;

static unsigned int qd_chunk(unsigned int nfft)
{
    if (g_chunk) return g_chunk;
    unsigned int c = QD_CHUNK_SAMPLES / nfft;
    if (c < QD_CHUNK_MIN) c = QD_CHUNK_MIN;
    if (c > QD_CHUNK_MAX) c = QD_CHUNK_MAX;
    return c;
}

qdetector_cccf qdetector_cccf_create(liquid_float_complex *_s, unsigned int _s_len)
{
    if (_s_len == 0) LQ_FAIL("error: qdetector_cccf_create(), sequence length cannot be zero\n");
    if (_s_len > (1u << 22)) LQ_FAIL("error: qdetector_cccf_create(), sequence longer than 2^22 samples\n");
    lqrt_require_device("qdetector_cccf_create");
    qdetector_cccf q = (qdetector_cccf)lq_xmalloc(sizeof(*q));
    q->s_len = _s_len;
    q->s = (float complex *)lq_xmalloc((size_t)_s_len * sizeof(float complex));
    memmove(q->s, _s, (size_t)_s_len * sizeof(float complex));
    float s2 = 0.0f;
    for (unsigned int i = 0; i < _s_len; i++) s2 += crealf(q->s[i]) * crealf(q->s[i]) + cimagf(q->s[i]) * cimagf(q->s[i]);
    q->nfft = 1u << liquid_nextpow2(2 * _s_len);
    const size_t fb = (size_t)q->nfft * 8;
    qdw_init(&q->w, q->nfft, _s_len, s2);
    lq_ctx_init(&q->ctx);
    lq_hist_init(&q->hist, q->nfft, 8, LQ_HIST_MIRROR);
    lq_hist_zero(&q->hist, q->ctx.stream);
    q->ds = lqrt_malloc(fb);   /* zero padded */
    q->dS = lqrt_malloc(fb);
    q->dframe = lqrt_malloc(fb);
    q->dalign = lqrt_malloc(lqk_qdetector_align_bytes(q->nfft));
    q->dout = (unsigned int *)lqrt_malloc(64);
    q->hout = (unsigned int *)lqrt_host_alloc(64);
    q->frame = (float complex *)lq_xmalloc(fb);
    lqrt_h2d(q->ds, q->s, (size_t)_s_len * 8, q->ctx.stream);
    lqk_qdetector_spectrum(q->nfft, q->ds, q->dS, q->dalign, q->ctx.stream);
    lqrt_sync(q->ctx.stream);
    return q;
}

qdetector_cccf qdetector_cccf_create_linear(liquid_float_complex *_sequence, unsigned int _sequence_len, int _ftype,
                                            unsigned int _k, unsigned int _m, float _beta)
{
    if (_sequence_len == 0) LQ_FAIL("error: qdetector_cccf_create_linear(), sequence length cannot be zero\n");
    if (_k < 2 || _k > 80) LQ_FAIL("error: qdetector_cccf_create_linear(), samples per symbol must be in [2,80]\n");
    if (_m < 1 || _m > 100) LQ_FAIL("error: qdetector_cccf_create_linear(), filter delay must be in [1,100]\n");
    if (_beta < 0.0f || _beta > 1.0f)
        LQ_FAIL("error: qdetector_cccf_create_linear(), excess bandwidth factor must be in [0,1]\n");
    /* the time-domain template: sequence_len + 2m symbols, the tail zero,
     * through the prototype's k-phase interpolator (qdetector_cccf.c:173-180) */
    const unsigned int hlen = 2 * _k * _m + 1, nsym = _sequence_len + 2 * _m, s_len = _k * nsym;
    float *h = (float *)lq_xmalloc(hlen * sizeof(float));
    liquid_firdes_prototype((liquid_firfilt_type)_ftype, _k, _m, _beta, 0, h);
    float complex *s = (float complex *)lq_xmalloc((size_t)s_len * sizeof(float complex));
    for (unsigned int i = 0; i < nsym; i++)
        for (unsigned int p = 0; p < _k; p++) {
            float complex acc = 0;
            for (unsigned int l = 0; l <= 2 * _m && l <= i; l++)
                if (p + l * _k < hlen && i - l < _sequence_len) acc += _sequence[i - l] * h[p + l * _k];
            s[_k * i + p] = acc;
        }
    qdetector_cccf q = qdetector_cccf_create(s, s_len);
    free(s);
    free(h);
    return q;
}

void qdetector_cccf_destroy(qdetector_cccf _q)
{
    lqrt_sync(_q->ctx.stream);
    lq_devbuf_free(&_q->xbuf);
    lq_devbuf_free(&_q->sbuf);
    lqrt_free(_q->ds);
    lqrt_free(_q->dS);
    lqrt_free(_q->dframe);
    lqrt_free(_q->dalign);
    lqrt_free(_q->dout);
    if (_q->drec) lqrt_free(_q->drec);
    lqrt_host_free(_q->hout);
    lqrt_host_free(_q->hrec);
    lq_hist_free(&_q->hist);
    lq_ctx_free(&_q->ctx);
    free(_q->frame);
    free(_q->s);
    free(_q);
}

void qdetector_cccf_print(qdetector_cccf _q)
{
    printf("qdetector_cccf: template of %u samples, buffer (nfft) %u, threshold %.4f, range %d bins, "
           "template energy %.2f\n", _q->s_len, _q->nfft, _q->w.threshold, _q->w.range, _q->w.s2_sum);
}

void qdetector_cccf_reset(qdetector_cccf _q)
{
    lq_hist_zero(&_q->hist, _q->ctx.stream);
    qdw_reset(&_q->w);
}

void qdetector_cccf_set_threshold(qdetector_cccf _q, float _threshold)
{
    if (!qdw_set_threshold(&_q->w, _threshold))
        fprintf(stderr, "warning: qdetector_cccf_set_threshold(), %g is outside (0, 2]; the threshold stays as it was\n", _threshold);
}

void qdetector_cccf_set_range(qdetector_cccf _q, float _dphi_max)
{
    if (!qdw_set_range(&_q->w, _dphi_max))
        fprintf(stderr, "warning: qdetector_cccf_set_range(), %g is outside [0, 0.5]; the range stays as it was\n", _dphi_max);
}

unsigned int qdetector_cccf_get_seq_len(qdetector_cccf _q) { return _q->s_len; }
const void *qdetector_cccf_get_sequence(qdetector_cccf _q) { return (const void *)_q->s; }
unsigned int qdetector_cccf_get_buf_len(qdetector_cccf _q) { return _q->nfft; }
float qdetector_cccf_get_tau(qdetector_cccf _q) { return _q->w.tau_hat; }
float qdetector_cccf_get_gamma(qdetector_cccf _q) { return _q->w.gamma_hat; }
float qdetector_cccf_get_dphi(qdetector_cccf _q) { return _q->w.dphi_hat; }
float qdetector_cccf_get_phi(qdetector_cccf _q) { return _q->w.phi_hat; }
int qdetector_cccf_get_range(qdetector_cccf _q) { return _q->w.range; }
float qdetector_cccf_get_threshold(qdetector_cccf _q) { return _q->w.threshold; }

/* ----------------------------------------------------------------- the device path */

static void qd_rec_room(qdetector_cccf q, unsigned int nw)
{
    if (nw <= q->rec_cap) return;
    if (q->drec) lqrt_free(q->drec);
    lqrt_host_free(q->hrec);
    q->rec_cap = nw;
    q->drec = lqrt_malloc((size_t)nw * sizeof(qdetector_cccf_record));
    q->hrec = (qdetector_cccf_record *)lqrt_host_alloc((size_t)nw * sizeof(qdetector_cccf_record));
}

/* the walk over ext = (the counter newest samples of the history) ++ dx[0 .. n) */
static void qd_run(qdetector_cccf q, const void *dx, unsigned long long n, qd_out *o)
{
    void *st = q->ctx.stream;
    const unsigned int nfft = q->nfft;
    qdw_begin(&q->w, n);
    const unsigned long long clen = q->w.c0;
    const unsigned char *hist = (const unsigned char *)lq_hist_dev(&q->hist, st);
    const void *carry = hist + ((size_t)nfft - clen) * 8;
    unsigned long long pos, count;
    int act;
    while ((act = qdw_next(&q->w, &pos, &count)) != QDW_DO_END) {
        if (act == QDW_DO_SEEK) {
            const unsigned int chunk = qd_chunk(nfft);
            const unsigned int nw = count < chunk ? (unsigned int)count : chunk;
            qd_rec_room(q, nw);
            void *scratch = NULL;
            const int route = qd_route(nfft);
            if (route == LQK_QD_ROUTE_COMPOSED) {
                unsigned int nb;
                scratch = lq_devbuf_get(&q->sbuf, lqk_qdetector_scratch_bytes(nfft, q->w.range, nw, &nb));
            }
            lqk_qdetector_seek(route, nfft, q->s_len, q->w.s2_sum, q->w.range, q->dS, carry, clen, dx, pos, nw,
                               scratch, q->drec, st);
            lqrt_d2h(q->hrec, q->drec, (size_t)nw * sizeof(qdetector_cccf_record), st);
            lqrt_sync(st);
            const unsigned long long used = qdw_seek(&q->w, q->hrec, nw);
            if (o->records) {
                unsigned char *dst = (unsigned char *)o->records + o->nrec * sizeof(qdetector_cccf_record);
                if (o->records_dev) lqrt_d2d(dst, q->drec, (size_t)used * sizeof(qdetector_cccf_record), st);
                else memcpy(dst, q->hrec, (size_t)used * sizeof(qdetector_cccf_record));
            }
            o->nrec += used;
            continue;
        }
        lqk_qdetector_align(nfft, q->s_len, q->w.offset, q->dS, q->ds, carry, clen, dx, pos, q->dframe, q->dalign,
                            q->dout, st);
        lqrt_d2h(q->hout, q->dout, 13 * 4, st);
        lqrt_sync(st);
        float sc[13];
        memcpy(sc, q->hout, sizeof(sc));
        qdw_align_fit(&q->w, sc, q->hout[6], sc + 7);
        lqk_qdetector_metric(q->s_len, q->w.dphi_hat, q->dalign, q->dout + 13, st);
        lqrt_d2h(q->hout + 13, q->dout + 13, 2 * 4, st);
        lqrt_sync(st);
        memcpy(sc, q->hout + 13, 2 * sizeof(float));
        const unsigned long long idx = qdw_align_finish(&q->w, sc[0], sc[1]);
        if (o->count < o->max_det) {
            const unsigned int k = o->count;
            if (o->idx) o->idx[k] = idx;
            if (o->tau) o->tau[k] = q->w.tau_hat;
            if (o->gamma) o->gamma[k] = q->w.gamma_hat;
            if (o->dphi) o->dphi[k] = q->w.dphi_hat;
            if (o->phi) o->phi[k] = q->w.phi_hat;
            if (o->frames) {
                unsigned char *dst = (unsigned char *)o->frames + (size_t)k * nfft * 8;
                if (o->frames_dev) lqrt_d2d(dst, q->dframe, (size_t)nfft * 8, st);
                else lqrt_d2h(dst, q->dframe, (size_t)nfft * 8, st);
                lqrt_sync(st);   /* dframe is written again by the next frame */
            }
        }
        o->count++;
    }
    if (n) {
        lqk_window_append(1, hist, nfft, dx, n, lq_hist_next(&q->hist), st);
        lq_hist_flip(&q->hist);
    }
    qdw_end(&q->w);
    lqrt_sync(st);
}

void *qdetector_cccf_execute(qdetector_cccf _q, liquid_float_complex _x)
{
    lq_hist_append(&_q->hist, &_x, 1, _q->ctx.stream);
    lq_hist_commit(&_q->hist, 1);
    if (++_q->w.counter < _q->nfft) return NULL;
    /* the buffer is full: one seek window, or the frame being aligned */
    qd_out o = {1, 0, NULL, NULL, NULL, NULL, NULL, _q->frame, 0, NULL, 0, 0};
    qd_run(_q, NULL, 0, &o);
    return o.count ? (void *)_q->frame : NULL;
}

unsigned int qdetector_cccf_execute_block_dev(qdetector_cccf _q, const liquid_float_complex *_dx,
                                              unsigned long long _n, unsigned int _max_det, unsigned long long *_idx,
                                              float *_tau_hat, float *_gamma_hat, float *_dphi_hat, float *_phi_hat,
                                              liquid_float_complex *_dframes, qdetector_cccf_record *_drecords,
                                              unsigned long long *_num_records)
{
    qd_out o = {_max_det, 0, _idx, _tau_hat, _gamma_hat, _dphi_hat, _phi_hat, _dframes, 1, _drecords, 1, 0};
    if (_n) qd_run(_q, _dx, _n, &o);
    if (_num_records) *_num_records = o.nrec;
    return o.count;
}

unsigned int qdetector_cccf_execute_block(qdetector_cccf _q, const liquid_float_complex *_x, unsigned long long _n,
                                          unsigned int _max_det, unsigned long long *_idx, float *_tau_hat,
                                          float *_gamma_hat, float *_dphi_hat, float *_phi_hat,
                                          liquid_float_complex *_frames, qdetector_cccf_record *_records,
                                          unsigned long long *_num_records)
{
    qd_out o = {_max_det, 0, _idx, _tau_hat, _gamma_hat, _dphi_hat, _phi_hat, _frames, 0, _records, 0, 0};
    if (_n) {
        const void *dx = lq_call_in(&_q->ctx, &_q->xbuf, _x, (size_t)_n * 8);
        qd_run(_q, dx, _n, &o);   /* synchronises: the staged input is free again */
        _q->ctx.in_busy = 0;
    }
    if (_num_records) *_num_records = o.nrec;
    return o.count;
}

void qdetector_cccf_set_stream(qdetector_cccf _q, void *_s) { lq_ctx_set_stream(&_q->ctx, _s); }

void qdetector_cccf_synchronize(qdetector_cccf _q) { lqrt_sync(_q->ctx.stream); }

int liquid_mi355x_qdetector_route(unsigned int _nfft, int _range, unsigned long long _num_windows)
{
    return qd_route(_nfft) == LQK_QD_ROUTE_FUSED ? LIQUID_MI355X_QDETECTOR_FUSED : LIQUID_MI355X_QDETECTOR_COMPOSED;
}

void liquid_mi355x_qdetector_set_route(int _route) { g_route = _route; }

void liquid_mi355x_qdetector_set_chunk(unsigned int _windows) { g_chunk = _windows; }
unsigned int liquid_mi355x_qdetector_chunk(unsigned int _nfft) { return qd_chunk(_nfft); }
