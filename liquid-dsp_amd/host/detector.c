/*
 * detector.c -- detector_cccf on the MI355X: the preamble correlator bank.
 *
 * API and semantics: include/liquid.h:4117-4152, src/framing/src/detector_cccf.c.
 *   m = max(2, ceil(|dphi_max / dphi_step|)) templates p_k[i] = conj(s[i])
 *   exp(-j dphi[k] i), dphi_step = 0.8 pi / n, dphi[k] = (k - (m-1)/2) dphi_step,
 *   formed in float32 as the reference forms them (:159-167).  For stream
 *   sample t with window w_t = x[t-n+1 .. t] (zeros before the last reset):
 *     r_k[t] = |sum_i p_k[i] w_t[i]| / sqrt(n E[t]),   E[t] = sum_i |w_t[i]|^2
 *   and the state machine of detector_cccf_correlate (:247-330) runs over the
 *   rows r[t], with the estimates of :396-454.
 *
 * State.  The last n samples in one lq_hist (host mirror; the device pair is
 * attached at the first block call), state / timer / imax / idetect, and the
 * rows of the last two samples at which the correlators ran (ra older, rb
 * newer: the reference's rxy1 and rxy on entry to a sample, its rxy0 and rxy1
 * once the new row is in).  correlate() and the block calls share all of it.
 *
 * correlate() computes its row on the host: one lq_host_dot per template and
 * the window's energy.  It needs no GPU.
 *
 * Block calls (k_detector.hip) form every row on the device; no per-sample data
 * comes back.  The kernel appends (t, E, row) of each marked sample -- a row
 * maximum above the threshold, a neighbour of one in the same tile, the first
 * or last sample of the call -- to a device list, and keeps every tile's first
 * and last sample in an array of their own with a word of flags per tile, from
 * which the host fetches those whose neighbour across the seam is above the
 * threshold; the host sorts the records by t and walks them with the same step
 * function correlate() uses.  Between two marked samples the
 * state machine can only count: its timer runs down, and each sample at which
 * the correlators would have run shifts the two stored rows.  Those samples'
 * rows are at most the threshold, so SEEK stays SEEK; FINDMAX cannot be
 * pending, because the sample after a row above the threshold is marked; and
 * the shifted-in rows are never read, because an estimate reads the row at the
 * peak (above the threshold, marked), the row before it (its neighbour, or
 * across a timer gap the row at the previous detection, a neighbour of that
 * peak) and the row after it (its neighbour).  tests/detector_model.py checks
 * this by poisoning the unmarked rows.  A call that marks more samples than
 * the list holds is redone in smaller pieces: the kernel writes the history to
 * the spare buffer and drxy rows are written again with the same values, so a
 * piece can be run twice.
 *
 * Three departures from the reference, all in include/liquid_mi355x.h: E[t] is
 * the sum of its own window (no running accumulator); r_k[t] = 0 where E[t] =
 * 0; reset zeroes both stored rows and the newest one.
 *
 * A sequence longer than LQK_DETECTOR_MAXLEN or a bank wider than
 * LQK_DETECTOR_MAXM runs block calls in a host loop over the mirror.
 */
#include <complex.h>

#include "lq_host.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

#define DET_LIST_DEFAULT (1u << 17)   /* records of the device list */
#define DET_PIECE_MAX (1ull << 26)    /* samples per launch: 2^15 tiles of flags and edge records */
#define DET_FIRST_COPY (16u << 10)    /* bytes of the list fetched with its counter */

enum { DET_SEEK = 0, DET_FINDMAX = 1 };

static unsigned int g_list_cap = 0;   /* tests: liquid_mi355x_detector_set_list_capacity */

struct detector_cccf_s {
    unsigned int n, m;
    float threshold, dphi_step, dphi_max;
    float *dphi;                  /* m */
    float *p;                     /* templates, m rows of n complex values */
    int eligible;
    lq_hist hist;                 /* the last n samples */
    int state;
    unsigned int timer, imax, idetect;
    float *ra, *rb, *row;         /* m each: the two stored rows, scratch for a new one */
    /* device side, from the first block call */
    int dev_ready;
    lq_ctx ctx;
    lq_devbuf xbuf, lbuf, ebuf;   /* staged input, the marked list, the tiles' edge records */
    void *dpt;                    /* templates tap-major, zero padded (lqk_detector) */
    unsigned int list_cap;
    unsigned int *hlist;          /* host copy of the list */
    size_t hlist_words;
    unsigned int *hedge;          /* the edge records fetched */
    size_t hedge_cap;
    unsigned int **order;         /* records sorted by sample */
    size_t order_cap;
    unsigned long long last_piece;
    float *ext;                   /* host loop: hist ++ x */
    size_t ext_cap;
};

/* one detection: the sample's offset in the call and the three estimates */
typedef struct {
    unsigned long long *index;
    float *tau, *dphi, *gamma;
    unsigned int max_det, count;
} det_out;

detector_cccf detector_cccf_create(liquid_float_complex *_s, unsigned int _n, float _threshold, float _dphi_max)
{
    if (_n == 0) LQ_FAIL("error: detector_cccf_create(), sequence length cannot be zero\n");
    if (_threshold <= 0.0f)
        LQ_FAIL("error: detector_cccf_create(), threshold must be greater than zero (0.6 recommended)\n");
    detector_cccf q = (detector_cccf)lq_xmalloc(sizeof(*q));
    q->n = _n;
    q->threshold = _threshold;
    q->dphi_step = 0.8f * M_PI / (float)_n;
    q->m = (unsigned int)(int)ceilf(fabsf(_dphi_max / q->dphi_step));
    if (q->m < 2) q->m = 2;
    q->dphi_max = q->m * q->dphi_step;
    q->dphi = (float *)lq_xmalloc(q->m * sizeof(float));
    q->p = (float *)lq_xmalloc((size_t)q->m * _n * 2 * sizeof(float));
    for (unsigned int k = 0; k < q->m; k++) {
        q->dphi[k] = ((float)k - (float)(q->m - 1) / 2) * q->dphi_step;
        float complex *pk = (float complex *)(q->p + (size_t)k * _n * 2);
        for (unsigned int i = 0; i < _n; i++) pk[i] = conjf(_s[i]) * cexpf(-_Complex_I * q->dphi[k] * i);
    }
    q->eligible = _n <= LQK_DETECTOR_MAXLEN && q->m <= LQK_DETECTOR_MAXM;
    q->ra = (float *)lq_xmalloc(q->m * sizeof(float));
    q->rb = (float *)lq_xmalloc(q->m * sizeof(float));
    q->row = (float *)lq_xmalloc(q->m * sizeof(float));
    lq_hist_init_host(&q->hist, _n, sizeof(liquid_float_complex));
    detector_cccf_reset(q);
    return q;
}

void detector_cccf_destroy(detector_cccf _q)
{
    if (_q->dev_ready) {
        lqrt_sync(_q->ctx.stream);
        lq_devbuf_free(&_q->xbuf);
        lq_devbuf_free(&_q->lbuf);
        lq_devbuf_free(&_q->ebuf);
        lqrt_free(_q->dpt);
        lq_ctx_free(&_q->ctx);
    }
    lq_hist_free(&_q->hist);
    free(_q->dphi);
    free(_q->p);
    free(_q->ra);
    free(_q->rb);
    free(_q->row);
    free(_q->hlist);
    free(_q->hedge);
    free(_q->order);
    free(_q->ext);
    free(_q);
}

void detector_cccf_print(detector_cccf _q)
{
    printf("detector_cccf:\n");
    printf("    sequence length     :   %-u\n", _q->n);
    printf("    threshold           :   %8.4f\n", _q->threshold);
    printf("    maximum carrier     :   %8.4f rad/sample\n", _q->dphi_max);
    printf("    num. correlators    :   %u\n", _q->m);
}

void detector_cccf_reset(detector_cccf _q)
{
    lq_hist_zero(&_q->hist, _q->dev_ready ? _q->ctx.stream : NULL);
    _q->timer = _q->n;
    _q->state = DET_SEEK;
    _q->imax = 0;
    _q->idetect = 0;
    memset(_q->ra, 0, _q->m * sizeof(float));
    memset(_q->rb, 0, _q->m * sizeof(float));
}

unsigned int detector_cccf_get_num_correlators(detector_cccf _q) { return _q->m; }

void detector_cccf_get_templates(detector_cccf _q, liquid_float_complex *_p)
{
    memcpy(_p, _q->p, (size_t)_q->m * _q->n * 2 * sizeof(float));
}

int detector_cccf_device_eligible(detector_cccf _q) { return _q->eligible; }

/* ----------------------------------------------------------------- the state machine */

/* detector_cccf_estimate_offsets (:396-454) with rm = the row before the
 * peak's, r0 = the peak's, rp = the row after it */
static void det_estimate(const detector_cccf q, const float *rm, const float *r0, const float *rp, float *tau,
                         float *dphi)
{
    const unsigned int d = q->idetect;
    const float rm0 = rm[d];
    const float r0m = d == 0 ? r0[d + 1] : r0[d - 1];
    const float r00 = r0[d];
    const float r0p = d == q->m - 1 ? r0[d - 1] : r0[d + 1];
    const float rp0 = rp[d];
    *dphi = q->dphi[d] - q->dphi_step * 0.5f * (r0p - r0m) / (r0p + r0m - 2 * r00);
    float t = 0.5f * (rp0 - rm0) / (rp0 + rm0 - 2 * r00);
    if (t < -0.499f) t = -0.499f;
    if (t > 0.499f) t = 0.499f;
    *tau = t;
}

/* one sample at which the correlators ran (the timer is 0): its row and
 * energy.  Returns 1 at a detection, with the estimates. */
static int det_step(detector_cccf q, const float *row, float E, float *tau, float *dphi, float *gamma)
{
    float rmax = 0.0f;
    for (unsigned int k = 0; k < q->m; k++)
        if (row[k] > rmax) {
            rmax = row[k];
            q->imax = k;
        }
    const float v = row[q->imax];
    int det = 0;
    if (q->state == DET_SEEK) {
        if (v > q->threshold) {
            q->idetect = q->imax;
            q->state = DET_FINDMAX;
        }
    } else if (v > q->rb[q->idetect]) {
        q->idetect = q->imax;
    } else {
        det_estimate(q, q->ra, q->rb, row, tau, dphi);
        *gamma = sqrtf(E / (float)q->n);
        q->state = DET_SEEK;
        q->timer = q->n / 4;
        det = 1;
    }
    /* the rows shift: rb becomes the older one, the new row the newer */
    float *t = q->ra;
    q->ra = q->rb;
    q->rb = t;
    memcpy(q->rb, row, q->m * sizeof(float));
    return det;
}

/* c samples whose rows are not known to the host pass (unmarked: see the file
 * comment): the timer runs down, and each further sample shifts in a row that
 * is never read */
static void det_skip(detector_cccf q, unsigned long long c)
{
    if (c <= q->timer) {
        q->timer -= (unsigned int)c;
        return;
    }
    c -= q->timer;
    q->timer = 0;
    if (c == 1) {
        float *t = q->ra;
        q->ra = q->rb;
        q->rb = t;
    } else {
        memset(q->ra, 0, q->m * sizeof(float));
    }
    memset(q->rb, 0, q->m * sizeof(float));
}

static void det_report(det_out *o, unsigned long long index, float tau, float dphi, float gamma)
{
    if (o->count < o->max_det) {
        if (o->index) o->index[o->count] = index;
        if (o->tau) o->tau[o->count] = tau;
        if (o->dphi) o->dphi[o->count] = dphi;
        if (o->gamma) o->gamma[o->count] = gamma;
    }
    o->count++;
}

/* the row and energy of the window of n samples at w, on the host */
static float det_host_row(const detector_cccf q, const float *w, float *row)
{
    float E;
    lq_host_dot(LQ_RRRF, w, w, 2 * q->n, &E);
    const float den = sqrtf((float)q->n * E);
    for (unsigned int k = 0; k < q->m; k++) {
        float c[2];
        lq_host_dot(LQ_CCCF, q->p + (size_t)k * q->n * 2, w, q->n, c);
        row[k] = E > 0.0f ? sqrtf(c[0] * c[0] + c[1] * c[1]) / den : 0.0f;
    }
    return E;
}

int detector_cccf_correlate(detector_cccf _q, liquid_float_complex _x, float *_tau_hat, float *_dphi_hat,
                            float *_gamma_hat)
{
    void *st = _q->dev_ready ? _q->ctx.stream : NULL;
    const float *w = (const float *)lq_hist_append(&_q->hist, &_x, 1, st) + 2;
    lq_hist_commit(&_q->hist, 1);
    if (_q->timer) {
        _q->timer--;
        return 0;
    }
    const float E = det_host_row(_q, w, _q->row);
    return det_step(_q, _q->row, E, _tau_hat, _dphi_hat, _gamma_hat);
}

/* ----------------------------------------------------------------- block calls */

static void det_scratch(detector_cccf q, size_t nf)
{
    if (nf <= q->ext_cap) return;
    free(q->ext);
    q->ext_cap = nf;
    q->ext = (float *)lq_xmalloc(nf * sizeof(float));
}

/* the host loop: host pointers; rxy NULL or n*m floats on the host.  Rows are
 * formed where the state machine reads them, and everywhere when rxy is wanted */
static void det_block_host(detector_cccf q, const void *x, unsigned long long n, float *rxy, det_out *o)
{
    const size_t H = q->n;
    void *st = q->dev_ready ? q->ctx.stream : NULL;
    det_scratch(q, (H + (size_t)n) * 2);
    memcpy(q->ext, lq_hist_host(&q->hist, st), H * 8);
    memcpy(q->ext + H * 2, x, (size_t)n * 8);
    lq_hist_append(&q->hist, x, (size_t)n, st);
    lq_hist_commit(&q->hist, (size_t)n);
    for (unsigned long long i = 0; i < n; i++) {
        const float *w = q->ext + (i + 1) * 2;   /* the window that ends at sample i */
        float *row = rxy ? rxy + i * q->m : q->row;
        float E = 0.0f;
        if (rxy || q->timer == 0) E = det_host_row(q, w, row);
        if (q->timer) {
            q->timer--;
            continue;
        }
        float tau, dphi, gamma;
        if (det_step(q, row, E, &tau, &dphi, &gamma)) det_report(o, i, tau, dphi, gamma);
    }
}

static void det_device(detector_cccf q)
{
    if (q->dev_ready) return;
    lqrt_require_device("detector_cccf_correlate_block");
    lq_ctx_init(&q->ctx);
    lq_hist_attach(&q->hist);
    if (q->eligible) {
        const size_t np = LQK_DETECTOR_PADLEN(q->n);
        float *pt = (float *)lq_xmalloc(np * q->m * 2 * sizeof(float));   /* zeroed */
        for (unsigned int k = 0; k < q->m; k++)
            for (unsigned int i = 0; i < q->n; i++)
                memcpy(pt + ((size_t)i * q->m + k) * 2, q->p + ((size_t)k * q->n + i) * 2, 2 * sizeof(float));
        q->dpt = lqrt_malloc(np * q->m * 2 * sizeof(float));
        lqrt_h2d(q->dpt, pt, np * q->m * 2 * sizeof(float), q->ctx.stream);
        lqrt_sync(q->ctx.stream);
        free(pt);
    }
    q->dev_ready = 1;
}

static int det_by_sample(const void *a, const void *b)
{
    const unsigned int ta = **(unsigned int *const *)a, tb = **(unsigned int *const *)b;
    return ta < tb ? -1 : ta > tb;
}

/* one launch over dx[0..n): the number of marked samples; up to cap of their
 * records, the per-tile flags and the edge records the flags ask for in
 * q->hlist / q->hedge, q->order pointing at all of them, *nrec their number.
 * The history goes to the spare buffer (no flip here). */
static unsigned int det_launch(detector_cccf q, const void *dx, unsigned long long n, float *drxy, unsigned int cap,
                               unsigned int *nrec)
{
    const size_t rw = 2 + q->m, nt = (size_t)((n + LQK_DETECTOR_TILE - 1) / LQK_DETECTOR_TILE);
    const size_t words = LQK_DETECTOR_LIST_WORDS(q->m, nt, cap), first_rec = LQK_DETECTOR_LIST_HEAD + nt;
    unsigned int *dl = (unsigned int *)lq_devbuf_get(&q->lbuf, words * 4);
    unsigned int *de = (unsigned int *)lq_devbuf_get(&q->ebuf, 2 * nt * rw * 4);
    if (words > q->hlist_words) {
        free(q->hlist);
        q->hlist = (unsigned int *)lq_xmalloc(words * 4);
        q->hlist_words = words;
    }
    lqk_detector(q->n, q->m, q->threshold, q->dpt, lq_hist_dev(&q->hist, q->ctx.stream), dx, n, drxy, dl, cap, de,
                 lq_hist_next(&q->hist), q->ctx.stream);
    /* the counter, the flags and the first records in one copy; the rest if there are more */
    size_t first = first_rec * 4 + DET_FIRST_COPY;
    if (first > words * 4) first = words * 4;
    lqrt_d2h(q->hlist, dl, first, q->ctx.stream);
    lqrt_sync(q->ctx.stream);
    const unsigned int cnt = q->hlist[0];
    if (cnt > cap) return cnt;
    const size_t need = (first_rec + (size_t)cnt * rw) * 4;
    int pending = 0;
    if (need > first) {
        lqrt_d2h((unsigned char *)q->hlist + first, (const unsigned char *)dl + first, need - first, q->ctx.stream);
        pending = 1;
    }
    /* a tile's first / last sample that is not in the list and whose neighbour across the seam has a
     * row maximum above the threshold: its record comes from the edge array */
    const unsigned int *fl = q->hlist + LQK_DETECTOR_LIST_HEAD;
    size_t ne = 0;
    for (size_t b = 0; b + 1 < nt; b++) ne += ((fl[b] & 4u) && !(fl[b + 1] & 2u)) + ((fl[b + 1] & 1u) && !(fl[b] & 8u));
    if (ne > q->hedge_cap) {
        free(q->hedge);
        q->hedge_cap = ne;
        q->hedge = (unsigned int *)lq_xmalloc(ne * rw * 4);
    }
    if ((size_t)cnt + ne > q->order_cap) {
        free(q->order);
        q->order_cap = (size_t)cnt + ne;
        q->order = (unsigned int **)lq_xmalloc(q->order_cap * sizeof(*q->order));
    }
    size_t k = 0;
    for (size_t b = 0; ne && b + 1 < nt; b++) {
        if ((fl[b] & 4u) && !(fl[b + 1] & 2u)) {   /* the next tile's first sample */
            lqrt_d2h(q->hedge + k * rw, de + (2 * (b + 1)) * rw, rw * 4, q->ctx.stream);
            q->order[cnt + k] = q->hedge + k * rw;
            k++;
        }
        if ((fl[b + 1] & 1u) && !(fl[b] & 8u)) {   /* this tile's last sample */
            lqrt_d2h(q->hedge + k * rw, de + (2 * b + 1) * rw, rw * 4, q->ctx.stream);
            q->order[cnt + k] = q->hedge + k * rw;
            k++;
        }
    }
    if (pending || ne) lqrt_sync(q->ctx.stream);
    for (unsigned int i = 0; i < cnt; i++) q->order[i] = q->hlist + first_rec + i * rw;
    *nrec = cnt + (unsigned int)ne;
    return cnt;
}

/* the host pass over one piece of n samples that starts at offset base of the
 * call: q->order[0 .. cnt) are its records */
static void det_walk_list(detector_cccf q, unsigned int cnt, unsigned long long n, unsigned long long base, det_out *o)
{
    qsort(q->order, cnt, sizeof(*q->order), det_by_sample);
    unsigned long long pos = 0;
    for (unsigned int i = 0; i < cnt; i++) {
        const unsigned int *rec = q->order[i];
        const unsigned long long t = rec[0];
        det_skip(q, t - pos);
        pos = t + 1;
        if (q->timer) {
            q->timer--;
            continue;
        }
        float E, tau, dphi, gamma;
        memcpy(&E, rec + 1, 4);
        if (det_step(q, (const float *)(rec + 2), E, &tau, &dphi, &gamma)) det_report(o, base + t, tau, dphi, gamma);
    }
    det_skip(q, n - pos);
}

static void det_block_dev(detector_cccf q, const void *dx, unsigned long long n, float *drxy, det_out *o)
{
    if (n == 0) return;
    det_device(q);
    if (!q->eligible) {
        /* device pointers on an object the kernel does not take: through the host loop */
        const size_t bytes = (size_t)n * 8;
        unsigned char *hx = (unsigned char *)lq_xmalloc(bytes);
        float *hr = drxy ? (float *)lq_xmalloc((size_t)n * q->m * sizeof(float)) : NULL;
        lqrt_d2h(hx, dx, bytes, q->ctx.stream);
        lqrt_sync(q->ctx.stream);
        det_block_host(q, hx, n, hr, o);
        if (drxy) lqrt_h2d(drxy, hr, (size_t)n * q->m * sizeof(float), q->ctx.stream);
        lqrt_sync(q->ctx.stream);
        free(hx);
        free(hr);
        return;
    }
    /* one tile always fits a list of TILE records */
    unsigned int cap = g_list_cap ? g_list_cap : DET_LIST_DEFAULT;
    if (cap < LQK_DETECTOR_TILE) cap = LQK_DETECTOR_TILE;
    /* a stream that was cut keeps its piece from call to call (it doubles after every piece that fits) */
    unsigned long long done = 0, piece = q->last_piece ? q->last_piece : DET_PIECE_MAX;
    while (done < n) {
        if (piece > n - done) piece = n - done;
        if (piece > DET_PIECE_MAX) piece = DET_PIECE_MAX;
        const unsigned char *px = (const unsigned char *)dx + done * 8;
        float *pr = drxy ? drxy + done * q->m : NULL;
        unsigned int nrec = 0;
        const unsigned int cnt = det_launch(q, px, piece, pr, cap, &nrec);
        if (cnt > cap) {   /* redo in pieces that would half fill the list at this density: whole tiles, at least one */
            piece = piece * (cap / 2) / cnt / LQK_DETECTOR_TILE * LQK_DETECTOR_TILE;
            if (piece < LQK_DETECTOR_TILE) piece = LQK_DETECTOR_TILE;
            continue;
        }
        lq_hist_flip(&q->hist);
        det_walk_list(q, nrec, piece, done, o);
        done += piece;
        q->last_piece = piece;
        if (cnt < cap / 4) piece *= 2;   /* room for twice as many */
    }
    if (q->last_piece >= n) q->last_piece = 0;   /* nothing was cut: the next call starts whole again */
}

unsigned int detector_cccf_correlate_block_dev(detector_cccf _q, const liquid_float_complex *_dx,
                                               unsigned long long _n, float *_drxy, unsigned long long *_index,
                                               float *_tau_hat, float *_dphi_hat, float *_gamma_hat,
                                               unsigned int _max_det)
{
    det_out o = {_index, _tau_hat, _dphi_hat, _gamma_hat, _max_det, 0};
    det_block_dev(_q, _dx, _n, _drxy, &o);
    return o.count;
}

unsigned int detector_cccf_correlate_block(detector_cccf _q, liquid_float_complex *_x, unsigned int _n,
                                           unsigned int *_index, float *_tau_hat, float *_dphi_hat,
                                           float *_gamma_hat, unsigned int _max_det)
{
    if (_n == 0) return 0;
    unsigned long long *idx = _index ? (unsigned long long *)lq_xmalloc((size_t)(_max_det ? _max_det : 1) * 8) : NULL;
    det_out o = {idx, _tau_hat, _dphi_hat, _gamma_hat, _max_det, 0};
    if (!_q->eligible) {
        det_block_host(_q, _x, _n, NULL, &o);
    } else {
        det_device(_q);
        const void *dx = lq_call_in(&_q->ctx, &_q->xbuf, _x, (size_t)_n * 8);
        det_block_dev(_q, dx, _n, NULL, &o);   /* synchronises: the staged input is free again */
        _q->ctx.in_busy = 0;
    }
    for (unsigned int i = 0; idx && i < o.count && i < _max_det; i++) _index[i] = (unsigned int)idx[i];
    free(idx);
    return o.count;
}

void detector_cccf_set_stream(detector_cccf _q, void *_s)
{
    det_device(_q);
    lq_ctx_set_stream(&_q->ctx, _s);
}

void detector_cccf_synchronize(detector_cccf _q)
{
    if (_q->dev_ready) lqrt_sync(_q->ctx.stream);
}

unsigned int liquid_mi355x_detector_tile(void) { return LQK_DETECTOR_TILE; }
unsigned int liquid_mi355x_detector_max_len(void) { return LQK_DETECTOR_MAXLEN; }
unsigned int liquid_mi355x_detector_max_correlators(void) { return LQK_DETECTOR_MAXM; }
void liquid_mi355x_detector_set_list_capacity(unsigned int _records) { g_list_cap = _records; }
