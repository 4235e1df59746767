/*
 * lq_hist.c -- the streaming history shared by the host objects (lq_host.h):
 * the device ping-pong pair, and by mode the host mirror (lq_small.c) that
 * push() and the single-sample calls work on.
 */
#include "lq_host.h"

void lq_hist_init(lq_hist *h, size_t n, size_t esz, int mode)
{
    memset(h, 0, sizeof(*h));
    h->mode = mode;
    for (int i = 0; i < 2; i++) h->d[i] = lqrt_malloc((n ? n : 1) * esz);   /* n = 0: a flip stays harmless */
    h->m.n = n;
    h->m.esz = esz;
    if (mode != LQ_HIST_DEV) lq_mirror_init(&h->m, n, esz, mode == LQ_HIST_PINNED);
}

void lq_hist_init_host(lq_hist *h, size_t n, size_t esz)
{
    memset(h, 0, sizeof(*h));
    h->mode = LQ_HIST_MIRROR;
    lq_mirror_init(&h->m, n, esz, 0);
}

void lq_hist_attach(lq_hist *h)
{
    if (h->d[0]) return;
    for (int i = 0; i < 2; i++) h->d[i] = lqrt_malloc((h->m.n ? h->m.n : 1) * h->m.esz);
    h->m.dev_valid = 0;   /* the mirror is authoritative */
}

void lq_hist_free(lq_hist *h)
{
    if (h->d[0]) {
        lqrt_free(h->d[0]);
        lqrt_free(h->d[1]);
    }
    if (h->mode != LQ_HIST_DEV) lq_mirror_free(&h->m);
}

void lq_hist_zero(lq_hist *h, void *stream)
{
    if (h->d[0]) {
        for (int i = 0; i < 2; i++) lqrt_memset(h->d[i], h->m.n * h->m.esz, stream);
        lqrt_sync(stream);
    }
    if (h->mode != LQ_HIST_DEV) lq_mirror_zero(&h->m);
}

void *lq_hist_dev(lq_hist *h, void *stream)
{
    if (h->mode != LQ_HIST_DEV) lq_mirror_need_dev(&h->m, h->d[h->cur], stream);
    return h->d[h->cur];
}

const void *lq_hist_read(lq_hist *h)
{
    if (h->mode == LQ_HIST_PINNED && !h->m.dev_valid) return lq_mirror_ptr(&h->m);
    return h->d[h->cur];
}
