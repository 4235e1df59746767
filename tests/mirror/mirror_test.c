/*
 * mirror_test.c -- the streaming history (host/lq_hist.c) and its host mirror
 * (host/lq_small.c) against a plain array model, without a GPU: the runtime
 * calls they make are the memcpy / malloc stand-ins below.  Built with
 * -fsanitize=address,undefined and run by tests/test_mirror.py.
 *
 * For n in {0, 1, 5, 64}, esz in {4, 8} and both allocators (MIRROR: malloc,
 * PINNED: the pinned allocator): more than three capacities of single appends,
 * appends of n, n + 65 and 3n + 200 samples (compaction and growth), a round
 * trip through the device buffers in both directions, and zero.  After every
 * step the n + k samples at the window pointer must equal the model exactly.
 */
#include <stdint.h>

#include "../../liquid-dsp_amd/host/lq_host.h"

/* ---- stand-ins for the runtime */
static long n_sync, n_pin_alloc, n_pin_free, n_dev_alloc, n_dev_free;

void *lq_xmalloc(size_t bytes) { return calloc(1, bytes ? bytes : 1); }
void *lqrt_malloc(size_t bytes)
{
    n_dev_alloc++;
    return calloc(1, bytes ? bytes : 1);
}
void lqrt_free(void *p)
{
    if (p) n_dev_free++;
    free(p);
}
void *lqrt_host_alloc(size_t bytes)
{
    n_pin_alloc++;
    unsigned char *p = (unsigned char *)malloc(bytes ? bytes : 1);
    memset(p, 0xa5, bytes ? bytes : 1);   /* pinned memory comes uninitialised */
    return p;
}
void lqrt_host_free(void *p)
{
    if (p) n_pin_free++;
    free(p);
}
void lqrt_h2d(void *dst, const void *src, size_t bytes, void *stream) { memcpy(dst, src, bytes); }
void lqrt_d2h(void *dst, const void *src, size_t bytes, void *stream) { memcpy(dst, src, bytes); }
void lqrt_memset(void *dst, size_t bytes, void *stream) { memset(dst, 0, bytes); }
void lqrt_sync(void *stream) { n_sync++; }

/* ---- the model: the last n samples of everything appended, oldest first */
#define MAXN 64
#define MAXK (3 * MAXN + 200)
static unsigned char model[MAXN * 8], blk[MAXK * 8];
static size_t N, ESZ;
static uint32_t next_byte = 1;
static const char *where = "";

static void fill(unsigned char *p, size_t bytes)
{
    for (size_t i = 0; i < bytes; i++) {
        next_byte = next_byte * 1664525u + 1013904223u;
        p[i] = (unsigned char)(next_byte >> 24);
    }
}

static void model_push(const unsigned char *x, size_t k)
{
    if (k >= N) {
        memcpy(model, x + (k - N) * ESZ, N * ESZ);
    } else {
        memmove(model, model + k * ESZ, (N - k) * ESZ);
        memcpy(model + (N - k) * ESZ, x, k * ESZ);
    }
}

static void fail(const char *what)
{
    fprintf(stderr, "FAIL n=%zu esz=%zu %s: %s\n", N, ESZ, where, what);
    exit(1);
}

static void expect(int ok, const char *what)
{
    if (!ok) fail(what);
}

/* append k samples of blk: the n + k samples at the pointer, then the window after the commit */
static void append_check(lq_hist *h, size_t k)
{
    fill(blk, k * ESZ);
    const unsigned char *w = lq_hist_append(h, blk, k, NULL);
    expect(memcmp(w, model, N * ESZ) == 0, "window before the appended samples");
    expect(memcmp(w + N * ESZ, blk, k * ESZ) == 0, "appended samples");
    lq_hist_commit(h, k);
    model_push(blk, k);
    expect(memcmp(lq_hist_host(h, NULL), model, N * ESZ) == 0, "window after commit");
}

static void run(size_t n, size_t esz, int mode)
{
    N = n;
    ESZ = esz;
    memset(model, 0, sizeof(model));
    const long pin0 = n_pin_alloc;
    lq_hist h;
    where = "init";
    lq_hist_init(&h, n, esz, mode);
    expect(memcmp(lq_hist_host(&h, NULL), model, n * esz) == 0, "zero initial window");
    expect((n_pin_alloc > pin0) == (mode == LQ_HIST_PINNED), "allocator of the mode");

    where = "single appends";
    const size_t cap = h.m.cap;
    for (size_t i = 0; i < 3 * cap + 7; i++) append_check(&h, 1);

    where = "block appends";
    const size_t ks[3] = {n, n + 65, 3 * n + 200};
    for (int i = 0; i < 3; i++) {
        append_check(&h, ks[i]);
        append_check(&h, 1);
    }
    expect(h.m.cap >= n + 3 * n + 200, "buffer grown");

    where = "host -> device";
    const void *host_win = lq_hist_host(&h, NULL);
    expect(lq_hist_read(&h) == (mode == LQ_HIST_PINNED ? host_win : h.d[h.cur]), "read before the upload");
    unsigned char *dev = (unsigned char *)lq_hist_dev(&h, NULL);
    expect(memcmp(dev, model, n * esz) == 0, "device copy after the upload");
    expect(lq_hist_read(&h) == dev, "read after the upload");

    where = "device -> host";
    /* a device block of 7 samples: the kernel writes the next buffer, then the flip */
    fill(blk, 7 * esz);
    model_push(blk, 7);
    unsigned char *nxt = (unsigned char *)lq_hist_next(&h);
    expect(nxt != dev, "next is the other buffer");
    memcpy(nxt, model, n * esz);
    lq_hist_flip(&h);
    expect(lq_hist_dev(&h, NULL) == nxt && lq_hist_read(&h) == nxt, "next became current");
    const long s0 = n_sync;
    expect(memcmp(lq_hist_host(&h, NULL), model, n * esz) == 0, "host copy after a device block");
    expect(n == 0 || n_sync > s0, "the download waits for the device");
    for (size_t i = 0; i < cap + 3; i++) append_check(&h, 1);

    where = "zero";
    lq_hist_zero(&h, NULL);
    memset(model, 0, sizeof(model));
    expect(memcmp(lq_hist_host(&h, NULL), model, n * esz) == 0, "host window zero");
    expect(memcmp(h.d[0], model, n * esz) == 0 && memcmp(h.d[1], model, n * esz) == 0, "device buffers zero");
    expect(lq_hist_read(&h) == h.d[h.cur], "both sides in step after zero");
    for (size_t i = 0; i < cap + 3; i++) append_check(&h, 1);
    append_check(&h, n + 65);

    lq_hist_free(&h);
}

int main(void)
{
    static const size_t ns[] = {0, 1, 5, 64}, eszs[] = {4, 8};
    for (int mode = LQ_HIST_MIRROR; mode <= LQ_HIST_PINNED; mode++)
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 2; j++) run(ns[i], eszs[j], mode);
    where = "end";
    expect(n_pin_alloc == n_pin_free && n_pin_alloc > 0, "pinned allocations freed");
    expect(n_dev_alloc == n_dev_free, "device allocations freed");
    printf("mirror ok\n");
    return 0;
}
