/* host/qdetector_walk.c on its own (no HIP): the scenarios written by
 * tests/test_qdetector_walk.py -- window records keyed by their position in the
 * whole stream (preceded by the nfft/2 zeros of a fresh object) and the align
 * stage's scalars keyed by the frame's position, both from the Python model --
 * are fed to the walk across several cuts of the stream into calls, and the
 * windows it consumes, its detections, their indices, the estimates and the
 * carried state are compared with the model's and with the single call's.
 * A position the model never visited answers with a record that would detect:
 * windows computed ahead of a detection must be thrown away. */
#include <stdint.h>

#include "lq_host.h"

typedef struct { unsigned long long pos; qdetector_cccf_record r; } win_t;
typedef struct { unsigned long long pos, idx; unsigned i0; float rxy[6], v[6], mre, mim, est[4]; } det_t;
typedef struct { unsigned long long idx; float est[4]; } got_t;

static unsigned nfft, s_len, NW, ND;
static float s2, thr;
static int range;
static unsigned long long N;
static win_t *W;
static det_t *D;

static float rdf(FILE *f) { uint32_t b; float v; if (fscanf(f, "%u", &b) != 1) exit(2); memcpy(&v, &b, 4); return v; }

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)

/* one pass over the stream cut into calls of `step` samples (0: one call), with
 * one extra cut at `extra` (0: none); chunk: windows per seek launch */
static void run(unsigned long long step, unsigned long long extra, unsigned chunk, got_t *got, unsigned *ngot,
                qd_walk *final)
{
    qd_walk w;
    qdw_init(&w, nfft, s_len, s2);
    qdw_set_threshold(&w, thr);
    w.range = range;
    unsigned long long fed = 0, nwin = 0;
    *ngot = 0;
    qdetector_cccf_record *rec = (qdetector_cccf_record *)malloc(chunk * sizeof(*rec));
    while (fed < N) {
        unsigned long long n = step ? step : N;
        if (n > N - fed) n = N - fed;
        if (extra > fed && extra < fed + n) n = extra - fed;
        const unsigned long long abs0 = fed + nfft / 2 - w.counter;
        qdw_begin(&w, n);
        unsigned long long pos, count;
        int act;
        while ((act = qdw_next(&w, &pos, &count)) != QDW_DO_END) {
            if (act == QDW_DO_SEEK) {
                const unsigned nw = count < chunk ? (unsigned)count : chunk;
                for (unsigned k = 0; k < nw; k++) {
                    const unsigned long long p = abs0 + pos + (unsigned long long)k * (nfft / 2);
                    rec[k] = (qdetector_cccf_record){9.0f, 0, 0, 1.0f};   /* never visited by the model */
                    for (unsigned j = 0; j < NW; j++)
                        if (W[j].pos == p) rec[k] = W[j].r;
                }
                const unsigned long long used = qdw_seek(&w, rec, nw);
                for (unsigned long long k = 0; k < used; k++, nwin++) {
                    if (nwin >= NW) FAIL("step %llu: more windows than the model's %u", step, NW);
                    if (W[nwin].pos != abs0 + pos + k * (nfft / 2))
                        FAIL("step %llu: window %llu at %llu, model %llu", step, nwin, abs0 + pos + k * (nfft / 2),
                             W[nwin].pos);
                }
            } else {
                const det_t *d = NULL;
                for (unsigned j = 0; j < ND; j++)
                    if (D[j].pos == abs0 + pos) d = &D[j];
                if (!d) FAIL("step %llu: align at %llu, which the model never aligned", step, abs0 + pos);
                if (w.offset != W[nwin - 1].r.offset) FAIL("step %llu: coarse offset not carried", step);
                qdw_align_fit(&w, d->rxy, d->i0, d->v);
                const unsigned long long idx = qdw_align_finish(&w, d->mre, d->mim);
                if (idx >= n) FAIL("step %llu: idx %llu outside a call of %llu", step, idx, n);
                got[*ngot].idx = fed + idx;
                got[*ngot].est[0] = w.tau_hat;
                got[*ngot].est[1] = w.gamma_hat;
                got[*ngot].est[2] = w.dphi_hat;
                got[*ngot].est[3] = w.phi_hat;
                (*ngot)++;
            }
        }
        qdw_end(&w);
        if (w.counter == 0 || w.counter >= nfft) FAIL("step %llu: counter %u carried", step, w.counter);
        fed += n;
    }
    if (nwin != NW) FAIL("step %llu: %llu windows, model %u", step, nwin, NW);
    free(rec);
    *final = w;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned nscen;
    if (fscanf(f, "%u", &nscen) != 1) return 2;
    for (unsigned sc = 0; sc < nscen; sc++) {
        if (fscanf(f, "%u %u", &nfft, &s_len) != 2) return 2;
        s2 = rdf(f);
        thr = rdf(f);
        if (fscanf(f, "%d %llu %u", &range, &N, &NW) != 3) return 2;
        W = (win_t *)calloc(NW + 1, sizeof(*W));
        for (unsigned j = 0; j < NW; j++) {
            if (fscanf(f, "%llu", &W[j].pos) != 1) return 2;
            W[j].r.peak = rdf(f);
            if (fscanf(f, "%u %d", &W[j].r.index, &W[j].r.offset) != 2) return 2;
            W[j].r.energy = rdf(f);
        }
        if (fscanf(f, "%u", &ND) != 1) return 2;
        D = (det_t *)calloc(ND + 1, sizeof(*D));
        for (unsigned j = 0; j < ND; j++) {
            if (fscanf(f, "%llu %llu %u", &D[j].pos, &D[j].idx, &D[j].i0) != 3) return 2;
            for (int k = 0; k < 6; k++) D[j].rxy[k] = rdf(f);
            for (int k = 0; k < 6; k++) D[j].v[k] = rdf(f);
            D[j].mre = rdf(f);
            D[j].mim = rdf(f);
            for (int k = 0; k < 4; k++) D[j].est[k] = rdf(f);
        }
        got_t *ref = (got_t *)calloc(ND + 8, sizeof(*ref)), *got = (got_t *)calloc(ND + 8, sizeof(*got));
        unsigned nref, ngot;
        qd_walk wref, wgot;
        run(0, 0, 1u << 20, ref, &nref, &wref);
        if (nref != ND) FAIL("scenario %u: %u detections, model %u", sc, nref, ND);
        for (unsigned j = 0; j < ND; j++) {
            if (ref[j].idx != D[j].idx) FAIL("scenario %u: frame %u at %llu, model %llu", sc, j, ref[j].idx, D[j].idx);
            for (int k = 0; k < 4; k++)
                if (fabsf(ref[j].est[k] - D[j].est[k]) > 1e-6f * fmaxf(1.0f, fabsf(D[j].est[k])))
                    FAIL("scenario %u: frame %u estimate %d: %.9g, model %.9g", sc, j, k, ref[j].est[k], D[j].est[k]);
        }
        /* every cut: calls of 1, of nfft/2 - 1, nfft/2, nfft/2 + 1, and one call that ends inside each align stage */
        const unsigned long long h = nfft / 2;
        const unsigned long long steps[] = {1, h > 1 ? h - 1 : 1, h, h + 1, 0, 0, 0};
        for (unsigned c = 0; c < 4 + (ND ? ND : 0) && c < 7; c++) {
            const unsigned long long extra = c >= 4 ? D[c - 4].idx - (s_len > 2 ? 2 : 0) : 0;
            for (unsigned chunk = 1; chunk <= 5; chunk += 2) {
                run(steps[c], extra, chunk, got, &ngot, &wgot);
                if (ngot != nref || memcmp(got, ref, nref * sizeof(*got)))
                    FAIL("scenario %u cut %u chunk %u: detections differ from the single call's", sc, c, chunk);
                if (wgot.state != wref.state || wgot.counter != wref.counter || wgot.offset != wref.offset ||
                    memcmp(&wgot.tau_hat, &wref.tau_hat, 16))
                    FAIL("scenario %u cut %u chunk %u: carried state differs", sc, c, chunk);
            }
        }
        free(W);
        free(D);
        free(ref);
        free(got);
    }
    /* the closed forms' wrap of the bin index: a peak in the upper half is a negative frequency */
    if (!(qdw_fit_dphi(255, 0.5f, 1.0f, 0.5f, 256) < 0.0f) || !(qdw_fit_dphi(1, 0.5f, 1.0f, 0.5f, 256) > 0.0f))
        FAIL("bin wrap");
    printf("walk ok\n");
    return 0;
}
