/*
 * nco_plan.c -- the oscillator's phase plan.
 *
 * nco_crcf's phase is a float32 recurrence, theta += d_theta and one wrap
 * (nco.c:134-138, 355-361), that does not depend on the samples.  The block
 * kernel (csrc/k_nco.hip) cannot run it serially, so the host tabulates it:
 * one checkpoint per LQK_NCO_CK positions, from which a lane replays at most
 * LQK_NCO_CK - 1 steps.  The state is 32 bits and the map deterministic, so
 * every orbit ends in a cycle; where pre-period and period are short enough
 * one table of pre + P positions serves the orbit for good (the periodic
 * form), otherwise and on the first pass the table covers the next n positions
 * (the direct form).
 *
 * This module makes no runtime or kernel call and links with libc and libm
 * alone (tests/plan/nco_plan_test.c builds it on its own); the object
 * (host/nco.c) decides which form to build and when a plan stays valid.
 */
#include "lq_host.h"

void nco_plan_init(nco_plan *pl) { memset(pl, 0, sizeof(*pl)); }

void nco_plan_free(nco_plan *pl)
{
    free(pl->tab);
    nco_plan_init(pl);
}

/* room for checkpoint c; 0 when out of memory */
static int nco_plan_room(nco_plan *pl, size_t c)
{
    if (c < pl->cap) return 1;
    size_t cap = pl->cap ? pl->cap : 64;
    while (cap <= c) cap *= 2;
    float *t = (float *)realloc(pl->tab, cap * sizeof(float));
    if (!t) return 0;
    pl->tab = t;
    pl->cap = cap;
    return 1;
}

/* the walker passes position g with phase th: record it if a checkpoint */
static inline int nco_plan_record(nco_plan *pl, unsigned long long g, float th)
{
    if (g % LQK_NCO_CK) return 1;
    const size_t c = (size_t)(g / LQK_NCO_CK);
    if (!nco_plan_room(pl, c)) return 0;
    pl->tab[c] = th;
    if (c + 1 > pl->ntab) pl->ntab = c + 1;
    return 1;
}

static void nco_plan_begin(nco_plan *pl, float theta0, float d_theta)
{
    nco_plan_free(pl);
    pl->theta0 = theta0;
    pl->d_theta = d_theta;
}

int nco_plan_build_direct(nco_plan *pl, float theta0, float d_theta, unsigned long long n)
{
    nco_plan_begin(pl, theta0, d_theta);
    float th = theta0;
    for (unsigned long long g = 0;; g++) {
        if (!nco_plan_record(pl, g, th)) {
            nco_plan_free(pl);
            return 0;
        }
        if (g == n) break;
        th = nco_step_theta(th, d_theta);
    }
    pl->end = n;
    pl->valid = 1;
    return 1;
}

int nco_plan_build_periodic(nco_plan *pl, float theta0, float d_theta, unsigned long long cap)
{
    nco_plan_begin(pl, theta0, d_theta);
    /* Brent: the period P, in at most about 3 (pre + P) steps */
    float tort = theta0, hare = nco_step_theta(theta0, d_theta);
    unsigned long long power = 1, P = 1, steps = 1;
    while (!nco_same_bits(tort, hare)) {
        if (power == P) {
            tort = hare;
            power *= 2;
            P = 0;
        }
        hare = nco_step_theta(hare, d_theta);
        P++;
        if (++steps > 4 * cap + 4) return 0;
    }
    if (P > cap) return 0;
    /* the pre-period: two walkers P apart meet at position pre; the leading
     * one passes every position of [0, pre + P] and records the table */
    float lead = theta0, tail = theta0;
    unsigned long long g = 0, pre = 0;
    int ok = 1;
    for (; ok && g < P; g++) {
        ok = nco_plan_record(pl, g, lead);
        lead = nco_step_theta(lead, d_theta);
    }
    while (ok && !nco_same_bits(tail, lead)) {
        if (pre + P >= cap) ok = 0;
        else ok = nco_plan_record(pl, g, lead);
        lead = nco_step_theta(lead, d_theta);
        tail = nco_step_theta(tail, d_theta);
        g++;
        pre++;
    }
    if (!ok) {
        nco_plan_free(pl);
        return 0;
    }
    pl->ntab = (size_t)((pre + P + LQK_NCO_CK - 1) / LQK_NCO_CK);   /* [0, pre + P) */
    pl->pre = pre;
    pl->P = P;
    pl->th_pre = tail;
    pl->end = pre + P - 1;
    pl->periodic = 1;
    pl->valid = 1;
    return 1;
}

unsigned long long nco_plan_reduce(const nco_plan *pl, unsigned long long g)
{
    if (pl->periodic && g >= pl->pre + pl->P) return pl->pre + (g - pl->pre) % pl->P;
    return g;
}

float nco_plan_at(const nco_plan *pl, unsigned long long g)
{
    const unsigned long long p = nco_plan_reduce(pl, g);
    float th = pl->tab[p / LQK_NCO_CK];
    for (unsigned int s = (unsigned int)(p % LQK_NCO_CK); s; s--) th = nco_step_theta(th, pl->d_theta);
    return th;
}
