/*
 * plan_test.c -- the resampler's timing plan (host/resamp_plan.c) against the
 * timing state machine stepped straight from the plan's origin, without a
 * GPU: this file, the module, libc and libm are the whole program.  Built with
 * -fsanitize=address,undefined and run by tests/test_plan_module.py.
 *
 * For every case the reference is rs_step's pieces (lq_host.h) applied input
 * by input from the origin, and three things must equal it bit for bit:
 *   - rs_plan_at(g): state and K at every position g;
 *   - an input table (RS_D3): every entry, at input LQK_RS_CK * c;
 *   - an output table (RS_D4): (tau, input) of every output, from its entry
 *     expanded by k_resamp4's step rule (csrc/k_resamp4.hip).
 * Origins: the initial state and the states 1, 5 and 17 inputs later (an
 * object builds every later direct plan from where the last one ended).
 * Direct plans of 1, 15, 16, 17 and 4099 inputs (both sides of the host
 * checkpoint spacing 16 and of LQK_RS_CK), with lookups past the end, which
 * clamp; periodic plans over pre + P inputs and 1000 more; and a rate whose
 * orbit dies, where the periodic build must fail and leave nothing allocated.
 */
#include <stdint.h>

#include "../../liquid-dsp_amd/host/lq_host.h"

void *lq_xmalloc(size_t bytes) { return calloc(1, bytes ? bytes : 1); }

static char where[128];

static void fail(const char *what, unsigned long long at)
{
    fprintf(stderr, "FAIL %s: %s at %llu\n", where, what, at);
    exit(1);
}

static int same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

static rs_state origin_after(float del, unsigned int npfb, unsigned int skip)
{
    rs_state s = rs_initial;
    for (unsigned int i = 0; i < skip; i++) rs_step(&s, del, npfb);
    return s;
}

/* (tau, input) of output k as k_resamp4 derives it from the table */
static void expand4(const rs_plan *pl, unsigned long long k, float *tau_out, unsigned long long *i_out)
{
    const lqk_rs4_entry *t = (const lqk_rs4_entry *)pl->dtab;
    const float del = pl->del, z = 1.0f - 1.0f / (float)pl->npfb;
    unsigned long long idx = k >> 2, add = 0, skip = k & 3;
    if (k >= pl->opre) {
        const unsigned long long dt = k - pl->opre, c = dt / pl->QT, r = dt - c * pl->QT;
        idx = pl->npre + (r >> 2);
        skip = r & 3;
        add = c * pl->PT;
    }
    if (idx >= pl->dn) fail("output table too short for output", k);
    float tau = t[idx].tau;
    unsigned long long i = t[idx].i + add;
    for (unsigned long long s = 0; s < skip; s++) {
        tau = tau + del;
        if (del > 1.0f) {   /* the emitting input ends */
            tau = tau - 1.0f;
            i++;
        }
        if (!(tau < z)) {
            tau = tau - 1.0f;
            i++;
        }
        for (int e = 0; e < 2 && del >= 2.0f; e++)   /* 2 <= del < 4: up to two more silent inputs */
            if (!(tau < z)) {
                tau = tau - 1.0f;
                i++;
            }
    }
    *tau_out = tau;
    *i_out = i;
}

/* positions 0 .. n of the plan, and every table entry they reach, against the stepped reference */
static void check_plan(const rs_plan *pl, rs_state origin, unsigned long long n)
{
    rs_state s = origin;
    unsigned long long K = 0, nck = 0;
    for (unsigned long long g = 0; g <= n; g++) {
        unsigned long long Kp;
        const rs_state p = rs_plan_at(pl, g, &Kp);
        if (!rs_eq(&p, &s)) fail("rs_plan_at state", g);
        if (Kp != K) fail("rs_plan_at K", g);
        if (pl->dk == RS_D3 && g % LQK_RS_CK == 0 && g / LQK_RS_CK < pl->dn) {
            const size_t c = (size_t)(g / LQK_RS_CK);
            if (pl->p2) {
                const lqk_rs_entry_p2 *e = (const lqk_rs_entry_p2 *)pl->dtab + c;
                if (!same_bits(e->tau, s.tau) || e->K != (unsigned int)K) fail("input table entry", g);
            } else {
                const lqk_rs_entry *e = (const lqk_rs_entry *)pl->dtab + c;
                if (!same_bits(e->tau, s.tau) || !same_bits(e->mu, s.mu) || e->bst != (int)((unsigned int)s.b * 2u + (unsigned int)s.st) ||
                    e->K != (unsigned int)K)
                    fail("input table entry", g);
            }
            nck++;
        }
        if (g == n) break;
        for (; rs_due(&s, pl->npfb); rs_advance(&s, pl->del, pl->npfb), K++)
            if (pl->dk == RS_D4) {
                float tau;
                unsigned long long i;
                expand4(pl, K, &tau, &i);
                if (!same_bits(tau, s.tau) || i != g) fail("output table: output", K);
            }
        rs_end_input(&s, pl->npfb);
    }
    /* an input table covers the whole plan: positions 0 .. end, or 0 .. pre + P */
    if (pl->dk == RS_D3) {
        const unsigned long long span = pl->periodic ? pl->pre + pl->P : pl->end;
        if (pl->dn != span / LQK_RS_CK + 1) fail("input table length", pl->dn);
        if (nck != pl->dn) fail("input table entries not all reached", nck);
    }
}

static const unsigned int skips[] = {0, 1, 5, 17};

static void direct_cases(double rate, unsigned int npfb)
{
    static const unsigned long long nxs[] = {1, 15, 16, 17, 4099};
    const float del = 1.0f / (float)rate;
    for (size_t o = 0; o < 4; o++)
        for (size_t c = 0; c < 5; c++)
            for (int want = 0; want < 2; want++) {
                const rs_state origin = origin_after(del, npfb, skips[o]);
                rs_plan pl;
                rs_plan_init(&pl);
                snprintf(where, sizeof(where), "direct r=%g npfb=%u origin+%u nx=%llu want_d4=%d", rate, npfb,
                         skips[o], nxs[c], want);
                /* an object asks for an output table only below del = 4; it gets one where the timing is tau-only */
                const int d4 = want && del < 4.0f;
                if (rs_plan_build_direct(&pl, del, npfb, origin, nxs[c], d4) != 1) fail("no plan", 0);
                if (!pl.valid || pl.periodic || pl.end != nxs[c]) fail("plan header", 0);
                if (pl.dk != (d4 && rs_tau_only(del, npfb) ? RS_D4 : RS_D3)) fail("table kind", (unsigned long long)pl.dk);
                check_plan(&pl, origin, nxs[c]);
                /* past the end: the state and K at the end */
                unsigned long long Ke, Kp;
                const rs_state e = rs_plan_at(&pl, nxs[c], &Ke);
                for (unsigned long long g = nxs[c] + 1; g < nxs[c] + 40; g++) {
                    const rs_state p = rs_plan_at(&pl, g, &Kp);
                    if (!rs_eq(&p, &e) || Kp != Ke) fail("lookup past the end", g);
                }
                rs_plan_free(&pl);
            }
}

/* dk: the table kind the rate is there to reach */
static void periodic_case(double rate, unsigned int npfb, int dk, long long pre0)
{
    const float del = 1.0f / (float)rate;
    for (size_t o = 0; o < 4; o++) {
        const rs_state origin = origin_after(del, npfb, skips[o]);
        rs_plan pl;
        rs_plan_init(&pl);
        snprintf(where, sizeof(where), "periodic r=%g npfb=%u origin+%u", rate, npfb, skips[o]);
        if (!rs_plan_build_periodic(&pl, del, npfb, origin, rs_tau_only(del, npfb) && del < 4.0f))
            fail("no plan", 0);
        if (!pl.valid || !pl.periodic || pl.P == 0) fail("plan header", 0);
        if (pl.dk != dk) fail("table kind", (unsigned long long)pl.dk);
        if (o == 0 && pre0 >= 0 && pl.pre != (unsigned long long)pre0) fail("pre-period", pl.pre);
        if (dk == RS_D4 && pl.QT < 256) fail("output period below a tile", pl.QT);
        check_plan(&pl, origin, pl.pre + pl.P + 1000);
        printf("%s: pre %llu P %llu Q %llu table %d x %zu\n", where, pl.pre, pl.P, pl.Q, pl.dk, pl.dn);
        rs_plan_free(&pl);
    }
}

int main(void)
{
    direct_cases(1.037, 64);     /* output plan, one or two outputs per input */
    direct_cases(0.3, 64);       /* ... silent inputs */
    direct_cases(0.2, 64);       /* tau-only input table */
    direct_cases(0.8131, 37);    /* full-state input table */
    direct_cases(83.3, 64);      /* the orbit dies (full state: del < 1/npfb) */

    periodic_case(1.5, 64, RS_D4, 0);          /* period 3 outputs, table repeated to QT >= 256 */
    periodic_case(1.037, 64, RS_D4, 0);         /* pure cycle, search recording reused */
    periodic_case(1.00624001, 64, RS_D4, 3);    /* pre-period 3 inputs (none from the later origin) */
    periodic_case(3.7, 64, RS_D4, 864961);      /* pre-period 864 961: Brent's tortoise */
    periodic_case(0.3, 64, RS_D4, -1);         /* silent inputs; a pre-period, period 10 inputs */
    periodic_case(0.2, 64, RS_D3, -1);         /* tau-only input table */
    periodic_case(0.8131, 37, RS_D3, -1);       /* full-state walk, period 5 158 411 inputs */
    periodic_case(1.037, 50, RS_D3, -1);        /* full-state walk */
    periodic_case(1.752, 37, RS_D3, 5);         /* ... pre-period 5 inputs: Brent on the full state, second pass */

    /* r = 83.3: b keeps decreasing, no state returns -- no plan, nothing allocated */
    rs_plan pl;
    rs_plan_init(&pl);
    snprintf(where, sizeof(where), "periodic r=83.3 npfb=64");
    if (rs_plan_build_periodic(&pl, 1.0f / 83.3f, 64, rs_initial, 0)) fail("a period on a dying orbit", pl.P);
    if (pl.valid || pl.tab || pl.dtab) fail("failed build left memory", 0);

    printf("plan ok\n");
    return 0;
}
