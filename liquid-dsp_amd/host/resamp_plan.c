/*
 * resamp_plan.c -- the resampler's timing plan (declarations in lq_host.h).
 *
 * The resampler's timing state (tau, b, mu, INTERP/BOUNDARY) evolves
 * independently of the data, so it is tabulated on the host -- a "plan" --
 * and the GPU replays it: entry j = state before input j, K[j] = outputs
 * before input j.  The float32 recurrence visits a finite set of states and
 * is eventually periodic (r = 1.037, npfb = 64: period 1 011 163 inputs);
 * a periodic plan holds the pre-period and period, found once with Brent's
 * cycle detection, and serves every later position.  A direct plan covers
 * just the next nx inputs (short calls, and rates whose period exceeds
 * RS_MAX_PERIOD).  When to build which is the object's policy
 * (host/resamp.c), and so is the upload of the device table.
 *
 * Nothing here touches the runtime or a kernel: the file links with libc and
 * libm alone (tests/plan/plan_test.c does so under the sanitizers).
 */
#include "lq_host.h"

#define RS_MAX_PERIOD (1ull << 25)     /* give up on periodic plans beyond this many inputs */
#define RS_EARLY 4                     /* a cycle may start at any of the first RS_EARLY states */
#define RS_HCK 16                      /* host checkpoints: one per RS_HCK inputs */
#define RS_REC_CAP (1ull << 22)        /* device entries recorded during the period search (<= 64 MB) */
#define RS_D4_MAXOUT (1ull << 26)      /* output plans cover at most this many outputs (128 MB of entries) */

static unsigned int rs_bits(float t)
{
    unsigned int u;
    memcpy(&u, &t, 4);
    return u;
}

static void rs_put(lqk_rs_entry *e, const rs_state *s, unsigned long long K)
{
    e->tau = s->tau;
    e->mu = s->mu;
    e->bst = (int)((unsigned int)s->b * 2u + (unsigned int)s->st);   /* b wraps modulo 2^32 on a dying orbit (rs_due) */
    e->K = (unsigned int)K;
}

static rs_state rs_get(const lqk_rs_entry *e)
{
    rs_state s = {e->tau, e->mu, e->bst >> 1, e->bst & 1};
    return s;
}

/* ---- device-table recording: a table as a walk records it, n entries of
 * esz bytes at buf; the finished one moves into the plan (rs_plan_device) */
typedef struct {
    int kind;                     /* RS_D3 or RS_D4 */
    unsigned char *buf;
    size_t n, cap, esz, max;
    int overflow;                 /* more than `max` entries were due */
    int d4_ok;                    /* RS_D4: the outputs keep the shape k_resamp4 steps through (rs_rec4_shape) */
    unsigned int zr;              /* RS_D4: silent inputs in a row */
    unsigned long long opre;      /* RS_D4: outputs 0, 4, .. below opre, then opre, opre + 4, .. */
    unsigned long long kmax;      /* RS_D4: ... below kmax */
} rs_rec;

static void rs_rec_init(rs_rec *r, int kind, int p2, size_t max)
{
    free(r->buf);
    memset(r, 0, sizeof(*r));
    r->kind = kind;
    r->esz = kind == RS_D4 ? sizeof(lqk_rs4_entry) : (p2 ? sizeof(lqk_rs_entry_p2) : sizeof(lqk_rs_entry));
    r->max = max;
    r->d4_ok = 1;
    r->opre = ~0ull;
    r->kmax = ~0ull;
}

static void *rs_rec_push(rs_rec *r)
{
    if (r->n >= r->max) {
        r->overflow = 1;
        return NULL;
    }
    if (r->n == r->cap) {
        size_t c = r->cap ? r->cap * 2 : 4096;
        unsigned char *b = (unsigned char *)lq_xmalloc(c * r->esz);
        if (r->buf) memcpy(b, r->buf, r->n * r->esz);
        free(r->buf);
        r->buf = b;
        r->cap = c;
    }
    return r->buf + (r->n++) * r->esz;
}

/* RS_D3 checkpoint before input i (i a multiple of LQK_RS_CK): tau-only / full state */
static void rs_rec3_p2(rs_rec *r, float tau, unsigned long long K)
{
    lqk_rs_entry_p2 *e = (lqk_rs_entry_p2 *)rs_rec_push(r);
    if (e) {
        e->tau = tau;
        e->K = (unsigned int)K;
    }
}

static void rs_rec3(rs_rec *r, const rs_state *s, unsigned long long K)
{
    lqk_rs_entry *e = (lqk_rs_entry *)rs_rec_push(r);
    if (e) rs_put(e, s, K);
}

/* RS_D4: output K, due at tau on input i, is recorded if it is one of the table's */
static inline void rs_rec4_output(rs_rec *r, unsigned long long K, float tau, unsigned long long i)
{
    if (K < r->kmax && ((K < r->opre ? K : K - r->opre) & 3) == 0) {
        lqk_rs4_entry *e = (lqk_rs4_entry *)rs_rec_push(r);
        if (e) {
            e->tau = tau;
            e->i = (unsigned int)i;
        }
    }
}

/* RS_D4: input i emitted c outputs, K so far.  k_resamp4 steps from an entry
 * to the next three outputs in straight-line code, which holds one or two
 * outputs per input (1/2 <= del <= 1; past r = 2 any count works, the
 * kernel's R4 class) or an output every one or two (1 < del < 2) / two to
 * four (2 <= del < 4) inputs once outputs began */
static inline void rs_rec4_shape(rs_rec *r, float del, unsigned int c, unsigned long long K, unsigned long long i)
{
    if (del <= 1.0f) {
        if ((del >= 0.5f && c > 2) || (c == 0 && K > 0)) r->d4_ok = 0;
    } else {
        r->zr = c == 0 && K > 0 ? r->zr + 1 : 0;
        if (c > 1 || r->zr > (del >= 2.0f ? 3u : 1u)) r->d4_ok = 0;
    }
    if (i > 0xffffffffull) r->d4_ok = 0;
}

/* Power-of-two banks: tau*npfb is exact, so the state before an input is a
 * function of tau alone -- b < npfb <=> tau < 1, the INTERP check b == npfb-1
 * <=> tau in [1 - 1/npfb, 1), BOUNDARY <=> tau < 0 (b = 0), and mu =
 * frac(tau*npfb) equals the fraction of the last update (tau then differed by
 * whole samples).  One input is then: add del until tau reaches z = 1 -
 * 1/npfb, subtract 1 (the same float32 operations as rs_step, in the same
 * order).  With r4, the output plan's entries are recorded on the way: K
 * outputs came before this input, which is input i. */
static inline unsigned int rs_step_p2_rec(float *t, float del, float z, rs_rec *r4, unsigned long long K,
                                          unsigned long long i)
{
    float x = *t;
    unsigned int n = 0;
    while (x < z) {
        if (r4) rs_rec4_output(r4, K + n, x, i);
        x += del;
        n++;
    }
    *t = x - 1.0f;
    return n;
}

static inline unsigned int rs_step_p2(float *t, float del, float z) { return rs_step_p2_rec(t, del, z, NULL, 0, 0); }

static rs_state rs_from_tau(float tau, unsigned int npfb)
{
    rs_state s;
    const float bf = tau * (float)npfb, fb = floorf(bf);
    s.tau = tau;
    s.mu = bf - fb;
    s.st = tau < 0.0f ? RS_BOUNDARY : RS_INTERP;
    s.b = s.st == RS_INTERP ? (int)fb : 0;
    return s;
}

/* the tau-only form needs a power-of-two bank count and del >= 1/npfb: then
 * tau >= 0 after every update (a BOUNDARY update adds del to a tau in
 * [-1/npfb, 0), exactly) and b never goes negative.  Rates above npfb keep
 * the full state, whose unsigned loop test stops a negative b (rs_due). */
int rs_tau_only(float del, unsigned int npfb) { return (npfb & (npfb - 1)) == 0 && del * (float)npfb >= 1.0f; }

unsigned long long rs_count_outputs(rs_state s, float del, unsigned int npfb, unsigned long long nx)
{
    unsigned long long total = 0;
    if (rs_tau_only(del, npfb)) {
        const float z = 1.0f - 1.0f / (float)npfb;
        float t = s.tau;
        for (; nx > 0; nx--) total += rs_step_p2(&t, del, z);
    } else {
        for (; nx > 0; nx--) total += rs_step(&s, del, npfb);
    }
    return total;
}

/* ---- host checkpoints */
static void rs_plan_ckpt(rs_plan *pl, const rs_state *s, unsigned long long K)
{
    if (pl->nck == pl->cap) {
        const size_t c = pl->cap ? pl->cap * 2 : 1024;
        lqk_rs_entry *t = (lqk_rs_entry *)lq_xmalloc(c * sizeof(lqk_rs_entry));
        if (pl->tab) memcpy(t, pl->tab, pl->nck * sizeof(lqk_rs_entry));
        free(pl->tab);
        pl->tab = t;
        pl->cap = c;
    }
    rs_put(&pl->tab[pl->nck++], s, K);
}

/* state and K at position j inside the recorded walk (no period wrap): the
 * host checkpoint at or before j, then the remaining (< RS_HCK) inputs stepped */
static rs_state rs_plan_lin(const rs_plan *pl, unsigned long long j, unsigned long long *K)
{
    const lqk_rs_entry *e = &pl->tab[j / RS_HCK];
    rs_state s = rs_get(e);
    unsigned long long k = e->K;
    for (unsigned long long i = j & ~(unsigned long long)(RS_HCK - 1); i < j; i++) k += rs_step(&s, pl->del, pl->npfb);
    *K = k;
    return s;
}

static unsigned long long rs_K_lin(const rs_plan *pl, unsigned long long j)
{
    unsigned long long K;
    rs_plan_lin(pl, j, &K);
    return K;
}

rs_state rs_plan_at(const rs_plan *pl, unsigned long long g, unsigned long long *K)
{
    unsigned long long j = g, add = 0;
    if (g > pl->end) j = pl->end;
    if (j >= pl->pre) {
        unsigned long long t = j - pl->pre, c = t / pl->P;
        j = pl->pre + (t - c * pl->P);
        add = c * pl->Q;
    }
    const rs_state s = rs_plan_lin(pl, j, K);
    *K += add;
    return s;
}

/* ---- the walk: n inputs from the plan's origin, a host checkpoint every
 * RS_HCK inputs (from the plan's first) and, with rec, the device table:
 * RS_D3 a checkpoint every LQK_RS_CK inputs, RS_D4 the (tau, input) of every
 * fourth output.  With `early` set it stops as soon as the state returns to
 * one it has kept. */
enum { RS_HIT_NONE = 0, RS_HIT_EARLY, RS_HIT_TORTOISE };
typedef struct {
    unsigned long long n;     /* inputs walked: where it stopped (0: K does not fit the table's 32 bits) */
    unsigned long long K;     /* their outputs */
    int hit;
    unsigned long long q0;    /* RS_HIT_EARLY: the state at n is the state at q0 < RS_EARLY */
    unsigned long long lam;   /* RS_HIT_TORTOISE: ... is the state lam inputs before: a cycle of length lam */
} rs_walked;

/* tau-only cycle detection: every state is compared (branch-free) with the
 * first and with Brent's tortoise, the state at position 2^k - 1 (and the
 * first RS_EARLY states with each other): a pure cycle ends the walk on its
 * first return, any other once the tortoise sits on the cycle (r = 1.037:
 * 1 011 163 steps) */
typedef struct {
    unsigned int eb[RS_EARLY], tort;
    unsigned long long tpos, reset;
} rs_cycle;

static inline int rs_cycle_hit(rs_cycle *c, unsigned long long i, unsigned int tb, rs_walked *w)
{
    if (i < RS_EARLY) {
        for (unsigned long long k = 0; k < i; k++)
            if (c->eb[k] == tb) {
                w->hit = RS_HIT_EARLY;
                w->q0 = k;
                return 1;
            }
        c->eb[i] = tb;
    } else if ((tb == c->eb[0]) | (tb == c->tort)) {
        w->hit = RS_HIT_TORTOISE;
        w->lam = i - c->tpos;
        for (unsigned long long k = 0; k < RS_EARLY; k++)
            if (c->eb[k] == tb) {
                w->hit = RS_HIT_EARLY;
                w->q0 = k;
            }
        return 1;
    }
    if (i == c->reset) {   /* the tortoise moves to position 2^k - 1 */
        c->tort = tb;
        c->tpos = i;
        c->reset = 2 * i + 1;
    }
    return 0;
}

/* rk: the kind of table recorded into rec (0: none).  rs_walk_p2 below
 * instantiates this walker once per kind, so r3 / r4 (and rs_step_p2_rec's
 * test of its rec) are constants at build time and each hot loop carries
 * only its own recording */
static inline __attribute__((always_inline)) rs_walked rs_walk_p2_rk(rs_plan *pl, unsigned long long n, int early,
                                                                     rs_rec *rec, const int rk)
{
    const float del = pl->del, z = 1.0f - 1.0f / (float)pl->npfb;
    const int r3 = rk == RS_D3, r4 = rk == RS_D4;
    rs_walked w = {0, 0, RS_HIT_NONE, 0, 0};
    rs_cycle cyc = {{0}, rs_bits(pl->origin.tau), 0, 1};
    float t = pl->origin.tau;
    unsigned long long K = 0, i = 0;
    for (;;) {   /* i: a multiple of RS_HCK, or n */
        if ((i & (RS_HCK - 1)) == 0) {
            const rs_state s = i == 0 ? pl->origin : rs_from_tau(t, pl->npfb);
            rs_plan_ckpt(pl, &s, K);
        }
        if (K > 0xffffffffull || i == n) break;
        /* the hot loop: up to the next host checkpoint */
        const unsigned long long stop = n - i < RS_HCK ? n : i + RS_HCK;
        for (; i < stop; i++) {
            if (early && rs_cycle_hit(&cyc, i, rs_bits(t), &w)) {
                w.n = i;
                w.K = K;
                return w;
            }
            if (r3 && (i & (LQK_RS_CK - 1)) == 0) rs_rec3_p2(rec, t, K);
            if (r4) {
                const unsigned int c = rs_step_p2_rec(&t, del, z, rec, K, i);
                K += c;
                rs_rec4_shape(rec, del, c, K, i);
            } else {
                K += rs_step_p2(&t, del, z);
            }
        }
    }
    if (r3 && (i & (LQK_RS_CK - 1)) == 0) rs_rec3_p2(rec, t, K);   /* the checkpoint at the end */
    w.n = K > 0xffffffffull ? 0 : i;
    w.K = K;
    return w;
}

static rs_walked rs_walk_p2(rs_plan *pl, unsigned long long n, int early, rs_rec *rec)
{
    if (rec && rec->kind == RS_D3) return rs_walk_p2_rk(pl, n, early, rec, RS_D3);
    if (rec && rec->kind == RS_D4) return rs_walk_p2_rk(pl, n, early, rec, RS_D4);
    return rs_walk_p2_rk(pl, n, early, NULL, 0);
}

/* full state: the early stop is a return to one of the first RS_EARLY states */
static rs_walked rs_walk_full(rs_plan *pl, unsigned long long n, int early, rs_rec *rec)
{
    const int r3 = rec && rec->kind == RS_D3;
    rs_walked w = {0, 0, RS_HIT_NONE, 0, 0};
    rs_state s = pl->origin, e[RS_EARLY];
    int ne = 0;
    unsigned long long K = 0, i = 0;
    for (;;) {
        if ((i & (RS_HCK - 1)) == 0) rs_plan_ckpt(pl, &s, K);
        if (r3 && (i & (LQK_RS_CK - 1)) == 0) rs_rec3(rec, &s, K);
        if (K > 0xffffffffull || i == n) break;
        if (early) {
            for (int k = 0; k < ne; k++)
                if (rs_eq(&e[k], &s)) {
                    w.hit = RS_HIT_EARLY;
                    w.q0 = (unsigned long long)k;
                    w.n = i;
                    w.K = K;
                    return w;
                }
            if (ne < RS_EARLY) e[ne++] = s;
        }
        K += rs_step(&s, pl->del, pl->npfb);
        i++;
    }
    w.n = K > 0xffffffffull ? 0 : i;
    w.K = K;
    return w;
}

static rs_walked rs_walk(rs_plan *pl, unsigned long long n, int early, rs_rec *rec)
{
    pl->nck = 0;
    return pl->p2 ? rs_walk_p2(pl, n, early, rec) : rs_walk_full(pl, n, early, rec);
}

/* ---- the device table of a plan whose host part (origin, pre, P, Q or end)
 * is built.  Either kind reuses what the walk before already recorded where
 * that is the table (r = 1.037: a second walk of a million inputs saved). */

/* a walk of n inputs that records the device table (at most max entries; an
 * output plan's entries at outputs 0, 4, .. below opre and opre, opre + 4, ..
 * below kmax; the host checkpoints it rewrites are the ones recorded before,
 * same origin); 0 if the walk or an output plan's shape check fails */
static int rs_rec_walk(rs_plan *pl, rs_rec *r, unsigned long long n, int kind, size_t max, unsigned long long opre,
                       unsigned long long kmax)
{
    rs_rec_init(r, kind, pl->p2, max);
    r->opre = opre;
    r->kmax = kmax;
    if (rs_walk(pl, n, 0, r).n != n) return 0;
    return kind != RS_D4 || r->d4_ok;
}

static int rs_table_out(rs_plan *pl, rs_rec *r)
{
    if (!(r->kind == RS_D4 && r->d4_ok)) return 0;
    if (!pl->periodic) {
        pl->opre = ~0ull;
        pl->npre = 0;
        pl->QT = pl->PT = 0;
        return !r->overflow;
    }
    /* entries at outputs 0, 4, .. below opre = K(pre), then opre, opre + 4, ..
     * over one period of QT = mQ outputs (mP inputs), QT >= 256 so a
     * 256-output tile wraps at most once.  A pure cycle (pre = 0) with
     * Q >= 256 is exactly what the search walk recorded */
    const unsigned long long Q = pl->Q;
    unsigned long long m = 1;
    while (Q > 0 && m * Q < 256) m++;
    pl->opre = rs_K_lin(pl, pl->pre);
    pl->npre = (pl->opre + 3) / 4;
    pl->QT = m * Q;
    pl->PT = m * pl->P;
    const unsigned long long need = pl->npre + (pl->QT + 3) / 4;
    if (Q == 0 || need > RS_D4_MAXOUT / 4) return 0;
    if (!(pl->opre == 0 && m == 1 && r->n >= need) &&
        !rs_rec_walk(pl, r, pl->pre + m * pl->P + 1, RS_D4, (size_t)need, pl->opre, pl->opre + pl->QT))
        return 0;
    if (r->n < need) return 0;
    r->n = need;
    return 1;
}

static int rs_table_in(rs_plan *pl, rs_rec *r)
{
    const unsigned long long n = pl->periodic ? pl->pre + pl->P : pl->end;
    const size_t need = (size_t)(n / LQK_RS_CK + 1);
    if (!(r->kind == RS_D3 && r->n >= need) && !rs_rec_walk(pl, r, n, RS_D3, need, ~0ull, ~0ull)) return 0;
    if (r->n < need) return 0;
    r->n = need;
    return 1;
}

/* the recording ends here: the table moves into the plan, or is freed */
static int rs_plan_device(rs_plan *pl, rs_rec *r)
{
    pl->dk = rs_table_out(pl, r) ? RS_D4 : (rs_table_in(pl, r) ? RS_D3 : 0);
    if (pl->dk) {
        pl->dtab = r->buf;
        pl->dn = r->n;
        pl->desz = r->esz;
    } else {
        free(r->buf);
    }
    r->buf = NULL;
    return pl->dk != 0;
}

/* ---- building */
void rs_plan_init(rs_plan *pl) { memset(pl, 0, sizeof(*pl)); }

void rs_plan_drop_table(rs_plan *pl)
{
    free(pl->dtab);
    pl->dtab = NULL;
    pl->dn = 0;
}

void rs_plan_free(rs_plan *pl)
{
    rs_plan_drop_table(pl);
    free(pl->tab);
    pl->tab = NULL;
    pl->cap = pl->nck = 0;
    pl->valid = 0;
}

/* a build starts here; returns the kind of table to record: an output plan
 * only with tau-only timing */
static int rs_plan_begin(rs_plan *pl, float del, unsigned int npfb, rs_state origin, int want_d4)
{
    pl->del = del;
    pl->npfb = npfb;
    pl->p2 = rs_tau_only(del, npfb);
    pl->origin = origin;
    pl->valid = 0;
    rs_plan_drop_table(pl);
    return want_d4 && pl->p2 ? RS_D4 : RS_D3;
}

/* Brent's cycle detection on the full state: the cycle's length, 0 beyond RS_MAX_PERIOD */
static unsigned long long rs_brent(const rs_plan *pl)
{
    rs_state tort = pl->origin, hare = pl->origin;
    unsigned long long power = 1, lam = 1;
    rs_step(&hare, pl->del, pl->npfb);
    while (!rs_eq(&tort, &hare)) {
        if (power == lam) {
            if (power > RS_MAX_PERIOD) return 0;
            tort = hare;
            power *= 2;
            lam = 0;
        }
        rs_step(&hare, pl->del, pl->npfb);
        lam++;
    }
    return lam;
}

/* pre-period of a cycle of length lam: one copy lam steps ahead, both walked
 * until they meet; 0 beyond RS_MAX_PERIOD */
static int rs_preperiod(const rs_plan *pl, unsigned long long lam, unsigned long long *pre)
{
    unsigned long long mu = 0;
    if (pl->p2) {
        const float z = 1.0f - 1.0f / (float)pl->npfb;
        float a = pl->origin.tau, h = pl->origin.tau;
        for (unsigned long long i = 0; i < lam; i++) rs_step_p2(&h, pl->del, z);
        while (memcmp(&a, &h, 4) != 0) {
            if (mu > RS_MAX_PERIOD) return 0;
            rs_step_p2(&a, pl->del, z);
            rs_step_p2(&h, pl->del, z);
            mu++;
        }
    } else {
        rs_state tort = pl->origin, hare = pl->origin;
        for (unsigned long long i = 0; i < lam; i++) rs_step(&hare, pl->del, pl->npfb);
        while (!rs_eq(&tort, &hare)) {
            if (mu > RS_MAX_PERIOD) return 0;
            rs_step(&tort, pl->del, pl->npfb);
            rs_step(&hare, pl->del, pl->npfb);
            mu++;
        }
    }
    *pre = mu;
    return 1;
}

/* The timing state visits a finite set, so the walk is eventually periodic;
 * usually the orbit returns to one of its first states (r = 1.037: to the
 * initial state after 1 011 163 inputs), found in one pass that records the
 * checkpoints as it goes.  Otherwise Brent's cycle detection finds pre-period
 * and period -- the tau-only walk's tortoise on the way, and the walk then
 * already covers both; else on the full state, and a second pass records them. */
int rs_plan_build_periodic(rs_plan *pl, float del, unsigned int npfb, rs_state origin, int want_d4)
{
    const int kind = rs_plan_begin(pl, del, npfb, origin, want_d4);
    rs_rec rec = {0};
    rs_rec_init(&rec, kind, pl->p2, RS_REC_CAP);
    const rs_walked w = rs_walk(pl, RS_MAX_PERIOD + RS_EARLY, 1, &rec);
    if (w.hit == RS_HIT_EARLY) {
        pl->pre = w.q0;
        pl->P = w.n - w.q0;
    } else {
        pl->P = w.hit == RS_HIT_TORTOISE ? w.lam : rs_brent(pl);
        if (pl->P == 0 || !rs_preperiod(pl, pl->P, &pl->pre)) goto fail;
        if (w.hit == RS_HIT_NONE) {
            rs_rec_init(&rec, kind, pl->p2, RS_REC_CAP);
            if (rs_walk(pl, pl->pre + pl->P, 0, &rec).n != pl->pre + pl->P) goto fail;
        }
    }
    pl->end = ~0ull;
    pl->Q = rs_K_lin(pl, pl->pre + pl->P) - rs_K_lin(pl, pl->pre);
    pl->periodic = 1;
    if (!rs_plan_device(pl, &rec)) goto fail;
    pl->valid = 1;
    return 1;
fail:
    free(rec.buf);
    rs_plan_free(pl);   /* the search's host checkpoints too (up to RS_MAX_PERIOD / RS_HCK entries) */
    return 0;
}

int rs_plan_build_direct(rs_plan *pl, float del, unsigned int npfb, rs_state origin, unsigned long long nx,
                         int want_d4)
{
    /* an output plan is capped at RS_D4_MAXOUT outputs (past it an input plan is recorded instead) */
    const int kind = rs_plan_begin(pl, del, npfb, origin, want_d4);
    rs_rec rec = {0};
    rs_rec_init(&rec, kind, pl->p2, kind == RS_D4 ? RS_D4_MAXOUT / 4 : (size_t)-1);
    const rs_walked w = rs_walk(pl, nx, 0, &rec);
    pl->pre = nx + 1;
    pl->P = 1;
    pl->Q = 0;
    pl->end = nx;
    pl->periodic = 0;
    int ret = 1;
    if (w.n != nx || w.K > 0xffffffffull) {
        free(rec.buf);
        ret = 0;
    } else if (!rs_plan_device(pl, &rec)) {
        ret = -1;
    }
    if (ret == 1) pl->valid = 1;
    else rs_plan_free(pl);
    return ret;
}
