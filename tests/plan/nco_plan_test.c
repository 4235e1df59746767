/*
 * nco_plan_test.c -- host/nco_plan.c on its own (no HIP, libc and libm only):
 * plan lookups and the checkpoint table the device replays from, bit for bit
 * against the recurrence stepped from each plan's origin; pre-period and
 * period checked for what they claim; the period-cap fall-back; orbits that
 * wrap upward and downward.  Built and run by tests/test_nco_plan.py under the
 * address and undefined-behaviour sanitizers.
 */
#include <stdint.h>

#include "../../liquid-dsp_amd/host/lq_host.h"

static int failures;

#define CHECK(c, ...)                                                                              \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            if (failures++ < 20) {                                                                 \
                printf("FAIL %s:%d: ", __FILE__, __LINE__);                                        \
                printf(__VA_ARGS__);                                                               \
                printf("\n");                                                                      \
            }                                                                                      \
        }                                                                                          \
    } while (0)

static uint32_t bits(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

/* every lookup of [0, n) and every table entry against the stepped walk */
static void check_positions(const char *what, const nco_plan *pl, float theta0, float d, unsigned long long n,
                            unsigned long long dense)
{
    float th = theta0;
    const unsigned long long seam = pl->periodic ? pl->pre + pl->P : ~0ull;
    for (unsigned long long g = 0; g < n; g++) {
        /* all of the first `dense` positions, then around every seam and a stride */
        const unsigned long long r = pl->periodic && g >= pl->pre ? (g - pl->pre) % pl->P : g;
        if (g < dense || r < 130 || (pl->periodic && r + 130 >= pl->P) || g % 997 == 0 || g + 130 >= n)
            CHECK(bits(nco_plan_at(pl, g)) == bits(th), "%s: position %llu: %a, stepped %a", what, g, nco_plan_at(pl, g), th);
        if (g % LQK_NCO_CK == 0 && g < seam && g / LQK_NCO_CK < pl->ntab)
            CHECK(bits(pl->tab[g / LQK_NCO_CK]) == bits(th), "%s: table entry %llu", what, g / LQK_NCO_CK);
        th = nco_step_theta(th, d);
    }
}

static void check_direct(float theta0, float d, unsigned long long n)
{
    char what[96];
    snprintf(what, sizeof what, "direct theta0=%g d=%g n=%llu", theta0, d, n);
    nco_plan pl;
    nco_plan_init(&pl);
    CHECK(nco_plan_build_direct(&pl, theta0, d, n) == 1, "%s: build", what);
    CHECK(pl.valid && !pl.periodic && pl.end == n && pl.ntab == n / LQK_NCO_CK + 1, "%s: shape", what);
    check_positions(what, &pl, theta0, d, n + 1, n + 1);
    nco_plan_free(&pl);
}

/* returns pre + P */
static unsigned long long check_periodic(float theta0, float d, int wraps)
{
    char what[96];
    snprintf(what, sizeof what, "periodic theta0=%g d=%g", theta0, d);
    nco_plan pl;
    nco_plan_init(&pl);
    CHECK(nco_plan_build_periodic(&pl, theta0, d, 1ull << 27) == 1, "%s: build", what);
    if (!pl.valid) return 0;
    const unsigned long long pre = pl.pre, P = pl.P;
    CHECK(pl.periodic && P >= 1 && pl.ntab == (pre + P + LQK_NCO_CK - 1) / LQK_NCO_CK, "%s: shape", what);
    /* the phase at pre returns after P steps and not before; the one before pre does not return */
    float a = theta0, before = theta0;
    int up = 0, down = 0;
    for (unsigned long long g = 0; g < pre; g++) {
        before = a;
        a = nco_step_theta(a, d);
    }
    CHECK(bits(a) == bits(pl.th_pre), "%s: th_pre", what);
    float b = a, bb = before;
    for (unsigned long long k = 1; k <= P; k++) {
        const float nb = nco_step_theta(b, d);
        if (d > 0 && nb < b) up = 1;
        if (d < 0 && nb > b) down = 1;
        b = nb;
        bb = nco_step_theta(bb, d);
        if (k < P) CHECK(bits(b) != bits(a), "%s: the phase at pre returns after %llu < P steps", what, k);
    }
    CHECK(bits(b) == bits(a), "%s: the phase at pre does not return after P steps", what);
    if (pre) CHECK(bits(bb) != bits(before), "%s: pre is not minimal", what);
    if (wraps > 0) CHECK(up, "%s: the cycle never wraps upward", what);
    if (wraps < 0) CHECK(down, "%s: the cycle never wraps downward", what);
    check_positions(what, &pl, theta0, d, pre + 2 * P + 5, 70000);
    printf("%s: pre-period %llu, period %llu, %zu table entries\n", what, pre, P, pl.ntab);
    nco_plan_free(&pl);
    return pre + P;
}

static void check_cap(float theta0, float d, unsigned long long span)
{
    nco_plan pl;
    nco_plan_init(&pl);
    const unsigned long long caps[3] = {span - 1, span / 2, 1000};
    for (int i = 0; i < 3; i++) {
        CHECK(nco_plan_build_periodic(&pl, theta0, d, caps[i]) == 0, "cap %llu: a plan of %llu positions", caps[i], span);
        CHECK(!pl.valid && pl.tab == NULL && pl.ntab == 0, "cap %llu: something is left allocated", caps[i]);
    }
    CHECK(nco_plan_build_periodic(&pl, theta0, d, span) == 1 && pl.pre + pl.P == span, "cap %llu: no plan", span);
    /* a failed build over a plan at hand frees it */
    CHECK(nco_plan_build_periodic(&pl, theta0, d, 1000) == 0 && pl.tab == NULL, "failed build keeps a table");
    nco_plan_free(&pl);
}

int main(void)
{
    const float pi32 = (float)NCO_PI;
    /* the step itself: (float)pi is above the double pi and wraps; the wrap is one rounding of a double */
    CHECK(bits(nco_step_theta(pi32, 0.0f)) == bits((float)((double)pi32 - 2 * NCO_PI)), "wrap at (float)pi");
    CHECK(bits(nco_step_theta(-pi32, 0.0f)) == bits((float)(2 * NCO_PI - (double)pi32)), "wrap at -(float)pi");
    CHECK(bits(nco_step_theta(3.0f, 0.1f)) == bits(3.0f + 0.1f), "no wrap below pi");
    CHECK(nco_step_theta(1.0f, 10.0f) > (float)NCO_PI, "one wrap only");
    CHECK(nco_table_index(0.0f) == 0 && nco_table_index(-pi32) == 128 && nco_table_index(1.5707964f) == 64, "index");

    const unsigned long long lens[] = {0, 1, 63, 64, 65, 4096, 100003};
    const float ds[] = {0.0f, 0.1f, -0.7f, 3.0f, 1e-3f, 2.5f, pi32, -pi32, -3.0f};
    for (unsigned i = 0; i < sizeof lens / sizeof *lens; i++)
        for (unsigned j = 0; j < sizeof ds / sizeof *ds; j++) check_direct(0.3f, ds[j], lens[i]);

    const unsigned long long span = check_periodic(0.0f, 0.1f, +1);
    check_periodic(0.3f, 0.0f, 0);
    check_periodic(0.0f, (float)(NCO_PI / 2), +1);
    check_periodic(0.0f, 2.5f, +1);
    check_periodic(0.3f, -3.0f, -1);
    check_periodic(-1.0f, -0.7f, -1);
    check_periodic(0.3f, pi32, +1);
    if (span) check_cap(0.0f, 0.1f, span);

    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("nco plan ok\n");
    return 0;
}
