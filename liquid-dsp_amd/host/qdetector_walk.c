/*
 * qdetector_walk.c -- qdetector_cccf's host decisions, free of any GPU
 * dependency (libc and libm alone): the walk over seek-window records, the
 * realignment arithmetic between the seek grid and an aligned frame, and the
 * closed-form estimates of the align stage (src/framing/src/qdetector_cccf.c
 * :373-607).  host/qdetector.c does the device work this module asks for;
 * tests/plan/qdetector_walk_test.c drives it alone.
 *
 * Positions are in ext = carried samples ++ the call's samples (lq_host.h).
 * The reference's counter is ext-length minus base at every sample, so its
 * per-sample machine and this walk visit the same windows:
 *   SEEK   a window completes whenever counter reaches nfft; no detection
 *          moves the grid by nfft/2.
 *   hit    at (window, index): the frame starts index samples into the window
 *          and needs index more samples (none when index == 0: the window is
 *          the frame, and the align stage runs on it at once -- the reference
 *          overruns its buffer there).
 *   ALIGN  when the frame is whole the estimates are formed, the frame is
 *          reported at its last sample, and the grid restarts nfft/2 into the
 *          frame, so the next window is (second half of the frame, the nfft/2
 *          samples after it).
 */
#include "lq_host.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

void qdw_reset(qd_walk *w)
{
    w->state = QDW_SEEK;
    w->counter = w->nfft / 2;
    w->offset = 0;
    w->tau_hat = w->gamma_hat = w->dphi_hat = w->phi_hat = 0.0f;
    w->total = w->base = w->c0 = 0;
}

void qdw_init(qd_walk *w, unsigned int nfft, unsigned int s_len, float s2_sum)
{
    memset(w, 0, sizeof(*w));
    w->nfft = nfft;
    w->s_len = s_len;
    w->s2_sum = s2_sum;
    qdw_reset(w);
    qdw_set_threshold(w, 0.5f);
    qdw_set_range(w, 0.3f);
}

int qdw_set_threshold(qd_walk *w, float threshold)
{
    if (threshold <= 0.0f || threshold > 2.0f) return 0;
    w->threshold = threshold;
    return 1;
}

int qdw_set_range(qd_walk *w, float dphi_max)
{
    if (dphi_max < 0.0f || dphi_max > 0.5f) return 0;
    w->range = (int)(dphi_max * w->nfft / (2 * M_PI));
    if (w->range < 0) w->range = 0;
    return 1;
}

void qdw_begin(qd_walk *w, unsigned long long n)
{
    w->c0 = w->counter;
    w->total = w->c0 + n;
    w->base = 0;
}

int qdw_next(const qd_walk *w, unsigned long long *pos, unsigned long long *count)
{
    const unsigned long long left = w->total - w->base;
    *pos = w->base;
    if (left >= w->nfft) {
        if (w->state == QDW_ALIGN) {
            *count = 1;
            return QDW_DO_ALIGN;
        }
        *count = (left - w->nfft) / (w->nfft / 2) + 1;
        return QDW_DO_SEEK;
    }
    *count = left;
    return QDW_DO_END;
}

int qdw_detects(const qd_walk *w, const qdetector_cccf_record *rec)
{
    return rec->peak > w->threshold && rec->index < w->nfft - w->s_len;
}

unsigned long long qdw_seek(qd_walk *w, const qdetector_cccf_record *rec, unsigned long long nrec)
{
    const unsigned long long h = w->nfft / 2;
    for (unsigned long long k = 0; k < nrec; k++) {
        if (!qdw_detects(w, &rec[k])) continue;
        w->state = QDW_ALIGN;
        w->offset = rec[k].offset;
        w->base += k * h + rec[k].index;
        return k + 1;
    }
    w->base += nrec * h;
    return nrec;
}

void qdw_fit_tau_gamma(float aneg, float a0, float apos, unsigned int nfft, float s2_sum, float *tau, float *gamma)
{
    const float yneg = sqrtf(aneg), y0 = sqrtf(a0), ypos = sqrtf(apos);
    const float a = 0.5f * (ypos + yneg) - y0;
    const float b = 0.5f * (ypos - yneg);
    const float c = y0;
    const float t = -b / (2.0f * a);
    const float g_hat = (a * t * t + b * t + c);
    *tau = t;
    *gamma = g_hat * g_hat / ((float)nfft * s2_sum);
}

float qdw_fit_dphi(unsigned int i0, float vneg, float v0, float vpos, unsigned int nfft)
{
    const float a = 0.5f * (vpos + vneg) - v0;
    const float b = 0.5f * (vpos - vneg);
    const float idx = -b / (2.0f * a);
    const float index = (float)i0 + idx;
    /* the bin index wraps to a negative frequency past nfft/2 */
    return (float)((i0 > nfft / 2 ? index - (float)nfft : index) * 2 * M_PI / (float)nfft);
}

void qdw_align_fit(qd_walk *w, const float rxy[6], unsigned int i0, const float v[6])
{
    qdw_fit_tau_gamma(hypotf(rxy[0], rxy[1]), hypotf(rxy[2], rxy[3]), hypotf(rxy[4], rxy[5]), w->nfft, w->s2_sum,
                      &w->tau_hat, &w->gamma_hat);
    w->dphi_hat = qdw_fit_dphi(i0, hypotf(v[0], v[1]), hypotf(v[2], v[3]), hypotf(v[4], v[5]), w->nfft);
}

unsigned long long qdw_align_finish(qd_walk *w, float mre, float mim)
{
    w->phi_hat = atan2f(mim, mre);
    const unsigned long long end = w->base + w->nfft - 1;
    const unsigned long long idx = end >= w->c0 ? end - w->c0 : ~0ull;
    w->base += w->nfft / 2;
    w->state = QDW_SEEK;
    return idx;
}

void qdw_end(qd_walk *w)
{
    w->counter = (unsigned int)(w->total - w->base);
    w->total = w->base = w->c0 = 0;
}
