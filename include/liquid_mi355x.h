/*
 * liquid_mi355x.h -- drop-in replacement for the streaming filter /
 * channelizer subset of liquid-dsp's include/liquid.h (liquid-dsp 1.2.0),
 * executed on AMD Instinct MI355X (gfx950) by hand-written HIP kernels.
 *
 * Every declaration in the "liquid.h subset" sections keeps the reference
 * signature and semantics (create / execute / destroy, opaque handles,
 * unsigned sizes, liquid_float_complex samples, invalid arguments print to
 * stderr and exit(1)).  The line references name the liquid.h declaration
 * each symbol replaces.  A program that only uses these objects compiles
 * against this header unchanged and links -lliquid_mi355x instead of
 * -lliquid.
 *
 * The "extensions" sections are additive (new names): batched and
 * device-pointer entry points, explicit stream control.  liquid.h's per-call
 * granularity (e.g. firpfbch2_crcf_execute = M/2 samples) cannot feed a GPU;
 * the block/batch forms can.  All original symbols still return only after
 * their output is written.
 *
 * There is no CPU fallback: without a usable HIP device every constructor
 * prints an error and exits (same failure style as the reference).  The
 * exceptions are nco_crcf, freqmod and freqdem, whose per-sample interface is
 * host arithmetic: they need the device only from their first block call on.
 */
#ifndef LIQUID_MI355X_H
#define LIQUID_MI355X_H

#ifdef __cplusplus
extern "C" {
#define LIQUID_USE_COMPLEX_H 0
#else
#define LIQUID_USE_COMPLEX_H 1
#endif

/* liquid.h:49-50 */
#define LIQUID_VERSION "1.2.0"
#define LIQUID_VERSION_NUMBER 1002000

/* liquid.h:55-57 */
extern const char liquid_version[];
const char *liquid_libversion(void);
int liquid_libversion_number(void);

/* liquid.h:77-88: C99 complex in C, std::complex<float> in C++ (same layout) */
#if LIQUID_USE_COMPLEX_H == 1
#include <complex.h>
#define LIQUID_DEFINE_COMPLEX(R, C) typedef R _Complex C
#elif defined _GLIBCXX_COMPLEX || defined _LIBCPP_COMPLEX
#define LIQUID_DEFINE_COMPLEX(R, C) typedef std::complex<R> C
#else
#define LIQUID_DEFINE_COMPLEX(R, C) typedef struct { R real; R imag; } C;
#endif
LIQUID_DEFINE_COMPLEX(float, liquid_float_complex);

/* liquid.h:6662 (src/utility/src/msb_index.c:110-135): index of the most
   significant set bit, 1-based (floor(log2 x)+1), 0 for x = 0 */
unsigned int liquid_msb_index(unsigned int _x);

/* liquid.h:5651-5652 */
#define LIQUID_ANALYZER 0
#define LIQUID_SYNTHESIZER 1

/* ------------------------------------------------------------------------ */
/* filter design (liquid.h:1476 kaiser_beta_As, :1548 liquid_firdes_kaiser)  */
/* ------------------------------------------------------------------------ */
float kaiser_beta_As(float _As);
void liquid_firdes_kaiser(unsigned int _n, float _fc, float _As, float _mu, float *_h);
/* liquid.h:1413-1435: prototype filter types */
typedef enum {
    LIQUID_FIRFILT_UNKNOWN = 0,
    LIQUID_FIRFILT_KAISER,
    LIQUID_FIRFILT_PM,
    LIQUID_FIRFILT_RCOS,
    LIQUID_FIRFILT_FEXP,
    LIQUID_FIRFILT_FSECH,
    LIQUID_FIRFILT_FARCSECH,
    LIQUID_FIRFILT_ARKAISER,
    LIQUID_FIRFILT_RKAISER,
    LIQUID_FIRFILT_RRC,
    LIQUID_FIRFILT_hM3,
    LIQUID_FIRFILT_GMSKTX,
    LIQUID_FIRFILT_GMSKRX,
    LIQUID_FIRFILT_RFEXP,
    LIQUID_FIRFILT_RFSECH,
    LIQUID_FIRFILT_RFARCSECH,
} liquid_firfilt_type;
/* liquid.h:1444-1471 */
void liquid_firdes_prototype(liquid_firfilt_type _type, unsigned int _k, unsigned int _m, float _beta, float _dt,
                             float *_h);
int liquid_getopt_str2firfilt(const char *_str);
unsigned int estimate_req_filter_len(float _df, float _As);
float estimate_req_filter_As(float _df, unsigned int _N);
float estimate_req_filter_df(float _As, unsigned int _N);
/* liquid.h:1481-1512: Parks-McClellan (this build designs band-pass filters) */
typedef enum {
    LIQUID_FIRDESPM_BANDPASS = 0,
    LIQUID_FIRDESPM_DIFFERENTIATOR,
    LIQUID_FIRDESPM_HILBERT
} liquid_firdespm_btype;
typedef enum {
    LIQUID_FIRDESPM_FLATWEIGHT = 0,
    LIQUID_FIRDESPM_EXPWEIGHT,
    LIQUID_FIRDESPM_LINWEIGHT,
} liquid_firdespm_wtype;
void firdespm_run(unsigned int _h_len, unsigned int _num_bands, float *_bands, float *_des, float *_weights,
                  liquid_firdespm_wtype *_wtype, liquid_firdespm_btype _btype, float *_h);
/* liquid.h:1573-1605 */
void liquid_firdes_rcos(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
void liquid_firdes_rrcos(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
void liquid_firdes_rkaiser(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
void liquid_firdes_arkaiser(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
float rkaiser_approximate_rho(unsigned int _m, float _beta);
void liquid_firdes_hM3(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
void liquid_firdes_gmsktx(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
void liquid_firdes_gmskrx(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
void liquid_firdes_fexp(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
void liquid_firdes_rfexp(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
void liquid_firdes_fsech(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
void liquid_firdes_rfsech(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
void liquid_firdes_farcsech(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
void liquid_firdes_rfarcsech(unsigned int _k, unsigned int _m, float _beta, float _dt, float *_h);
/* liquid.h:1635-1668 */
float liquid_filter_autocorr(float *_h, unsigned int _h_len, int _lag);
void liquid_filter_isi(float *_h, unsigned int _k, unsigned int _m, float *_rms, float *_max);
/* liquid.h:4396 */
float liquid_Qf(float _z);
/* windows, liquid.h:4425-4465 */
float kaiser(unsigned int _n, unsigned int _N, float _beta, float _mu);
float hamming(unsigned int _n, unsigned int _N);
float hann(unsigned int _n, unsigned int _N);
float blackmanharris(unsigned int _n, unsigned int _N);
float liquid_rcostaper_windowf(unsigned int _n, unsigned int _t, unsigned int _N);
float liquid_kbd(unsigned int _n, unsigned int _N, float _beta);
void liquid_kbd_window(unsigned int _n, float _beta, float *_w);

/* ------------------------------------------------------------------------ */
/* random helpers (liquid.h:6301-6315): test-signal generation on the host   */
/* ------------------------------------------------------------------------ */
float randf(void);
float randnf(void);
void awgn(float *_x, float _nstd);
void crandnf(liquid_float_complex *_y);
void cawgn(liquid_float_complex *_x, float _nstd);

/* ------------------------------------------------------------------------ */
/* window buffers (liquid.h:296-349): the last _n samples, contiguous,       */
/* oldest first.  A host container by contract (read() hands the caller a    */
/* host pointer); the streaming objects below keep their own history on the */
/* device and do not use it.                                                 */
/* ------------------------------------------------------------------------ */
#define LQMI_WINDOW_API(WINDOW, T)                                                              \
    typedef struct WINDOW##_s *WINDOW;                                                          \
    WINDOW WINDOW##_create(unsigned int _n);                                                    \
    WINDOW WINDOW##_recreate(WINDOW _q, unsigned int _n);                                       \
    void WINDOW##_destroy(WINDOW _q);                                                           \
    void WINDOW##_print(WINDOW _q);                                                             \
    void WINDOW##_debug_print(WINDOW _q);                                                       \
    void WINDOW##_clear(WINDOW _q);                                                             \
    void WINDOW##_read(WINDOW _q, T **_v);                                                      \
    void WINDOW##_index(WINDOW _q, unsigned int _i, T *_v);                                     \
    void WINDOW##_push(WINDOW _q, T _v);                                                        \
    void WINDOW##_write(WINDOW _q, T *_v, unsigned int _n);

LQMI_WINDOW_API(windowf, float)
LQMI_WINDOW_API(windowcf, liquid_float_complex)

/* ------------------------------------------------------------------------ */
/* dotprod (liquid.h:503-560): rrrf, crcf, cccf                              */
/* ------------------------------------------------------------------------ */
#define LQMI_DOTPROD_API(DOTPROD, TO, TC, TI)                                                   \
    typedef struct DOTPROD##_s *DOTPROD;                                                        \
    void DOTPROD##_run(TC *_h, TI *_x, unsigned int _n, TO *_y);                                \
    void DOTPROD##_run4(TC *_h, TI *_x, unsigned int _n, TO *_y);                               \
    DOTPROD DOTPROD##_create(TC *_v, unsigned int _n);                                          \
    DOTPROD DOTPROD##_recreate(DOTPROD _q, TC *_v, unsigned int _n);                            \
    void DOTPROD##_destroy(DOTPROD _q);                                                         \
    void DOTPROD##_print(DOTPROD _q);                                                           \
    void DOTPROD##_execute(DOTPROD _q, TI *_v, TO *_y);                                         \
    /* extension: Y[v] = dot(h, X[v*_n .. v*_n+_n)), host pointers */                          \
    void DOTPROD##_execute_batch(DOTPROD _q, TI *_X, unsigned long long _nvec, TO *_Y);         \
    /* extension: same on device pointers, asynchronous on the object's stream */               \
    void DOTPROD##_execute_batch_dev(DOTPROD _q, const TI *_dX, unsigned long long _nvec,       \
                                     TO *_dY);                                                  \
    void DOTPROD##_set_stream(DOTPROD _q, void *_hip_stream);                                   \
    void *DOTPROD##_get_stream(DOTPROD _q);

LQMI_DOTPROD_API(dotprod_rrrf, float, float, float)
LQMI_DOTPROD_API(dotprod_crcf, liquid_float_complex, float, liquid_float_complex)
LQMI_DOTPROD_API(dotprod_cccf, liquid_float_complex, liquid_float_complex, liquid_float_complex)

/* ------------------------------------------------------------------------ */
/* firfilt (liquid.h:1985-2090): rrrf, crcf, cccf                            */
/* ------------------------------------------------------------------------ */
#define LQMI_FIRFILT_API(FIRFILT, TO, TC, TI)                                                   \
    typedef struct FIRFILT##_s *FIRFILT;                                                        \
    FIRFILT FIRFILT##_create(TC *_h, unsigned int _n);                                          \
    FIRFILT FIRFILT##_create_kaiser(unsigned int _n, float _fc, float _As, float _mu);          \
    FIRFILT FIRFILT##_create_rect(unsigned int _n);                                             \
    FIRFILT FIRFILT##_create_rnyquist(int _type, unsigned int _k, unsigned int _m, float _beta, float _mu);\
    FIRFILT FIRFILT##_recreate(FIRFILT _q, TC *_h, unsigned int _n);                            \
    void FIRFILT##_destroy(FIRFILT _q);                                                         \
    void FIRFILT##_reset(FIRFILT _q);                                                           \
    void FIRFILT##_print(FIRFILT _q);                                                           \
    void FIRFILT##_set_scale(FIRFILT _q, TC _scale);                                            \
    void FIRFILT##_push(FIRFILT _q, TI _x);                                                     \
    void FIRFILT##_execute(FIRFILT _q, TO *_y);                                                 \
    void FIRFILT##_execute_block(FIRFILT _q, TI *_x, unsigned int _n, TO *_y);                  \
    unsigned int FIRFILT##_get_length(FIRFILT _q);                                              \
    void FIRFILT##_freqresponse(FIRFILT _q, float _fc, liquid_float_complex *_H);               \
    float FIRFILT##_groupdelay(FIRFILT _q, float _fc);                                          \
    /* extension: device pointers (x == y allowed), asynchronous on the object's stream */      \
    void FIRFILT##_execute_block_dev(FIRFILT _q, const TI *_dx, unsigned long long _n,          \
                                     TO *_dy);                                                  \
    void FIRFILT##_set_stream(FIRFILT _q, void *_hip_stream);                                   \
    void *FIRFILT##_get_stream(FIRFILT _q);                                                     \
    void FIRFILT##_synchronize(FIRFILT _q);

LQMI_FIRFILT_API(firfilt_rrrf, float, float, float)
LQMI_FIRFILT_API(firfilt_crcf, liquid_float_complex, float, liquid_float_complex)
LQMI_FIRFILT_API(firfilt_cccf, liquid_float_complex, liquid_float_complex, liquid_float_complex)

/* ------------------------------------------------------------------------ */
/* firdecim (liquid.h:2664-2735): rrrf, crcf, cccf                           */
/* ------------------------------------------------------------------------ */
#define LQMI_FIRDECIM_API(FIRDECIM, TO, TC, TI)                                                 \
    typedef struct FIRDECIM##_s *FIRDECIM;                                                      \
    FIRDECIM FIRDECIM##_create(unsigned int _M, TC *_h, unsigned int _h_len);                   \
    FIRDECIM FIRDECIM##_create_kaiser(unsigned int _M, unsigned int _m, float _As);             \
    FIRDECIM FIRDECIM##_create_prototype(int _type, unsigned int _M, unsigned int _m, float _beta, float _dt);\
    void FIRDECIM##_destroy(FIRDECIM _q);                                                       \
    void FIRDECIM##_print(FIRDECIM _q);                                                         \
    void FIRDECIM##_clear(FIRDECIM _q);                                                         \
    void FIRDECIM##_execute(FIRDECIM _q, TI *_x, TO *_y);                                       \
    void FIRDECIM##_execute_block(FIRDECIM _q, TI *_x, unsigned int _n, TO *_y);                \
    /* extension: _n = number of outputs; _dx holds _n*M samples (device) */                    \
    void FIRDECIM##_execute_block_dev(FIRDECIM _q, const TI *_dx, unsigned long long _n,        \
                                      TO *_dy);                                                 \
    void FIRDECIM##_set_stream(FIRDECIM _q, void *_hip_stream);

LQMI_FIRDECIM_API(firdecim_rrrf, float, float, float)
LQMI_FIRDECIM_API(firdecim_crcf, liquid_float_complex, float, liquid_float_complex)
LQMI_FIRDECIM_API(firdecim_cccf, liquid_float_complex, liquid_float_complex, liquid_float_complex)

/* ------------------------------------------------------------------------ */
/* firinterp (liquid.h:2496-2565): rrrf, crcf, cccf                          */
/* ------------------------------------------------------------------------ */
#define LQMI_FIRINTERP_API(FIRINTERP, TO, TC, TI)                                               \
    typedef struct FIRINTERP##_s *FIRINTERP;                                                    \
    FIRINTERP FIRINTERP##_create(unsigned int _M, TC *_h, unsigned int _h_len);                 \
    FIRINTERP FIRINTERP##_create_kaiser(unsigned int _M, unsigned int _m, float _As);           \
    FIRINTERP FIRINTERP##_create_prototype(int _type, unsigned int _M, unsigned int _m, float _beta, float _dt);\
    void FIRINTERP##_destroy(FIRINTERP _q);                                                     \
    void FIRINTERP##_print(FIRINTERP _q);                                                       \
    void FIRINTERP##_reset(FIRINTERP _q);                                                       \
    void FIRINTERP##_execute(FIRINTERP _q, TI _x, TO *_y);                                      \
    void FIRINTERP##_execute_block(FIRINTERP _q, TI *_x, unsigned int _n, TO *_y);              \
    /* extension: _n inputs -> _n*M outputs, device pointers */                                 \
    void FIRINTERP##_execute_block_dev(FIRINTERP _q, const TI *_dx, unsigned long long _n,      \
                                       TO *_dy);                                                \
    void FIRINTERP##_set_stream(FIRINTERP _q, void *_hip_stream);

LQMI_FIRINTERP_API(firinterp_rrrf, float, float, float)
LQMI_FIRINTERP_API(firinterp_crcf, liquid_float_complex, float, liquid_float_complex)
LQMI_FIRINTERP_API(firinterp_cccf, liquid_float_complex, liquid_float_complex, liquid_float_complex)

/* ------------------------------------------------------------------------ */
/* firpfb (liquid.h:2392-2486): rrrf, crcf, cccf                             */
/* ------------------------------------------------------------------------ */
#define LQMI_FIRPFB_API(FIRPFB, TO, TC, TI)                                                     \
    typedef struct FIRPFB##_s *FIRPFB;                                                          \
    FIRPFB FIRPFB##_create(unsigned int _M, TC *_h, unsigned int _h_len);                       \
    FIRPFB FIRPFB##_create_kaiser(unsigned int _M, unsigned int _m, float _fc, float _As);      \
    FIRPFB FIRPFB##_create_rnyquist(int _type, unsigned int _M, unsigned int _k, unsigned int _m, float _beta);\
    FIRPFB FIRPFB##_create_drnyquist(int _type, unsigned int _M, unsigned int _k, unsigned int _m, float _beta);\
    FIRPFB FIRPFB##_recreate(FIRPFB _q, unsigned int _M, TC *_h, unsigned int _h_len);          \
    void FIRPFB##_destroy(FIRPFB _q);                                                           \
    void FIRPFB##_print(FIRPFB _q);                                                             \
    void FIRPFB##_set_scale(FIRPFB _q, TC _g);                                                  \
    void FIRPFB##_reset(FIRPFB _q);                                                             \
    void FIRPFB##_push(FIRPFB _q, TI _x);                                                       \
    void FIRPFB##_execute(FIRPFB _q, unsigned int _i, TO *_y);                                  \
    /* extension: push each of _n inputs and evaluate every bank after it:                   */ \
    /* _y[t*M + i] = execute(i) after push(_x[t]); host / device pointers                    */ \
    void FIRPFB##_execute_block(FIRPFB _q, TI *_x, unsigned long long _n, TO *_y);              \
    void FIRPFB##_execute_block_dev(FIRPFB _q, const TI *_dx, unsigned long long _n, TO *_dy);  \
    void FIRPFB##_set_stream(FIRPFB _q, void *_hip_stream);

LQMI_FIRPFB_API(firpfb_rrrf, float, float, float)
LQMI_FIRPFB_API(firpfb_crcf, liquid_float_complex, float, liquid_float_complex)
LQMI_FIRPFB_API(firpfb_cccf, liquid_float_complex, liquid_float_complex, liquid_float_complex)

/* ------------------------------------------------------------------------ */
/* resamp (liquid.h:2938-3015): rrrf, crcf, cccf                            */
/* ------------------------------------------------------------------------ */
#define LQMI_RESAMP_API(RESAMP, T)                                                                  \
    typedef struct RESAMP##_s *RESAMP;                                                              \
    RESAMP RESAMP##_create(float _rate, unsigned int _m, float _fc, float _As, unsigned int _npfb);  \
    RESAMP RESAMP##_create_default(float _rate);                                                    \
    void RESAMP##_destroy(RESAMP _q);                                                               \
    void RESAMP##_print(RESAMP _q);                                                                 \
    void RESAMP##_reset(RESAMP _q);                                                                 \
    unsigned int RESAMP##_get_delay(RESAMP _q);                                                     \
    void RESAMP##_set_rate(RESAMP _q, float _rate);                                                 \
    void RESAMP##_adjust_rate(RESAMP _q, float _delta);                                             \
    void RESAMP##_execute(RESAMP _q, T _x, T *_y, unsigned int *_num_written);                      \
    void RESAMP##_execute_block(RESAMP _q, T *_x, unsigned int _nx, T *_y, unsigned int *_ny);      \
    /* extension: number of outputs the next _nx inputs will produce (size _y with it) */          \
    unsigned long long RESAMP##_num_output(RESAMP _q, unsigned long long _nx);                      \
    /* extension: device pointers, asynchronous on the object's stream; *_ny is                     \
     * known (and written) before the call returns */                                               \
    void RESAMP##_execute_block_dev(RESAMP _q, const T *_dx, unsigned long long _nx, T *_dy,         \
                                    unsigned long long *_ny);                                       \
    void RESAMP##_set_stream(RESAMP _q, void *_hip_stream);                                         \
    void RESAMP##_synchronize(RESAMP _q);

LQMI_RESAMP_API(resamp_rrrf, float)
LQMI_RESAMP_API(resamp_crcf, liquid_float_complex)
LQMI_RESAMP_API(resamp_cccf, liquid_float_complex)

/* ------------------------------------------------------------------------ */
/* fft (liquid.h:1113-1216): plans bind host arrays; the transform runs on   */
/* the GPU.  liquid_nextpow2: liquid.h (math), src/math/src/math.c:143       */
/* ------------------------------------------------------------------------ */
typedef enum {
    LIQUID_FFT_UNKNOWN = 0,
    LIQUID_FFT_FORWARD = +1,
    LIQUID_FFT_BACKWARD = -1,
    LIQUID_FFT_REDFT00 = 10,
    LIQUID_FFT_REDFT10 = 11,
    LIQUID_FFT_REDFT01 = 12,
    LIQUID_FFT_REDFT11 = 13,
    LIQUID_FFT_RODFT00 = 20,
    LIQUID_FFT_RODFT10 = 21,
    LIQUID_FFT_RODFT01 = 22,
    LIQUID_FFT_RODFT11 = 23,
    LIQUID_FFT_MDCT = 30,
    LIQUID_FFT_IMDCT = 31,
} liquid_fft_type;
typedef struct fftplan_s *fftplan;
fftplan fft_create_plan(unsigned int _n, liquid_float_complex *_x, liquid_float_complex *_y, int _dir, int _flags);
fftplan fft_create_plan_r2r_1d(unsigned int _n, float *_x, float *_y, int _type, int _flags);
void fft_destroy_plan(fftplan _p);
void fft_print_plan(fftplan _p);
void fft_execute(fftplan _p);
void fft_run(unsigned int _n, liquid_float_complex *_x, liquid_float_complex *_y, int _dir, int _flags);
void fft_r2r_1d_run(unsigned int _n, float *_x, float *_y, int _type, int _flags);
void fft_shift(liquid_float_complex *_x, unsigned int _n);
unsigned int liquid_nextpow2(unsigned int _x);
/* extension: _batch transforms of the plan's size/direction (contiguous);
 * host arrays or device pointers (asynchronous on the plan's stream) */
void fft_execute_batch(fftplan _p, const void *_x, void *_y, unsigned long long _batch);
void fft_execute_batch_dev(fftplan _p, const void *_dx, void *_dy, unsigned long long _batch);
void fft_set_stream(fftplan _p, void *_hip_stream);

/* ------------------------------------------------------------------------ */
/* spgram (liquid.h:1220-1290): spgramcf (complex in), spgramf (real in)     */
/* ------------------------------------------------------------------------ */
#define LQMI_SPGRAM_API(SPGRAM, TI)                                                                 \
    typedef struct SPGRAM##_s *SPGRAM;                                                              \
    SPGRAM SPGRAM##_create(unsigned int _nfft, float *_window, unsigned int _window_len);          \
    SPGRAM SPGRAM##_create_kaiser(unsigned int _nfft, unsigned int _window_len, float _beta);      \
    SPGRAM SPGRAM##_create_default(unsigned int _nfft);                                             \
    void SPGRAM##_destroy(SPGRAM _q);                                                               \
    void SPGRAM##_reset(SPGRAM _q);                                                                 \
    void SPGRAM##_push(SPGRAM _q, TI _x);                                                           \
    void SPGRAM##_write(SPGRAM _q, TI *_x, unsigned int _n);                                        \
    void SPGRAM##_execute(SPGRAM _q, liquid_float_complex *_X);                                     \
    void SPGRAM##_execute_psd(SPGRAM _q, float *_X);                                                \
    void SPGRAM##_accumulate_psd(SPGRAM _q, TI *_x, float _alpha, unsigned int _n);                 \
    void SPGRAM##_write_accumulation(SPGRAM _q, float *_x);                                         \
    void SPGRAM##_estimate_psd(SPGRAM _q, TI *_x, unsigned int _n, float *_psd);                    \
    /* extensions: device-resident input (and psd output), asynchronous */                          \
    void SPGRAM##_accumulate_psd_dev(SPGRAM _q, const TI *_dx, float _alpha, unsigned long long _n); \
    void SPGRAM##_estimate_psd_dev(SPGRAM _q, const TI *_dx, unsigned long long _n, float *_dpsd);  \
    void SPGRAM##_set_stream(SPGRAM _q, void *_hip_stream);                                         \
    void SPGRAM##_synchronize(SPGRAM _q);

LQMI_SPGRAM_API(spgramcf, liquid_float_complex)
LQMI_SPGRAM_API(spgramf, float)

/* ------------------------------------------------------------------------ */
/* resamp2 (liquid.h:2840-2925), msresamp2 (:3027-3090), msresamp (:3094-3140) */
/* ------------------------------------------------------------------------ */
/* liquid.h:3022-3025 */
typedef enum {
    LIQUID_RESAMP_INTERP = 0,
    LIQUID_RESAMP_DECIM,
} liquid_resamp_type;

/* extension: mode argument of resamp2_*_execute_block[_dev] */
enum {
    LQMI_RESAMP2_FILTER = 0,       /* n calls: x[n] -> y0[n] (low band), y1[n] (high band) */
    LQMI_RESAMP2_ANALYZER,         /* x[2n] -> y0[2n] */
    LQMI_RESAMP2_SYNTHESIZER,      /* x[2n] -> y0[2n] */
    LQMI_RESAMP2_DECIM,            /* x[2n] -> y0[n] */
    LQMI_RESAMP2_INTERP,           /* x[n]  -> y0[2n] */
};

#define LQMI_RESAMP2_API(RESAMP2, T)                                                                \
    typedef struct RESAMP2##_s *RESAMP2;                                                            \
    RESAMP2 RESAMP2##_create(unsigned int _m, float _f0, float _As);                                \
    RESAMP2 RESAMP2##_recreate(RESAMP2 _q, unsigned int _m, float _f0, float _As);                  \
    void RESAMP2##_destroy(RESAMP2 _q);                                                             \
    void RESAMP2##_print(RESAMP2 _q);                                                               \
    void RESAMP2##_clear(RESAMP2 _q);                                                               \
    unsigned int RESAMP2##_get_delay(RESAMP2 _q);                                                   \
    void RESAMP2##_filter_execute(RESAMP2 _q, T _x, T *_y0, T *_y1);                                \
    void RESAMP2##_analyzer_execute(RESAMP2 _q, T *_x, T *_y);                                      \
    void RESAMP2##_synthesizer_execute(RESAMP2 _q, T *_x, T *_y);                                   \
    void RESAMP2##_decim_execute(RESAMP2 _q, T *_x, T *_y);                                         \
    void RESAMP2##_interp_execute(RESAMP2 _q, T _x, T *_y);                                         \
    /* extension: _n consecutive calls of one mode (LQMI_RESAMP2_*); _y1 only for FILTER */         \
    void RESAMP2##_execute_block(RESAMP2 _q, int _mode, T *_x, unsigned long long _n, T *_y0, T *_y1); \
    void RESAMP2##_execute_block_dev(RESAMP2 _q, int _mode, const T *_dx, unsigned long long _n,    \
                                     T *_dy0, T *_dy1);                                             \
    void RESAMP2##_set_stream(RESAMP2 _q, void *_hip_stream);                                       \
    void RESAMP2##_synchronize(RESAMP2 _q);

LQMI_RESAMP2_API(resamp2_rrrf, float)
LQMI_RESAMP2_API(resamp2_crcf, liquid_float_complex)
LQMI_RESAMP2_API(resamp2_cccf, liquid_float_complex)

#define LQMI_MSRESAMP2_API(MSRESAMP2, T)                                                            \
    typedef struct MSRESAMP2##_s *MSRESAMP2;                                                        \
    MSRESAMP2 MSRESAMP2##_create(int _type, unsigned int _num_stages, float _fc, float _f0, float _As); \
    void MSRESAMP2##_destroy(MSRESAMP2 _q);                                                         \
    void MSRESAMP2##_print(MSRESAMP2 _q);                                                           \
    void MSRESAMP2##_reset(MSRESAMP2 _q);                                                           \
    float MSRESAMP2##_get_delay(MSRESAMP2 _q);                                                      \
    void MSRESAMP2##_execute(MSRESAMP2 _q, T *_x, T *_y);                                           \
    /* extension: _n consecutive calls (interp: 1 in, 2^s out; decim: 2^s in, 1 out) */            \
    void MSRESAMP2##_execute_block(MSRESAMP2 _q, T *_x, unsigned long long _n, T *_y);              \
    void MSRESAMP2##_execute_block_dev(MSRESAMP2 _q, const T *_dx, unsigned long long _n, T *_dy);  \
    void MSRESAMP2##_set_stream(MSRESAMP2 _q, void *_hip_stream);                                   \
    void MSRESAMP2##_synchronize(MSRESAMP2 _q);

LQMI_MSRESAMP2_API(msresamp2_rrrf, float)
LQMI_MSRESAMP2_API(msresamp2_crcf, liquid_float_complex)
LQMI_MSRESAMP2_API(msresamp2_cccf, liquid_float_complex)

#define LQMI_MSRESAMP_API(MSRESAMP, T)                                                              \
    typedef struct MSRESAMP##_s *MSRESAMP;                                                          \
    MSRESAMP MSRESAMP##_create(float _r, float _As);                                                \
    void MSRESAMP##_destroy(MSRESAMP _q);                                                           \
    void MSRESAMP##_print(MSRESAMP _q);                                                             \
    void MSRESAMP##_reset(MSRESAMP _q);                                                             \
    float MSRESAMP##_get_delay(MSRESAMP _q);                                                        \
    void MSRESAMP##_execute(MSRESAMP _q, T *_x, unsigned int _nx, T *_y, unsigned int *_ny);        \
    /* extension: outputs the next _nx inputs produce; device-pointer form */                       \
    unsigned long long MSRESAMP##_num_output(MSRESAMP _q, unsigned long long _nx);                  \
    void MSRESAMP##_execute_block_dev(MSRESAMP _q, const T *_dx, unsigned long long _nx, T *_dy,    \
                                      unsigned long long *_ny);                                     \
    void MSRESAMP##_set_stream(MSRESAMP _q, void *_hip_stream);                                     \
    void MSRESAMP##_synchronize(MSRESAMP _q);

LQMI_MSRESAMP_API(msresamp_rrrf, float)
LQMI_MSRESAMP_API(msresamp_crcf, liquid_float_complex)
LQMI_MSRESAMP_API(msresamp_cccf, liquid_float_complex)

/* ------------------------------------------------------------------------ */
/* firhilbf (liquid.h:2097-2176): Hilbert transform filter, real <-> complex */
/* ------------------------------------------------------------------------ */
/* _m: filter semi-length (4m+1 taps, delay 2m+1), at least 2; _As: stop-band
   attenuation [dB].  decim: 2 real in, 1 complex out per call; interp: 1
   complex in, 2 real out; r2c: 1 real in, 1 complex out; c2r: the real part.
   All modes share the object's two windows. */
typedef struct firhilbf_s *firhilbf;
firhilbf firhilbf_create(unsigned int _m, float _As);
void firhilbf_destroy(firhilbf _q);
void firhilbf_print(firhilbf _q);
void firhilbf_reset(firhilbf _q);
void firhilbf_r2c_execute(firhilbf _q, float _x, liquid_float_complex *_y);
void firhilbf_c2r_execute(firhilbf _q, liquid_float_complex _x, float *_y);
void firhilbf_decim_execute(firhilbf _q, float *_x, liquid_float_complex *_y);
void firhilbf_decim_execute_block(firhilbf _q, float *_x, unsigned int _n, liquid_float_complex *_y);
void firhilbf_interp_execute(firhilbf _q, liquid_float_complex _x, float *_y);
void firhilbf_interp_execute_block(firhilbf _q, liquid_float_complex *_x, unsigned int _n, float *_y);
/* extensions: _n consecutive r2c / c2r calls; device-pointer forms of the
   four block calls (_n counts calls: decim outputs, interp / r2c / c2r
   inputs).  In the _dev forms the input and output ranges must not overlap:
   a workgroup reads inputs that another may already have overwritten. */
void firhilbf_r2c_execute_block(firhilbf _q, float *_x, unsigned long long _n, liquid_float_complex *_y);
void firhilbf_c2r_execute_block(firhilbf _q, liquid_float_complex *_x, unsigned long long _n, float *_y);
void firhilbf_decim_execute_block_dev(firhilbf _q, const float *_dx, unsigned long long _n,
                                      liquid_float_complex *_dy);
void firhilbf_interp_execute_block_dev(firhilbf _q, const liquid_float_complex *_dx, unsigned long long _n,
                                       float *_dy);
void firhilbf_r2c_execute_block_dev(firhilbf _q, const float *_dx, unsigned long long _n,
                                    liquid_float_complex *_dy);
void firhilbf_c2r_execute_block_dev(firhilbf _q, const liquid_float_complex *_dx, unsigned long long _n,
                                    float *_dy);
void firhilbf_set_stream(firhilbf _q, void *_hip_stream);
void firhilbf_synchronize(firhilbf _q);

/* ------------------------------------------------------------------------ */
/* iirfilt (liquid.h:2247-2378): rrrf, crcf, cccf                            */
/* ------------------------------------------------------------------------ */
/* Recursive filters from given coefficients: create (numerator / denominator,
   divided by _a[0]; direct form II), create_sos (a cascade of second-order
   sections, 3 coefficients each), and the ready-made DC blocker, PLL loop
   filter, integrator and differentiator.  create_prototype and
   create_lowpass are deliberately not declared: design the coefficients with
   liquid_iirdes (below) and pass them to create_sos (SOS format) or create
   (TF format).  A TF design of order above 2, and a cascade of more than 8
   sections, run in the host loop. */
typedef enum {
    LIQUID_IIRDES_BUTTER = 0,
    LIQUID_IIRDES_CHEBY1,
    LIQUID_IIRDES_CHEBY2,
    LIQUID_IIRDES_ELLIP,
    LIQUID_IIRDES_BESSEL
} liquid_iirdes_filtertype;
typedef enum {
    LIQUID_IIRDES_LOWPASS = 0,
    LIQUID_IIRDES_HIGHPASS,
    LIQUID_IIRDES_BANDPASS,
    LIQUID_IIRDES_BANDSTOP
} liquid_iirdes_bandtype;
typedef enum { LIQUID_IIRDES_SOS = 0, LIQUID_IIRDES_TF } liquid_iirdes_format;

#define LQMI_IIRFILT_API(IIRFILT, TO, TC, TI)                                                   \
    typedef struct IIRFILT##_s *IIRFILT;                                                        \
    IIRFILT IIRFILT##_create(TC *_b, unsigned int _nb, TC *_a, unsigned int _na);               \
    IIRFILT IIRFILT##_create_sos(TC *_B, TC *_A, unsigned int _nsos);                           \
    IIRFILT IIRFILT##_create_integrator(void);                                                  \
    IIRFILT IIRFILT##_create_differentiator(void);                                              \
    IIRFILT IIRFILT##_create_dc_blocker(float _alpha);                                          \
    IIRFILT IIRFILT##_create_pll(float _w, float _zeta, float _K);                              \
    void IIRFILT##_destroy(IIRFILT _q);                                                         \
    void IIRFILT##_print(IIRFILT _q);                                                           \
    void IIRFILT##_reset(IIRFILT _q);                                                           \
    void IIRFILT##_execute(IIRFILT _q, TI _x, TO *_y);                                          \
    void IIRFILT##_execute_block(IIRFILT _q, TI *_x, unsigned int _n, TO *_y);                  \
    unsigned int IIRFILT##_get_length(IIRFILT _q);                                              \
    void IIRFILT##_freqresponse(IIRFILT _q, float _fc, liquid_float_complex *_H);               \
    float IIRFILT##_groupdelay(IIRFILT _q, float _fc);                                          \
    /* extensions: device pointers (_dy == _dx allowed); whether block calls run on the GPU   \
       (SOS form up to 8 sections or at most 3 coefficients, no pole outside the unit         \
       circle) or in the host loop */                                                          \
    void IIRFILT##_execute_block_dev(IIRFILT _q, const TI *_dx, unsigned long long _n, TO *_dy); \
    int IIRFILT##_device_eligible(IIRFILT _q);                                                  \
    void IIRFILT##_set_stream(IIRFILT _q, void *_hip_stream);                                   \
    void IIRFILT##_synchronize(IIRFILT _q);

LQMI_IIRFILT_API(iirfilt_rrrf, float, float, float)
LQMI_IIRFILT_API(iirfilt_crcf, liquid_float_complex, float, liquid_float_complex)
LQMI_IIRFILT_API(iirfilt_cccf, liquid_float_complex, liquid_float_complex, liquid_float_complex)

/* liquid.h:1621, 1829, 1848, 1864: the design helpers those constructors use */
float iir_group_delay(float *_b, unsigned int _nb, float *_a, unsigned int _na, float _fc);
void iirdes_dzpk2sosf(liquid_float_complex *_zd, liquid_float_complex *_pd, unsigned int _n,
                      liquid_float_complex _kd, float *_B, float *_A);
void iirdes_pll_active_lag(float _w, float _zeta, float _K, float *_b, float *_a);
void iirdes_pll_active_PI(float _w, float _zeta, float _K, float *_b, float *_a);

/* Recursive filter design (liquid.h:1688-1880; host code, no GPU).
   liquid_iirdes: _n the order of the low-pass prototype, _fc its cut-off,
   _f0 the centre frequency of a band-pass or band-stop design (whose order is
   2 _n), _Ap / _As the pass-band ripple and stop-band attenuation [dB] where
   the type has one.  _B, _A: 3 coefficients per section, ceil(order / 2)
   sections (SOS), or order + 1 coefficients each (TF). */
void liquid_iirdes(liquid_iirdes_filtertype _ftype, liquid_iirdes_bandtype _btype, liquid_iirdes_format _format,
                   unsigned int _n, float _fc, float _f0, float _Ap, float _As, float *_B, float *_A);
/* analog low-pass prototypes: zeros, poles (conjugate pairs together, the real
   pole of an odd order last) and gain */
void butter_azpkf(unsigned int _n, liquid_float_complex *_za, liquid_float_complex *_pa, liquid_float_complex *_ka);
void cheby1_azpkf(unsigned int _n, float _ep, liquid_float_complex *_z, liquid_float_complex *_p,
                  liquid_float_complex *_k);
void cheby2_azpkf(unsigned int _n, float _es, liquid_float_complex *_z, liquid_float_complex *_p,
                  liquid_float_complex *_k);
void ellip_azpkf(unsigned int _n, float _ep, float _es, liquid_float_complex *_z, liquid_float_complex *_p,
                 liquid_float_complex *_k);
void bessel_azpkf(unsigned int _n, liquid_float_complex *_z, liquid_float_complex *_p, liquid_float_complex *_k);
/* transforms between the analog and digital planes and between forms */
float iirdes_freqprewarp(liquid_iirdes_bandtype _btype, float _fc, float _f0);
void bilinear_zpkf(liquid_float_complex *_za, unsigned int _nza, liquid_float_complex *_pa, unsigned int _npa,
                   liquid_float_complex _ka, float _m, liquid_float_complex *_zd, liquid_float_complex *_pd,
                   liquid_float_complex *_kd);
void iirdes_dzpk_lp2hp(liquid_float_complex *_zd, liquid_float_complex *_pd, unsigned int _n,
                       liquid_float_complex *_zdt, liquid_float_complex *_pdt);
void iirdes_dzpk_lp2bp(liquid_float_complex *_zd, liquid_float_complex *_pd, unsigned int _n, float _f0,
                       liquid_float_complex *_zdt, liquid_float_complex *_pdt);
void iirdes_dzpk2tff(liquid_float_complex *_zd, liquid_float_complex *_pd, unsigned int _n,
                     liquid_float_complex _kd, float *_b, float *_a);
/* 1 unless a root of _a (_n coefficients) lies outside the unit circle */
int iirdes_isstable(float *_b, float *_a, unsigned int _n);
/* _z sorted into conjugate pairs (within _tol; negative imaginary part first,
   pairs by increasing real part), the real values after them, increasing */
void liquid_cplxpair(liquid_float_complex *_z, unsigned int _n, float _tol, liquid_float_complex *_p);
void liquid_cplxpair_cleanup(liquid_float_complex *_p, unsigned int _n, unsigned int _num_pairs);

/* extension: samples per lane, per workgroup, and tiles per scan block of the
   block-parallel kernels (csrc/k_iirfilt.hip) */
unsigned int liquid_mi355x_iirfilt_run(void);
unsigned int liquid_mi355x_iirfilt_tile(void);
unsigned int liquid_mi355x_iirfilt_scan(void);
/* extension: the launches a device call of _n full-rate samples takes (no GPU
   call): 0 the apply stage alone (at most one tile), 1 one scan launch
   between the tile and apply stages (at most scan tiles), 2 three scan
   launches (reduce per chunk, scan the chunk totals, scan within the chunks) */
int liquid_mi355x_iirfilt_route(unsigned long long _n);

/* ------------------------------------------------------------------------ */
/* iirdecim (liquid.h:2738-2820), iirinterp (liquid.h:2570-2650)             */
/* ------------------------------------------------------------------------ */
/* A recursive filter at the full rate, decimated or interpolated by _M >= 2.
   iirdecim: execute reads _M samples and returns the filter's output for the
   first of them; execute_block reads _n _M samples and writes _n.  iirinterp:
   execute feeds _x and _M - 1 zeros and writes _M outputs (no gain
   compensation); execute_block reads _n samples and writes _n _M.
   create_default is the Butterworth low-pass of the given order at 0.5 / _M.
   Extensions: device pointers (_n counted as for execute_block; the input
   and output ranges must not overlap -- in particular the decimator's
   execute_block_dev does not support overlapping device ranges, although
   its host-pointer execute_block allows _y == _x); device_eligible: block
   calls run on the GPU (the filter is eligible as for iirfilt and _M is at
   most liquid_mi355x_iirfilt_tile()), else in the host loop. */
#define LQMI_IIRRATE_API(OBJ, TO, TC, TI, XARG)                                                 \
    typedef struct OBJ##_s *OBJ;                                                                \
    OBJ OBJ##_create(unsigned int _M, TC *_b, unsigned int _nb, TC *_a, unsigned int _na);      \
    OBJ OBJ##_create_default(unsigned int _M, unsigned int _order);                             \
    OBJ OBJ##_create_prototype(unsigned int _M, liquid_iirdes_filtertype _ftype,                \
                               liquid_iirdes_bandtype _btype, liquid_iirdes_format _format,     \
                               unsigned int _order, float _fc, float _f0, float _Ap,            \
                               float _As);                                                      \
    void OBJ##_destroy(OBJ _q);                                                                 \
    void OBJ##_print(OBJ _q);                                                                   \
    void OBJ##_reset(OBJ _q);                                                                   \
    void OBJ##_execute(OBJ _q, XARG _x, TO *_y);                                                \
    void OBJ##_execute_block(OBJ _q, TI *_x, unsigned int _n, TO *_y);                          \
    float OBJ##_groupdelay(OBJ _q, float _fc);                                                  \
    void OBJ##_execute_block_dev(OBJ _q, const TI *_dx, unsigned long long _n, TO *_dy);        \
    int OBJ##_device_eligible(OBJ _q);                                                          \
    void OBJ##_set_stream(OBJ _q, void *_hip_stream);                                           \
    void OBJ##_synchronize(OBJ _q);

LQMI_IIRRATE_API(iirdecim_rrrf, float, float, float, float *)
LQMI_IIRRATE_API(iirdecim_crcf, liquid_float_complex, float, liquid_float_complex, liquid_float_complex *)
LQMI_IIRRATE_API(iirdecim_cccf, liquid_float_complex, liquid_float_complex, liquid_float_complex,
                 liquid_float_complex *)
LQMI_IIRRATE_API(iirinterp_rrrf, float, float, float, float)
LQMI_IIRRATE_API(iirinterp_crcf, liquid_float_complex, float, liquid_float_complex, liquid_float_complex)
LQMI_IIRRATE_API(iirinterp_cccf, liquid_float_complex, liquid_float_complex, liquid_float_complex,
                 liquid_float_complex)

/* ------------------------------------------------------------------------ */
/* autocorr (liquid.h:1908-1970): cccf, rrrf                                 */
/* ------------------------------------------------------------------------ */
/* Windowed delay autocorrelation: after each sample n,
     rxx[n] = sum_{k=n-W+1..n} x[k] conj(x[k-d])      (rrrf: x[k] x[k-d])
   with W = _window_size >= 1, d = _delay >= 0 (W + d < 2^31) and zero samples
   before the last reset.  Every output is one float32 sum of the W products of
   its own window -- in the kernel too, whose cost per output does not grow
   with W (csrc/k_autocorr.hip) -- so its error is proportional to the samples
   it sees.  push, execute and the block calls may be mixed in any order;
   execute without a new push returns the same value again; _rxx == _x is
   allowed in execute_block.
   get_energy is the float32 sum of |x|^2 over the last W samples, computed
   when asked.  It does not replay the reference's running accumulator
   (autocorr.c:123-127: add the newest, subtract the oldest), whose rounding
   error grows over the life of the stream: the two differ by that drift.
   Extensions: execute_block_dev takes device pointers; _de2 may be NULL, else
   it receives e2[n] = sum_{k=n-W+1..n} |x[k]|^2 per sample; the input range
   must not overlap either output range (unlike the host-pointer
   execute_block, which allows _rxx == _x).  device_eligible: block calls run
   on the GPU (W <= liquid_mi355x_autocorr_max_window()), else in a host loop.
   The delay is not limited beyond W + d < 2^31: it only sets the length of
   the history.  push, execute and get_energy follow the small-call rule
   (liquid_mi355x_set_small_calls). */
#define LQMI_AUTOCORR_API(AUTOCORR, TO, TC, TI)                                                 \
    typedef struct AUTOCORR##_s *AUTOCORR;                                                      \
    AUTOCORR AUTOCORR##_create(unsigned int _window_size, unsigned int _delay);                 \
    void AUTOCORR##_destroy(AUTOCORR _q);                                                       \
    void AUTOCORR##_reset(AUTOCORR _q);                                                         \
    void AUTOCORR##_print(AUTOCORR _q);                                                         \
    void AUTOCORR##_push(AUTOCORR _q, TI _x);                                                   \
    void AUTOCORR##_execute(AUTOCORR _q, TO *_rxx);                                             \
    void AUTOCORR##_execute_block(AUTOCORR _q, TI *_x, unsigned int _n, TO *_rxx);              \
    float AUTOCORR##_get_energy(AUTOCORR _q);                                                   \
    void AUTOCORR##_execute_block_dev(AUTOCORR _q, const TI *_dx, unsigned long long _n,        \
                                      TO *_drxx, float *_de2);                                  \
    int AUTOCORR##_device_eligible(AUTOCORR _q);                                                \
    void AUTOCORR##_set_stream(AUTOCORR _q, void *_hip_stream);                                 \
    void AUTOCORR##_synchronize(AUTOCORR _q);

LQMI_AUTOCORR_API(autocorr_cccf, liquid_float_complex, liquid_float_complex, liquid_float_complex)
LQMI_AUTOCORR_API(autocorr_rrrf, float, float, float)

/* extension: outputs per workgroup of the block kernel, and the largest
   window it takes */
unsigned int liquid_mi355x_autocorr_tile(void);
unsigned int liquid_mi355x_autocorr_max_window(void);

/* ------------------------------------------------------------------------ */
/* detector_cccf (liquid.h:4117-4152): preamble correlator bank              */
/* ------------------------------------------------------------------------ */
/* Cross-correlates the stream against the sequence s (n samples) in a bank of
   m frequency-shifted copies, m = max(2, ceil(|dphi_max / dphi_step|)),
   dphi_step = 0.8 pi / n, template k = conj(s[i]) exp(-j dphi[k] i) with
   dphi[k] = (k - (m-1)/2) dphi_step.  For stream sample t (counted from the
   last reset, zeros before it) and its window w_t = x[t-n+1 .. t]:
     r_k[t] = |sum_i p_k[i] w_t[i]| / sqrt(n E[t]),   E[t] = sum_i |w_t[i]|^2,
   and correlate() runs the reference's SEEK / FINDMAX state machine over the
   rows r[t] (detector_cccf.c:247-330), returning 1 at the sample after a peak
   with the timing, carrier and gain estimates (:396-454).
   Where this differs from the reference: (1) E[t] is the float32 sum of its
   own window, not the reference's running add-and-subtract, whose rounding
   error grows over the life of the stream; (2) where E[t] = 0 every r_k[t] is
   exactly 0 (the reference divides 0 by 0; its NaN compares above nothing, so
   the decisions are the same); (3) reset zeroes all three stored rows (the
   reference leaves the newest as it was).
   correlate() runs on the host and needs no GPU; the block calls need one at
   their first use.  Per-sample and block calls share one state and may follow
   each other in any order.
   Extensions: correlate_block reports every detection correlate() would have
   reported over _x[0.._n): it returns their number and writes the first
   _max_det of them -- _index (offset in this call of the sample at which
   correlate returns 1), _tau_hat, _dphi_hat, _gamma_hat; any of the four
   arrays may be NULL.  correlate_block_dev takes _dx in device memory; _drxy
   is NULL or _n*m floats in device memory, row t = r_0[t] .. r_{m-1}[t],
   formed for every sample whether the detector's timer runs or not.  The
   detections come back in host arrays, so correlate_block_dev synchronises
   the object's stream before it returns.  device_eligible: block calls run on
   the GPU (n <= liquid_mi355x_detector_max_len() and m <=
   liquid_mi355x_detector_max_correlators()), else in a host loop.
   get_templates copies the m*n template values as held (row k = p_k). */
typedef struct detector_cccf_s *detector_cccf;
detector_cccf detector_cccf_create(liquid_float_complex *_s, unsigned int _n, float _threshold, float _dphi_max);
void detector_cccf_destroy(detector_cccf _q);
void detector_cccf_print(detector_cccf _q);
void detector_cccf_reset(detector_cccf _q);
int detector_cccf_correlate(detector_cccf _q, liquid_float_complex _x, float *_tau_hat, float *_dphi_hat,
                            float *_gamma_hat);
unsigned int detector_cccf_correlate_block(detector_cccf _q, liquid_float_complex *_x, unsigned int _n,
                                           unsigned int *_index, float *_tau_hat, float *_dphi_hat,
                                           float *_gamma_hat, unsigned int _max_det);
unsigned int detector_cccf_correlate_block_dev(detector_cccf _q, const liquid_float_complex *_dx,
                                               unsigned long long _n, float *_drxy, unsigned long long *_index,
                                               float *_tau_hat, float *_dphi_hat, float *_gamma_hat,
                                               unsigned int _max_det);
unsigned int detector_cccf_get_num_correlators(detector_cccf _q);
void detector_cccf_get_templates(detector_cccf _q, liquid_float_complex *_p);
int detector_cccf_device_eligible(detector_cccf _q);
void detector_cccf_set_stream(detector_cccf _q, void *_hip_stream);
void detector_cccf_synchronize(detector_cccf _q);

/* extension: outputs per workgroup of the block kernel, the longest sequence
   and the widest bank it takes */
unsigned int liquid_mi355x_detector_tile(void);
unsigned int liquid_mi355x_detector_max_len(void);
unsigned int liquid_mi355x_detector_max_correlators(void);
/* tests only: records the block call's device list holds (0: the default);
   a call that marks more samples than that runs in pieces, with the same
   result */
void liquid_mi355x_detector_set_list_capacity(unsigned int _records);

/* ------------------------------------------------------------------------ */
/* qdetector_cccf (liquid.h "qdetector_cccf"): FFT preamble detector         */
/* ------------------------------------------------------------------------ */
/* The stream is cut into windows of nfft = 2^nextpow2(2 s_len) samples that
   overlap by half.  Each window is transformed, multiplied by conj(S) (S =
   FFT(s zero padded)) shifted by every carrier offset in [-range, range],
   transformed back, and the largest |rxy| over all offsets and lags, scaled by
   g = 1 / (nfft sqrt(energy) sqrt(s_len / nfft) sqrt(sum |s|^2)), is the
   window's peak (qdetector_cccf.c:373-477).  A window with peak > threshold
   && index < nfft - s_len starts the align stage: the buffer is realigned to
   the peak, filled, and tau_hat, gamma_hat, dphi_hat, phi_hat are estimated
   (:480-607).  execute() returns the object's nfft aligned samples (host
   memory) at the sample that completes them, NULL at every other sample.
   create_linear keeps the reference's argument checks; set_threshold (0, 2]
   and set_range [0, 0.5] ignore values out of range with a warning.
   qdetector_cccf_create_gmsk is not provided (there is no gmskmod).

   What is held to, and where this differs from the reference:
   1. A seek window's record depends only on that window's nfft samples.
      energy = x2_sum_0 + x2_sum_1, each a fixed-order float32 sum over its
      own half window (the reference keeps a running sum in arrival order).
   2. The object carries the buffered samples, the counter, the state, the
      coarse offset and the estimates between calls, and every window goes
      through the same device code: records and detections of block calls are
      bit identical however the stream is cut into calls, across host and
      device pointers and alignments of the input.
   3. execute() buffers on the host and sends a window through that same
      device path when it fills, once per nfft/2 samples; per-sample and block
      calls may be mixed and agree bit for bit.
   4. Where energy == 0 the record is (0, 0, 0) and nothing is detected (the
      reference forms 0 inf = NaN, which compares above nothing).
   5. The peak is the first maximum in the reference's order: offset ascending
      from -range, then lag ascending; squared magnitudes are compared.
   6. A seek hit at index == 0: the window is already aligned and the align
      stage runs on it at once (the reference sets counter = nfft and writes
      one element past its buffer at the next sample).
   7. reset() returns the object to its state after create and keeps
      threshold and range (it is empty in the reference).
   8. After a frame seek resumes as in the reference: the window grid restarts
      at (frame start + nfft/2).

   Extensions.  execute_block reports every frame completed within _x[0.._n):
   it returns their number and writes the first _max_det of them: _idx (index
   within this call of the sample at which execute() would have returned
   non-NULL), the four estimates, and in _frames (NULL, or _max_det x nfft
   samples) the aligned buffers.  _records (NULL, or room for
   1 + (_n + nfft) / (nfft / 2) records) receives one record per seek window
   completed in the call, in stream order, *_num_records their number.
   execute_block_dev takes _dx in device memory; _frames and _records are then
   device pointers (or NULL) and stay on the device; only each chunk's records
   and, per detection, the scalars cross the bus, so the call synchronises the
   object's stream.  Any output pointer may be NULL. */
typedef struct {
    float peak;          /* g max |rxy| */
    unsigned int index;  /* its lag */
    int offset;          /* its carrier offset (bins) */
    float energy;        /* sum |x|^2 of the window */
} qdetector_cccf_record;
typedef struct qdetector_cccf_s *qdetector_cccf;
qdetector_cccf qdetector_cccf_create(liquid_float_complex *_s, unsigned int _s_len);
qdetector_cccf qdetector_cccf_create_linear(liquid_float_complex *_sequence, unsigned int _sequence_len, int _ftype,
                                            unsigned int _k, unsigned int _m, float _beta);
void qdetector_cccf_destroy(qdetector_cccf _q);
void qdetector_cccf_print(qdetector_cccf _q);
void qdetector_cccf_reset(qdetector_cccf _q);
void *qdetector_cccf_execute(qdetector_cccf _q, liquid_float_complex _x);
void qdetector_cccf_set_threshold(qdetector_cccf _q, float _threshold);
void qdetector_cccf_set_range(qdetector_cccf _q, float _dphi_max);
unsigned int qdetector_cccf_get_seq_len(qdetector_cccf _q);
const void *qdetector_cccf_get_sequence(qdetector_cccf _q);
unsigned int qdetector_cccf_get_buf_len(qdetector_cccf _q);
float qdetector_cccf_get_tau(qdetector_cccf _q);
float qdetector_cccf_get_gamma(qdetector_cccf _q);
float qdetector_cccf_get_dphi(qdetector_cccf _q);
float qdetector_cccf_get_phi(qdetector_cccf _q);
unsigned int qdetector_cccf_execute_block(qdetector_cccf _q, const liquid_float_complex *_x, unsigned long long _n,
                                          unsigned int _max_det, unsigned long long *_idx, float *_tau_hat,
                                          float *_gamma_hat, float *_dphi_hat, float *_phi_hat,
                                          liquid_float_complex *_frames, qdetector_cccf_record *_records,
                                          unsigned long long *_num_records);
unsigned int qdetector_cccf_execute_block_dev(qdetector_cccf _q, const liquid_float_complex *_dx,
                                              unsigned long long _n, unsigned int _max_det, unsigned long long *_idx,
                                              float *_tau_hat, float *_gamma_hat, float *_dphi_hat, float *_phi_hat,
                                              liquid_float_complex *_dframes, qdetector_cccf_record *_drecords,
                                              unsigned long long *_num_records);
int qdetector_cccf_get_range(qdetector_cccf _q);        /* in bins */
float qdetector_cccf_get_threshold(qdetector_cccf _q);
void qdetector_cccf_set_stream(qdetector_cccf _q, void *_hip_stream);
void qdetector_cccf_synchronize(qdetector_cccf _q);
/* the seek kernel a launch takes (fused at nfft 512 and 1024, composed
   elsewhere) -- a function of nfft alone, so that a window's bits do not
   depend on how many windows a call completes */
enum { LIQUID_MI355X_QDETECTOR_COMPOSED = 0, LIQUID_MI355X_QDETECTOR_FUSED = 1 };
int liquid_mi355x_qdetector_route(unsigned int _nfft, int _range, unsigned long long _num_windows);
/* tests only: seek windows per launch chunk (0: the default, which depends on
   nfft alone); results do not depend on it.  Measurements only: set_route
   (LIQUID_MI355X_QDETECTOR_COMPOSED) sends every size's later launches to the
   composed path, and liquid_mi355x_qdetector_route answers accordingly; -1
   restores the default.  Both settings are process-wide and not thread-safe:
   set them while no other thread runs a qdetector. */
void liquid_mi355x_qdetector_set_route(int _route);
void liquid_mi355x_qdetector_set_chunk(unsigned int _windows);
unsigned int liquid_mi355x_qdetector_chunk(unsigned int _nfft);

/* ------------------------------------------------------------------------ */
/* fftfilt (liquid.h:2192-2240): rrrf, crcf, cccf                            */
/* ------------------------------------------------------------------------ */
#define LQMI_FFTFILT_API(FFTFILT, TO, TC, TI)                                                   \
    typedef struct FFTFILT##_s *FFTFILT;                                                        \
    FFTFILT FFTFILT##_create(TC *_h, unsigned int _h_len, unsigned int _n);                     \
    void FFTFILT##_destroy(FFTFILT _q);                                                         \
    void FFTFILT##_reset(FFTFILT _q);                                                           \
    void FFTFILT##_print(FFTFILT _q);                                                           \
    void FFTFILT##_set_scale(FFTFILT _q, TC _scale);                                            \
    void FFTFILT##_execute(FFTFILT _q, TI *_x, TO *_y);                                         \
    unsigned int FFTFILT##_get_length(FFTFILT _q);                                              \
    /* extension: arbitrary-length stream (any _n), host / device pointers */                   \
    void FFTFILT##_execute_block(FFTFILT _q, TI *_x, unsigned long long _n, TO *_y);            \
    void FFTFILT##_execute_block_dev(FFTFILT _q, const TI *_dx, unsigned long long _n,          \
                                     TO *_dy);                                                  \
    void FFTFILT##_set_stream(FFTFILT _q, void *_hip_stream);

LQMI_FFTFILT_API(fftfilt_rrrf, float, float, float)
LQMI_FFTFILT_API(fftfilt_crcf, liquid_float_complex, float, liquid_float_complex)
LQMI_FFTFILT_API(fftfilt_cccf, liquid_float_complex, liquid_float_complex, liquid_float_complex)

/* ------------------------------------------------------------------------ */
/* firpfbch (liquid.h:5667-5739): crcf, cccf                                 */
/* ------------------------------------------------------------------------ */
#define LQMI_FIRPFBCH_API(FIRPFBCH, TC)                                                             \
    typedef struct FIRPFBCH##_s *FIRPFBCH;                                                          \
    FIRPFBCH FIRPFBCH##_create(int _type, unsigned int _M, unsigned int _p, TC *_h);                \
    FIRPFBCH FIRPFBCH##_create_kaiser(int _type, unsigned int _M, unsigned int _m, float _As);      \
    FIRPFBCH FIRPFBCH##_create_rnyquist(int _type, unsigned int _M, unsigned int _m, float _beta,   \
                                        int _ftype);                                                \
    void FIRPFBCH##_destroy(FIRPFBCH _q);                                                           \
    void FIRPFBCH##_reset(FIRPFBCH _q);                                                             \
    void FIRPFBCH##_print(FIRPFBCH _q);                                                             \
    void FIRPFBCH##_synthesizer_execute(FIRPFBCH _q, liquid_float_complex *_x,                      \
                                        liquid_float_complex *_y);                                  \
    void FIRPFBCH##_analyzer_execute(FIRPFBCH _q, liquid_float_complex *_x,                         \
                                     liquid_float_complex *_y);                                     \
    /* extension: _nblocks consecutive M-sample blocks (analyzer or synthesizer) */                 \
    void FIRPFBCH##_execute_block(FIRPFBCH _q, liquid_float_complex *_x, unsigned long long _nblocks, \
                                  liquid_float_complex *_y);                                        \
    void FIRPFBCH##_execute_block_dev(FIRPFBCH _q, const liquid_float_complex *_dx,                 \
                                      unsigned long long _nblocks, liquid_float_complex *_dy);      \
    void FIRPFBCH##_set_stream(FIRPFBCH _q, void *_hip_stream);

LQMI_FIRPFBCH_API(firpfbch_crcf, float)
LQMI_FIRPFBCH_API(firpfbch_cccf, liquid_float_complex)

/* ------------------------------------------------------------------------ */
/* firpfbch2 (liquid.h:5754-5799): crcf                                      */
/* ------------------------------------------------------------------------ */
typedef struct firpfbch2_crcf_s *firpfbch2_crcf;
firpfbch2_crcf firpfbch2_crcf_create(int _type, unsigned int _M, unsigned int _m, float *_h);
firpfbch2_crcf firpfbch2_crcf_create_kaiser(int _type, unsigned int _M, unsigned int _m, float _As);
void firpfbch2_crcf_destroy(firpfbch2_crcf _q);
void firpfbch2_crcf_reset(firpfbch2_crcf _q);
void firpfbch2_crcf_print(firpfbch2_crcf _q);
void firpfbch2_crcf_execute(firpfbch2_crcf _q, liquid_float_complex *_x, liquid_float_complex *_y);
/* extension: _nblocks consecutive execute() calls.  analyzer: _x = _nblocks*M/2 inputs,
 * _y = _nblocks*M outputs; synthesizer: _nblocks*M in, _nblocks*M/2 out */
void firpfbch2_crcf_execute_block(firpfbch2_crcf _q, liquid_float_complex *_x,
                                  unsigned long long _nblocks, liquid_float_complex *_y);
void firpfbch2_crcf_execute_block_dev(firpfbch2_crcf _q, const liquid_float_complex *_dx,
                                      unsigned long long _nblocks, liquid_float_complex *_dy);
void firpfbch2_crcf_set_stream(firpfbch2_crcf _q, void *_hip_stream);
void *firpfbch2_crcf_get_stream(firpfbch2_crcf _q);
void firpfbch2_crcf_synchronize(firpfbch2_crcf _q);

/* What a channelizer call launches (no reference counterpart; for tests).
 * The answer is the launch's own decision: the launches call the same host
 * functions.  No GPU call is made.  Returns the route, an index into
 * liquid_mi355x_channelizer_route_name(0 .. liquid_mi355x_channelizer_route_count() - 1),
 * or -1 for arguments no object can have (and a size the GPU path refuses).
 * A route is one kernel family plus what a test must tell apart: paired or
 * 8-byte input loads (`_unpaired'), the few-block form and its signalling
 * variant, real or complex taps (`_c'); DESIGN.md has the table.
 *   _type: LIQUID_ANALYZER / LIQUID_SYNTHESIZER; _kind: 1 crcf, 2 cccf;
 *   _first_block_parity: blocks the object has run so far, mod 2;
 *   _x_aligned16 / _y_aligned16: the device pointers' alignment (8 bytes is
 *     taken as given);
 *   _host_call: the call comes through execute_block on host pointers, which
 *     tries the signalling few-block launch when the output fits the pinned
 *     completion buffer (liquid_mi355x_copyout_max());
 *   *_run: blocks one workgroup (or one of its column sets) walks;
 *   *_workgroups: the grid (of the filter kernel where a batched transform
 *     goes with it); both of the call's first launch;
 *   *_chunks: launches the call is cut into.  Any of the three may be NULL.
 * The queries answer as the launches do under LQ_PFB2_TWO_PASS /
 * LQ_PFB_TWO_PASS, liquid_mi355x_set_max_workgroups and
 * liquid_mi355x_set_channelizer_chunk. */
int liquid_mi355x_firpfbch2_route(int _type, unsigned int _M, unsigned int _m, unsigned long long _nblocks,
                                  int _first_block_parity, int _x_aligned16, int _y_aligned16, int _host_call,
                                  unsigned long long *_run, unsigned long long *_workgroups,
                                  unsigned long long *_chunks);
int liquid_mi355x_firpfbch_route(int _kind, int _type, unsigned int _M, unsigned int _p, unsigned long long _nblocks,
                                 int _x_aligned16, int _y_aligned16, int _host_call, unsigned long long *_run,
                                 unsigned long long *_workgroups, unsigned long long *_chunks);
int liquid_mi355x_channelizer_route_count(void);
const char *liquid_mi355x_channelizer_route_name(int _i);
/* tests only: blocks per launch of the analyzers that cut a long call into
 * chunks (firpfbch2 at M >= 64 a power of two, firpfbch at M = 1024 with 4 or
 * 8 real taps per branch).  0 (default): 2^27 / M, 2^18 and 2^17 blocks.
 * Refused (-1, nothing changes): values below 64 or no multiple of 32 -- the
 * block parity is carried per chunk, the M = 1024 kernels count groups of 16
 * blocks from the absolute block index, and a later chunk takes its history
 * from the input before it (at most 31 blocks).  A value past the default
 * leaves the default.  Results do not depend on it.  Process-wide. */
int liquid_mi355x_set_channelizer_chunk(unsigned long long _blocks);
unsigned long long liquid_mi355x_get_channelizer_chunk(void);

/* ------------------------------------------------------------------------ */
/* nco (liquid.h:5919-5999): crcf                                            */
/* ------------------------------------------------------------------------ */
/* Oscillator with PLL and mixer.  The per-sample interface runs on the host
   and is the reference's arithmetic bit for bit (float32 phase, one wrap per
   step, LIQUID_NCO: 256-entry sine table, LIQUID_VCO: sinf / cosf); create
   needs no device.  mix_block_up / mix_block_down run on the GPU
   (csrc/k_nco.hip): the phase of every sample is replayed bit for bit from a
   host-built plan of checkpoints (host/nco_plan.c), so the phase after a block
   equals the reference's and get_phase does not wait for the device.
   LIQUID_NCO block outputs equal the reference's bit for bit where finite;
   LIQUID_VCO ones use the device's sinf / cosf of the same phase.  In-place
   (_y == _x) is allowed; otherwise the arrays must not overlap.  An object
   with |frequency| > 2 pi, or a phase beyond 2 pi or not finite, runs block
   calls in the host loop (device_eligible() == 0). */
typedef enum { LIQUID_NCO = 0, LIQUID_VCO } liquid_ncotype;
typedef struct nco_crcf_s *nco_crcf;
nco_crcf nco_crcf_create(liquid_ncotype _type);
void nco_crcf_destroy(nco_crcf _q);
void nco_crcf_print(nco_crcf _q);
void nco_crcf_reset(nco_crcf _q);
float nco_crcf_get_frequency(nco_crcf _q);
void nco_crcf_set_frequency(nco_crcf _q, float _f);
void nco_crcf_adjust_frequency(nco_crcf _q, float _df);
float nco_crcf_get_phase(nco_crcf _q);
void nco_crcf_set_phase(nco_crcf _q, float _phi);
void nco_crcf_adjust_phase(nco_crcf _q, float _dphi);
void nco_crcf_step(nco_crcf _q);
float nco_crcf_sin(nco_crcf _q);
float nco_crcf_cos(nco_crcf _q);
void nco_crcf_sincos(nco_crcf _q, float *_s, float *_c);
void nco_crcf_cexpf(nco_crcf _q, liquid_float_complex *_y);
void nco_crcf_pll_set_bandwidth(nco_crcf _q, float _bandwidth);
void nco_crcf_pll_step(nco_crcf _q, float _dphi);
void nco_crcf_mix_up(nco_crcf _q, liquid_float_complex _x, liquid_float_complex *_y);
void nco_crcf_mix_down(nco_crcf _q, liquid_float_complex _x, liquid_float_complex *_y);
void nco_crcf_mix_block_up(nco_crcf _q, liquid_float_complex *_x, liquid_float_complex *_y, unsigned int _N);
void nco_crcf_mix_block_down(nco_crcf _q, liquid_float_complex *_x, liquid_float_complex *_y, unsigned int _N);
/* liquid.h:5995-5999 */
void liquid_unwrap_phase(float *_theta, unsigned int _n);
void liquid_unwrap_phase2(float *_theta, unsigned int _n);
/* extensions: device pointers (stream-ordered, no wait), stream control, the
 * kernel's tile (samples per workgroup) and the plan's checkpoint spacing */
void nco_crcf_mix_block_up_dev(nco_crcf _q, const liquid_float_complex *_dx, liquid_float_complex *_dy,
                               unsigned long long _n);
void nco_crcf_mix_block_down_dev(nco_crcf _q, const liquid_float_complex *_dx, liquid_float_complex *_dy,
                                 unsigned long long _n);
int nco_crcf_device_eligible(nco_crcf _q);
void nco_crcf_set_stream(nco_crcf _q, void *_hip_stream);
void nco_crcf_synchronize(nco_crcf _q);
unsigned int liquid_mi355x_nco_tile(void);
unsigned int liquid_mi355x_nco_checkpoint(void);
/* The phases (and, LIQUID_NCO, table indices) a plan serves for positions
 * 0 .. _n-1 from (_theta0, _d_theta), with its pre-period and period (0, 0 for
 * the direct form); _theta / _index / _pre / _period may be NULL.  Returns _n,
 * or -1 when the orbit has no period within the search limit.  No GPU call.
 * The environment variable LQ_NCO_PLAN=direct or =periodic, read at create,
 * makes an object build only that form (for tests). */
long long liquid_mi355x_nco_walk(liquid_ncotype _type, float _theta0, float _d_theta, unsigned long long _n,
                                 int _periodic, float *_theta, unsigned int *_index, unsigned long long *_pre,
                                 unsigned long long *_period);

/* ------------------------------------------------------------------------ */
/* freqmod (liquid.h:5329-5372), freqdem (liquid.h:5548-5591)                */
/* ------------------------------------------------------------------------ */
/* Analog FM modulator and demodulator.  As with nco, the per-sample calls run
   on the host and are the reference's arithmetic, and create needs no device;
   the block calls run on the GPU (csrc/k_freqmodem.hip).
   freqmod: a phase accumulator modulo 2^16, advanced by (int)roundf(kf 2^16 m),
   indexes a 1024-entry table; the block call is a prefix sum over the integer
   increments, so outputs and accumulator equal the per-sample loop's bit for
   bit.  A product that is not finite or reaches 2^31 in magnitude adds 0.
   freqdem: m[n] = arg(conj(r[n-1]) r[n]) / (2 pi kf); block outputs are within
   5 2^-23 (relative) of that argument taken exactly of the float32 product. */
typedef struct freqmod_s *freqmod;
freqmod freqmod_create(float _kf);
void freqmod_destroy(freqmod _q);
void freqmod_print(freqmod _q);
void freqmod_reset(freqmod _q);
void freqmod_modulate(freqmod _q, float _m, liquid_float_complex *_s);
void freqmod_modulate_block(freqmod _q, float *_m, unsigned int _n, liquid_float_complex *_s);
typedef struct freqdem_s *freqdem;
freqdem freqdem_create(float _kf);
void freqdem_destroy(freqdem _q);
void freqdem_print(freqdem _q);
void freqdem_reset(freqdem _q);
void freqdem_demodulate(freqdem _q, liquid_float_complex _r, float *_m);
void freqdem_demodulate_block(freqdem _q, liquid_float_complex *_r, unsigned int _n, float *_m);
/* extensions.  Device pointers: stream-ordered, no wait; input and output must
 * not overlap (their element sizes differ).  freqmod_get_phase: the
 * accumulator (after a device call it waits for it); freqmod_get_table: the
 * 1024 table entries.
 * freqdem_create_channels: the lag-_M discriminator m[n] = arg(conj(r[n-_M])
 * r[n]) / (2 pi kf), state the last _M samples (zero after create and reset):
 * fed a channelizer's frame-major output it demodulates every channel, in the
 * same layout.  freqdem_create(kf) is _M = 1; every call works on either, a
 * block need not be a multiple of _M and may be shorter than _M.
 * Tiles (samples per workgroup); freqmod_scan_pass: the tiles one pass of the
 * scan across tile sums covers (the one carry boundary above the tile);
 * freqdem_switch: the _M from which a lane walks the frames of its own
 * channel instead of reading its neighbour from a staged tile;
 * freqdem_frames: the frames of one such walk. */
void freqmod_modulate_block_dev(freqmod _q, const float *_dm, unsigned long long _n, liquid_float_complex *_ds);
unsigned int freqmod_get_phase(freqmod _q);
void freqmod_get_table(freqmod _q, liquid_float_complex *_tab);
void freqmod_set_stream(freqmod _q, void *_hip_stream);
void freqmod_synchronize(freqmod _q);
freqdem freqdem_create_channels(float _kf, unsigned int _M);
unsigned int freqdem_get_channels(freqdem _q);
void freqdem_demodulate_block_dev(freqdem _q, const liquid_float_complex *_dr, unsigned long long _n, float *_dm);
void freqdem_set_stream(freqdem _q, void *_hip_stream);
void freqdem_synchronize(freqdem _q);
unsigned int liquid_mi355x_freqmod_tile(void);
unsigned int liquid_mi355x_freqmod_scan_pass(void);
unsigned int liquid_mi355x_freqdem_tile(void);
unsigned int liquid_mi355x_freqdem_switch(void);
unsigned int liquid_mi355x_freqdem_frames(void);

/* ------------------------------------------------------------------------ */
/* runtime extensions                                                        */
/* ------------------------------------------------------------------------ */
/* device memory helpers for callers without their own HIP code */
void *liquid_mi355x_malloc(unsigned long long _bytes);
void liquid_mi355x_free(void *_p);
void liquid_mi355x_memcpy_h2d(void *_dst, const void *_src, unsigned long long _bytes);
void liquid_mi355x_memcpy_d2h(void *_dst, const void *_src, unsigned long long _bytes);
void liquid_mi355x_device_synchronize(void);
/* build identification (gfx target the kernels were compiled for) */
const char *liquid_mi355x_build_target(void);
/* Small-call mode (no reference counterpart).  1 (default): the
 * single-sample / single-vector entry points -- firfilt_*_execute after push,
 * dotprod_*_execute / _run / _run4, firdecim_*_execute, firinterp_*_execute,
 * resamp_*_execute, autocorr_*_push / _execute / _get_energy, and
 * fftfilt_*_execute when n * h_len <= 65536 -- compute
 * on the host (host/lq_small.c); every *_execute_block[_dev] call, the
 * channelizers, FFT plans and spgram run on the GPU.  0: every call runs on
 * the GPU.  The environment variable LQ_SMALL_CALLS=gpu sets 0 at load. */
void liquid_mi355x_set_small_calls(int _host);
int liquid_mi355x_get_small_calls(void);
/* Workgroup limit (no reference counterpart; for tests).  The persistent
 * kernels launch min(tiles, cap) workgroups and each walks further tiles;
 * _n > 0 launches at most _n, so a short call walks many tiles per
 * workgroup.  0 (default): no limit.  Results do not depend on it. */
void liquid_mi355x_set_max_workgroups(unsigned int _n);
unsigned int liquid_mi355x_get_max_workgroups(void);
/* The two staging seams of a host-pointer call (no reference counterpart; for
 * tests): an input of up to _pinned_input_max bytes is copied to pinned host
 * memory that the kernel reads in place, a larger one goes to device memory
 * by DMA; a result of up to _copyout_max bytes returns through the copy-out
 * kernel and its completion flag, a larger one by DMA and a stream sync. */
unsigned int liquid_mi355x_pinned_input_max(void);
unsigned int liquid_mi355x_copyout_max(void);
/* Which launch a dotprod batch call of _nvec rows of _n samples takes (_kind:
 * 0 rrrf, 1 crcf, 2 cccf; _x_aligned16: the input pointer is 16-byte aligned),
 * computed by the launch's own decision (no GPU call).  Bit 4
 * (LIQUID_MI355X_DOTPROD_VEC): k_dot_vec, 16-byte loads -- _n a multiple of
 * the chunk (4 real, 2 complex samples) and an aligned input; clear:
 * k_dot_scalar.  Bits 0-3 (LIQUID_MI355X_DOTPROD_LG_MASK): lg G, G = 1, 2, 4,
 * 8 or 16 lanes per row.  -1: invalid kind.  _blocks: the grid of that launch,
 * 256 lanes each, at most _block_cap; a capped grid walks the rows in
 * ceil(_nvec G / (256 _blocks)) passes. */
enum {
    LIQUID_MI355X_DOTPROD_LG_MASK = 15,
    LIQUID_MI355X_DOTPROD_VEC = 16
};
int liquid_mi355x_dotprod_route(int _kind, unsigned int _n, int _x_aligned16, unsigned long long _nvec);
unsigned int liquid_mi355x_dotprod_blocks(int _kind, unsigned int _n, int _x_aligned16, unsigned long long _nvec);
unsigned int liquid_mi355x_dotprod_block_cap(void);
/* Which kernel a firdecim device call of _nout outputs takes (_kind: 0 rrrf,
 * 1 crcf, 2 cccf; _x_aligned16: the input pointer is 16-byte aligned), and
 * the outputs per tile and the grid cap of that launch (0: not capped). */
enum {
    LIQUID_MI355X_FIRDECIM_PF_R4X128 = 0, /* persistent, 4 outputs per lane, 128 lanes */
    LIQUID_MI355X_FIRDECIM_PF_R2X256 = 1, /* persistent, 2 per lane, 256 lanes */
    LIQUID_MI355X_FIRDECIM_PH2 = 2,       /* one-shot, 2 per lane, 256 lanes */
    LIQUID_MI355X_FIRDECIM_PF_R1X256 = 3, /* persistent, 1 per lane, 256 lanes */
    LIQUID_MI355X_FIRDECIM_PH_R1X64 = 4,  /* one-shot, 1 per lane, 64 lanes */
    LIQUID_MI355X_FIRDECIM_PLAIN = 5,     /* one-shot, undivided taps, 256 lanes */
    LIQUID_MI355X_FIRDECIM_REFUSED = 6    /* M and filter length past the GPU tile limit */
};
int liquid_mi355x_firdecim_route(int _kind, unsigned int _M, unsigned int _h_len, int _x_aligned16,
                                 unsigned long long _nout);
unsigned int liquid_mi355x_firdecim_tile(int _route);
unsigned int liquid_mi355x_firdecim_grid_cap(int _kind, unsigned int _M, unsigned int _h_len, int _route);
/* Which kernel a firinterp or firpfb device call takes for _M phases of _L
 * taps each (firinterp: _L = ceil(h_len / M); firpfb: floor) and an output
 * pointer that is (_y_aligned16) or is not 16-byte aligned, computed by the
 * launch's own decision: 0 the plain kernel (complex taps, _L > 32, _M > 64,
 * an unaligned output, or taps, tile and staged outputs past 64 KB of LDS),
 * else the register-window kernel's tap class 8, 12, 16, 20, 24 or 32. */
int liquid_mi355x_firinterp_route(int _kind, unsigned int _M, unsigned int _L, int _y_aligned16);
/* The longest phase, in taps, a firinterp or firpfb object accepts (the plain
 * kernel's LDS); _create with a longer one exits with a message. */
unsigned int liquid_mi355x_firinterp_max_taps(int _kind);
/* Which kernels a transform of the FFT plan API takes for _n points read from
 * a pointer that is (_aligned16) or is not 16-byte aligned, computed by the
 * launch's own decision (no GPU call).  Bits 0-3 the family below; bit 4 the
 * 16-byte loads of the 8192- and 16384-point kernels; bits 8-12 and 16-20 lg
 * N1 and lg N2 of the two-pass split (columns in k_fft2p_cols_r / k_bs_cols_r
 * <N1 / 256>; rows in k_bs_rows_s<N2 / 16> when bit 5 is set, else in
 * k_fft2p_rows_r / k_bs_rows_r<N2 / 256>); bits 24-28 lg M of Bluestein's
 * padded transform (BLUESTEIN: its M-point transforms take the route of M). */
enum {
    LIQUID_MI355X_FFT_REFUSED = 0,          /* 0, or past 2^24 (2^23 when not a power of two) */
    LIQUID_MI355X_FFT_DFT = 1,              /* direct sums: n = 1 and other n <= 16 */
    LIQUID_MI355X_FFT_BATCH = 2,            /* k_fft_batch<n>: 2, 4, 8, 16 */
    LIQUID_MI355X_FFT_SMALL = 3,            /* k_fftsmall_batch<n / 16>: 32, 64, 128 */
    LIQUID_MI355X_FFT_R16 = 4,              /* k_fftr16_batch<n / 256>: 256, 512, 2048 */
    LIQUID_MI355X_FFT_1024 = 5,
    LIQUID_MI355X_FFT_4096 = 6,
    LIQUID_MI355X_FFT_8192 = 7,
    LIQUID_MI355X_FFT_16384 = 8,
    LIQUID_MI355X_FFT_FOUR_STEP = 9,        /* powers of two from 32768, two passes */
    LIQUID_MI355X_FFT_BLUESTEIN = 10,       /* M <= 4096: chirp products as kernels of their own */
    LIQUID_MI355X_FFT_BLUESTEIN_FUSED = 11  /* M > 4096: chirp products inside the two passes */
};
int liquid_mi355x_fft_route(unsigned int _n, int _aligned16);
/* spgram's reduction as the launches decide it (no GPU call).  _route: the
 * path of a call of _n samples -- 0 gather, batch transform and k_spg_part,
 * else k_spg_fused1024<S, HALF, TR> as 1 + 2 HALF + 4 TR; _chunk: transforms
 * per chunk; _fold_group: chunks per first-level fold group (more chunks fold
 * in two levels); _batch_samples: transforms per launch batch of the plain
 * path, in samples (batch_samples / nfft transforms). */
int liquid_mi355x_spgram_route(int _real_in, unsigned int _nfft, unsigned int _window_len, unsigned long long _n);
unsigned int liquid_mi355x_spgram_chunk(void);
unsigned int liquid_mi355x_spgram_fold_group(void);
unsigned long long liquid_mi355x_spgram_batch_samples(void);
/* Which kernel the first block call of _nx inputs takes on a fresh resamp
 * object (_kind as above; no GPU call), computed by the launch's own
 * decision, and in *_tile (may be NULL) its tile: inputs per wave tile for
 * the input-plan kernels (RESAMP3: tin; RESAMP: 2048 per workgroup; GENERIC:
 * 256 per workgroup), outputs per wave tile (256) for the four rate classes
 * of the output-plan kernel k_resamp4.  -1: bad arguments. */
enum {
    LIQUID_MI355X_RESAMP3_CONST = 0,   /* k_resamp3, constant pair-table stride (npfb <= 64) */
    LIQUID_MI355X_RESAMP3_STRIDE = 1,  /* k_resamp3, run-time stride */
    LIQUID_MI355X_RESAMP = 2,          /* k_resamp: 8 inputs per lane (r > ~52, or the table outside LDS) */
    LIQUID_MI355X_RESAMP_GENERIC = 3,  /* k_resamp_generic: m > 16 */
    LIQUID_MI355X_RESAMP4_UP = 4,      /* k_resamp4, 1 <= r <= 2 */
    LIQUID_MI355X_RESAMP4_UP_R4 = 5,   /* k_resamp4, r > 2 */
    LIQUID_MI355X_RESAMP4_DOWN = 6,    /* k_resamp4, 1/2 < r < 1 */
    LIQUID_MI355X_RESAMP4_DOWN_DN = 7  /* k_resamp4, 1/4 < r <= 1/2 */
};
int liquid_mi355x_resamp_route(int _kind, float _rate, unsigned int _m, unsigned int _npfb, unsigned long long _nx,
                               unsigned int *_tile);
/* Which kernel a resamp2 block call of this mode (LQMI_RESAMP2_*), _m and _bytes of input
 * takes, and in *_tile (may be NULL) the calls per workgroup tile.  -1: bad
 * arguments. */
enum {
    LIQUID_MI355X_RESAMP2_K_FILTER = 0,  /* k_resamp2: filter mode, one call per lane */
    LIQUID_MI355X_RESAMP2_K_TILED_B = 1, /* k_resamp2_tiled_b: m <= 16 */
    LIQUID_MI355X_RESAMP2_K_TILED = 2    /* k_resamp2_tiled */
};
int liquid_mi355x_resamp2_route(int _mode, unsigned int _m, unsigned long long _bytes, unsigned int *_tile);
/* The resampler kernel (LIQUID_MI355X_RESAMP*) of the first block call of _nx
 * inputs on a fresh msresamp, its tile, and in *_hm (may be NULL) the
 * semi-length of the half-band stage fused into that launch (0: none; the
 * fused launch's tile is shorter by the stage's halo). */
int liquid_mi355x_msresamp_route(int _kind, float _rate, float _As, unsigned long long _nx, unsigned int *_tile,
                                 unsigned int *_hm);

#ifdef __cplusplus
}
#endif

#endif /* LIQUID_MI355X_H */
