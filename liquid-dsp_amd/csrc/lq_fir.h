// lq_fir.h -- what the streaming FIR kernel files (k_firfilt.hip,
// k_firdecim.hip, k_firinterp.hip) share: the sample / tap types of the three
// kinds and their arithmetic, 16-byte sample vectors, the padded LDS tile
// layout, and the run-time kind -> template argument dispatch.  Private to
// csrc/; the exported C ABI is lq_kernels.h.
#pragma once

#include "lq_device.h"

#include <cstdint>

namespace {

constexpr int NT = 256;      // threads per workgroup of the one-shot kernels

// kind: 0 rrrf, 1 crcf, 2 cccf -> sample type T, tap type TC
template <int KIND>
struct kt;
template <>
struct kt<0> {
    typedef float T;
    typedef float TC;
};
template <>
struct kt<1> {
    typedef float2 T;
    typedef float TC;
};
template <>
struct kt<2> {
    typedef float2 T;
    typedef float2 TC;
};

// run-time kind -> f(std::integral_constant<int, KIND>)
template <class F>
bool fir_kind(int kind, F &&f) { return lq_switch<0, 1, 2>(kind, f); }

template <typename T>
__device__ __forceinline__ T zero();
template <>
__device__ __forceinline__ float zero<float>() { return 0.0f; }
template <>
__device__ __forceinline__ float2 zero<float2>() { return make_float2(0.0f, 0.0f); }

// acc += h * v for the three type combinations
__device__ __forceinline__ void mac(float &acc, float h, float v) { acc = fmaf(h, v, acc); }
__device__ __forceinline__ void mac(float2 &acc, float h, float2 v)
{
    acc.x = fmaf(h, v.x, acc.x);
    acc.y = fmaf(h, v.y, acc.y);
}
__device__ __forceinline__ void mac(float2 &acc, float2 h, float2 v)
{
    acc.x = fmaf(h.x, v.x, acc.x);
    acc.x = fmaf(-h.y, v.y, acc.x);
    acc.y = fmaf(h.x, v.y, acc.y);
    acc.y = fmaf(h.y, v.x, acc.y);
}

__device__ __forceinline__ float apply_scale(float a, float sre, float) { return a * sre; }
__device__ __forceinline__ float2 apply_scale(float2 a, float sre, float sim)
{
    return make_float2(a.x * sre - a.y * sim, a.x * sim + a.y * sre);
}
__device__ __forceinline__ float2 apply_scale_real(float2 a, float s) { return make_float2(a.x * s, a.y * s); }
// output scale as the reference applies it (firfilt.c:337, firpfb.c:343,
// `*y *= scale`): a real scale (rrrf / crcf) multiplies each component, a
// complex one (cccf) is a complex product -- they differ for Inf samples
template <int KIND, typename T>
__device__ __forceinline__ T oscale(T a, float sre, float sim)
{
    if constexpr (KIND == 2) return apply_scale(a, sre, sim);
    else if constexpr (sizeof(T) == 8) return apply_scale_real(a, sre);
    else return a * sre;
}

__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float2 vadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }

// LDS image of a sample tile: rows of 16 samples followed by 16 bytes of pad.
// Lanes whose windows start 16 samples apart then hit disjoint bank sets on
// every ds_read_b128 (complex: 36-dword row pitch; real: 20-dword pitch), and
// every 16-byte vector of samples stays 16-byte aligned.
template <typename T>
__host__ __device__ __forceinline__ int lds_off(int u) // in bytes
{
    return u * (int)sizeof(T) + 16 * (u >> 4);
}
template <typename T>
__host__ __device__ __forceinline__ int lds_bytes(int nsamp)
{
    return lds_off<T>(nsamp) + 16;
}

template <typename T>
struct vec16;
template <>
struct vec16<float> {
    static constexpr int N = 4;
};
template <>
struct vec16<float2> {
    static constexpr int N = 2;
};

// 16-byte vector of samples (V: float4 or a 4-float ext vector)
template <typename T, typename V>
__device__ __forceinline__ void unpack16(const V &v, T (&o)[vec16<T>::N])
{
    if constexpr (sizeof(T) == 8) {
        o[0] = make_float2(v.x, v.y);
        o[1] = make_float2(v.z, v.w);
    } else {
        o[0] = v.x;
        o[1] = v.y;
        o[2] = v.z;
        o[3] = v.w;
    }
}
template <typename T>
__device__ __forceinline__ void load16(const T *p, T (&o)[vec16<T>::N])
{
    unpack16(*reinterpret_cast<const float4 *>(p), o);
}
template <typename T>
__device__ __forceinline__ float4 pack16(const T (&o)[vec16<T>::N])
{
    if constexpr (sizeof(T) == 8) return make_float4(o[0].x, o[0].y, o[1].x, o[1].y);
    else return make_float4(o[0], o[1], o[2], o[3]);
}

// dynamic LDS budget of a tile kernel (k_firfilt, the decimators): the 160 KB of a CU minus a margin for the
// kernel's own (static) group segment, which the dispatch adds on top (a
// 163 600-byte request dispatched as 163 856 bytes and faulted)
constexpr size_t FIR_LDS_MAX = 160 * 1024 - 1024;

inline size_t elem_size(int kind) { return kind == 0 ? sizeof(float) : sizeof(float2); }

} // namespace
