// Typed element I/O of the activation storages (f32, bf16, sp32 pairs) and the small device helpers every kernel file shares.
// A new kernel file includes this header: it gets the sp32 contract (split_dev.h: one f32 number per split, the range
// contract's counter) through stf / st4 / st8<sp32_t> instead of restating it.  gfx950 only.
#pragma once

#include "common.h"
#include "split_dev.h"

__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }
__device__ __forceinline__ float bf2f(bf16_t b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }

// ReLU that keeps a NaN a NaN like torch (any sign, any payload: the comparison is false for it), in TWO vector instructions
// (v_cmp_lt + v_cndmask) -- the (v > 0 ? v : (v != v ? v : 0)) form costs four, and the fused bottleneck kernels run this
// on every element they store.  -0.0 stays -0.0, which no consumer can tell from +0.0.
__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- one element
template <typename T> __device__ __forceinline__ float ldf(const T* p, long i);
template <> __device__ __forceinline__ float ldf<float>(const float* p, long i) { return p[i]; }
template <> __device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p, long i) { return bf2f(p[i]); }
template <> __device__ __forceinline__ float ldf<sp32_t>(const sp32_t* p, long i) {
    const char* b = reinterpret_cast<const char*>(p) + sp32_byte(i);
    return sp2f(*reinterpret_cast<const uint16_t*>(b)) + sp2f(*reinterpret_cast<const uint16_t*>(b + 64));
}
// `ovf`: the context's range-contract counter (split_dev.h); only the sp32 forms look at it.  These kernels are HBM-bound:
// the test rides along and counts on the spot (sp_count_now)
template <typename T> __device__ __forceinline__ void stf(T* p, long i, float v, unsigned* ovf = nullptr);
template <> __device__ __forceinline__ void stf<float>(float* p, long i, float v, unsigned*) { p[i] = v; }
template <> __device__ __forceinline__ void stf<bf16_t>(bf16_t* p, long i, float v, unsigned*) { p[i] = f2bf(v); }
template <> __device__ __forceinline__ void stf<sp32_t>(sp32_t* p, long i, float v, unsigned* ovf) {
    char* b = reinterpret_cast<char*>(p) + sp32_byte(i);
    float amax = 0.f;
    uint16_t h, l;
    sp_split1(v, amax, h, l);
    sp_count_now(ovf, amax);
    *reinterpret_cast<uint16_t*>(b) = h;
    *reinterpret_cast<uint16_t*>(b + 64) = l;
}

// ---- 4 consecutive elements (i a multiple of 4)
template <typename T> __device__ __forceinline__ void ld4(const T* p, long i, float* v);
template <> __device__ __forceinline__ void ld4<float>(const float* p, long i, float* v) {
    const float4 t = *reinterpret_cast<const float4*>(p + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <> __device__ __forceinline__ void ld4<bf16_t>(const bf16_t* p, long i, float* v) {
    const uint2 t = *reinterpret_cast<const uint2*>(p + i);
    v[0] = bf2f((bf16_t)(t.x & 0xffff)); v[1] = bf2f((bf16_t)(t.x >> 16));
    v[2] = bf2f((bf16_t)(t.y & 0xffff)); v[3] = bf2f((bf16_t)(t.y >> 16));
}
template <> __device__ __forceinline__ void ld4<sp32_t>(const sp32_t* p, long i, float* v) {
    const char* b = reinterpret_cast<const char*>(p) + sp32_byte(i);
    sp_join4(*reinterpret_cast<const uint2*>(b), *reinterpret_cast<const uint2*>(b + 64), v);
}
template <typename T> __device__ __forceinline__ void st4(T* p, long i, const float* v, unsigned* ovf = nullptr);
template <> __device__ __forceinline__ void st4<float>(float* p, long i, const float* v, unsigned*) {
    *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void st4<bf16_t>(bf16_t* p, long i, const float* v, unsigned*) {
    uint2 t;
    t.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
    t.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
    *reinterpret_cast<uint2*>(p + i) = t;
}
template <> __device__ __forceinline__ void st4<sp32_t>(sp32_t* p, long i, const float* v, unsigned* ovf) {
    char* b = reinterpret_cast<char*>(p) + sp32_byte(i);
    float amax = 0.f;
    uint2 h, l;
    sp_split4(v, amax, h, l);
    sp_count_now(ovf, amax);
    *reinterpret_cast<uint2*>(b) = h;
    *reinterpret_cast<uint2*>(b + 64) = l;
}

// ---- 8 consecutive elements (i a multiple of 8).  The sp32 forms move ONE 16-byte piece per half: 8-byte accesses run at
// 0.54-0.70 x the 16-byte rate on this part (MI355X_MICROARCH.md), and conv0 / LayerNorm / the average pool were written
// with the 4-element helpers above (conv0 at 2 x its write floor, the pool at 2 x its read floor: round-4 review, item 7b).
template <typename T> __device__ __forceinline__ void ld8(const T* p, long i, float* v) {
    ld4<T>(p, i, v);
    ld4<T>(p, i + 4, v + 4);
}
template <> __device__ __forceinline__ void ld8<sp32_t>(const sp32_t* p, long i, float* v) {
    const char* b = reinterpret_cast<const char*>(p) + sp32_byte(i);
    sp_join8(*reinterpret_cast<const uint4*>(b), *reinterpret_cast<const uint4*>(b + 64), v);
}
template <typename T> __device__ __forceinline__ void st8(T* p, long i, const float* v, unsigned* ovf = nullptr) {
    st4<T>(p, i, v, ovf);
    st4<T>(p, i + 4, v + 4, ovf);
}
template <> __device__ __forceinline__ void st8<sp32_t>(sp32_t* p, long i, const float* v, unsigned* ovf) {
    char* b = reinterpret_cast<char*>(p) + sp32_byte(i);
    float amax = 0.f;
    uint4 h, l;
    sp_split8(v, amax, h, l);
    sp_count_now(ovf, amax);
    *reinterpret_cast<uint4*>(b) = h;
    *reinterpret_cast<uint4*>(b + 64) = l;
}
