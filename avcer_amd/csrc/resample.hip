// Source audio -> mono float32 at the model's rate in one launch (data/utils.py:50-57: torchaudio.load's int16 / 32768, the
// channel mean, torchaudio.transforms.Resample with its defaults).  Definition and table layout: include/avcer_hip.h
// avcer_resample; the tap table is built on the host (avcer_amd/audio_pipeline.py resample_plan).
//
// Shape.  The resampler is a polyphase FIR with period o samples in / n samples out.  One block owns `qb` whole periods: it
// stages the qb * o + 2 * width mono samples they read in LDS once -- converted and downmixed on the way, so the source is read
// from HBM once -- and every thread then produces RS_R outputs of ONE phase p in RS_R consecutive periods, so a tap is loaded
// once for RS_R products.  Taps come straight from global memory in tap-major order ([span][n]: lanes of a wave hold consecutive
// p, the load is coalesced and the whole table stays in L1 / L2); they are never staged, so the table's size is bounded by the
// documented limits alone, not by LDS.  Each output is accumulated in f64 -- a product of two f32 values is exact there, the
// running sum rounds at 2^-53 per FMA -- and converted to f32 once at the end, so its error against the exact sum is that one
// f32 rounding plus ~1e-16: what no f32 summation order, the reference's conv1d included, improves on.  The f64 FMAs run at half
// the f32 rate; what that costs is in profiles/resample_bench.json ("Audio front end").
#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_R = 4;               // outputs per thread that share a tap
constexpr int RS_LDS_FLOATS = 12288;  // staged mono samples per block (48 KiB)
constexpr int RS_ITEMS = 512;         // (phase, period group) items a block aims for: two per thread

inline long cdivl(long a, long b) { return (a + b - 1) / b; }

// kinds of `src`: what the launch functions select from (src_kind, channels, alignment)
enum { K_S16 = 0, K_S16_STEREO = 1, K_F32 = 2 };

// Sample i of the mono signal, 0 outside [0, len).  int16: s / 32768 (exact); channels > 1: the f32 sum in channel order
// divided by the channel count, as wav.mean(dim=0) -- exact for <= 2 channels, and for int16 input at any count up to 8.
template <int KIND>
__device__ __forceinline__ float mono_at(const void* __restrict__ src, long i, long len, int ch) {
    if (i < 0 || i >= len) return 0.f;
    constexpr float s16 = 1.f / 32768.f;
    if (KIND == K_S16_STEREO) {  // one aligned 4-byte load per frame
        const int32_t v = ((const int32_t*)src)[i];
        return ((float)(int16_t)(v & 0xffff) * s16 + (float)(int16_t)(v >> 16) * s16) / 2.f;
    }
    float a = 0.f;
    if (KIND == K_S16) {
        const int16_t* s = (const int16_t*)src + i * ch;
        for (int c = 0; c < ch; ++c) a += (float)s[c] * s16;
    } else {
        const float* s = (const float*)src + i;
        for (int c = 0; c < ch; ++c) a += s[(long)c * len];
    }
    return ch > 1 ? a / (float)ch : a;
}

template <int KIND>
__global__ void __launch_bounds__(RS_THREADS) resample_kernel(const void* __restrict__ src, long len, int ch,
                                                              const float* __restrict__ taps, const int32_t* __restrict__ first,
                                                              int o, int n, int span, int width, int qb, long n_out,
                                                              float* __restrict__ y) {
    extern __shared__ float xs[];  // xs[s] = mono(q0 * o - width + s): the zero-padded signal the dense form convolves
    const int tid = threadIdx.x;
    const long q0 = (long)blockIdx.x * qb;
    const int staged = qb * o + 2 * width;
    const long b0 = q0 * o - width;
    for (int s = tid; s < staged; s += RS_THREADS) xs[s] = mono_at<KIND>(src, b0 + s, len, ch);
    __syncthreads();
    const int items = n * (qb / RS_R);
    for (int it = tid; it < items; it += RS_THREADS) {
        const int p = it % n, qg = it / n;
        const int base = qg * RS_R * o + first[p];
        double acc[RS_R];
#pragma unroll
        for (int r = 0; r < RS_R; ++r) acc[r] = 0.0;
        for (int j = 0; j < span; ++j) {
            const double t = (double)taps[(long)j * n + p];
            // 0 <= first[p] and first[p] + span <= 2 * width + o by the table's contract, so 0 <= base + r * o + j < staged; the
            // clamp to both ends makes a table that breaks it give wrong numbers instead of reading outside the block's LDS
#pragma unroll
            for (int r = 0; r < RS_R; ++r) acc[r] = fma(t, (double)xs[min(max(base + r * o + j, 0), staged - 1)], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < RS_R; ++r) {
            const long m = (q0 + qg * RS_R + r) * n + p;
            if (m < n_out) y[m] = (float)acc[r];
        }
    }
}

// orig_freq == new_freq: conversion and downmix alone (data/utils.py:50-54 skips the transform)
template <int KIND>
__global__ void __launch_bounds__(RS_THREADS) downmix_kernel(const void* __restrict__ src, long len, int ch, float* __restrict__ y) {
    for (long i = (long)blockIdx.x * RS_THREADS + threadIdx.x; i < len; i += (long)gridDim.x * RS_THREADS)
        y[i] = mono_at<KIND>(src, i, len, ch);
}

}  // namespace

extern "C" int avcer_resample(avcer_ctx* ctx, const void* src, int src_kind, int64_t len, int channels, const float* taps,
                              const int32_t* first, int o, int n, int span, int width, float* out, int64_t n_out,
                              avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (len < 0 || len > AVCER_RESAMPLE_MAX_LEN || channels < 1 || channels > AVCER_RESAMPLE_MAX_CHANNELS ||
        (src_kind != AVCER_PCM_S16_INTERLEAVED && src_kind != AVCER_PCM_F32_PLANAR))
        return set_err(ctx, AVCER_EINVAL, "resample: bad arguments (len %lld, channels %d, src_kind %d)", (long long)len, channels,
                       src_kind);
    const bool same = taps == nullptr;  // no table: equal rates
    if (same ? (first != nullptr || o != 1 || n != 1)
             : (!first || o < 1 || n < 1 || o > AVCER_RESAMPLE_MAX_O || n > AVCER_RESAMPLE_MAX_N || span < 1 ||
                span > AVCER_RESAMPLE_MAX_SPAN || width < 0 || span > 2 * width + o))
        return set_err(ctx, AVCER_EINVAL, "resample: reduced rates %d -> %d with %d taps per phase (width %d) are outside the supported "
                       "range (o <= %d, n <= %d, span <= %d)", o, n, span, width, AVCER_RESAMPLE_MAX_O, AVCER_RESAMPLE_MAX_N,
                       AVCER_RESAMPLE_MAX_SPAN);
    if (n_out != (same ? len : (int64_t)cdivl((long)n * len, o)))
        return set_err(ctx, AVCER_EINVAL, "resample: n_out %lld, expected ceil(n * len / o)", (long long)n_out);
    if (len == 0) return AVCER_OK;
    if (!src || !out) return set_err(ctx, AVCER_EINVAL, "resample: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int kind = src_kind == AVCER_PCM_F32_PLANAR ? K_F32
                     : (channels == 2 && ((uintptr_t)src & 3) == 0) ? K_S16_STEREO : K_S16;
    if (same) {
        const int grid = (int)(cdivl(len, RS_THREADS) < 2048 ? cdivl(len, RS_THREADS) : 2048);
        if (kind == K_F32) downmix_kernel<K_F32><<<grid, RS_THREADS, 0, st>>>(src, len, channels, out);
        else if (kind == K_S16_STEREO) downmix_kernel<K_S16_STEREO><<<grid, RS_THREADS, 0, st>>>(src, len, channels, out);
        else downmix_kernel<K_S16><<<grid, RS_THREADS, 0, st>>>(src, len, channels, out);
        HIP_TRY(ctx, hipGetLastError());
        return AVCER_OK;
    }
    // periods per block: a multiple of RS_R, about RS_ITEMS (phase, period group) items, within the LDS budget.  A table of the
    // documented limits has width <= span / 2 + 1, so RS_R * o + 2 * width <= 4 * 2048 + 130 floats fits; any other width is refused.
    int qb = RS_R * (int)cdivl(RS_ITEMS, n);
    const int fit = (RS_LDS_FLOATS - 2 * width) / o / RS_R * RS_R;
    if (fit < RS_R) return set_err(ctx, AVCER_EINVAL, "resample: width %d does not fit the staging buffer", width);
    if (qb > fit) qb = fit;
    const long periods = cdivl(n_out, n);
    const long grid = cdivl(periods, qb);
    if (grid >= (1L << 31)) return set_err(ctx, AVCER_EINVAL, "resample: signal too long");
    const size_t lds = (size_t)(qb * o + 2 * width) * sizeof(float);
#define RS_LAUNCH(K) resample_kernel<K><<<(unsigned)grid, RS_THREADS, lds, st>>>(src, len, channels, taps, first, o, n, span, width, qb, n_out, out)
    if (kind == K_F32) RS_LAUNCH(K_F32);
    else if (kind == K_S16_STEREO) RS_LAUNCH(K_S16_STEREO);
    else RS_LAUNCH(K_S16);
#undef RS_LAUNCH
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}
