// The waveform augmentations of the reference's AUGMENTATION=True recipe on the padded windows avcer_audio_chunks wrote, in place:
// RandomChoice([PolarityInversion(), WhiteNoise(), Gain()]) of src/audio/train_c_audio.py:112-119,
// src/audio/augmentation/wave_augmentation.py:8-108.  Definition: include/avcer_hip.h avcer_wave_augment; stated in numpy by
// avcer_amd/augment.py (augment_numpy, philox4x32, normal_stream), which referees tests/test_gpu_augment.py.
//   Gain is torchaudio.transforms.Vol(gain, "db") (torchaudio==2.1.2, third party, BSD-2): transforms/_transforms.py Vol.forward
//   calls functional/functional.py gain -- `ratio = 10 ** (gain_db / 20); return waveform * ratio`, a Python float times a float32
//   tensor, that is a float32 scalar -- and ends in `torch.clamp(waveform, -1, 1)`.
//
// Shape.  A window is cut into P = ceil(win / CH) parts of CH samples, CH = 4096 * ceil(win / 2^20): P <= 256 at every win and
// P = 16 at the 64 000 samples of a 4 s window, so a pass of 128 windows is 2048 workgroups on 256 CUs where one workgroup a
// window would leave half of them idle.  Two launches of n * P workgroups:
//   aug_stats_kernel   kind 2 alone: the part's sum in f64 and, around the part's own mean, its sum of squared deviations; both
//                      go to parts[w][p].  The part is read twice, the second time from L2 (16 KB).
//   aug_apply_kernel   every workgroup of a kind-2 window folds the window's P pairs -- the same P pairs in the same order, so
//                      all of them hold the same std -- and then works on its own part: one Philox4x32-10 block per four samples.
// Every fold is fixed: a thread chains the samples of its quads (four consecutive samples) t, t + 256, .. upwards, 256 partials
// fold in halves through LDS.  Nothing depends on n, on the window's place in the call or on a neighbour: no atomics, no tickets,
// no waits but workgroup barriers.  A workgroup of kind 0 leaves before it reads or writes a sample.
//
// Traffic: kinds 1 and 3 read and write a sample once; kind 2 reads it three times (the part's second sweep from L2) and writes
// it once, and pays ten Philox rounds, one logf and sqrtf and a cospif / sinpif pair per two samples.  Measured
// (tools/augment_bench.py, profiles/augment_bench.json: 228 windows of 64 000 samples, 58 MB, the whole call between two events):
// 0.042 ms gain, 0.054 ms polarity, 0.063 ms noise, against 0.020 ms for a device-to-device copy of the same buffer.  The noise
// path costs 0.02 ms more than the others for twice their reads and the whole generator, so neither binds the call at this
// size; the call's fixed part (the record upload, one or two launches) is inside every figure and was not separated.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AG_THREADS = 256;
constexpr int AG_TILE = 4096;           // samples a workgroup takes per sweep: four quads a thread
constexpr long AG_SPLIT = 1L << 20;     // a part grows by one tile per 2^20 samples of the window: P <= 256
static_assert(AVCER_AUGMENT_PARTS == AG_THREADS, "a window's parts are folded one per thread");

__host__ __device__ inline long ag_part_len(long win) { return (long)AG_TILE * ((win + AG_SPLIT - 1) / AG_SPLIT); }
__host__ __device__ inline int ag_parts(long win) { const long ch = ag_part_len(win); return (int)((win + ch - 1) / ch); }

// 256 f64 partials folded in halves: every thread gets the sum
__device__ __forceinline__ double fold_f64(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = AG_THREADS / 2; d >= 1; d >>= 1) {
        if (t < d) sh[t] = sh[t] + sh[t + d];
        __syncthreads();
    }
    const double s = sh[0];
    __syncthreads();
    return s;
}

// the quad at samples i0 .. i0 + 3 of a window of `win` samples: a 16-byte access where the window's rows are aligned, else by
// sample; samples at and behind `win` read as 0 and are not written
__device__ __forceinline__ void load_quad(const float* row, long i0, long win, bool vec, float (&v)[4]) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(row + i0);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < win ? row[i0 + j] : 0.0f;
    }
}
__device__ __forceinline__ void store_quad(float* row, long i0, long win, bool vec, const float (&v)[4]) {
    if (vec) {
        *reinterpret_cast<float4*>(row + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < win) row[i0 + j] = v[j];
    }
}

__global__ void __launch_bounds__(AG_THREADS) aug_stats_kernel(const float* __restrict__ chunks, const avcer_augment_rec* __restrict__ recs,
                                                               long win, int P, long ch, bool vec, double* __restrict__ parts) {
    __shared__ double sh[AG_THREADS];
    const long w = blockIdx.x / P;
    const int p = blockIdx.x % P;
    if (recs[w].kind != AVCER_AUGMENT_NOISE) return;  // the whole workgroup
    const float* row = chunks + w * win;
    const long lo = (long)p * ch, hi = lo + ch < win ? lo + ch : win;
    double s = 0.0;
    for (long i0 = lo + 4L * threadIdx.x; i0 < hi; i0 += 4L * AG_THREADS) {
        float v[4];
        load_quad(row, i0, win, vec, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) s = s + (double)v[j];  // a sample behind `win` adds +0
    }
    s = fold_f64(s, sh);
    const double mean = s / (double)(hi - lo);
    double m2 = 0.0;
    for (long i0 = lo + 4L * threadIdx.x; i0 < hi; i0 += 4L * AG_THREADS) {
        float v[4];
        load_quad(row, i0, win, vec, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double d = (double)v[j] - mean;
            m2 = i0 + j < hi ? m2 + d * d : m2;
        }
    }
    m2 = fold_f64(m2, sh);
    if (threadIdx.x == 0) {
        parts[(w * P + p) * 2] = s;
        parts[(w * P + p) * 2 + 1] = m2;
    }
}

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0, c[1] = (uint32_t)p1, c[2] = n2, c[3] = (uint32_t)p0;
}

// Philox4x32-10 (Salmon et al., SC'11) at counter (q, 0) under `key`, and the four normal values of its two Box-Muller pairs
__device__ __forceinline__ void normal_quad(uint64_t key, uint64_t q, float (&z)[4]) {
    uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), 0u, 0u};
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = (float)((c[2 * h] >> 8) + 1u) * 0x1p-24f;   // (0, 1]: exact
        const float u2 = (float)(c[2 * h + 1] >> 8) * 0x1p-23f;      // 2 * u2 in [0, 2): exact
        const float r = sqrtf(-2.0f * logf(u1));
        z[2 * h] = r * cospif(u2);
        z[2 * h + 1] = r * sinpif(u2);
    }
}

__global__ void __launch_bounds__(AG_THREADS) aug_apply_kernel(float* __restrict__ chunks, const avcer_augment_rec* __restrict__ recs,
                                                               long win, int P, long ch, bool vec, double min_snr, double max_snr,
                                                               const float* __restrict__ noise, const double* __restrict__ parts,
                                                               float* __restrict__ std_out) {
    __shared__ double sh[AG_THREADS];
    const long w = blockIdx.x / P;
    const int p = blockIdx.x % P, t = threadIdx.x;
    const avcer_augment_rec rec = recs[w];
    if (rec.kind == AVCER_AUGMENT_NONE) return;  // the whole workgroup: not a byte of the window is touched
    float* row = chunks + w * win;
    const long lo = (long)p * ch, hi = lo + ch < win ? lo + ch : win;

    double noise_std = 0.0;
    if (rec.kind == AVCER_AUGMENT_NOISE && !noise) {
        // torch.std: sqrt(sum((x - mean)^2) / (win - 1)); the window's sum of squared deviations from those of its parts
        const long len = (long)t * ch + ch < win ? ch : win - (long)t * ch;  // of part t
        const double s = t < P ? parts[(w * P + t) * 2] : 0.0;
        const double mean = fold_f64(s, sh) / (double)win;
        double m2 = 0.0;
        if (t < P) {
            const double d = s / (double)len - mean;
            m2 = parts[(w * P + t) * 2 + 1] + (double)len * (d * d);
        }
        m2 = fold_f64(m2, sh);
        const float std32 = (float)sqrt(m2 / (double)(win - 1));  // win == 1: 0 / 0
        if (std_out && p == 0 && t == 0) std_out[w] = std32;
        const double a = min_snr * (double)std32, b = max_snr * (double)std32;
        noise_std = a + (b - a) * rec.u;  // random.uniform(a, b)
    }
    const float* nz = noise ? noise + w * win : nullptr;
    for (long i0 = lo + 4L * t; i0 < hi; i0 += 4L * AG_THREADS) {
        float v[4];
        load_quad(row, i0, win, vec, v);
        if (rec.kind == AVCER_AUGMENT_POLARITY) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = -v[j];
        } else if (rec.kind == AVCER_AUGMENT_GAIN) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float g = v[j] * rec.ratio;
                v[j] = g < -1.0f ? -1.0f : (g > 1.0f ? 1.0f : g);  // torch.clamp: NaN stays NaN
            }
        } else if (nz) {
            float e[4];
            load_quad(nz, i0, win, vec, e);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] + e[j];
        } else {
            float z[4];
            normal_quad(rec.key, (uint64_t)(i0 >> 2), z);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] + (float)(noise_std * (double)z[j]);
        }
        store_quad(row, i0, win, vec, v);
    }
}

bool ag_finite(double v) { return v == v && v < 1.0e300 && v > -1.0e300; }

}  // namespace

extern "C" int avcer_wave_augment(avcer_ctx* ctx, float* chunks, int64_t n, int64_t win, const avcer_augment_rec* recs,
                                  avcer_augment_rec* recs_dev, double min_snr, double max_snr, const float* noise, double* parts,
                                  float* std_out, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (n == 0) return AVCER_OK;
    if (n < 0 || win < 1 || win > AVCER_AUGMENT_MAX_WIN)
        return set_err(ctx, AVCER_EINVAL, "wave augment: %lld windows (>= 0) of %lld samples (1..%lld)", (long long)n, (long long)win,
                       (long long)AVCER_AUGMENT_MAX_WIN);
    const int P = ag_parts((long)win);
    if (n > AVCER_AUGMENT_MAX_ELEMS / win || n * (int64_t)P > 2147483647LL)
        return set_err(ctx, AVCER_EINVAL, "wave augment: %lld windows of %lld samples: n * win <= 2^40 and n * %d parts < 2^31", (long long)n,
                       (long long)win, P);
    if (!chunks || !recs || !recs_dev || !parts) return set_err(ctx, AVCER_EINVAL, "wave augment: null buffer");
    if (!ag_finite(min_snr) || !ag_finite(max_snr) || min_snr > max_snr)
        return set_err(ctx, AVCER_EINVAL, "wave augment: min_snr %g <= max_snr %g expected, both finite", min_snr, max_snr);
    bool any = false, any_noise = false;
    for (int64_t i = 0; i < n; ++i) {
        const avcer_augment_rec& r = recs[i];
        if (r.kind < AVCER_AUGMENT_NONE || r.kind > AVCER_AUGMENT_GAIN || !(r.u >= 0.0 && r.u < 1.0) ||
            (r.kind == AVCER_AUGMENT_GAIN && r.ratio != r.ratio))
            return set_err(ctx, AVCER_EINVAL, "wave augment: window %lld: kind %d (0 none, 1 polarity, 2 noise, 3 gain), u %g in [0, 1), ratio %g",
                           (long long)i, r.kind, r.u, (double)r.ratio);
        any = any || r.kind != AVCER_AUGMENT_NONE;
        any_noise = any_noise || r.kind == AVCER_AUGMENT_NOISE;
    }
    if (!any) return AVCER_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, hipMemcpyAsync(recs_dev, recs, sizeof(avcer_augment_rec) * (size_t)n, hipMemcpyHostToDevice, st));
    const long ch = ag_part_len((long)win);
    const int grid = (int)(n * P);
    // 16-byte accesses where every row starts on one; the order of the sums is the same either way
    const bool vec = (win & 3) == 0 && ((uintptr_t)chunks & 15) == 0 && ((uintptr_t)noise & 15) == 0;
    if (any_noise && !noise) {
        aug_stats_kernel<<<grid, AG_THREADS, 0, st>>>(chunks, recs_dev, (long)win, P, ch, vec, parts);
        CHECK_LAUNCH(ctx, "wave augment stats");
    }
    aug_apply_kernel<<<grid, AG_THREADS, 0, st>>>(chunks, recs_dev, (long)win, P, ch, vec, min_snr, max_snr, noise, parts, std_out);
    CHECK_LAUNCH(ctx, "wave augment");
    return AVCER_OK;
}
