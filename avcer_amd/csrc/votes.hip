// Window-wise majority voting of the audio model's corpus pass: the softmax of test_c_audio.py:48 and majority_voting
// (src/audio/utils/common_utils.py:74-108) for a whole corpus in ONE launch.  Definition: include/avcer_hip.h avcer_window_votes;
// stated in numpy by avcer_amd/audio_corpus.py (votes_numpy), which referees tests/test_gpu_audio_corpus.py.
//
// One wave per file.  Lane l takes the file's windows l, l + 64, ..: it reads the window's logits, writes its probabilities and its
// class, and counts the class and the target in registers (c <= 8 classes, targets from -2: 10 counters each).  A shuffle tree adds
// the 64 lanes' counters; every lane then holds the file's two histograms, picks the modes, and lanes 0 .. c-1 store the one-hot row.
// No LDS, no barrier, no atomics: a wave neither shares nor waits for anything, so the waves of a block are independent files.
//
// The kernel is launch-bound at any real corpus size (a few windows per file, 36 bytes in and 36 out per window): nothing here is
// tuned beyond one launch for the whole corpus.
//
// file_off comes from device memory: both ends of a file's range are clamped to [0, n] before they address anything.
//
// Every sum and quotient rounds on its own, as numpy's do: contraction is off for this whole file (see search.hip).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int VT_THREADS = 256;
constexpr int VT_WAVE = 64;
constexpr int VT_WAVES = VT_THREADS / VT_WAVE;  // files per block
constexpr int VT_C = AVCER_VOTES_MAX_CLASSES;
constexpr int VT_TBINS = VT_C - AVCER_VOTES_TARGET_MIN;  // target values AVCER_VOTES_TARGET_MIN .. VT_C - 1

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = VT_WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, VT_WAVE);
    return v;
}

// the smallest bin with the largest count, or -1 when every bin is empty
template <int N>
__device__ __forceinline__ int mode_bin(const int (&cnt)[N], int bins) {
    int best = 0, at = -1;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const bool take = k < bins && cnt[k] > best;
        best = take ? cnt[k] : best;
        at = take ? k : at;
    }
    return at;
}

__global__ void __launch_bounds__(VT_THREADS) window_votes_kernel(const float* __restrict__ logits, const int32_t* __restrict__ targets,
                                                                  const int32_t* __restrict__ file_off, long n, int c, int n_files,
                                                                  float* __restrict__ probs, int32_t* __restrict__ pred,
                                                                  int32_t* __restrict__ file_pred, int32_t* __restrict__ file_target,
                                                                  int32_t* __restrict__ file_onehot) {
    const int lane = threadIdx.x & (VT_WAVE - 1);
    const int f = blockIdx.x * VT_WAVES + (threadIdx.x >> 6);
    if (f >= n_files) return;  // the whole wave leaves: nothing below waits for another wave
    long w0 = file_off[f], w1 = file_off[f + 1];
    w0 = w0 < 0 ? 0 : (w0 > n ? n : w0);
    w1 = w1 < w0 ? w0 : (w1 > n ? n : w1);
    int cp[VT_C], ct[VT_TBINS];
#pragma unroll
    for (int k = 0; k < VT_C; ++k) cp[k] = 0;
#pragma unroll
    for (int k = 0; k < VT_TBINS; ++k) ct[k] = 0;
    for (long i = w0 + lane; i < w1; i += VT_WAVE) {
        float x[VT_C];
#pragma unroll
        for (int k = 0; k < VT_C; ++k) x[k] = k < c ? logits[i * c + k] : 0.f;
        // np.argmax: the first index of the maximum; the first NaN wins and nothing displaces it
        float best = x[0];
        int am = 0;
#pragma unroll
        for (int k = 1; k < VT_C; ++k) {
            const bool take = k < c && !(x[k] <= best) && best == best;
            best = take ? x[k] : best;
            am = take ? k : am;
        }
        float e[VT_C], den = 0.f;
#pragma unroll
        for (int k = 0; k < VT_C; ++k) {
            e[k] = k < c ? expf(x[k] - best) : 0.f;
            den = k == 0 ? e[0] : (k < c ? den + e[k] : den);
        }
#pragma unroll
        for (int k = 0; k < VT_C; ++k)
            if (k < c) probs[i * c + k] = e[k] / den;
        pred[i] = am;
        const int t = targets[i] - AVCER_VOTES_TARGET_MIN;
#pragma unroll
        for (int k = 0; k < VT_C; ++k) cp[k] += k == am;
#pragma unroll
        for (int k = 0; k < VT_TBINS; ++k) ct[k] += k == t && k < c - AVCER_VOTES_TARGET_MIN;
    }
#pragma unroll
    for (int k = 0; k < VT_C; ++k) cp[k] = wave_sum(cp[k]);
#pragma unroll
    for (int k = 0; k < VT_TBINS; ++k) ct[k] = wave_sum(ct[k]);
    const int fp = mode_bin(cp, c);
    const int tb = mode_bin(ct, c - AVCER_VOTES_TARGET_MIN);
    if (lane == 0) {
        file_pred[f] = fp;
        file_target[f] = tb < 0 ? -1 : tb + AVCER_VOTES_TARGET_MIN;
    }
    if (lane < c) file_onehot[(long)f * c + lane] = lane == fp;
}

}  // namespace

extern "C" int avcer_window_votes(avcer_ctx* ctx, const float* logits, const int32_t* targets, const int32_t* file_off, int64_t n, int c,
                                  int n_files, float* probs, int32_t* pred, int32_t* file_pred, int32_t* file_target,
                                  int32_t* file_onehot, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (n_files < 1 || n_files > AVCER_VOTES_MAX_FILES || n < 0 || n > AVCER_VOTES_MAX_WINDOWS || c < 2 || c > AVCER_VOTES_MAX_CLASSES)
        return set_err(ctx, AVCER_EINVAL, "window votes: %d files (1..%d), %lld windows (0..%lld), %d classes (2..%d)", n_files,
                       AVCER_VOTES_MAX_FILES, (long long)n, (long long)AVCER_VOTES_MAX_WINDOWS, c, AVCER_VOTES_MAX_CLASSES);
    if (!file_off || !file_pred || !file_target || !file_onehot || (n && (!logits || !targets || !probs || !pred)))
        return set_err(ctx, AVCER_EINVAL, "window votes: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    window_votes_kernel<<<cdiv(n_files, VT_WAVES), VT_THREADS, 0, (hipStream_t)stream>>>(logits, targets, file_off, (long)n, c, n_files, probs,
                                                                                         pred, file_pred, file_target, file_onehot);
    CHECK_LAUNCH(ctx, "window votes");
    return AVCER_OK;
}
