// Validation of audio checkpoints: the epoch loss of a corpus's window logits (NetTrainer.iterate_model's bookkeeping,
// src/audio/net_trainer/net_trainer.py:391-465, over torch's CrossEntropyLoss(weight, label_smoothing) or the SoftFocalLoss of
// src/audio/loss/loss.py:125-137) and the concordance coefficient of accuracy_utils.ccc_score.  Definitions: include/avcer_hip.h
// avcer_window_losses, avcer_ccc; stated in numpy by avcer_amd/validate.py (losses_numpy, ccc_numpy), which referee
// tests/test_gpu_validate.py.  All arithmetic is float64.
//
// avcer_window_losses: ONE launch, one block per DataLoader batch.  Thread t takes the batch's rows t, t + 256, ..: the
// max-subtracted log-softmax of the row, its loss terms, and three running sums.  The 256 partial sums fold in halves through LDS
// (block_fold): the order of every addition is fixed by the shapes alone, and there is no floating-point atomic anywhere, so a
// result is a pure function of its inputs.  The epoch figures need every batch: each block publishes its batch loss and draws an
// integer ticket; the block that draws the last one reads all batch losses back and folds them the same way.  The hand-off is
// the release / ticket / acquire sequence of a split-K reduction: plain store, agent-scope release, relaxed agent-scope add;
// the last arriver's agent-scope acquire, a workgroup barrier, and loads that pass the CU's vector cache by.
//
// Both kernels are launch-bound at any real size (a corpus has thousands of windows of 7 or 8 logits: tens of kilobytes);
// nothing here is tuned beyond one launch per call.
//
// targets comes from device memory: a value outside [0, c) selects nothing (every class-indexed read is a select over k < c)
// and turns its row into NaN.
//
// Every product, sum and quotient rounds on its own, as numpy's do: contraction is off for this whole file (see search.hip).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_C = AVCER_LOSS_MAX_CLASSES;
constexpr int LS_FLAG = 3 * LS_THREADS;  // the slot of the "this block drew the last ticket" word behind the three sum columns

// K columns of 256 partial sums, one per thread, folded in halves: v[k] of EVERY thread becomes the column's sum
template <int K>
__device__ __forceinline__ void block_fold(double (&v)[K], double* sh) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k * LS_THREADS + t] = v[k];
    __syncthreads();
    for (int d = LS_THREADS / 2; d >= 1; d >>= 1) {
        if (t < d)
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k * LS_THREADS + t] = sh[k * LS_THREADS + t] + sh[k * LS_THREADS + t + d];
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sh[k * LS_THREADS];
    __syncthreads();  // the columns may be written again
}

__global__ void __launch_bounds__(LS_THREADS) window_losses_kernel(const float* __restrict__ logits, const int32_t* __restrict__ targets,
                                                                   const float* __restrict__ weights, long n, int c, int kind,
                                                                   double keep, double smooth, double gamma, long bsz, long n_batches,
                                                                   double* __restrict__ row_loss, double* batch_loss,
                                                                   double* __restrict__ epoch, int* ticket) {
    __shared__ double sh[3 * LS_THREADS + 1];
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    const long r0 = b * bsz, r1 = r0 + bsz < n ? r0 + bsz : n;
    double w[LS_C];
#pragma unroll
    for (int k = 0; k < LS_C; ++k) w[k] = k < c ? (weights ? (double)weights[k] : 1.0) : 0.0;
    double acc[3] = {0.0, 0.0, 0.0};  // A, G, U of include/avcer_hip.h
    for (long i = r0 + t; i < r1; i += LS_THREADS) {
        const int y = targets[i];
        double d[LS_C];
#pragma unroll
        for (int k = 0; k < LS_C; ++k) d[k] = k < c ? (double)logits[i * c + k] : 0.0;
        double m = d[0];
#pragma unroll
        for (int k = 1; k < LS_C; ++k) m = (k < c && d[k] > m) ? d[k] : m;
        double s = 0.0, wy = NAN, dy = NAN, ey = NAN;  // a target outside [0, c) selects nothing
#pragma unroll
        for (int k = 0; k < LS_C; ++k) {
            if (k < c) {
                d[k] = d[k] - m;
                const double e = exp(d[k]);
                s = k == 0 ? e : s + e;
                wy = k == y ? w[k] : wy;
                dy = k == y ? d[k] : dy;
                ey = k == y ? e : ey;
            }
        }
        double a, g = 0.0, row;
        if (kind == AVCER_LOSS_CE) {
            const double l = log(s);
            a = wy * -(dy - l);
#pragma unroll
            for (int k = 0; k < LS_C; ++k) {
                if (k < c) {
                    const double term = w[k] * -(d[k] - l);
                    g = k == 0 ? term : g + term;
                }
            }
            row = keep * a + smooth * g;
        } else {
            double p = ey / s;
            p = p < 1e-7 ? 1e-7 : (p > 1.0 - 1e-7 ? 1.0 - 1e-7 : p);
            const double q = 1.0 - p;
            const double f = gamma == 0.0 ? 1.0 : (gamma == 2.0 ? q * q : pow(q, gamma));
            a = (wy * f) * -log(p);
            row = a;
        }
        row_loss[i] = row;
        acc[0] = acc[0] + a;
        acc[1] = acc[1] + g;
        acc[2] = acc[2] + wy;
    }
    block_fold<3>(acc, sh);
    if (t == 0) {
        const double loss = kind == AVCER_LOSS_CE ? keep * (acc[0] / acc[2]) + smooth * (acc[1] / acc[2]) : acc[0] / (double)(r1 - r0);
        batch_loss[b] = loss;
        // publish, then draw the ticket: the store has left this wave, the agent-scope release has written it back, and only
        // then does the counter move
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int drawn = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = drawn == (int)(n_batches - 1);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        sh[LS_FLAG] = last ? 1.0 : 0.0;
    }
    __syncthreads();
    if (sh[LS_FLAG] == 0.0) return;  // the whole block leaves
    // the last block: every batch loss is published.  The loads below are agent-scope atomic loads (they pass this CU's vector
    // cache by) behind the acquire above.
    double ep[2] = {0.0, 0.0};
    const unsigned long long* pub = (const unsigned long long*)batch_loss;
    for (long bb = t; bb < n_batches; bb += LS_THREADS) {
        const double loss = __longlong_as_double((long long)__hip_atomic_load(pub + bb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const long q0 = bb * bsz, q1 = q0 + bsz < n ? q0 + bsz : n;
        ep[0] = ep[0] + loss * (double)bsz;       // net_trainer.py:441: `loss_value.item() * dataloader.batch_size`, the short batch too
        ep[1] = ep[1] + loss * (double)(q1 - q0);
    }
    block_fold<2>(ep, sh);
    if (t == 0) {
        epoch[0] = ep[0] / (double)n_batches;     // :460: `running_loss / iters`
        epoch[1] = ep[1] / (double)n;
    }
}

__global__ void __launch_bounds__(LS_THREADS) ccc_kernel(const double* __restrict__ targets, const double* __restrict__ predicts, long n,
                                                         long stride, double* __restrict__ out) {
    __shared__ double sh[3 * LS_THREADS];
    const int t = threadIdx.x;
    double mean[2] = {0.0, 0.0};
    for (long i = t; i < n; i += LS_THREADS) {
        mean[0] = mean[0] + targets[i * stride];
        mean[1] = mean[1] + predicts[i * stride];
    }
    block_fold<2>(mean, sh);
    const double mt = mean[0] / (double)n, mp = mean[1] / (double)n;
    double sq[3] = {0.0, 0.0, 0.0};  // sxy, sxx, syy
    for (long i = t; i < n; i += LS_THREADS) {
        const double vy = targets[i * stride] - mt, vx = predicts[i * stride] - mp;
        sq[0] = sq[0] + vx * vy;
        sq[1] = sq[1] + vx * vx;
        sq[2] = sq[2] + vy * vy;
    }
    block_fold<3>(sq, sh);
    if (t == 0) {
        const double cor = sq[0] / (sqrt(sq[1]) * sqrt(sq[2]));
        const double sdt = sqrt(sq[2] / (double)n), sdp = sqrt(sq[1] / (double)n);
        out[0] = ((2.0 * cor) * sdt) * sdp / ((sdt * sdt + sdp * sdp) + (mt - mp) * (mt - mp));
    }
}

}  // namespace

extern "C" int avcer_window_losses(avcer_ctx* ctx, const float* logits, const int32_t* targets, const float* weights, int64_t n, int c,
                                   int kind, double label_smoothing, double gamma, int64_t batch_size, double* row_loss,
                                   double* batch_loss, double* epoch, int32_t* ticket, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (n < 1 || n > AVCER_VOTES_MAX_WINDOWS || c < 2 || c > AVCER_LOSS_MAX_CLASSES || batch_size < 1 || batch_size > 2147483647LL)
        return set_err(ctx, AVCER_EINVAL, "window losses: %lld windows (1..%lld), %d classes (2..%d), batch size %lld (1..2^31-1)",
                       (long long)n, (long long)AVCER_VOTES_MAX_WINDOWS, c, AVCER_LOSS_MAX_CLASSES, (long long)batch_size);
    if ((kind != AVCER_LOSS_CE && kind != AVCER_LOSS_SOFT_FOCAL) || !(label_smoothing >= 0.0 && label_smoothing <= 1.0) ||
        !(gamma >= 0.0 && gamma <= 1.0e300))
        return set_err(ctx, AVCER_EINVAL, "window losses: kind %d (0: CE, 1: soft focal), label smoothing %g (0..1), gamma %g (>= 0)", kind,
                       label_smoothing, gamma);
    if (!logits || !targets || !row_loss || !batch_loss || !epoch || !ticket) return set_err(ctx, AVCER_EINVAL, "window losses: null buffer");
    const long n_batches = ((long)n + (long)batch_size - 1) / (long)batch_size;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, hipMemsetAsync(ticket, 0, sizeof(int32_t), st));
    window_losses_kernel<<<(int)n_batches, LS_THREADS, 0, st>>>(logits, targets, weights, (long)n, c, kind, 1.0 - label_smoothing,
                                                                label_smoothing / (double)c, gamma, (long)batch_size, n_batches, row_loss,
                                                                batch_loss, epoch, ticket);
    CHECK_LAUNCH(ctx, "window losses");
    return AVCER_OK;
}

extern "C" int avcer_ccc(avcer_ctx* ctx, const double* targets, const double* predicts, int64_t n, int64_t stride, double* out,
                         avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (n < 1 || stride < 1 || stride > (1LL << 40) || (n - 1) > ((1LL << 40) - 1) / stride)
        return set_err(ctx, AVCER_EINVAL, "ccc: %lld elements (>= 1) at stride %lld (>= 1), (n - 1) * stride < 2^40", (long long)n,
                       (long long)stride);
    if (!targets || !predicts || !out) return set_err(ctx, AVCER_EINVAL, "ccc: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ccc_kernel<<<1, LS_THREADS, 0, (hipStream_t)stream>>>(targets, predicts, (long)n, (long)stride, out);
    CHECK_LAUNCH(ctx, "ccc");
    return AVCER_OK;
}
