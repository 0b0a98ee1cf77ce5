// Fitting the audio classifier head (feature_downsample, Linear F -> C) on extracted features: the train phase of
// NetTrainer.run (src/audio/net_trainer/net_trainer.py:357-467, 574-604; src/audio/train_c_audio.py:236-260) for the last layer
// alone, and the logits of a feature table under many fitted heads.  Definitions: include/avcer_hip.h avcer_head_fit,
// avcer_head_fit_views (an epoch's rows from one of several tables; one body, avcer_head_fit is its views = 1), avcer_head_apply;
// stated in numpy float64 by avcer_amd/head_fit.py (head_fit_numpy), which referees tests/test_gpu_head_fit.py.
//
// avcer_head_fit: ONE launch, one workgroup of 256 threads per run, nothing shared between workgroups.  A step is half a
// megaflop and waits for the step before it, so a run is launch-bound in any framework; here the whole run -- every epoch, every
// batch -- is one workgroup's loop, and a sweep of K runs is K workgroups of the same launch.
//   * thread t owns the feature columns t, t + 256, .. (J = 1, 2 or 4 of them) of W and of Adam's m and v, for all classes, in
//     REGISTERS from the first step to the last: 3 * CP * J floats (CP = 8 or 16 class slots), 192 at most.  The weight gradient
//     dW[:, f] = sum_b G[b, :] * x[b, f] then needs no other thread.
//   * the logits need all threads: 32 (row, class) values at a time, every thread's partial goes through LDS (32 x 256 floats),
//     eight threads add one value's 256 partials in a fixed order.  The B x C logits and then the B x C gradient rows live in LDS.
//   * the loss, its fold over the batch and its gradient are taken by thread b for row b (B <= 256), in f32.
// LDS: 33.1 KB of partials + 16 KB of logits + 7 KB of folds and row tables = 56 KB; registers: 246 VGPRs at 8 classes x 1024
// features, 256 + 119 accumulation registers at 16 x 1024, of the 512 a thread of a 256-thread workgroup can have.  The register
// file binds: above 256 registers a SIMD holds ONE wave, so a CU holds one workgroup; LDS (56 of 160 KB) would allow two.
//
// Loop bounds are arguments; the only waits are __syncthreads; no atomics, no tickets.  Row numbers, mixup positions and
// targets come from device memory: each is range-checked where it is read and an invalid one turns the step into NaN; nothing
// is indexed with an unchecked value.
//
// Products and sums round on their own (contraction is off for this file, see search.hip) EXCEPT the two dot products, which
// are explicit fmaf chains in the order the header states.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int HF_THREADS = 256;
constexpr int HF_VALUES = 32;                    // (row, class) logits reduced per LDS pass
constexpr int HF_GROUP = HF_THREADS / HF_VALUES; // 8 threads add one value's partials, 32 each
constexpr int HF_SPAN = HF_THREADS / HF_GROUP;   // 32 partials per adding thread
constexpr int HF_QSTRIDE = HF_SPAN + 1;          // a group's 32 partials and one pad word: the eight groups start in different banks
constexpr int HF_VSTRIDE = HF_GROUP * HF_QSTRIDE + 1;
constexpr int HF_MAX_B = AVCER_HEAD_MAX_BATCH;
constexpr int HF_HYPER = AVCER_HEAD_HYPER;

struct HeadFitArgs {
    const float* feats;
    const int32_t* view;  // [k_runs, epochs]: the table of feats [views, n, f] an epoch reads, or null: table 0
    const int32_t* targets;
    const double* hyper;
    const float* class_w;
    const float* w0;
    const float* b0;
    const int32_t* order;
    const float* mix_lam;
    const int32_t* mix_index;
    float* w_hist;
    float* b_hist;
    float* batch_loss;
    double* epoch_loss;
    int n, f, c, epochs, bsz, n_batches, views;
};

// three columns of 256 partial sums folded in halves: v[k] of EVERY thread becomes the column's sum (block_fold of losses.hip in f32)
__device__ __forceinline__ void fold3(float (&v)[3], float* sh) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 3; ++k) sh[k * HF_THREADS + t] = v[k];
    __syncthreads();
    for (int d = HF_THREADS / 2; d >= 1; d >>= 1) {
        if (t < d)
#pragma unroll
            for (int k = 0; k < 3; ++k) sh[k * HF_THREADS + t] = sh[k * HF_THREADS + t] + sh[k * HF_THREADS + t + d];
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = sh[k * HF_THREADS];
    __syncthreads();
}

// the J feature values of batch row b this thread owns, from the epoch's table `feats`: the row itself, or its mixup with the row
// at the drawn position
template <int J>
__device__ __forceinline__ void load_row(const HeadFitArgs& a, const float* feats, const int* row_sh, const int* mix_sh, int b, bool mix, float lam, float onem,
                                         float (&x)[J]) {
    const int t = threadIdx.x;
    const int r = row_sh[b];
    const int r2 = mix ? mix_sh[b] : 0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int f = t + HF_THREADS * j;
        float v = 0.0f;
        if (f < a.f) {
            v = r >= 0 ? feats[(long)r * a.f + f] : NAN;
            if (mix) {
                const float v2 = r2 >= 0 ? feats[(long)r2 * a.f + f] : NAN;
                v = lam * v + onem * v2;  // net_trainer.py:602 in f32
            }
        }
        x[j] = v;
    }
}

template <int CP, int J>
__global__ void __launch_bounds__(HF_THREADS) head_fit_kernel(HeadFitArgs a) {
    __shared__ float part[HF_VALUES * HF_VSTRIDE];
    __shared__ __attribute__((aligned(16))) float lg[HF_MAX_B * CP];  // the batch's logits, then its gradient rows
    __shared__ float fold_sh[3 * HF_THREADS];
    __shared__ float bias_sh[CP];
    __shared__ int row_sh[HF_MAX_B], mix_sh[HF_MAX_B], tgt_sh[HF_MAX_B], lab_sh[HF_MAX_B];
    constexpr int RP = HF_VALUES / CP;  // rows per reduction pass

    const int t = threadIdx.x;
    const long run = blockIdx.x;
    const int c = a.c, F = a.f, n = a.n;
    const double* hy = a.hyper + run * HF_HYPER;
    const int kind = (int)hy[0];
    const float keep = (float)(1.0 - hy[1]), smooth = (float)(hy[1] / (double)c), gamma = (float)hy[2];
    const double lr0 = hy[3], beta1 = hy[4], beta2 = hy[5], t0 = hy[7], eta_min = hy[8];
    const float epsf = (float)hy[6], w1 = (float)(1.0 - beta1), beta2f = (float)beta2, w2 = (float)(1.0 - beta2);
    const bool mix = hy[9] != 0.0;
    const double epoch0 = hy[10];  // the trainer's number of the first epoch (NetTrainer.run counts from 1)

    float cw[CP];
    float wsum = 0.0f;
#pragma unroll
    for (int k = 0; k < CP; ++k) {
        cw[k] = k < c ? a.class_w[run * c + k] : 0.0f;
        if (k < c) wsum = k == 0 ? cw[k] : wsum + cw[k];
    }

    float W[CP][J], M[CP][J], V[CP][J];
#pragma unroll
    for (int k = 0; k < CP; ++k)
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int f = t + HF_THREADS * j;
            W[k][j] = (k < c && f < F) ? a.w0[(run * c + k) * F + f] : 0.0f;
            M[k][j] = 0.0f;
            V[k][j] = 0.0f;
        }
    float bias = t < c ? a.b0[run * c + t] : 0.0f, bm = 0.0f, bv = 0.0f;  // thread k < c owns bias k
    if (t < CP) bias_sh[t] = bias;

    double lr = lr0, b1t = 1.0, b2t = 1.0;
    const int v_red = t / HF_GROUP, q_red = t % HF_GROUP;  // the value this thread adds partials of, and which 32 of them
    __syncthreads();

    for (int e = 0; e < a.epochs; ++e) {
        double running = 0.0;
        // the epoch's table of feature rows; a view out of range makes every row of the epoch invalid
        const int view = a.view ? a.view[run * a.epochs + e] : 0;
        const bool view_ok = view >= 0 && view < a.views;
        const float* feats = a.feats + (view_ok ? (long)view * n * F : 0L);
        for (int i = 0; i < a.n_batches; ++i) {
            const int r0 = i * a.bsz;
            const int nb = n - r0 < a.bsz ? n - r0 : a.bsz;
            const float lam = mix ? a.mix_lam[(run * a.epochs + e) * a.n_batches + i] : 1.0f;
            const float onem = 1.0f - lam;
            // ---- the batch's rows, targets and mixup partners
            int pos = -1;
            if (t < nb) {
                const long at = (run * a.epochs + e) * (long)n + r0 + t;
                const int r = a.order[at];
                const bool ok = view_ok && r >= 0 && r < n;
                row_sh[t] = ok ? r : -1;
                tgt_sh[t] = ok ? a.targets[r] : -1;
                if (mix) {
                    pos = a.mix_index[at];
                    pos = (pos >= 0 && pos < nb) ? pos : -1;
                }
            }
            __syncthreads();
            if (t < nb) {
                int y = tgt_sh[t];
                if (mix) {
                    mix_sh[t] = pos >= 0 ? row_sh[pos] : -1;
                    const int y2 = pos >= 0 ? tgt_sh[pos] : -1;
                    // argmax(lam * onehot(y) + (1 - lam) * onehot(y2)), the first maximum (net_trainer.py:603-604)
                    y = (y < 0 || y2 < 0) ? -1 : (lam > onem ? y : (lam < onem ? y2 : (y < y2 ? y : y2)));
                }
                lab_sh[t] = y;
            }
            __syncthreads();

            // ---- forward: logits[b, k] = fold(partials) + bias[k], RP rows per pass
            for (int p0 = 0; p0 < nb; p0 += RP) {
#pragma unroll
                for (int rr = 0; rr < RP; ++rr) {
                    const int b = p0 + rr;
                    float x[J];
                    if (b < nb) load_row<J>(a, feats, row_sh, mix_sh, b, mix, lam, onem, x);
#pragma unroll
                    for (int k = 0; k < CP; ++k) {
                        float s = 0.0f;
                        if (b < nb && k < c) {
#pragma unroll
                            for (int j = 0; j < J; ++j) s = fmaf(x[j], W[k][j], s);
                        }
                        part[(rr * CP + k) * HF_VSTRIDE + (t / HF_SPAN) * HF_QSTRIDE + (t % HF_SPAN)] = s;
                    }
                }
                __syncthreads();
                {
                    const float* src = part + v_red * HF_VSTRIDE + q_red * HF_QSTRIDE;
                    float s = src[0];
                    for (int k = 1; k < HF_SPAN; ++k) s = s + src[k];
                    s = s + __shfl_xor(s, 1);
                    s = s + __shfl_xor(s, 2);
                    s = s + __shfl_xor(s, 4);
                    const int b = p0 + v_red / CP, k = v_red % CP;
                    if (q_red == 0 && b < nb && k < c) lg[b * CP + k] = s + bias_sh[k];
                }
                __syncthreads();
            }

            // ---- the loss of row t, the batch sums, the gradient row
            float acc3[3] = {0.0f, 0.0f, 0.0f};  // A, G, U of avcer_window_losses
            float pk[CP];
            float wy = NAN, py = NAN, dldp = 0.0f;
            int y = -1;
            if (t < nb) {
                y = lab_sh[t];
                float d[CP];
#pragma unroll
                for (int k = 0; k < CP; ++k) d[k] = k < c ? lg[t * CP + k] : 0.0f;
                float m = d[0];
#pragma unroll
                for (int k = 1; k < CP; ++k) m = (k < c && d[k] > m) ? d[k] : m;
                float s = 0.0f, dy = NAN, ey = NAN;
#pragma unroll
                for (int k = 0; k < CP; ++k) {
                    pk[k] = 0.0f;
                    if (k < c) {
                        d[k] = d[k] - m;
                        pk[k] = expf(d[k]);
                        s = k == 0 ? pk[k] : s + pk[k];
                        wy = k == y ? cw[k] : wy;
                        dy = k == y ? d[k] : dy;
                        ey = k == y ? pk[k] : ey;
                    }
                }
#pragma unroll
                for (int k = 0; k < CP; ++k) pk[k] = pk[k] / s;  // the softmax row
                py = ey / s;
                if (kind == AVCER_LOSS_CE) {
                    const float l = logf(s);
                    float g = 0.0f;
#pragma unroll
                    for (int k = 0; k < CP; ++k) {
                        if (k < c) {
                            const float term = cw[k] * -(d[k] - l);
                            g = k == 0 ? term : g + term;
                        }
                    }
                    acc3[0] = wy * -(dy - l);
                    acc3[1] = g;
                } else {
                    const float lo = 1e-7f, hi = 1.0f - 1e-7f;
                    const float p = py < lo ? lo : (py > hi ? hi : py);
                    const float q = 1.0f - p, lp = logf(p);
                    const float fo = gamma == 0.0f ? 1.0f : (gamma == 2.0f ? q * q : powf(q, gamma));
                    acc3[0] = (wy * fo) * -lp;
                    // d/dp of w * (1 - p)^gamma * (-log p); the clip passes no gradient outside [lo, hi]
                    const float df = gamma == 0.0f ? 0.0f : (gamma == 2.0f ? 2.0f * q : gamma * powf(q, gamma - 1.0f));
                    dldp = (py >= lo && py <= hi) ? wy * (df * lp - fo / p) : 0.0f;
                }
                acc3[2] = wy;
            }
            fold3(acc3, fold_sh);
            float loss;
            if (kind == AVCER_LOSS_CE)
                loss = keep * (acc3[0] / acc3[2]) + smooth * (acc3[1] / acc3[2]);
            else
                loss = acc3[0] / (float)nb;
            if (t < nb) {
#pragma unroll
                for (int k = 0; k < CP; ++k) {
                    if (k < c) {
                        const float hot = k == y ? 1.0f : 0.0f;
                        float g;
                        if (kind == AVCER_LOSS_CE)
                            g = (keep * (wy * (pk[k] - hot)) + smooth * (wsum * pk[k] - cw[k])) / acc3[2];
                        else
                            g = ((dldp * py) * (hot - pk[k])) / (float)nb;
                        lg[t * CP + k] = g;
                    }
                }
            }
            if (t == 0) {
                a.batch_loss[(run * a.epochs + e) * a.n_batches + i] = loss;
                running = running + (double)loss * (double)a.bsz;  // net_trainer.py:441: the short batch counts with the full size
            }
            __syncthreads();

            // ---- backward: dW[k, f] = sum_b G[b, k] * x[b, f] for the owned columns, db[k] by thread k
            float dW[CP][J];
#pragma unroll
            for (int k = 0; k < CP; ++k)
#pragma unroll
                for (int j = 0; j < J; ++j) dW[k][j] = 0.0f;
            for (int b = 0; b < nb; ++b) {
                float x[J];
                load_row<J>(a, feats, row_sh, mix_sh, b, mix, lam, onem, x);
                const float4* g4 = reinterpret_cast<const float4*>(lg + b * CP);
#pragma unroll
                for (int k4 = 0; k4 < CP / 4; ++k4) {
                    const float4 g = g4[k4];
                    const float gk[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (k4 * 4 + u < c) {
#pragma unroll
                            for (int j = 0; j < J; ++j) dW[k4 * 4 + u][j] = fmaf(gk[u], x[j], dW[k4 * 4 + u][j]);
                        }
                    }
                }
            }
            float db = 0.0f;
            if (t < c)
                for (int b = 0; b < nb; ++b) db = db + lg[b * CP + t];

            // ---- Adam (torch.optim.Adam: no weight decay, no amsgrad), scalars in double as torch's Python side has them
            b1t = b1t * beta1;
            b2t = b2t * beta2;
            const float step_size = (float)(lr / (1.0 - b1t));
            const float bc2s = (float)sqrt(1.0 - b2t);
#pragma unroll
            for (int k = 0; k < CP; ++k)
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    if (k < c && t + HF_THREADS * j < F) {
                        const float g = dW[k][j];
                        M[k][j] = M[k][j] + w1 * (g - M[k][j]);
                        V[k][j] = V[k][j] * beta2f + (w2 * g) * g;
                        const float denom = sqrtf(V[k][j]) / bc2s + epsf;
                        W[k][j] = W[k][j] - step_size * (M[k][j] / denom);
                    }
                }
            if (t < c) {
                bm = bm + w1 * (db - bm);
                bv = bv * beta2f + (w2 * db) * db;
                bias = bias - step_size * (bm / (sqrtf(bv) / bc2s + epsf));
                bias_sh[t] = bias;
            }
            // ---- CosineAnnealingWarmRestarts.step(epoch + i / iters), T_mult = 1: the rate of the NEXT step
            {
                const double at = (epoch0 + (double)e) + (double)i / (double)a.n_batches;
                const double tcur = at >= t0 ? fmod(at, t0) : at;
                lr = eta_min + (lr0 - eta_min) * (1.0 + cos(M_PI * tcur / t0)) / 2.0;
            }
            __syncthreads();  // the row tables, lg and bias_sh are written again
        }
        // ---- the state at the end of the epoch
#pragma unroll
        for (int k = 0; k < CP; ++k)
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int f = t + HF_THREADS * j;
                if (k < c && f < F) a.w_hist[((run * a.epochs + e) * c + k) * F + f] = W[k][j];
            }
        if (t < c) a.b_hist[(run * a.epochs + e) * c + t] = bias;
        if (t == 0) a.epoch_loss[run * a.epochs + e] = running / (double)a.n_batches;  // :460
    }
}

constexpr int HA_ROWS = 4;   // feature rows per wave
constexpr int HA_WAVES = 4;  // waves per block

template <int CP>
__global__ void __launch_bounds__(64 * HA_WAVES) head_apply_kernel(const float* __restrict__ feats, const float* __restrict__ w,
                                                                   const float* __restrict__ bias, long m, int F, int c,
                                                                   float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long h = blockIdx.y;
    const long row0 = ((long)blockIdx.x * HA_WAVES + wave) * HA_ROWS;
    if (row0 >= m) return;  // the whole wave leaves; there is no barrier in this kernel
    float acc[HA_ROWS][CP];
#pragma unroll
    for (int r = 0; r < HA_ROWS; ++r)
#pragma unroll
        for (int k = 0; k < CP; ++k) acc[r][k] = 0.0f;
    for (int f = lane; f < F; f += 64) {
        float x[HA_ROWS];
#pragma unroll
        for (int r = 0; r < HA_ROWS; ++r) x[r] = row0 + r < m ? feats[(row0 + r) * F + f] : 0.0f;
#pragma unroll
        for (int k = 0; k < CP; ++k) {
            if (k < c) {
                const float wv = w[(h * c + k) * F + f];
#pragma unroll
                for (int r = 0; r < HA_ROWS; ++r) acc[r][k] = fmaf(x[r], wv, acc[r][k]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < HA_ROWS; ++r)
#pragma unroll
        for (int k = 0; k < CP; ++k) {
            if (k < c) {
                float s = acc[r][k];
                for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_xor(s, d);
                if (lane == 0 && row0 + r < m) out[(h * m + row0 + r) * c + k] = s + bias[h * c + k];
            }
        }
}

template <int CP>
void launch_fit(const HeadFitArgs& a, int k_runs, hipStream_t st) {
    const int j = (a.f + HF_THREADS - 1) / HF_THREADS;
    if (j == 1)
        head_fit_kernel<CP, 1><<<k_runs, HF_THREADS, 0, st>>>(a);
    else if (j == 2)
        head_fit_kernel<CP, 2><<<k_runs, HF_THREADS, 0, st>>>(a);
    else
        head_fit_kernel<CP, 4><<<k_runs, HF_THREADS, 0, st>>>(a);
}

bool hf_finite(double v) { return v == v && v < 1.0e300 && v > -1.0e300; }

}  // namespace

extern "C" int avcer_head_fit_views(avcer_ctx* ctx, const float* feats, int views, const int32_t* view, const int32_t* targets, int64_t n,
                                    int f, int c, int k_runs, int epochs, int batch_size, const double* hyper, double* hyper_dev,
                                    const float* class_w, const float* w0, const float* b0, const int32_t* order, const float* mix_lam,
                                    const int32_t* mix_index, float* w_hist, float* b_hist, float* batch_loss, double* epoch_loss,
                                    avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (n < 1 || n > AVCER_HEAD_MAX_ROWS || c < 2 || c > AVCER_LOSS_MAX_CLASSES || f < 64 || f > AVCER_HEAD_MAX_FEATURES || f % 64 != 0 ||
        (long)c * f > AVCER_HEAD_MAX_STATE || batch_size < 1 || batch_size > AVCER_HEAD_MAX_BATCH || epochs < 1 ||
        epochs > AVCER_HEAD_MAX_EPOCHS || k_runs < 1 || k_runs > AVCER_HEAD_MAX_RUNS)
        return set_err(ctx, AVCER_EINVAL,
                       "head fit: %lld rows (1..%lld), %d features (a multiple of 64 up to %d), %d classes (2..%d), c * f <= %d, batch size "
                       "%d (1..%d), %d epochs (1..%d), %d runs (1..%d)",
                       (long long)n, (long long)AVCER_HEAD_MAX_ROWS, f, AVCER_HEAD_MAX_FEATURES, c, AVCER_LOSS_MAX_CLASSES,
                       AVCER_HEAD_MAX_STATE, batch_size, AVCER_HEAD_MAX_BATCH, epochs, AVCER_HEAD_MAX_EPOCHS, k_runs, AVCER_HEAD_MAX_RUNS);
    if (views < 1 || views > AVCER_HEAD_MAX_ROWS / n)
        return set_err(ctx, AVCER_EINVAL, "head fit: %d views of %lld rows (views >= 1, views * rows <= %lld)", views, (long long)n,
                       (long long)AVCER_HEAD_MAX_ROWS);
    if (!feats || !targets || !hyper || !hyper_dev || !class_w || !w0 || !b0 || !order || !w_hist || !b_hist || !batch_loss || !epoch_loss)
        return set_err(ctx, AVCER_EINVAL, "head fit: null buffer");
    const long n_batches = ((long)n + batch_size - 1) / batch_size;
    if ((long)epochs * n_batches > AVCER_HEAD_MAX_STEPS || (long)k_runs * epochs * (long)n > (1LL << 40))
        return set_err(ctx, AVCER_EINVAL, "head fit: %lld steps a run (1..%lld), runs * epochs * rows <= 2^40", (long long)(epochs * n_batches),
                       (long long)AVCER_HEAD_MAX_STEPS);
    for (int r = 0; r < k_runs; ++r) {
        const double* h = hyper + (long)r * HF_HYPER;
        const bool known = h[0] == (double)AVCER_LOSS_CE || h[0] == (double)AVCER_LOSS_SOFT_FOCAL;
        bool ok = known && h[1] >= 0.0 && h[1] <= 1.0 && h[2] >= 0.0 && hf_finite(h[2]) && hf_finite(h[3]) && h[4] >= 0.0 && h[4] < 1.0 &&
                  h[5] >= 0.0 && h[5] < 1.0 && h[6] >= 0.0 && hf_finite(h[6]) && h[7] >= 1.0 && h[7] <= 2147483647.0 && h[7] == floor(h[7]) &&
                  hf_finite(h[8]) && (h[9] == 0.0 || h[9] == 1.0) && h[10] >= 0.0 && h[10] <= 2147483647.0 && h[10] == floor(h[10]);
        if (!ok)
            return set_err(ctx, AVCER_EINVAL,
                           "head fit: run %d: kind %g (0: CE, 1: soft focal), label smoothing %g (0..1), gamma %g (>= 0), lr %g, betas %g, %g "
                           "(in [0, 1)), eps %g (>= 0), t0 %g (an integer >= 1), eta_min %g, mixup flag %g (0 or 1), first epoch %g (an integer >= 0); all finite",
                           r, h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10]);
        if (h[9] != 0.0 && (!mix_lam || !mix_index)) return set_err(ctx, AVCER_EINVAL, "head fit: run %d asks for mixup without its tables", r);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, hipMemcpyAsync(hyper_dev, hyper, sizeof(double) * HF_HYPER * (size_t)k_runs, hipMemcpyHostToDevice, st));
    HeadFitArgs a{feats,  view,       targets,    hyper_dev, class_w, w0, b0,     order,      mix_lam,        mix_index, w_hist,
                  b_hist, batch_loss, epoch_loss, (int)n,    f,       c,  epochs, batch_size, (int)n_batches, views};
    if (c <= 8)
        launch_fit<8>(a, k_runs, st);
    else
        launch_fit<16>(a, k_runs, st);
    CHECK_LAUNCH(ctx, "head fit");
    return AVCER_OK;
}

extern "C" int avcer_head_fit(avcer_ctx* ctx, const float* feats, const int32_t* targets, int64_t n, int f, int c, int k_runs, int epochs,
                              int batch_size, const double* hyper, double* hyper_dev, const float* class_w, const float* w0,
                              const float* b0, const int32_t* order, const float* mix_lam, const int32_t* mix_index, float* w_hist,
                              float* b_hist, float* batch_loss, double* epoch_loss, avcer_stream_t stream) {
    return avcer_head_fit_views(ctx, feats, 1, nullptr, targets, n, f, c, k_runs, epochs, batch_size, hyper, hyper_dev, class_w, w0, b0,
                                order, mix_lam, mix_index, w_hist, b_hist, batch_loss, epoch_loss, stream);
}

extern "C" int avcer_head_apply(avcer_ctx* ctx, const float* feats, const float* w, const float* b, int64_t m, int f, int c, int heads,
                                float* logits, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (m < 1 || m > AVCER_HEAD_MAX_ROWS || c < 2 || c > AVCER_LOSS_MAX_CLASSES || f < 64 || f > AVCER_HEAD_MAX_FEATURES || f % 64 != 0 ||
        heads < 1 || heads > AVCER_HEAD_MAX_HEADS)
        return set_err(ctx, AVCER_EINVAL, "head apply: %lld rows (1..%lld), %d features (a multiple of 64 up to %d), %d classes (2..%d), %d heads (1..%d)",
                       (long long)m, (long long)AVCER_HEAD_MAX_ROWS, f, AVCER_HEAD_MAX_FEATURES, c, AVCER_LOSS_MAX_CLASSES, heads,
                       AVCER_HEAD_MAX_HEADS);
    if (!feats || !w || !b || !logits) return set_err(ctx, AVCER_EINVAL, "head apply: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const dim3 grid(cdiv((long)m, HA_ROWS * HA_WAVES), heads);
    if (c <= 8)
        head_apply_kernel<8><<<grid, 64 * HA_WAVES, 0, (hipStream_t)stream>>>(feats, w, b, (long)m, f, c, logits);
    else
        head_apply_kernel<16><<<grid, 64 * HA_WAVES, 0, (hipStream_t)stream>>>(feats, w, b, (long)m, f, c, logits);
    CHECK_LAUNCH(ctx, "head apply");
    return AVCER_OK;
}
