// Fusion weight search: per-candidate argmax counts of the weighted sum of M probability tables (data/utils.py:151-154, the
// Dirichlet search; :176 and :200, the grid searches, are the same expression with a weight constant over the classes).
// Definition: include/avcer_hip.h avcer_weight_search_counts; the host turns the counts into the reference's objective
// (avcer_amd/weight_search.py metrics_from_counts), so the device side is integers out and no tolerance anywhere.
//
// Shape.  One thread owns one candidate and keeps its M * C weights in registers for the whole launch; a block is 256
// candidates, blockIdx.y a slab of frames.  A frame's M * C probabilities and its label are the same for every lane, so the
// kernel reads them through uniform addresses of read-only arguments: the compiler turns those into scalar loads (SGPR
// operands of the f64 multiplies, served by the scalar cache and L2; every block of one slab reads the same rows), and no
// LDS, barrier or vector load is left in the loop.  Per (candidate, frame): M * C f64 multiplies, (M - 1) * C f64 adds, the
// argmax and 2 * C compare-and-add counter updates, all unrolled (M and C are template arguments: a counter indexed by a run-time
// class would live in scratch).  Slabs are combined with integer atomicAdd: the sum does not depend on the order.
//
// Every product and every sum rounds on its own, as numpy's do.  -O3 contracts a * b + c into one FMA by default, and the
// single rounding moves a near-tie to another class (tests/test_gpu_weight_search.py builds such frames): contraction is off
// for this whole file.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int WS_THREADS = 256;
constexpr int WS_MIN_SLAB = 256;      // frames: a thread's 2 * C atomics are paid once per slab
constexpr int WS_TARGET_BLOCKS = 4096;  // 256 CUs x ~5 resident blocks (about 100 VGPRs at M = 4, C = 8), a few rounds

template <int M, int C>
__global__ void __launch_bounds__(WS_THREADS) weight_search_kernel(const double* __restrict__ preds, const int32_t* __restrict__ labels,
                                                                   long n, const double* __restrict__ weights, int w, int slab,
                                                                   int32_t* __restrict__ tp, int32_t* __restrict__ pred) {
    const int cand = blockIdx.x * WS_THREADS + threadIdx.x;
    const int ci = cand < w ? cand : w - 1;  // the tail lanes of the last block redo its last candidate and write nothing
    double wt[M][C];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int c = 0; c < C; ++c) wt[m][c] = weights[((long)ci * M + m) * C + c];
    int n_tp[C], n_pred[C];
#pragma unroll
    for (int c = 0; c < C; ++c) n_tp[c] = n_pred[c] = 0;
    const long i0 = (long)blockIdx.y * slab;
    const long i1 = i0 + slab < n ? i0 + slab : n;
    for (long i = i0; i < i1; ++i) {
        const int lab = labels[i];
        double f[C];
#pragma unroll
        for (int c = 0; c < C; ++c) f[c] = preds[i * C + c] * wt[0][c];
#pragma unroll
        for (int m = 1; m < M; ++m)
#pragma unroll
            for (int c = 0; c < C; ++c) f[c] = f[c] + preds[((long)m * n + i) * C + c] * wt[m][c];
        // np.argmax: the first index of the maximum; a NaN is the maximum, so the first NaN wins and nothing displaces it
        double best = f[0];
        int am = 0;
#pragma unroll
        for (int c = 1; c < C; ++c) {
            const bool take = !(f[c] <= best) && best == best;
            best = take ? f[c] : best;
            am = take ? c : am;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int hit = am == c;
            n_pred[c] += hit;
            n_tp[c] += hit & (lab == c);
        }
    }
    if (cand < w) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (n_pred[c]) atomicAdd(&pred[cand * C + c], n_pred[c]);
            if (n_tp[c]) atomicAdd(&tp[cand * C + c], n_tp[c]);
        }
    }
}

template <int M>
void launch_m(int c, dim3 grid, hipStream_t st, const double* preds, const int32_t* labels, long n, const double* weights, int w,
              int slab, int32_t* tp, int32_t* pred) {
#define WS_CASE(CC) \
    case CC: weight_search_kernel<M, CC><<<grid, WS_THREADS, 0, st>>>(preds, labels, n, weights, w, slab, tp, pred); break;
    switch (c) {
        WS_CASE(2) WS_CASE(3) WS_CASE(4) WS_CASE(5) WS_CASE(6) WS_CASE(7) WS_CASE(8)
    }
#undef WS_CASE
}

}  // namespace

extern "C" int avcer_weight_search_counts(avcer_ctx* ctx, const double* preds, const int32_t* labels, int64_t n, int m, int c,
                                          const double* weights, int w, int32_t* tp, int32_t* pred, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (m < 1 || m > AVCER_SEARCH_MAX_MODELS || c < 2 || c > AVCER_SEARCH_MAX_CLASSES || n < 1 || n > AVCER_SEARCH_MAX_FRAMES ||
        w < 1 || w > AVCER_SEARCH_MAX_CANDIDATES)
        return set_err(ctx, AVCER_EINVAL, "weight search: %d models (1..%d), %d classes (2..%d), %lld frames (1..2^31-1), %d "
                       "candidates (1..%d)", m, AVCER_SEARCH_MAX_MODELS, c, AVCER_SEARCH_MAX_CLASSES, (long long)n, w,
                       AVCER_SEARCH_MAX_CANDIDATES);
    if (!preds || !labels || !weights || !tp || !pred) return set_err(ctx, AVCER_EINVAL, "weight search: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, hipMemsetAsync(tp, 0, (size_t)w * c * sizeof(int32_t), st));
    HIP_TRY(ctx, hipMemsetAsync(pred, 0, (size_t)w * c * sizeof(int32_t), st));
    // slabs: enough blocks to fill the GPU a few times over, none shorter than WS_MIN_SLAB frames
    const long gx = ((long)w + WS_THREADS - 1) / WS_THREADS;  // <= 2^16
    long slabs = (WS_TARGET_BLOCKS + gx - 1) / gx;
    const long most = ((long)n + WS_MIN_SLAB - 1) / WS_MIN_SLAB;
    if (slabs > most) slabs = most;
    long slab = ((long)n + slabs - 1) / slabs;  // <= n < 2^31
    slabs = ((long)n + slab - 1) / slab;        // <= 4096
    const dim3 grid((unsigned)gx, (unsigned)slabs);
    switch (m) {
        case 1: launch_m<1>(c, grid, st, preds, labels, (long)n, weights, w, (int)slab, tp, pred); break;
        case 2: launch_m<2>(c, grid, st, preds, labels, (long)n, weights, w, (int)slab, tp, pred); break;
        case 3: launch_m<3>(c, grid, st, preds, labels, (long)n, weights, w, (int)slab, tp, pred); break;
        case 4: launch_m<4>(c, grid, st, preds, labels, (long)n, weights, w, (int)slab, tp, pred); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}
