// The S3FD face detector (ibug.face_detection S3FDNet / S3FDPredictor): the kernels it has that nothing else here needs.  gfx950 only.
// ref: s3fd/s3fd_net.py:8-25 (L2Norm), :35-105 (VGG-16 trunk, extras, heads), :113-171 (forward); s3fd/utils.py:6-24 (decode),
// :94-128 (nms_np), :131-171 (Detect); s3fd/s3fd_predictor.py:45-68 (preprocessing, the threshold loop).
//
// conv1_2 .. conv5_3, fc6, fc7 and the extras are contractions of the library (gemm.hip) on activations in the mode's storage:
// NHWC f32 (AVCER_MODE_FP32) or sp32 pairs (AVCER_MODE_F16X3).  Here:
//   s3fd_stem_kernel     u8 frame -> (optional BGR flip) pixel - integer mean -> conv1_1 3x3 pad 1 (3 -> 64, K = 27) + bias + ReLU ->
//                        the mode's storage.  f32 VALU in both modes: the launch is bound by its 256 bytes of output per pixel.
//   s3fd_invnorm_kernel  1 / (sqrt(sum_c x^2) + 1e-10) per position of an L2Norm level (one wave per position).
//   s3fd_head_kernel     one level's `loc` and `conf` 3x3 convolutions as ONE direct f32 convolution with 8 (level 0) or 6 outputs:
//                        a wave owns 8 neighbouring positions of a row, its lanes share the input channels, every tap is scaled by
//                        its position's inverse norm on the L2Norm levels (the layer's weight is folded into the packed head
//                        weights), a butterfly leaves lane 8p + o with output o of position p; the epilogue adds the bias, takes
//                        level 0's max-out background label and the 2-class softmax, and writes the rows at the level's offset.
//   s3fd_decode / order / nms   Detect and the predictor's loop on the device, see below.
// A wave's work is fixed by (frame, row, tile) alone, so a frame's result does not depend on the batch around it.
#include "act_io.h"

#include <cmath>

namespace {

// ------------------------------------------------------------------------------------------------ stem (conv1_1)
// One thread per (pixel, 16 output channels): the four threads of a pixel are neighbours, so a wave writes 16 whole pixels = 4 KiB
// in a row.  wt: [27][64] ((ky, kx, c) major), c in the network's order (R, G, B); the frame is BGR unless `rgb`.
template <typename T>
__global__ __launch_bounds__(256) void s3fd_stem_kernel(const uint8_t* __restrict__ frames, long npix, int h, int w, int rgb,
                                                        const float* __restrict__ wt, const float* __restrict__ bias, T* __restrict__ y,
                                                        unsigned* ovf) {
    __shared__ __align__(16) float sw[28 * 64];
    for (int i = threadIdx.x; i < 28 * 64; i += 256) sw[i] = i < 27 * 64 ? wt[i] : bias[i - 27 * 64];
    __syncthreads();
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long pix = idx >> 2;
    const int c0 = (int)(idx & 3) * 16;
    if (pix >= npix) return;
    const int ox = (int)(pix % w);
    const long t = pix / w;
    const int oy = (int)(t % h);
    const uint8_t* img = frames + (size_t)(t / h) * h * w * 3;
    const int mean[3] = {123, 117, 104};  // s3fd_predictor.py:49, in the network's channel order
    float acc[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) acc[o] = sw[27 * 64 + c0 + o];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy - 1 + ky;
        if (iy < 0 || iy >= h) continue;  // zero padding of the mean-subtracted image: the tap adds nothing
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox - 1 + kx;
            if (ix < 0 || ix >= w) continue;
            const uint8_t* px = img + ((size_t)iy * w + ix) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = (float)((int)px[rgb ? c : 2 - c] - mean[c]);
                const float* wr = sw + ((ky * 3 + kx) * 3 + c) * 64 + c0;
#pragma unroll
                for (int o = 0; o < 16; ++o) acc[o] = __builtin_fmaf(v, wr[o], acc[o]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < 16; ++o) acc[o] = relu_nan(acc[o]);
#pragma unroll
    for (int q = 0; q < 4; ++q) st4<T>(y, pix * 64 + c0 + 4 * q, acc + 4 * q, ovf);
}

// ------------------------------------------------------------------------------------------------ heads
// L2Norm.forward's `norm` (s3fd_net.py:22), inverted: one wave per position, c a multiple of 4
template <typename T>
__global__ __launch_bounds__(256) void s3fd_invnorm_kernel(const T* __restrict__ x, long npos, int c, float* __restrict__ inv) {
    const long pos = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pos >= npos) return;
    float s = 0.f;
    for (int cc = lane * 4; cc < c; cc += 256) {
        float v[4];
        ld4<T>(x, pos * c + cc, v);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) inv[pos] = 1.0f / (sqrtf(s) + 1e-10f);
}

// x [nb, h, w, c] (c a multiple of 256) in storage T; inv [nb * h * w] or null; wt [9][c][NO] ((ky, kx) major; columns 0-3 loc,
// 4.. conf); bias [NO].  One wave per 8 positions of a row; lane l takes channels 4l .. 4l + 3 of every group of 256.
// Rows of frame f start at (f * P + row0); loc [.., 4], conf [.., 2].
template <typename T, int NO>
__global__ __launch_bounds__(256) void s3fd_head_kernel(const T* __restrict__ x, const float* __restrict__ inv, const float* __restrict__ wt,
                                                        const float* __restrict__ bias, int nb, int h, int w, int c, int row0, int P,
                                                        float* __restrict__ loc, float* __restrict__ conf) {
    const int lane = threadIdx.x & 63;
    const int tw = (w + 7) / 8;
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= (long)nb * h * tw) return;  // wave-uniform: the shuffles below see whole waves
    const int ox0 = (int)(tile % tw) * 8;
    const long t = tile / tw;
    const int oy = (int)(t % h);
    const long f = t / h;
    float acc[64];  // [position][8]; columns NO.. stay zero
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[i] = 0.f;
    for (int c0 = lane * 4; c0 < c; c0 += 256) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy - 1 + ky;
            if (iy < 0 || iy >= h) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                float wr[4 * NO];  // [channel][output]
                const float4* wp = reinterpret_cast<const float4*>(wt + ((long)(ky * 3 + kx) * c + c0) * NO);
#pragma unroll
                for (int q = 0; q < NO; ++q) {
                    const float4 t4 = wp[q];
                    wr[4 * q] = t4.x; wr[4 * q + 1] = t4.y; wr[4 * q + 2] = t4.z; wr[4 * q + 3] = t4.w;
                }
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const int ix = ox0 + p - 1 + kx;
                    if (ox0 + p >= w || ix < 0 || ix >= w) continue;  // uniform across the wave
                    const long pos = (f * h + iy) * w + ix;
                    float v[4];
                    ld4<T>(x, pos * c + c0, v);
                    if (inv != nullptr) {
                        const float s = inv[pos];
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] *= s;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int o = 0; o < NO; ++o) acc[p * 8 + o] = __builtin_fmaf(v[j], wr[j * NO + o], acc[p * 8 + o]);
                }
            }
        }
    }
    // sum over the lanes, halving what a lane holds at every step: lane l ends with element l = 8 * position + output
#pragma unroll
    for (int half = 32; half >= 1; half >>= 1) {
        const bool up = (lane & half) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const float keep = up ? acc[i + half] : acc[i];
            const float send = up ? acc[i] : acc[i + half];
            acc[i] = keep + __shfl_xor(send, half, 64);
        }
    }
    const int p = lane >> 3, o = lane & 7;
    const float r = acc[0] + (o < NO ? bias[o] : 0.f);
    float cf[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cf[k] = __shfl(r, (lane & ~7) + 4 + k, 64);
    const int ox = ox0 + p;
    if (ox >= w) return;
    const long row = f * P + row0 + (long)oy * w + ox;
    if (o < 4) {
        loc[row * 4 + o] = r;
    } else if (o < 6) {
        // level 0: the background label is the maximum of its three (s3fd_net.py:148-149); then nn.Softmax(dim=-1) over 2 classes
        const float b0 = NO == 8 ? fmaxf(fmaxf(cf[0], cf[1]), cf[2]) : cf[0], b1 = NO == 8 ? cf[3] : cf[1];
        const float mx = fmaxf(b0, b1);
        const float e0 = expf(b0 - mx), e1 = expf(b1 - mx);
        conf[row * 2 + (o - 4)] = (o == 4 ? e0 : e1) / (e0 + e1);
    }
}

// ------------------------------------------------------------------------------------------------ Detect + the predictor's loop
// utils.py:6-24: every prior's box in NORMALISED corner form and its score -> dets [T, P, 5] = x0, y0, x1, y1, score.  The
// arithmetic follows torch's evaluation order in f32 with contraction off, so only expf may differ (<= 2 ulp).
__global__ void s3fd_decode_kernel(const float* __restrict__ loc, const float* __restrict__ conf, const float* __restrict__ priors, int P,
                                   float var0, float var1, float* __restrict__ dets) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const long f = blockIdx.y;
    const float4 pr = *reinterpret_cast<const float4*>(priors + 4L * i);
    const float4 l = *reinterpret_cast<const float4*>(loc + (f * P + i) * 4);
    const float cx = pr.x + (l.x * var0) * pr.z;
    const float cy = pr.y + (l.y * var0) * pr.w;
    const float w = pr.z * expf(l.z * var1);
    const float h = pr.w * expf(l.w * var1);
    const float x0 = cx - w / 2.0f, y0 = cy - h / 2.0f;
    float* o = dets + (f * P + i) * 5;
    o[0] = x0;
    o[1] = y0;
    o[2] = w + x0;
    o[3] = h + y0;
    o[4] = conf[(f * P + i) * 2 + 1];
}

// The visiting order of nms_np (utils.py:113: `scores.argsort()[: -top_k - 1 : -1]`, an ascending sort read backwards, so equal
// scores are visited HIGHER prior index first wherever that sort keeps ties in index order -- the rule of avcer_face_nms) of the
// candidates `score > conf_thresh` (Detect, utils.py:156: strict).  One workgroup per frame: the candidates' keys -- the score's
// bits made monotone, prior index + 1 in the low word -- are compacted into `keys` [T, P]; up to ORDER_LDS of them are sorted in
// LDS (bitonic, descending), more are ranked by counting from memory (every key is distinct, so the ranks are a permutation).
// order [T, nms_top_k] = prior index by rank, count [T] = candidates.
constexpr int ORDER_THREADS = 1024;
constexpr int ORDER_LDS = 16384;  // keys held in LDS (128 KiB)

__global__ void __launch_bounds__(ORDER_THREADS) s3fd_order_kernel(const float* __restrict__ dets, int P, float conf_thresh, int nms_top_k,
                                                                    unsigned long long* __restrict__ keys, int32_t* __restrict__ order,
                                                                    int32_t* __restrict__ count) {
    extern __shared__ __align__(16) unsigned long long s3fd_sort_keys[];
    unsigned long long* key = s3fd_sort_keys;
    __shared__ int cnt;
    const int f = blockIdx.x, tid = threadIdx.x;
    const float* d = dets + (long)f * P * 5;
    unsigned long long* gk = keys + (long)f * P;
    int32_t* ord = order + (long)f * nms_top_k;
    if (tid == 0) cnt = 0;
    __syncthreads();
    for (int i = tid; i < P; i += ORDER_THREADS) {
        const float s = d[5L * i + 4];
        if (s > conf_thresh) {
            unsigned v = __float_as_uint(s);
            if (v == 0x80000000u) v = 0u;  // -0.0 == +0.0 is a tie for numpy: index order decides, not the sign bit
            v = (v & 0x80000000u) ? ~v : (v | 0x80000000u);
            gk[atomicAdd(&cnt, 1)] = ((unsigned long long)v << 32) | (unsigned)(i + 1);
        }
    }
    __syncthreads();
    const int c = cnt;
    if (tid == 0) count[f] = c;
    if (c <= ORDER_LDS) {
        int N = 64;
        while (N < c) N <<= 1;
        for (int i = tid; i < N; i += ORDER_THREADS) key[i] = i < c ? gk[i] : 0ull;  // padding sinks to the end of a descending sort
        __syncthreads();
        for (int k = 2; k <= N; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < N / 2; t += ORDER_THREADS) {
                    const int i = 2 * t - (t & (j - 1));
                    const unsigned long long a = key[i], b = key[i + j];
                    if (((i & k) == 0) ? a < b : a > b) { key[i] = b; key[i + j] = a; }
                }
                __syncthreads();
            }
        }
        for (int r = tid; r < min(c, nms_top_k); r += ORDER_THREADS) ord[r] = (int)(unsigned)(key[r] & 0xffffffffu) - 1;
    } else {
        for (int i = tid; i < c; i += ORDER_THREADS) {
            const unsigned long long ki = gk[i];
            int rank = 0;
            for (int j = 0; j < c; ++j) rank += gk[j] > ki;
            if (rank < nms_top_k) ord[rank] = (int)(unsigned)(ki & 0xffffffffu) - 1;
        }
    }
}

// nms_np (utils.py:94-128), Detect's top_k cut (:167) and the predictor's loop (s3fd_predictor.py:56-64) for one frame per workgroup,
// in chunks of 1024 boxes of the visiting order, the scheme of face_nms_kernel (kernels.hip): a thread owns one box of the chunk,
// tests it against the boxes kept from earlier chunks, then the chunk is walked in order with one barrier per kept box.  Areas are
// (x1 - x0) * (y1 - y0) on the normalised boxes -- no "+1" --, a box stays when iou <= nms_thresh; the first min(kept, top_k) are
// Detect's rows, their prefix with score >= threshold the predictor's, scaled to pixels by (w, h, w, h) last.  f32 arithmetic in
// numpy's evaluation order, contraction off: the keep decisions are the reference's.
constexpr int S3FD_NMS_THREADS = 1024;

__global__ void __launch_bounds__(S3FD_NMS_THREADS) s3fd_nms_kernel(const float* __restrict__ dets, int P, const int32_t* __restrict__ order,
                                                                     const int32_t* __restrict__ count, int nms_top_k, float nms_thresh,
                                                                     int top_k, float threshold, float im_w, float im_h,
                                                                     float* __restrict__ out, int32_t* __restrict__ out_n) {
#pragma clang fp contract(off)
    __shared__ float cx1[S3FD_NMS_THREADS], cy1[S3FD_NMS_THREADS], cx2[S3FD_NMS_THREADS], cy2[S3FD_NMS_THREADS], car[S3FD_NMS_THREADS];
    __shared__ float kx1[1024], ky1[1024], kx2[1024], ky2[1024], kar[1024];  // kept so far
    __shared__ unsigned char cdead[S3FD_NMS_THREADS];
    __shared__ int kept[1024];  // position in the visiting order of every kept box
    __shared__ int out_rows;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(count[f], nms_top_k);
    const float* d = dets + (long)f * P * 5;
    const int32_t* ord = order + (long)f * nms_top_k;
    const int cap = min(top_k, 1024);
    int nkept = 0;  // uniform across the block
    for (int c0 = 0; c0 < n && nkept < cap; c0 += S3FD_NMS_THREADS) {
        const int cn = min(S3FD_NMS_THREADS, n - c0);
        float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, ar = 0.f;
        bool dead = tid >= cn;
        if (!dead) {
            const float* r = d + 5L * ord[c0 + tid];
            x1 = r[0]; y1 = r[1]; x2 = r[2]; y2 = r[3];
            ar = (x2 - x1) * (y2 - y1);
            for (int k = 0; k < nkept; ++k) {  // boxes kept from earlier chunks all precede this one in the order
                const float w = fmaxf(0.0f, fminf(kx2[k], x2) - fmaxf(kx1[k], x1));
                const float h = fmaxf(0.0f, fminf(ky2[k], y2) - fmaxf(ky1[k], y1));
                const float inter = w * h;
                const float ovr = inter / (kar[k] + ar - inter);
                if (!(ovr <= nms_thresh)) { dead = true; break; }
            }
        }
        __syncthreads();  // the previous chunk's arrays are free (every thread has left its walk)
        cx1[tid] = x1; cy1[tid] = y1; cx2[tid] = x2; cy2[tid] = y2; car[tid] = ar;
        cdead[tid] = dead ? 1 : 0;
        __syncthreads();
        for (int a = 0; a < cn; ++a) {
            if (cdead[a]) continue;  // uniform: every thread reads the same flag behind the previous barrier
            const float ax1 = cx1[a], ay1 = cy1[a], ax2 = cx2[a], ay2 = cy2[a], aar = car[a];
            if (tid == 0) {
                kept[nkept] = c0 + a;
                kx1[nkept] = ax1; ky1[nkept] = ay1; kx2[nkept] = ax2; ky2[nkept] = ay2; kar[nkept] = aar;
            }
            if (++nkept >= cap) break;
            if (tid > a && !dead) {
                const float w = fmaxf(0.0f, fminf(ax2, x2) - fmaxf(ax1, x1));
                const float h = fmaxf(0.0f, fminf(ay2, y2) - fmaxf(ay1, y1));
                const float inter = w * h;
                const float ovr = inter / (aar + ar - inter);
                if (!(ovr <= nms_thresh)) { dead = true; cdead[tid] = 1; }
            }
            __syncthreads();
        }
        __syncthreads();  // tid 0's last kept entry is visible before the next chunk tests against it
    }
    __syncthreads();
    const int nk = min(nkept, cap);
    if (tid == 0) {
        int m = 0;  // the kept boxes come in descending score: the loop `while score >= threshold` takes a prefix
        while (m < nk && d[5L * ord[kept[m]] + 4] >= threshold) { kept[m] = ord[kept[m]]; ++m; }
        out_rows = m;
        out_n[f] = m;
    }
    __syncthreads();
    for (int e = tid; e < out_rows * 5; e += S3FD_NMS_THREADS) {
        const int c = e % 5;
        const float v = d[5L * kept[e / 5] + c];
        out[((long)f * top_k + e / 5) * 5 + c] = c == 4 ? v : v * ((c & 1) ? im_h : im_w);
    }
}

}  // namespace

int launch_s3fd_stem(avcer_ctx* ctx, const uint8_t* frames, int n, int h, int w, int rgb, const float* wt, const float* b, void* y, int kind,
                     hipStream_t st) {
    const long npix = (long)n * h * w;
    if (kind != KIND_F32 && kind != KIND_SP32) return set_err(ctx, AVCER_EINVAL, "s3fd_stem: storage kind %d (f32 and sp32 only)", kind);
    with_storage<float, sp32_t>(kind, [&](auto tag) {
        using T = typename decltype(tag)::type;
        s3fd_stem_kernel<T><<<cdiv(npix * 4, 256), 256, 0, st>>>(frames, npix, h, w, rgb, wt, b, (T*)y, ctx->ovf);
    });
    CHECK_LAUNCH(ctx, "s3fd_stem");
    return AVCER_OK;
}

int launch_s3fd_head(avcer_ctx* ctx, const void* x, int kind, float* inv, const float* wt, const float* b, int nb, int h, int w, int c,
                     int n_out, int row0, int P, float* loc, float* conf, hipStream_t st) {
    if (c % 256 || (n_out != 6 && n_out != 8) || (kind != KIND_F32 && kind != KIND_SP32))
        return set_err(ctx, AVCER_EINVAL, "s3fd_head: %d channels, %d outputs, storage kind %d", c, n_out, kind);
    const long npos = (long)nb * h * w;
    const unsigned grid = cdiv((long)nb * h * ((w + 7) / 8), 4);
    if (inv != nullptr) {
        with_storage<float, sp32_t>(kind, [&](auto tag) {
            using T = typename decltype(tag)::type;
            s3fd_invnorm_kernel<T><<<cdiv(npos, 4), 256, 0, st>>>((const T*)x, npos, c, inv);
        });
        CHECK_LAUNCH(ctx, "s3fd_invnorm");
    }
    with_storage<float, sp32_t>(kind, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (n_out == 8) s3fd_head_kernel<T, 8><<<grid, 256, 0, st>>>((const T*)x, inv, wt, b, nb, h, w, c, row0, P, loc, conf);
        else s3fd_head_kernel<T, 6><<<grid, 256, 0, st>>>((const T*)x, inv, wt, b, nb, h, w, c, row0, P, loc, conf);
    });
    CHECK_LAUNCH(ctx, "s3fd_head");
    return AVCER_OK;
}

size_t s3fd_detect_ws_bytes(int T, int P, int nms_top_k) {
    return (size_t)T * P * 5 * 4 + (size_t)T * P * 8 + ((size_t)T * nms_top_k + T) * 4 + 768;
}

int launch_s3fd_detect(avcer_ctx* ctx, const float* loc, const float* conf, const float* priors, int T, int P, int im_h, int im_w, float var0,
                       float var1, float conf_thresh, float nms_thresh, int nms_top_k, int top_k, float threshold, void* ws, float* out,
                       int32_t* out_n, hipStream_t st) {
    // the workspace, in the order of s3fd_detect_ws_bytes: keys (8-byte aligned first), dets, order, count
    unsigned long long* keys = (unsigned long long*)ws;
    float* dets = (float*)(keys + (size_t)T * P);
    int32_t* order = (int32_t*)(dets + (size_t)T * P * 5);
    int32_t* count = order + (size_t)T * nms_top_k;
    static uint64_t attr_dev = 0;
    if (!((attr_dev >> (ctx->device & 63)) & 1)) {
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)s3fd_order_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ORDER_LDS * 8));
        attr_dev |= 1ull << (ctx->device & 63);
    }
    s3fd_decode_kernel<<<dim3(cdiv(P, 256), T), 256, 0, st>>>(loc, conf, priors, P, var0, var1, dets);
    CHECK_LAUNCH(ctx, "s3fd_decode");
    int N = 64;  // LDS for the worst case the sort takes; the kernel sorts the next power of two of ITS count
    while (N < P && N < ORDER_LDS) N <<= 1;
    s3fd_order_kernel<<<T, ORDER_THREADS, (size_t)N * 8, st>>>(dets, P, conf_thresh, nms_top_k, keys, order, count);
    CHECK_LAUNCH(ctx, "s3fd_order");
    s3fd_nms_kernel<<<T, S3FD_NMS_THREADS, 0, st>>>(dets, P, order, count, nms_top_k, nms_thresh, top_k, threshold, (float)im_w, (float)im_h,
                                                   out, out_n);
    CHECK_LAUNCH(ctx, "s3fd_nms");
    return AVCER_OK;
}
