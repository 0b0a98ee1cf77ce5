// The S3FD face detector (ibug.face_detection S3FDNet / S3FDPredictor): the kernels it has that nothing else here needs.  gfx950 only.
// ref: s3fd/s3fd_net.py:8-25 (L2Norm), :35-105 (VGG-16 trunk, extras, heads), :113-171 (forward);
// s3fd/s3fd_predictor.py:45-52 (preprocessing).
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
// Detect and the predictor's loop (avcer_s3fd_detect) are in detect_tail.hip, one source with RetinaFace's decode and NMS.
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
