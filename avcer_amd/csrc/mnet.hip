// The MobileNet-0.25 RetinaFace detector (RetinaFace(cfg_mnet)): its own kernels.  gfx950 only.
// ref: retina_face/retina_face_net.py:6-38 (conv_bn, conv_dw), 103-125 (MobileNetV1 stages), 41-101 (SSH, FPN at 64 channels,
// LeakyReLU(0.1) because out_channel <= 64), config.py:3-20 (cfg_mnet).
//
// Every activation of this network is plain NHWC f32 in both supported modes (8 and 16 channels do not fill an sp32 group of 32):
//   mnet_stem_kernel   u8 frame -> (optional RGB flip) pixel - integer mean -> conv 3x3/2 pad 1 (3 -> 8) + BN + leaky, f32 VALU (K = 27)
//   dwsep_kernel       one conv_dw block per launch: depthwise 3x3 (stride 1 / 2, pad 1) + BN + leaky in f32 on the VALU from a halo patch
//                      in LDS, its result handed through LDS to the pointwise 1x1 + BN + leaky as MFMA operands; the depthwise result
//                      never reaches HBM.  AVCER_MODE_F16X3: v_mfma_f32_16x16x32_f16, three products per term, every depthwise output
//                      split as ONE opaque f32 value (split_dev.h sp_value); weights = the model's split copies (scaled, row-permuted,
//                      trailer multiplier).  AVCER_MODE_FP32: v_mfma_f32_16x16x4_f32.
//   mnet_conv_kernel   the neck (FPN laterals and merges, SSH branches, merged heads: 64 / 32 / 16 output channels) as direct f32
//                      convolutions on the VALU, weights [taps * cin][cout] read through wave-uniform addresses.
// A block's work is fixed by (frame, tile) alone, so a frame's result does not depend on the batch around it.
#include "act_io.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4_t;

__device__ __forceinline__ float leaky01(float v) { return v >= 0.f ? v : 0.1f * v; }  // a NaN stays a NaN (0.1 * NaN)

// ------------------------------------------------------------------------------------------------ stem
// One thread per output pixel, all 8 channels.  w: [27][8] ((ky, kx, c) major), c in the network's order (B, G, R).
__global__ __launch_bounds__(256) void mnet_stem_kernel(const uint8_t* __restrict__ frames, int n, int h, int w, int oh, int ow, int rgb,
                                                        const float* __restrict__ wt, const float* __restrict__ s,
                                                        const float* __restrict__ b, float* __restrict__ y) {
    __shared__ float sw[27 * 8 + 16];
    for (int i = threadIdx.x; i < 27 * 8 + 16; i += 256) sw[i] = i < 216 ? wt[i] : (i < 224 ? s[i - 216] : b[i - 224]);
    __syncthreads();
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)n * oh * ow) return;
    const int ox = (int)(idx % ow);
    const long t = idx / ow;
    const int oy = (int)(t % oh), f = (int)(t / oh);
    const uint8_t* img = frames + (size_t)f * h * w * 3;
    const float mean[3] = {104.f, 117.f, 123.f};  // retina_face_predictor.py:63, in the network's channel order
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
        if (iy < 0 || iy >= h) continue;  // zero padding of the mean-subtracted image: the tap adds nothing
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if (ix < 0 || ix >= w) continue;
            const uint8_t* px = img + ((size_t)iy * w + ix) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = (float)px[rgb ? 2 - c : c] - mean[c];
                const float* wr = sw + ((ky * 3 + kx) * 3 + c) * 8;
#pragma unroll
                for (int o = 0; o < 8; ++o) acc[o] = __builtin_fmaf(v, wr[o], acc[o]);
            }
        }
    }
    f32x4_t o0, o1;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        o0[o] = leaky01(__builtin_fmaf(acc[o], sw[216 + o], sw[224 + o]));
        o1[o] = leaky01(__builtin_fmaf(acc[4 + o], sw[220 + o], sw[228 + o]));
    }
    f32x4_t* out = reinterpret_cast<f32x4_t*>(y + idx * 8);
    out[0] = o0;
    out[1] = o1;
}

// ------------------------------------------------------------------------------------------------ conv_dw block
constexpr int DW_TS = 8;  // a block computes DW_TS x DW_TS output positions of one frame (64 = four 16-position MFMA tiles)

// byte offset of 16-byte chunk `chunk` (0..7) of row `row` of the operand tile (128 bytes per row, XOR-swizzled chunks)
__device__ __forceinline__ int a_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

// stored row of output channel c in a split weight matrix (kernels.hip split_weight_rows_kernel: inside every group of 32
// channels, stored row 16t + 4g + r holds channel 8g + 4t + r)
__device__ __forceinline__ int split_row(int c) {
    const int j = c & 31;
    return (c & ~31) + 16 * ((j >> 2) & 1) + 4 * (j >> 3) + (j & 3);
}

template <int CIN, int COUT, int S, bool X3>
__global__ __launch_bounds__(256) void dwsep_kernel(const float* __restrict__ x, const float* __restrict__ dww,
                                                    const float* __restrict__ dws, const float* __restrict__ dwb,
                                                    const void* __restrict__ pw, const float* __restrict__ pws,
                                                    const float* __restrict__ pwb, float* __restrict__ y, int h, int w, int oh, int ow,
                                                    int tiles_x, unsigned* ovf) {
    constexpr int CK = CIN < 32 ? CIN : 32;     // channels of a K chunk that exist
    constexpr int NCH = (CIN + 31) / 32;        // K chunks of 32 (the last one zero-padded for 8 and 16 channels)
    constexpr int KP = NCH * 32;                // padded K: row length of the pointwise weights
    constexpr int NP = (COUT + 63) / 64 * 64;   // padded rows of the pointwise weights
    constexpr int PS = (DW_TS - 1) * S + 3;     // side of the input patch with its halo
    constexpr int Q = CK / 4;                   // float4 pieces per position and chunk
    constexpr int NT = COUT / 16;               // 16-channel tiles
    constexpr int NWN = NT < 4 ? NT : 4, NWM = 4 / NWN;  // the four waves: NWN along the channels x NWM along the positions
    constexpr int MTW = 4 / NWM, NTW = NT / NWN;          // tiles per wave
    __shared__ __attribute__((aligned(16))) float patch[PS * PS * CK];
    __shared__ __attribute__((aligned(16))) char at[64 * 128];  // the depthwise result of a chunk: 64 positions x 32 channels
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int frame = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int oy0 = ty * DW_TS, ox0 = tx * DW_TS;
    const int m0 = (wv % NWM) * MTW, n0 = (wv / NWM) * NTW;
    const int r = lane & 15, q = lane >> 4;
    f32x4_t acc[MTW][NTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (CK < 32) {  // the zero padding of the contraction (8 and 16 channels): written once, never overwritten
        for (int i = tid; i < 64 * 8; i += 256) *reinterpret_cast<f32x4_t*>(at + i * 16) = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    sp_flags_t flags = 0;
    const float* xf = x + (size_t)frame * h * w * CIN;
    for (int ch = 0; ch < NCH; ++ch) {
        const int c0 = ch * 32;
        // the previous chunk's MFMAs have read `at`, its depthwise pass has read `patch`
        __syncthreads();
        for (int i = tid; i < PS * PS * Q; i += 256) {
            const int pos = i / Q, cq = i - pos * Q;
            const int py = pos / PS, px = pos - py * PS;
            const int iy = oy0 * S - 1 + py, ix = ox0 * S - 1 + px;
            f32x4_t v = {0.f, 0.f, 0.f, 0.f};
            if (iy >= 0 && iy < h && ix >= 0 && ix < w)
                v = *reinterpret_cast<const f32x4_t*>(xf + ((size_t)iy * w + ix) * CIN + c0 + cq * 4);
            *reinterpret_cast<f32x4_t*>(patch + (size_t)i * 4) = v;
        }
        __syncthreads();
        for (int i = tid; i < 64 * Q; i += 256) {
            const int p = i / Q, cq = i - p * Q;
            const int py = p >> 3, px = p & 7;
            f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(patch + (((py * S + ky) * PS + px * S + kx) * Q + cq) * 4);
                    const f32x4_t wk = *reinterpret_cast<const f32x4_t*>(dww + (ky * 3 + kx) * CIN + c0 + cq * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) a[j] = __builtin_fmaf(v[j], wk[j], a[j]);
                }
            const f32x4_t sc = *reinterpret_cast<const f32x4_t*>(dws + c0 + cq * 4);
            const f32x4_t sh = *reinterpret_cast<const f32x4_t*>(dwb + c0 + cq * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = leaky01(__builtin_fmaf(a[j], sc[j], sh[j]));
            if (X3) {
                float amax = 0.f, a4[4] = {a[0], a[1], a[2], a[3]};
                uint2 hv, lv;
                sp_split4(a4, amax, hv, lv);  // split_dev.h: one f32 number per split
                sp_flag(flags, amax);
                *reinterpret_cast<uint2*>(at + a_off(p, cq >> 1) + (cq & 1) * 8) = hv;        // 32 hi halves: chunks 0-3
                *reinterpret_cast<uint2*>(at + a_off(p, 4 + (cq >> 1)) + (cq & 1) * 8) = lv;  // 32 lo halves: chunks 4-7
            } else {
                *reinterpret_cast<f32x4_t*>(at + a_off(p, cq)) = a;
            }
        }
        __syncthreads();
        if (X3) {
            const uint16_t* wsp = reinterpret_cast<const uint16_t*>(pw);
            spx8_t bh[MTW], bl[MTW];
#pragma unroll
            for (int mi = 0; mi < MTW; ++mi) {
                const int row = (m0 + mi) * 16 + r;
                bh[mi] = *reinterpret_cast<const spx8_t*>(at + a_off(row, q));
                bl[mi] = *reinterpret_cast<const spx8_t*>(at + a_off(row, 4 + q));
            }
#pragma unroll
            for (int ni = 0; ni < NTW; ++ni) {
                const uint16_t* wr = wsp + (size_t)split_row((n0 + ni) * 16 + r) * KP * 2 + ch * 64 + q * 8;
                const spx8_t ah = *reinterpret_cast<const spx8_t*>(wr);
                const spx8_t al = *reinterpret_cast<const spx8_t*>(wr + 32);
#pragma unroll
                for (int mi = 0; mi < MTW; ++mi) {
                    acc[mi][ni] = mfma_sp(al, bh[mi], acc[mi][ni]);
                    acc[mi][ni] = mfma_sp(ah, bl[mi], acc[mi][ni]);
                    acc[mi][ni] = mfma_sp(ah, bh[mi], acc[mi][ni]);
                }
            }
        } else {
            // lane group q owns K elements 8q .. 8q+7 of the chunk (both operands alike: any assignment of K to lanes is a sum order)
            const float* wf = reinterpret_cast<const float*>(pw);
            f32x4_t b0[MTW], b1[MTW];
#pragma unroll
            for (int mi = 0; mi < MTW; ++mi) {
                const int row = (m0 + mi) * 16 + r;
                b0[mi] = *reinterpret_cast<const f32x4_t*>(at + a_off(row, 2 * q));
                b1[mi] = *reinterpret_cast<const f32x4_t*>(at + a_off(row, 2 * q + 1));
            }
#pragma unroll
            for (int ni = 0; ni < NTW; ++ni) {
                const float* wr = wf + (size_t)((n0 + ni) * 16 + r) * KP + c0 + q * 8;
                const f32x4_t a0 = *reinterpret_cast<const f32x4_t*>(wr);
                const f32x4_t a1 = *reinterpret_cast<const f32x4_t*>(wr + 4);
#pragma unroll
                for (int mi = 0; mi < MTW; ++mi) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], b0[mi][j], acc[mi][ni], 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], b1[mi][j], acc[mi][ni], 0, 0, 0);
                }
            }
        }
    }
    // epilogue: the lane holds channels 16 nt + 4q .. + 3 of position 16 mt + r
    const float wmul = X3 ? split_wmul(reinterpret_cast<const char*>(pw), (size_t)NP * KP * 4) : 1.f;
    float* yf = y + (size_t)frame * oh * ow * COUT;
#pragma unroll
    for (int mi = 0; mi < MTW; ++mi) {
        const int p = (m0 + mi) * 16 + r;
        const int oy = oy0 + (p >> 3), ox = ox0 + (p & 7);
        if (oy >= oh || ox >= ow) continue;
#pragma unroll
        for (int ni = 0; ni < NTW; ++ni) {
            const int c = (n0 + ni) * 16 + 4 * q;
            const f32x4_t sc = *reinterpret_cast<const f32x4_t*>(pws + c);
            const f32x4_t sh = *reinterpret_cast<const f32x4_t*>(pwb + c);
            f32x4_t o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = leaky01(__builtin_fmaf(acc[mi][ni][j] * wmul, sc[j], sh[j]));
            *reinterpret_cast<f32x4_t*>(yf + ((size_t)oy * ow + ox) * COUT + c) = o;
        }
    }
    if (X3) sp_commit(ovf, flags);
}

// ------------------------------------------------------------------------------------------------ neck
// Direct convolution KS x KS (stride 1, pad KS / 2) of an NHWC f32 tensor [n, h, w, cin]: one thread per position and 16 output
// channels (blockIdx.y = the 16-channel group, so every weight address is wave-uniform).  wt: [KS * KS * cin][cout];
// y[pos * y_ld + y_coff + c] = act(acc * s[c] + b[c]) (s null: 1); act 0 none, 1 ReLU, 4 LeakyReLU(0.1).
template <int KS>
__global__ __launch_bounds__(256) void mnet_conv_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                        const float* __restrict__ s, const float* __restrict__ b, float* __restrict__ y,
                                                        long total, int h, int w, int cin, int cout, int y_ld, int y_coff, int act) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int co0 = blockIdx.y * 16;
    const int px = (int)(idx % w);
    const long t = idx / w;
    const int py = (int)(t % h);
    const long f = t / h;
    float acc[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) acc[o] = 0.f;
    for (int ky = 0; ky < KS; ++ky) {
        for (int kx = 0; kx < KS; ++kx) {
            const int iy = py + ky - KS / 2, ix = px + kx - KS / 2;
            const bool ok = iy >= 0 && iy < h && ix >= 0 && ix < w;
            const int cy = min(max(iy, 0), h - 1), cx = min(max(ix, 0), w - 1);  // a padded tap reads a valid address and adds zeros
            const float* xp = x + ((f * h + cy) * w + cx) * cin;
            const float* wp = wt + (size_t)((ky * KS + kx) * cin) * cout + co0;
            for (int ci = 0; ci < cin; ci += 4) {
                f32x4_t v = *reinterpret_cast<const f32x4_t*>(xp + ci);
                if (!ok) v = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float* wr = wp + (size_t)(ci + j) * cout;
#pragma unroll
                    for (int o = 0; o < 16; ++o) acc[o] = __builtin_fmaf(v[j], wr[o], acc[o]);
                }
            }
        }
    }
    float* yo = y + idx * y_ld + y_coff + co0;
#pragma unroll
    for (int o4 = 0; o4 < 4; ++o4) {
        f32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = co0 + o4 * 4 + j;
            float v = __builtin_fmaf(acc[o4 * 4 + j], s ? s[c] : 1.f, b[c]);
            if (act == 1) v = v < 0.f ? 0.f : v;
            else if (act == 4) v = leaky01(v);
            o[j] = v;
        }
        *reinterpret_cast<f32x4_t*>(yo + o4 * 4) = o;
    }
}

template <int CIN, int COUT, int S>
int launch_dwsep_t(avcer_ctx* ctx, int x3, const float* x, const float* dww, const float* dws, const float* dwb, const void* pw,
                   const float* pws, const float* pwb, float* y, int nb, int h, int w, hipStream_t st) {
    const int oh = (h - 1) / S + 1, ow = (w - 1) / S + 1;
    const int tiles_x = (ow + DW_TS - 1) / DW_TS, tiles_y = (oh + DW_TS - 1) / DW_TS;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)nb);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    const double M = (double)nb * oh * ow, flops = 2.0 * M * CIN * (9.0 + COUT);
    // compulsory traffic: the input once, the output once, the weights
    const double bytes = 4.0 * ((double)nb * h * w * CIN + M * COUT + 11.0 * CIN + (double)CIN * COUT + 2.0 * COUT);
    TRY(prof_begin(ctx, st, &ev0, &ev1, FAM_CHAIN, flops, bytes, (long)M, COUT, CIN));
    if (x3) dwsep_kernel<CIN, COUT, S, true><<<grid, 256, 0, st>>>(x, dww, dws, dwb, pw, pws, pwb, y, h, w, oh, ow, tiles_x, ctx->ovf);
    else dwsep_kernel<CIN, COUT, S, false><<<grid, 256, 0, st>>>(x, dww, dws, dwb, pw, pws, pwb, y, h, w, oh, ow, tiles_x, nullptr);
    if (ev1) (void)hipEventRecord(ev1, st);
    CHECK_LAUNCH(ctx, "dwsep");
    ctx->gemm_launches += 1;
    ctx->gemm_flops += flops;
    return AVCER_OK;
}

}  // namespace

int launch_mnet_stem(avcer_ctx* ctx, const uint8_t* frames, int n, int h, int w, int rgb, const float* wt, const float* s, const float* b,
                     float* y, hipStream_t st) {
    const int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;
    const long total = (long)n * oh * ow;
    if (n <= 0 || h < 1 || w < 1 || (total + 255) / 256 >= (1L << 31)) return set_err(ctx, AVCER_EINVAL, "mnet_stem: bad geometry");
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    const double flops = 2.0 * (double)total * 8 * 27;
    TRY(prof_begin(ctx, st, &ev0, &ev1, FAM_STEM, flops, (double)n * h * w * 3 + (double)total * 8 * 4, total, 8, 27));
    mnet_stem_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(frames, n, h, w, oh, ow, rgb, wt, s, b, y);
    if (ev1) (void)hipEventRecord(ev1, st);
    CHECK_LAUNCH(ctx, "mnet_stem");
    ctx->gemm_launches += 1;
    ctx->gemm_flops += flops;
    return AVCER_OK;
}

int launch_dwsep(avcer_ctx* ctx, int cin, int cout, int stride, int x3, const float* x, const float* dww, const float* dws,
                 const float* dwb, const void* pw, const float* pws, const float* pwb, float* y, int nb, int h, int w, hipStream_t st) {
    if (nb <= 0 || nb > 65535 || h < 1 || w < 1) return set_err(ctx, AVCER_EINVAL, "dwsep: bad geometry (1..65535 frames per launch)");
    if ((long)((h + 7) / 8) * ((w + 7) / 8) >= (1L << 31)) return set_err(ctx, AVCER_EINVAL, "dwsep: %d x %d is too many tiles for one launch", h, w);
#define DWSEP_CASE(CI, CO, S)                                                                                     \
    if (cin == CI && cout == CO && stride == S)                                                                   \
        return launch_dwsep_t<CI, CO, S>(ctx, x3, x, dww, dws, dwb, pw, pws, pwb, y, nb, h, w, st)
    DWSEP_CASE(8, 16, 1);
    DWSEP_CASE(16, 32, 2);
    DWSEP_CASE(32, 32, 1);
    DWSEP_CASE(32, 64, 2);
    DWSEP_CASE(64, 64, 1);
    DWSEP_CASE(64, 128, 2);
    DWSEP_CASE(128, 128, 1);
    DWSEP_CASE(128, 256, 2);
    DWSEP_CASE(256, 256, 1);
#undef DWSEP_CASE
    return set_err(ctx, AVCER_EINVAL, "dwsep: no kernel for %d -> %d channels at stride %d (the thirteen blocks of MobileNet-0.25 only)", cin,
                   cout, stride);
}

int launch_mnet_conv(avcer_ctx* ctx, int ks, const float* x, const float* wt, const float* s, const float* b, float* y, int n, int h, int w,
                     int cin, int cout, int y_ld, int y_coff, int act, hipStream_t st) {
    const long total = (long)n * h * w;
    if ((ks != 1 && ks != 3) || cin % 4 || cout % 16 || y_ld % 4 || y_coff % 4 || total <= 0 || (total + 255) / 256 >= (1L << 31))
        return set_err(ctx, AVCER_EINVAL, "mnet_conv: unsupported shape (%dx%d, %d -> %d channels)", ks, ks, cin, cout);
    const dim3 grid((unsigned)((total + 255) / 256), (unsigned)(cout / 16));
    if (ks == 3) mnet_conv_kernel<3><<<grid, 256, 0, st>>>(x, wt, s, b, y, total, h, w, cin, cout, y_ld, y_coff, act);
    else mnet_conv_kernel<1><<<grid, 256, 0, st>>>(x, wt, s, b, y, total, h, w, cin, cout, y_ld, y_coff, act);
    CHECK_LAUNCH(ctx, "mnet_conv");
    ctx->gemm_launches += 1;
    ctx->gemm_flops += 2.0 * (double)total * cout * cin * ks * ks;
    return AVCER_OK;
}
