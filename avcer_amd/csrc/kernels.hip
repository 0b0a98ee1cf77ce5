// Element-wise, normalisation, pooling and fusion kernels of the AVCER hot path (gfx950).
// All of these are HBM/LDS-bound: 16-byte vector accesses, one 64-lane wave per row for reductions,
// f32 statistics regardless of the activation storage type.
#include "act_io.h"

#include <cstdlib>
#include <type_traits>

namespace {

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
// erf from Abramowitz & Stegun 7.1.26, the arithmetic of gemm_dev.h gelu_fast (|gelu_fast - gelu| <= 4.7e-7 on [-8, 8]).  NOT
// the same code: the gemm_dev.h pair carries `#pragma clang fp contract(off)` (the forms of one contraction must round
// alike), this pair does not, so hipcc may contract these into the arithmetic around them in conv0 and LayerNorm.  Merging
// the two would change what one of the two sides computes; both stay.
__device__ __forceinline__ float gelu_fast(float x) {
    const float z = x * 0.70710678118654752440f, a = __builtin_fabsf(z);
    const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, a, 1.0f));
    float p = __builtin_fmaf(1.061405429f, t, -1.453152027f);
    p = __builtin_fmaf(p, t, 1.421413741f);
    p = __builtin_fmaf(p, t, -0.284496736f);
    p = __builtin_fmaf(p, t, 0.254829592f);
    p *= t;
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * a * a);
    const float erfz = __builtin_copysignf(__builtin_fmaf(-p, e, 1.0f), z);
    return 0.5f * x * (1.0f + erfz);
}

// ------------------------------------------------------------------------------------------------ preprocess
// data/utils.py:19-39.  u8 [n,in_h,in_w,3] RGB -> zero-bordered [n,230,230,4] (BGR - mean, 4th channel 0).
// The border materialises Conv2dSame's asymmetric padding (video.py:68-80: 2 before, 3 after) plus one extra
// row/column so that the stem runs as an un-padded 8x8-tap convolution with 32 contiguous values per tap row.
constexpr int PP = 230;
template <typename T>
__global__ void preprocess_kernel(const uint8_t* __restrict__ in, T* __restrict__ out, int n, int in_h, int in_w) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)n * PP * PP;
    if (idx >= total) return;
    const int x = idx % PP;
    const int y = (idx / PP) % PP;
    const int b = idx / ((long)PP * PP);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (y >= 2 && y < 226 && x >= 2 && x < 226) {
        // PIL NEAREST (common.h); at 224 source pixels it is the identity
        const uint8_t* px = in + (((long)b * in_h + nearest_src(y - 2, in_h)) * in_w + nearest_src(x - 2, in_w)) * 3;
        v[0] = (float)px[2] - 91.4953f;
        v[1] = (float)px[1] - 103.8827f;
        v[2] = (float)px[0] - 131.0912f;
    }
    st4<T>(out, idx * 4, v);
}

// Planar split-fp16 store (input of stem_pool_kernel): the same zero-bordered image as two fp16 planes
// [n,230,230,4], hi = bf16(v) and lo = bf16(v - hi), so that one 8-pixel tap row is 64 contiguous bytes per plane.
__device__ __forceinline__ void st4_planar(bf16_t* hi, bf16_t* lo, long idx, const float* v, unsigned* ovf) {
    float amax = 0.f;
    uint2 h, l;
    sp_split4(v, amax, h, l);
    sp_count_now(ovf, amax);  // range contract (split_dev.h)
    *reinterpret_cast<uint2*>(hi + idx * 4) = h;
    *reinterpret_cast<uint2*>(lo + idx * 4) = l;
}

// Same zero-bordered image from an ALREADY preprocessed float tensor [n,3,224,224] (the tensor the reference's
// pth_model_static is called with, get_prob_video.py:103-109), in storage T (lo null) or as the two planes out / lo.
template <typename T, bool PLANAR>
__global__ void pack_nchw_kernel(const float* __restrict__ in, T* __restrict__ out, T* __restrict__ lo, int n, unsigned* ovf) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)n * PP * PP;
    if (idx >= total) return;
    const int x = idx % PP;
    const int y = (idx / PP) % PP;
    const int b = idx / ((long)PP * PP);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (y >= 2 && y < 226 && x >= 2 && x < 226) {
        const long o = (long)b * 3 * 224 * 224 + (long)(y - 2) * 224 + (x - 2);
        v[0] = in[o]; v[1] = in[o + 224 * 224]; v[2] = in[o + 2 * 224 * 224];
    }
    if constexpr (PLANAR) st4_planar(out, lo, idx, v, ovf);  // arbitrary floats: the one input that can break the fp16 range by itself
    else st4<T>(out, idx * 4, v);
}

// ------------------------------------------------------------------------------------------------ face tiles (row f4)
// get_face_images.py:52-56 (crop of the decoded frame) + data/utils.py:34 (PIL NEAREST resize to 224x224) in one pass:
// tile pixel (y, x) = frame[f][y0 + floor((y + .5) * ch / 224)][x0 + floor((x + .5) * cw / 224)], channels swapped
// when the frames are BGR (cv2) so that the tile is RGB like the image PIL reads back.  One thread per 4 tile pixels.
__global__ void crop_tiles_kernel(const uint8_t* __restrict__ frames, int T, int H, int W, const int32_t* __restrict__ rects,
                                  int n, int swap_rb, uint8_t* __restrict__ tiles) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)n * 224 * 56;
    if (idx >= total) return;
    const int xq = idx % 56;
    const int y = (idx / 56) % 224;
    const int t = idx / (56L * 224);
    const int32_t* r = rects + 5L * t;
    const int f = r[0], x0 = r[1], y0 = r[2], cw = r[3] - r[1], ch = r[4] - r[2];
    uint8_t px[12];
    const bool ok = f >= 0 && f < T && x0 >= 0 && y0 >= 0 && cw > 0 && ch > 0 && x0 + cw <= W && y0 + ch <= H;
    if (ok) {
        const int sy = y0 + nearest_src(y, ch);
        const uint8_t* row = frames + ((long)f * H + sy) * W * 3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = xq * 4 + j;
            const int sx = x0 + nearest_src(x, cw);
            const uint8_t* s = row + 3L * sx;
            px[3 * j + 0] = swap_rb ? s[2] : s[0];
            px[3 * j + 1] = s[1];
            px[3 * j + 2] = swap_rb ? s[0] : s[2];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) px[j] = 0;
    }
    uint32_t* o = reinterpret_cast<uint32_t*>(tiles + ((long)t * 224 + y) * 224 * 3 + xq * 12);  // 12-byte aligned to 4
    o[0] = px[0] | (px[1] << 8) | (px[2] << 16) | ((uint32_t)px[3] << 24);
    o[1] = px[4] | (px[5] << 8) | (px[6] << 16) | ((uint32_t)px[7] << 24);
    o[2] = px[8] | (px[9] << 8) | (px[10] << 16) | ((uint32_t)px[11] << 24);
}

// ------------------------------------------------------------------------------------------------ RetinaFace network (row f4)
// retina_face_predictor.py:59-65: BGR pixels minus (104, 117, 123) (an RGB frame is flipped first), written as a
// zero-bordered NHWC4 image [n, ph, pw, 4] with the picture at offset (3, 3): the border is torchvision's conv1 padding
// of 3 plus the extra rows/columns that let the 7x7/2 stem run as an un-padded 8x(8 pixels x 4 channels) contraction.
template <typename T>
__global__ void face_pre_kernel(const uint8_t* __restrict__ in, T* __restrict__ out, int n, int h, int w, int ph, int pw,
                                int rgb) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)n * ph * pw;
    if (idx >= total) return;
    const int x = idx % pw;
    const int y = (idx / pw) % ph;
    const int b = idx / ((long)ph * pw);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const int sy = y - 3, sx = x - 3;
    if (sy >= 0 && sy < h && sx >= 0 && sx < w) {
        const uint8_t* px = in + (((long)b * h + sy) * w + sx) * 3;
        v[0] = (float)((int)px[rgb ? 2 : 0] - 104);
        v[1] = (float)((int)px[1] - 117);
        v[2] = (float)((int)px[rgb ? 0 : 2] - 123);
    }
    st4<T>(out, idx * 4, v);
}

// retina_face_net.py:92-98: y += nearest-upsampled coarser level (F.interpolate(mode="nearest"): src = floor(dst*in/out))
template <typename T>
__global__ void upsample_add_kernel(T* __restrict__ y, const T* __restrict__ coarse, int n, int h, int w, int ch, int cw, int c,
                                    unsigned* ovf) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c4 = c / 4;
    const long total = (long)n * h * w * c4;
    if (idx >= total) return;
    const int cc = (idx % c4) * 4;
    long t = idx / c4;
    const int x = t % w; t /= w;
    const int yy = t % h;
    const int b = t / h;
    const int sy = min((int)floorf((float)yy * ((float)ch / (float)h)), ch - 1);
    const int sx = min((int)floorf((float)x * ((float)cw / (float)w)), cw - 1);
    float a[4], u[4];
    const long o = (((long)b * h + yy) * w + x) * c + cc;
    ld4<T>(y, o, a);
    ld4<T>(coarse, (((long)b * ch + sy) * cw + sx) * c + cc, u);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] += u[j];
    st4<T>(y, o, a, ovf);
}

// retina_face.py:9-43,104-113: per position the fused head GEMM produced 32 values = class [2 anchors x 2], bbox
// [2 x 4], landmarks [2 x 10] (row stride ld); scatter them anchor-major into loc / conf (softmax over the 2 classes,
// F.softmax(dim=-1)) / landms at `row0` of an image with P rows in all.
__global__ void face_head_kernel(const float* __restrict__ hd, int ld, int n, int hw, int row0, int P, float* __restrict__ loc,
                                 float* __restrict__ conf, float* __restrict__ landms) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n * hw * 2) return;
    const int a = idx & 1;
    const long pos = idx >> 1;            // b * hw + cell
    const int b = pos / hw;
    const long cell = pos - (long)b * hw;
    const float* v = hd + pos * ld;
    const long r = (long)b * P + row0 + cell * 2 + a;
    const float c0 = v[2 * a], c1 = v[2 * a + 1];
    const float mx = fmaxf(c0, c1);
    const float e0 = expf(c0 - mx), e1 = expf(c1 - mx);
    conf[2 * r] = e0 / (e0 + e1);
    conf[2 * r + 1] = e1 / (e0 + e1);
#pragma unroll
    for (int j = 0; j < 4; ++j) loc[4 * r + j] = v[4 + 4 * a + j];
#pragma unroll
    for (int j = 0; j < 10; ++j) landms[10 * r + j] = v[12 + 10 * a + j];
}

// get_prob_video.py:115-123: window rows = relu(features) gathered by index into [nwin, 10, 512]
__global__ void gather_windows_kernel(const float* __restrict__ feats, const int32_t* __restrict__ idx, float* __restrict__ out,
                                      long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const long row = i / 128;  // 512 / 4 vectors per feature row
    const int c = (i % 128) * 4;
    float v[4];
    ld4<float>(feats, (long)idx[row] * 512 + c, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = relu_nan(v[j]);
    st4<float>(out, row * 512 + c, v);
}

// get_prob_audio_8_cl.py:79-86 + data/utils.py:63-89: chunk = wav[start:end] padded to `window` samples with the
// chunk mean (mode 0; NaN for an empty chunk, like torch.mean of an empty tensor), zeros (1) or by tiling (2).
__global__ void audio_chunks_kernel(const float* __restrict__ wav, const int32_t* __restrict__ starts,
                                    const int32_t* __restrict__ ends, int window, int mode, float* __restrict__ out) {
    __shared__ float red[8];
    __shared__ float bc;
    const int c = blockIdx.x;
    const int s = starts[c], len = ends[c] - starts[c];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    float fill = 0.f;
    if (mode == 0) {
        float a = 0.f;
        for (int i = tid; i < len; i += blockDim.x) a += wav[s + i];
        a = wave_sum(a);
        if (lane == 0) red[wv] = a;
        __syncthreads();
        if (tid == 0) { float t = 0.f; for (int i = 0; i < nw; ++i) t += red[i]; bc = t / (float)len; }
        __syncthreads();
        fill = bc;
    }
    float* o = out + (long)c * window;
    for (int i = tid; i < window; i += blockDim.x) {
        float v;
        if (i < len) v = wav[s + i];
        else if (mode == 2) v = len > 0 ? wav[s + i % len] : NAN;  // empty chunk: the reference raises (i % 0); never index
        else v = fill;
        o[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------ pooling
// The one max-pool on NHWC: a K x K window (K 2 or 3) at stride 2 behind `pad` (0 or 1) rows / columns of padding; one thread per
// output position and 4 channels.  video.py:103,117 MaxPool2d(3, 2); torchvision's ResNet MaxPool2d(3, 2, 1); S3FD's
// nn.MaxPool2d(2, 2[, ceil_mode=True]) (vgg.16).  oh / ow are the caller's (floor or ceil); a tap outside the input does not
// exist: it is loaded from the nearest pixel inside, so that the K * K loads are in flight together, and left out of the maximum.
// Taps in row-major order; a NaN in the window is the result, like torch.
template <typename T, int K>
__global__ void maxpool_kernel(const T* __restrict__ x, T* __restrict__ y, int n, int h, int w, int c, int oh, int ow, int pad) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c4 = c / 4;
    if (idx >= (long)n * oh * ow * c4) return;
    const int cc = (int)(idx % c4) * 4;
    long t = idx / c4;
    const int ox = (int)(t % ow); t /= ow;
    const int oy = (int)(t % oh);
    const long b = t / oh;
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    bool nan[4] = {false, false, false, false};
#pragma unroll
    for (int dy = 0; dy < K; ++dy) {
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            const int iy = 2 * oy - pad + dy, ix = 2 * ox - pad + dx;
            const bool in = iy >= 0 && iy < h && ix >= 0 && ix < w;
            float v[4];
            ld4<T>(x, ((b * h + min(max(iy, 0), h - 1)) * w + min(max(ix, 0), w - 1)) * c + cc, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // selects, no branch around a load: -inf never wins and leaves m's bits alone
                m[j] = fmaxf(m[j], in ? v[j] : -INFINITY);
                nan[j] |= in & (v[j] != v[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) if (nan[j]) m[j] = NAN;
    st4<T>(y, ((b * oh + oy) * ow + ox) * c + cc, m, nullptr);  // a maximum of stored values: nothing new to count
}

// video.py:110,124: AdaptiveAvgPool2d((1,1)) over hw positions of an NHWC tensor -> f32 [n,c]
// One thread per (frame, 8 consecutive channels): 16-byte loads (the one-channel form read an sp32 tensor two bytes at a
// time: 3.4 TB/s); every channel still adds its positions in order 0 .. hw-1, so the sums are the same bits.
// Positions are requested seven at a time before any is added (one frame per call is a single block: its 49 dependent
// round trips were 19 us), and added in the same order.  ysp: the same values once more as sp32 pairs (fc1's operand in x3 mode).
template <typename T>
__global__ void avgpool_kernel(const T* __restrict__ x, float* __restrict__ y, sp32_t* __restrict__ ysp, int n, int hw, int c,
                               unsigned* ovf) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c8 = c / 8;
    if (idx >= (long)n * c8) return;
    const int cc = (idx % c8) * 8;
    const long b = idx / c8;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    constexpr int U = 7;
    for (int i0 = 0; i0 < hw; i0 += U) {
        float v[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) ld8<T>(x, (b * hw + min(i0 + u, hw - 1)) * c + cc, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i0 + u < hw) {
#pragma unroll
                for (int j = 0; j < 8; ++j) s[j] += v[u][j];
            }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = s[j] / (float)hw;
    st8<float>(y, b * c + cc, s);
    if (ysp) st8<sp32_t>(ysp, b * c + cc, s, ovf);
}

// Grad-CAM of layer 4 (get_prob_video.py:137-149, data/utils.py:92-100) in closed form.  Above layer 4 the network is
// avgpool -> fc1 -> ReLU -> fc2 -> softmax, so d p_k / d A[c,y,x] is the same at all 49 positions:
//   s = p_k (e_k - p),  u = 1[h > 0] * (W2^T s),  g_k = (1/49) W1^T u            (cam_grad_kernel, all 7 classes)
//   cam[k,y,x] = mean_c g_k[c] * A[c,y,x]                                         (cam_map_kernel)
// f32 arithmetic in every mode.  cam_grad_kernel: one block per CAM_FR frames x 256 channels, u of those frames' 7 classes in
// 64-row chunks in LDS; each output row is its own sum in the same order whatever the batch, so a frame's map does not depend on
// the frames around it.
constexpr int CAM_FR = 2;  // 14 rows per block: 4 blocks per CU at 256 frames (8 frames per block left one wave per SIMD)
constexpr int CAM_ROWS = CAM_FR * 7;
constexpr int CAM_KC = 64;
__global__ void __launch_bounds__(256) cam_grad_kernel(const float* __restrict__ probs, const float* __restrict__ h,
                                                       const float* __restrict__ w1, const float* __restrict__ w2,
                                                       float* __restrict__ g, int n) {
    __shared__ float s[CAM_ROWS][8];
    __shared__ float u[CAM_KC][CAM_ROWS];
    const int tid = threadIdx.x;
    const int f0 = blockIdx.x * CAM_FR;
    const int c = blockIdx.y * 256 + tid;
    for (int e = tid; e < CAM_ROWS * 7; e += 256) {
        const int r = e / 7, j = e % 7, f = f0 + r / 7, k = r % 7;
        float v = 0.f;
        if (f < n) {
            const float pk = probs[(long)f * 7 + k], pj = probs[(long)f * 7 + j];
            v = pj * ((j == k ? 1.f : 0.f) - pk);   // softmax backward of e_k
        }
        s[r][j] = v;
    }
    float acc[CAM_ROWS];
#pragma unroll
    for (int r = 0; r < CAM_ROWS; ++r) acc[r] = 0.f;
    for (int i0 = 0; i0 < 512; i0 += CAM_KC) {
        __syncthreads();
        for (int e = tid; e < CAM_KC * CAM_ROWS; e += 256) {
            const int r = e / CAM_KC, i = i0 + e % CAM_KC, f = f0 + r / 7;
            float v = 0.f;
            if (f < n && h[(long)f * 512 + i] > 0.f) {
#pragma unroll
                for (int j = 0; j < 7; ++j) v += w2[j * 512 + i] * s[r][j];
            }
            u[e % CAM_KC][r] = v;
        }
        __syncthreads();
        for (int i = 0; i < CAM_KC; ++i) {
            const float w = w1[(long)(i0 + i) * 2048 + c];
#pragma unroll
            for (int r = 0; r < CAM_ROWS; ++r) acc[r] += u[i][r] * w;
        }
    }
#pragma unroll
    for (int r = 0; r < CAM_ROWS; ++r)
        if (f0 + r / 7 < n) g[((long)f0 * 7 + r) * 2048 + c] = acc[r] / 49.f;
}

// cam[f,k,p] = (1/2048) sum_c g[f,k,c] * A[f,p,c] over layer 4's NHWC map in its own storage (f32 / bf16 / sp32 pairs, as
// avgpool_kernel reads it).  One block per frame, lane l of wave w holds g of the 8 channels 512 w + 8 l for all 7 classes; per
// position the 64 lanes reduce by butterfly, the 4 waves in a fixed order through LDS.
template <typename T>
__global__ void __launch_bounds__(256) cam_map_kernel(const T* __restrict__ x, const float* __restrict__ g, float* __restrict__ cam) {
    __shared__ float part[4][7][49];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cc = wv * 512 + lane * 8;
    float gk[7][8];
#pragma unroll
    for (int k = 0; k < 7; ++k) ld8<float>(g, ((long)f * 7 + k) * 2048 + cc, gk[k]);
    for (int p0 = 0; p0 < 49; p0 += 7) {  // seven positions requested before any is used (49 dependent round trips otherwise)
        float a[7][8];
#pragma unroll
        for (int q = 0; q < 7; ++q) ld8<T>(x, ((long)f * 49 + p0 + q) * 2048 + cc, a[q]);
#pragma unroll
        for (int q = 0; q < 7; ++q)
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                float v = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) v += gk[k][j] * a[q][j];
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) part[wv][k][p0 + q] = v;
            }
    }
    __syncthreads();
    for (int e = tid; e < 7 * 49; e += 256) {
        const int k = e / 49, p = e % 49;
        cam[(long)f * 343 + e] = (((part[0][k][p] + part[1][k][p]) + part[2][k][p]) + part[3][k][p]) / 2048.f;
    }
}

// ------------------------------------------------------------------------------------------------ tiny heads
// out[m, j] = sum_k f(x[m,k]) * w[j,k] + b[j], n <= 16 outputs; optional ReLU on the input, optional softmax.
// video.py:131-132 (relu1 -> fc2) + get_prob_video.py:107-109 (softmax dim=1); LSTM fc (video.py:184);
// audio feature_downsample (audio_8_cl.py:189).  One wave per row.
__global__ void small_linear_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                    float* __restrict__ logits, float* __restrict__ probs, int m, int k, int n,
                                    int relu_in) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= m) return;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    // (unrolled: the loads of eight K positions are in flight together -- one row per call is one wave, and 8 dependent
    // round trips per output were the kernel; the adds keep their order)
    // and no load sits behind a branch of its own: `if (j < n) acc[j] += xv * w[..]` made n dependent round trips per K step
    // (3 us each: 59 us for the audio head's 1024 x 8); rows past n re-read row n - 1 into accumulators nobody uses)
#pragma unroll 4
    for (int kk = lane; kk < k; kk += 64) {
        float xv = x[(long)row * k + kk];
        if (relu_in) xv = relu_nan(xv);
        float wv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) wv[j] = w[(long)min(j, n - 1) * k + kk];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] += xv * wv[j];
    }
    float mx = -INFINITY;
    float bj[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) bj[j] = b[min(j, n - 1)];
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < n) {
            acc[j] = wave_sum(acc[j]) + bj[j];
            mx = fmaxf(mx, acc[j]);
        }
    if (lane == 0) {
        float den = 0.f;
        float e[16];
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < n) {
                if (logits) logits[(long)row * n + j] = acc[j];
                e[j] = expf(acc[j] - mx);
                den += e[j];
            }
        if (probs)
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < n) probs[(long)row * n + j] = e[j] / den;
    }
}

// ------------------------------------------------------------------------------------------------ LSTM cell
// torch.nn.LSTM cell (video.py:173-178), gate order i,f,g,o.  xproj already holds x W_ih^T + b_ih + b_hh.
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
// h_sp: h once more as sp32 pairs (same row stride), the operand of the next step's recurrent contraction in the x3 mode
__global__ void lstm_cell_kernel(const float* __restrict__ xproj, long xproj_ld, const float* __restrict__ hproj,
                                 float* __restrict__ c, float* __restrict__ h_out, sp32_t* __restrict__ h_sp, long h_ld, int n,
                                 int hid, int first, unsigned* ovf) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n * hid) return;
    const int j = idx % hid;
    const int r = idx / hid;
    const float* xp = xproj + (long)r * xproj_ld;
    float gi = xp[j], gf = xp[hid + j], gg = xp[2 * hid + j], go = xp[3 * hid + j];
    float cp = 0.f;
    if (!first) {
        const float* hp = hproj + (long)r * 4 * hid;
        gi += hp[j]; gf += hp[hid + j]; gg += hp[2 * hid + j]; go += hp[3 * hid + j];
        cp = c[idx];
    }
    const float cn = sigmoidf_(gf) * cp + sigmoidf_(gi) * tanhf(gg);
    c[idx] = cn;
    const float hn = sigmoidf_(go) * tanhf(cn);
    h_out[(long)r * h_ld + j] = hn;
    if (h_sp) stf<sp32_t>(h_sp, (long)r * h_ld + j, hn, ovf);
}

// ------------------------------------------------------------------------------------------------ audio front end
// HF Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm (call site get_prob_audio_8_cl.py:88-89):
// (x - mean) / sqrt(var + 1e-7), population variance, per row.  One block per row.
__global__ void wav_normalize_kernel(const float* __restrict__ x, float* __restrict__ y, int t) {
    __shared__ float red[8];
    __shared__ float bc;
    const float* xr = x + (long)blockIdx.x * t;
    float* yr = y + (long)blockIdx.x * t;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    // (every pass requests eight of a thread's samples before it uses one -- a 4 s window is one block, and 125 dependent
    // round trips per pass were 90 us; each thread still adds its samples in the same order)
    constexpr int U = 8;
    const int bd = blockDim.x;
    float s = 0.f;
    for (int i = tid; i < t; i += U * bd) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = xr[min(i + u * bd, t - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i + u * bd < t) s += v[u];
    }
    s = wave_sum(s);
    if (lane == 0) red[wv] = s;
    __syncthreads();
    if (tid == 0) { float a = 0.f; for (int i = 0; i < nw; ++i) a += red[i]; bc = a / (float)t; }
    __syncthreads();
    const float mean = bc;
    float q = 0.f;
    for (int i = tid; i < t; i += U * bd) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = xr[min(i + u * bd, t - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i + u * bd < t) { const float d = v[u] - mean; q += d * d; }
    }
    q = wave_sum(q);
    __syncthreads();
    if (lane == 0) red[wv] = q;
    __syncthreads();
    if (tid == 0) { float a = 0.f; for (int i = 0; i < nw; ++i) a += red[i]; bc = sqrtf(a / (float)t + 1e-7f); }
    __syncthreads();
    const float sd = bc;
    for (int i = tid; i < t; i += U * bd) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = xr[min(i + u * bd, t - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i + u * bd < t) yr[i + u * bd] = (v[u] - mean) / sd;
    }
}

// wav2vec2 feature-extractor layer 0: Conv1d(1 -> 512, k=10, stride 5, bias) -> LayerNorm(512) -> GELU, fused.
// Output [n, t_out, 512] time-major.  One wave per time step, each lane owns 8 consecutive channels whose
// 10-tap filters stay in registers for the whole block; the write (2 KiB contiguous per wave) is the cost.
template <typename T>
__global__ void __launch_bounds__(256) conv0_ln_gelu_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ b, const float* __restrict__ g,
                                                         const float* __restrict__ beta, T* __restrict__ y, int t_in,
                                                         int t_out, int steps_per_block, unsigned* ovf) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c0 = lane * 8;
    float wr[8][10], br[8], gr[8], ber[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int k = 0; k < 10; ++k) wr[j][k] = w[(c0 + j) * 10 + k];
        br[j] = b[c0 + j]; gr[j] = g[c0 + j]; ber[j] = beta[c0 + j];
    }
    const int row = blockIdx.y;
    const float* xr = x + (long)row * t_in;
    const int t_begin = blockIdx.x * steps_per_block;
    const int t_end = min(t_begin + steps_per_block, t_out);
    for (int t = t_begin + wv; t < t_end; t += 4) {
        float xv[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) xv[k] = xr[t * 5 + k];
        float v[8];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k) a += xv[k] * wr[j][k];
            v[j] = a + br[j];
            s += v[j];
        }
        const float mean = wave_sum(s) * (1.f / 512.f);
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[j] - mean; q += d * d; }
        const float rstd = rsqrtf(wave_sum(q) * (1.f / 512.f) + 1e-5f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float u = (v[j] - mean) * rstd * gr[j] + ber[j];
            if constexpr (std::is_same<T, float>::value) v[j] = gelu_erf(u);  // f32 mode: the library erff
            else v[j] = gelu_fast(u);
        }
        const long o = ((long)row * t_out + t) * 512 + c0;
        st8<T>(y, o, v, ovf);
    }
}

// LayerNorm over the last dimension (c in {512, 1024}), optional residual add in front, optional GELU behind,
// dual output (f32 residual-stream copy and/or bf16 GEMM-operand copy).  One wave per row.
template <typename TI, typename OB, int C>
__global__ void __launch_bounds__(256) layernorm_kernel(const TI* __restrict__ x, const TI* __restrict__ res,
                                                      const float* __restrict__ g, const float* __restrict__ b,
                                                      float* __restrict__ yf, OB* __restrict__ yb, long rows,
                                                      float eps, int act, unsigned* ovf) {
    constexpr int PER = C / 64;  // 8 or 16 consecutive elements per lane
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const long base = row * C + lane * PER;
    float v[PER];
#pragma unroll
    for (int i = 0; i < PER; i += 8) ld8<TI>(x, base + i, v + i);
    if (res) {
        float r[PER];
#pragma unroll
        for (int i = 0; i < PER; i += 8) ld8<TI>(res, base + i, r + i);
#pragma unroll
        for (int i = 0; i < PER; ++i) v[i] += r[i];
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) s += v[i];
    const float mean = wave_sum(s) * (1.f / C);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) { const float d = v[i] - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) * (1.f / C) + eps);
#pragma unroll
    for (int i = 0; i < PER; i += 4) {
        const float4 gg = *reinterpret_cast<const float4*>(g + lane * PER + i);
        const float4 bb = *reinterpret_cast<const float4*>(b + lane * PER + i);
        v[i + 0] = (v[i + 0] - mean) * rstd * gg.x + bb.x;
        v[i + 1] = (v[i + 1] - mean) * rstd * gg.y + bb.y;
        v[i + 2] = (v[i + 2] - mean) * rstd * gg.z + bb.z;
        v[i + 3] = (v[i + 3] - mean) * rstd * gg.w + bb.w;
    }
    if (act == 2) {
#pragma unroll
        for (int i = 0; i < PER; ++i) v[i] = gelu_erf(v[i]);
    } else if (act == 3) {
#pragma unroll
        for (int i = 0; i < PER; ++i) v[i] = gelu_fast(v[i]);
    }
#pragma unroll
    for (int i = 0; i < PER; i += 8) {
        if (yf) st8<float>(yf, base + i, v + i);
        if (yb) st8<OB>(yb, base + i, v + i, ovf);
    }
}

// attention_layers.py:206-211,249-254: x + pe[:, :S]; writes f32 (residual) and/or bf16 (GEMM operand).
template <typename OB>
__global__ void add_pe_kernel(const float* __restrict__ x, const float* __restrict__ pe, float* __restrict__ yf,
                              OB* __restrict__ yb, long total4, int s, int c, unsigned* ovf) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total4) return;
    const long e = idx * 4;
    const int cc = e % c;
    const int ss = (e / c) % s;
    float v[4], p[4];
    ld4<float>(x, e, v);
    ld4<float>(pe, (long)ss * c + cc, p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += p[j];
    if (yf) st4<float>(yf, e, v);
    if (yb) st4<OB>(yb, e, v, ovf);
}

// ------------------------------------------------------------------------------------------------ audio head
// audio_8_cl.py:151-152: MaxPool1d(5) (stride 5, floor) then ReLU over time of [n, t_in, c].
// ysp: the same values once more as sp32 pairs (the operand of the head's second convolution in the x3 mode)
__global__ void maxpool1d_relu_kernel(const float* __restrict__ x, float* __restrict__ y, sp32_t* __restrict__ ysp, int n, int t_in,
                                      int t_out, int c, int k, unsigned* ovf) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n * t_out * c) return;
    const int cc = idx % c;
    const int t = (idx / c) % t_out;
    const int b = idx / ((long)c * t_out);
    float m = -INFINITY;
    bool nan = false;
    for (int i = 0; i < k; ++i) {
        const float v = x[((long)b * t_in + t * k + i) * c + cc];
        m = fmaxf(m, v);
        nan |= v != v;
    }
    const float r = nan ? NAN : relu_nan(m);
    y[idx] = r;
    if (ysp) stf<sp32_t>(ysp, idx, r, ovf);
}

// audio_8_cl.py:155-156: AdaptiveAvgPool1d(1) then ReLU: [n, t, c] -> [n, c]
__global__ void mean_time_relu_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int t, int c) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n * c) return;
    const int cc = idx % c;
    const int b = idx / c;
    float s = 0.f;
    for (int i = 0; i < t; ++i) s += x[((long)b * t + i) * c + cc];
    y[idx] = relu_nan(s / (float)t);
}

// The sp32 split of an activation-shaped tensor (avcer_split_weights; also the LSTM's hidden state): per group of 32
// elements, 32 hi then 32 lo values of the split type (x = hi + lo + O(2^-22 |x|), split_dev.h); same 4 bytes per element
// as f32, so the DMA addressing is unchanged.  No scaling: activations are stored as they are.
__global__ void split_weights_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, size_t n, unsigned* ovf) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float amax = 0.f;
    uint16_t h, l;
    sp_split1(w[i], amax, h, l);
    sp_count_now(ovf, amax);  // range contract of an unscaled split (split_dev.h)
    const size_t g = i >> 5, j = i & 31;
    out[g * 64 + j] = h;
    out[g * 64 + 32 + j] = l;
}

// max |w| of a tensor as float bits (non-negative floats order like their bit patterns; NaN / inf end up largest)
__global__ void absmax_kernel(const float* __restrict__ w, size_t n, unsigned* __restrict__ slot) {
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        m = max(m, __float_as_uint(w[i]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(slot, m);
}

// The power of two a weight matrix is multiplied by before its fp16 split, from its largest magnitude (float bits): the one
// that puts that magnitude into [2^14, 2^15) -- hi halves stay under fp16's 65504, and a weight's lo half stays a NORMAL
// fp16 number down to 2^-18 of the largest weight (split_dev.h).  Returns (scale, 1 / scale) as float bits; (1, 1) for an
// all-zero, non-finite or absurdly scaled tensor, and always in the bf16 lab build (bf16 has f32's range).
__device__ __forceinline__ uint2 split_scale_bits(unsigned maxbits) {
    const unsigned e = (maxbits >> 23) & 0xffu;  // biased exponent of max |w|
#if defined(AVCER_SPLIT_BF16)
    return make_uint2(0x3f800000u, 0x3f800000u);
#else
    if (e < 15u || e > 254u) return make_uint2(0x3f800000u, 0x3f800000u);
    return make_uint2((268u - e) << 23, (e - 14u) << 23);  // 2^(141 - e), 2^(e - 141): max |w| * scale in [2^14, 2^15)
#endif
}

// The split of a WEIGHT matrix [n][k] for the x3 contractions: the layout above along K, every value multiplied by the
// tensor's power-of-two scale first, and the rows of every group of 32 output channels re-ordered: stored row 16t + 4g + r
// holds channel 8g + 4t + r (t = 0,1; g = 0..3; r = 0..3).  With weights as the MFMA A operand a lane's accumulators are 4
// consecutive ROWS of a 16-row tile, so this order leaves lane group g of two adjacent tiles with the 8 consecutive
// channels 8g..8g+7: a 16-byte piece of the output row (direct whole-line stores, no LDS staging) and, in fused.hip, the
// B fragment of the next contraction in natural K order.  Trailer behind the n * k * 4 bytes (AVCER_SPLIT_TRAILER_BYTES):
// word 1 = max |w| as float bits (written by absmax_kernel before this launch), word 0 = 1 / scale as a float, written
// here: the multiplier every consumer applies to its accumulators.
__global__ void split_weight_rows_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int n, int k) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned* trailer = reinterpret_cast<unsigned*>(out + (size_t)n * k * 2);
    const uint2 sc = split_scale_bits(trailer[1]);
    if (i == 0) trailer[0] = sc.y;
    if (i >= (size_t)n * k) return;
    const int row = i / k, col = i - (size_t)row * k;      // destination row / K index
    const int j = row & 31, t = j >> 4, g = (j >> 2) & 3, r = j & 3;
    const int src = (row & ~31) + 8 * g + 4 * t + r;
    float amax = 0.f;  // never read: the scale puts every weight under 2^15
    uint16_t h, l;
    sp_split1(w[(size_t)src * k + col] * __uint_as_float(sc.x), amax, h, l);
    const size_t o = (size_t)row * k * 2 + (size_t)(col >> 5) * 64 + (col & 31);
    out[o] = h;
    out[o + 32] = l;
}

// The row-split weights once more, in MFMA fragment order for conv_gemm_wd_kernel (gemm.hip): [N/16][K/32][hi, lo][64 lanes]
// [8 x 16 bit], lane l of a fragment = stored row 16 nt + (l & 15), K elements 8 (l >> 4) .. + 8 of the K-step -- the 16 bytes
// that lane feeds the MFMA as its A operand, so a wave fetches a whole fragment with one coalesced 1 KiB load.  `rows` is
// the output of split_weight_rows_kernel (rows already permuted, hi / lo per 32-element K group); one thread per 16 bytes.
// The trailer (scale words) is copied behind the fragments.
__global__ void weight_frags_kernel(const uint4* __restrict__ rows, uint4* __restrict__ out, int n, int k) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // destination 16-byte piece
    const int nk = k >> 5;
    const size_t pieces = (size_t)n * nk * 8;
    if (i < AVCER_SPLIT_TRAILER_BYTES / 16) out[pieces + i] = rows[pieces + i];
    if (i >= pieces) return;
    const int lane = i & 63, hl = (i >> 6) & 1;
    const size_t f = i >> 7;  // (n tile, K-step)
    const int ks = (int)(f % nk), nt = (int)(f / nk);
    const int row = nt * 16 + (lane & 15), chunk = lane >> 4;
    // source: row-major sp32, 128 bytes per (row, K-step): 64 hi then 64 lo, 16-byte chunks
    out[i] = rows[((size_t)row * nk + ks) * 8 + hl * 4 + chunk];
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = f2bf(x[i]);
}

// ------------------------------------------------------------------------------------------------ fusion
// get_prob_audio_8_cl.py:94-101 + run.py:90: frame f's audio logits = mean over the windows whose frame span
// [lo, hi) contains f (pandas float32 group mean).
__global__ void frame_mean_kernel(const float* __restrict__ win, const int32_t* __restrict__ lo,
                                  const int32_t* __restrict__ hi, int n_win, int c, int n_frames, float* __restrict__ out,
                                  int32_t* __restrict__ count) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_frames * c) return;
    const int f = idx / c, j = idx % c;
    double s = 0.0;
    int cnt = 0;
    for (int w = 0; w < n_win; ++w)
        if (lo[w] <= f && f < hi[w]) { s += (double)win[(long)w * c + j]; ++cnt; }
    out[idx] = cnt ? (float)(s / cnt) : 0.f;
    if (j == 0 && count) count[f] = cnt;
}

struct FuseParams {
    double w[21];  // weights_1[m][k] * weights_2[m]
    double pair_w[14];
    int has_w1, cmask;
};

__device__ __forceinline__ void softmax7(const float* in, float* out) {
    float mx = in[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) mx = fmaxf(mx, in[k]);  // NaN handling below
    bool nan = false;
#pragma unroll
    for (int k = 0; k < 7; ++k) nan |= in[k] != in[k];
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < 7; ++k) { out[k] = expf(in[k] - mx); den += out[k]; }
#pragma unroll
    for (int k = 0; k < 7; ++k) out[k] = nan ? NAN : out[k] / den;
}

// run.py:85-165 + data/utils.py:222-241.  One thread per frame; float32 tables promoted to float64 at the
// weight multiply exactly like numpy does for `float32 ndarray * python list`.
// Frame f of n: `al` is its audio row (mean window logits, audio order).  Shared by fuse_kernel and fuse_videos_kernel.
__device__ __forceinline__ void fuse_frame(const float* __restrict__ stat, const float* __restrict__ dyn, const float* al, int f,
                                           int n, const FuseParams& fp, double* __restrict__ comp_prob,
                                           int32_t* __restrict__ comp_argmax) {
    const int order[7] = {0, 6, 5, 4, 1, 2, 3};  // video column -> audio order (get_prob_video.py:56-64, run.py:56-65)
    const int p1[7] = {3, 4, 5, 2, 1, 3, 1}, p2[7] = {6, 6, 6, 6, 6, 5, 5};  // run.py:66-74
    float s[7], dl[7], d[7], a[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { s[k] = stat[(long)f * 7 + order[k]]; dl[k] = dyn[(long)f * 7 + order[k]]; }
    softmax7(dl, d);
    softmax7(al, a);
    if (fp.has_w1) {
        // float32 table * python list -> float64 (run.py:108-111)
        double pm[4][7];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            pm[1][k] = (double)s[k] * fp.w[k];
            pm[2][k] = (double)d[k] * fp.w[7 + k];
            pm[3][k] = (double)a[k] * fp.w[14 + k];
            pm[0][k] = pm[1][k] + pm[2][k] + pm[3][k];
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            double q[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) q[k] = fp.cmask ? (pm[m][k] > 1.0 / 7.0 ? pm[m][k] : 0.0) : pm[m][k];
            double best = 0.0;
            int bi = 0;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                const double v = q[p1[c]] * fp.pair_w[2 * c] + q[p2[c]] * fp.pair_w[2 * c + 1];
                comp_prob[((long)m * n + f) * 7 + c] = v;
                if (c == 0) { best = v; bi = 0; }
                else if (!(best != best) && (v > best || v != v)) { best = v; bi = c; }  // numpy argmax: first NaN wins
            }
            comp_argmax[(long)m * n + f] = bi;
        }
    } else {
        // run.py:113-114: np.sum of float32 tables / 3 stays float32, and so does get_compound_expression's
        // arithmetic (python scalars are weak); only the store into the float64 `prob` array widens.
        float pm[4][7];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            pm[1][k] = s[k]; pm[2][k] = d[k]; pm[3][k] = a[k];
            pm[0][k] = ((s[k] + d[k]) + a[k]) / 3.0f;
        }
        const float thr = (float)(1.0 / 7.0);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            float q[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) q[k] = fp.cmask ? (pm[m][k] > thr ? pm[m][k] : 0.0f) : pm[m][k];
            float best = 0.0f;
            int bi = 0;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                const float v = q[p1[c]] * (float)fp.pair_w[2 * c] + q[p2[c]] * (float)fp.pair_w[2 * c + 1];
                comp_prob[((long)m * n + f) * 7 + c] = (double)v;
                if (c == 0) { best = v; bi = 0; }
                else if (!(best != best) && (v > best || v != v)) { best = v; bi = c; }
            }
            comp_argmax[(long)m * n + f] = bi;
        }
    }
}

__global__ void fuse_kernel(const float* __restrict__ stat, const float* __restrict__ dyn, const float* __restrict__ aud,
                            int n, int n_aud, int aud_c, FuseParams fp, double* __restrict__ comp_prob,
                            int32_t* __restrict__ comp_argmax) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    float al[7];
    const int fa = f < n_aud ? f : n_aud - 1;  // run.py:99-103 tail padding with the last audio row
#pragma unroll
    for (int k = 0; k < 7; ++k) al[k] = aud[(long)fa * aud_c + k];
    fuse_frame(stat, dyn, al, f, n, fp, comp_prob, comp_argmax);
}

// frame_mean_kernel's row of ONE frame f (the video's own numbering) over the video's windows [wb, we): the same additions
// in the same (index) order, one rounding.  lo and hi do not decrease within a video (chunk_spans), which bounds the walk: it
// starts at the first window whose span ends behind f and stops at the first that starts behind f.
__device__ __forceinline__ int video_frame_mean(const float* __restrict__ win, const int32_t* __restrict__ lo,
                                                const int32_t* __restrict__ hi, int wb, int we, int c, int f, float* row) {
    int a = wb, b = we;
    while (a < b) {
        const int mid = a + ((b - a) >> 1);
        if (hi[mid] > f) b = mid; else a = mid + 1;
    }
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    for (int w = a; w < we && lo[w] <= f; ++w)
        if (f < hi[w]) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < c) s[j] += (double)win[(long)w * c + j];
            ++cnt;
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) row[j] = cnt ? (float)(s[j] / cnt) : 0.f;
    return cnt;
}

// frame_mean_kernel + fuse_kernel over a concatenation of videos in one launch.  One thread per frame: it finds its video by
// binary search in frame_off, computes the audio row it fuses with from that video's windows alone (a frame behind the
// covered prefix recomputes the row of frame n_aud[v] - 1 itself, run.py:99-103) and runs fuse_frame.
__global__ void fuse_videos_kernel(const float* __restrict__ stat, const float* __restrict__ dyn, const float* __restrict__ win,
                                   const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                   const int32_t* __restrict__ frame_off, const int32_t* __restrict__ win_off,
                                   const int32_t* __restrict__ n_aud, int n_videos, int n, int n_win, int c, FuseParams fp,
                                   float* __restrict__ aud_mean, int32_t* __restrict__ count, double* __restrict__ comp_prob,
                                   int32_t* __restrict__ comp_argmax) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    int a = 0, b = n_videos - 1;  // the video v with frame_off[v] <= f < frame_off[v + 1] (videos without frames are passed over)
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (frame_off[mid + 1] > f) b = mid; else a = mid + 1;
    }
    const int v = a, fl = f - frame_off[v];
    // the offsets come from device memory: whatever they hold, no window outside [0, n_win) is read
    const int wb = max(win_off[v], 0), we = min(win_off[v + 1], n_win);
    const int na = n_aud[v];
    float row[8];
    int cnt = video_frame_mean(win, lo, hi, wb, we, c, fl < na ? fl : na - 1, row);
    fuse_frame(stat, dyn, row, f, n, fp, comp_prob, comp_argmax);
    if (aud_mean || count) {
        if (fl >= na) cnt = video_frame_mean(win, lo, hi, wb, we, c, fl, row);  // what the frame's own group holds: nothing
        if (aud_mean)
            for (int j = 0; j < c; ++j) aud_mean[(long)f * c + j] = row[j];
        if (count) count[f] = cnt;
    }
}

}  // namespace

int k_preprocess(avcer_ctx* ctx, const uint8_t* frames, int n, int in_h, int in_w, void* out, int kind, hipStream_t st) {
    const long total = (long)n * PP * PP;
    with_storage<float, bf16_t>(kind, [&](auto tag) {
        using T = typename decltype(tag)::type;
        preprocess_kernel<T><<<cdiv(total, 256), 256, 0, st>>>(frames, (T*)out, n, in_h, in_w);
    });
    CHECK_LAUNCH(ctx, "preprocess");
    return AVCER_OK;
}

int k_maxpool(avcer_ctx* ctx, const void* x, void* y, int n, int h, int w, int c, int k, int pad, int oh, int ow, int kind, hipStream_t st) {
    if (c % 4 || (kind == KIND_SP32 && c % 32)) return set_err(ctx, AVCER_EINVAL, "maxpool%d: %d channels", k, c);
    if (oh < 1 || ow < 1) return set_err(ctx, AVCER_EINVAL, "maxpool%d: a %d x %d map has no %d x %d window", k, h, w, k, k);
    // built for what is called: 2 x 2 on f32 / sp32 (S3FD), 3 x 3 on f32 / bf16 (the ResNet stems; in the x3 mode they pool in the stem kernel)
    if ((k != 2 && k != 3) || pad < 0 || pad > 1 || kind == (k == 2 ? KIND_BF16 : KIND_SP32))
        return set_err(ctx, AVCER_EINVAL, "maxpool%d: no kernel for padding %d in storage kind %d", k, pad, kind);
    const int grid = cdiv((long)n * oh * ow * (c / 4), 256);
    auto launch = [&](auto tag, auto kk) {
        using T = typename decltype(tag)::type;
        maxpool_kernel<T, decltype(kk)::value><<<grid, 256, 0, st>>>((const T*)x, (T*)y, n, h, w, c, oh, ow, pad);
    };
    if (k == 2) with_storage<float, sp32_t>(kind, [&](auto tag) { launch(tag, std::integral_constant<int, 2>{}); });
    else with_storage<float, bf16_t>(kind, [&](auto tag) { launch(tag, std::integral_constant<int, 3>{}); });
    CHECK_LAUNCH(ctx, "maxpool");
    return AVCER_OK;
}

int k_avgpool_hw(avcer_ctx* ctx, const void* x, float* y, void* y_sp32, int n, int hw, int c, int kind, hipStream_t st) {
    if (c % 32) return set_err(ctx, AVCER_EINVAL, "avgpool: c=%d must be a multiple of 32", c);
    const long total = (long)n * (c / 8);
    // 64 threads per block: one frame per call is 256 threads, and four CUs run them in the time of one
    const int grid = cdiv(total, 64);
    sp32_t* ysp = (sp32_t*)y_sp32;
    with_storage(kind, [&](auto tag) {
        using T = typename decltype(tag)::type;
        avgpool_kernel<T><<<grid, 64, 0, st>>>((const T*)x, y, ysp, n, hw, c, ctx->ovf);
    });
    CHECK_LAUNCH(ctx, "avgpool");
    return AVCER_OK;
}

int k_cam_maps(avcer_ctx* ctx, const void* x, const float* probs, const float* h, const float* w1, const float* w2, float* g,
               float* cam, int n, int kind, hipStream_t st) {
    cam_grad_kernel<<<dim3(cdiv(n, CAM_FR), 2048 / 256), 256, 0, st>>>(probs, h, w1, w2, g, n);
    CHECK_LAUNCH(ctx, "cam_grad");
    with_storage(kind, [&](auto tag) {
        using T = typename decltype(tag)::type;
        cam_map_kernel<T><<<n, 256, 0, st>>>((const T*)x, g, cam);
    });
    CHECK_LAUNCH(ctx, "cam_map");
    return AVCER_OK;
}

int k_small_linear(avcer_ctx* ctx, const float* x, const float* w, const float* b, float* logits, float* probs, int m,
                   int k, int n, int relu_in, hipStream_t st) {
    if (n > 16) return set_err(ctx, AVCER_EINVAL, "small_linear: n=%d > 16", n);
    small_linear_kernel<<<cdiv(m, 4), 256, 0, st>>>(x, w, b, logits, probs, m, k, n, relu_in);
    CHECK_LAUNCH(ctx, "small_linear");
    return AVCER_OK;
}

int k_lstm_cell(avcer_ctx* ctx, const float* xproj, int64_t xproj_ld, const float* hproj, float* c, float* h_out, void* h_sp,
                int64_t h_ld, int n, int hid, int first, hipStream_t st) {
    if (h_sp && h_ld % 32) return set_err(ctx, AVCER_EINVAL, "lstm_cell: sp32 rows need a stride in whole groups of 32");
    lstm_cell_kernel<<<cdiv((long)n * hid, 256), 256, 0, st>>>(xproj, xproj_ld, hproj, c, h_out, (sp32_t*)h_sp, h_ld, n, hid, first,
                                                               ctx->ovf);
    CHECK_LAUNCH(ctx, "lstm_cell");
    return AVCER_OK;
}

int k_wav_normalize(avcer_ctx* ctx, const float* x, float* y, int n, int t, hipStream_t st) {
    wav_normalize_kernel<<<n, 512, 0, st>>>(x, y, t);
    CHECK_LAUNCH(ctx, "wav_normalize");
    return AVCER_OK;
}

int k_conv0_ln_gelu(avcer_ctx* ctx, const float* x, const float* w, const float* b, const float* g, const float* beta,
                    void* y, int n, int t_in, int t_out, int kind, hipStream_t st) {
    const int spb = 64;
    dim3 grid(cdiv(t_out, spb), n);
    with_storage(kind, [&](auto tag) {
        using T = typename decltype(tag)::type;
        conv0_ln_gelu_kernel<T><<<grid, 256, 0, st>>>(x, w, b, g, beta, (T*)y, t_in, t_out, spb, ctx->ovf);
    });
    CHECK_LAUNCH(ctx, "conv0_ln_gelu");
    return AVCER_OK;
}

namespace {
template <typename TI, typename OB>
int ln_launch(avcer_ctx* ctx, const void* x, const void* res, const float* g, const float* b, void* yf, void* yb, int64_t rows,
              int c, float eps, int act, hipStream_t st) {
    const int grid = cdiv(rows, 4);
    if (c == 512)
        layernorm_kernel<TI, OB, 512><<<grid, 256, 0, st>>>((const TI*)x, (const TI*)res, g, b, (float*)yf, (OB*)yb, rows, eps, act, ctx->ovf);
    else if (c == 1024)
        layernorm_kernel<TI, OB, 1024><<<grid, 256, 0, st>>>((const TI*)x, (const TI*)res, g, b, (float*)yf, (OB*)yb, rows, eps, act, ctx->ovf);
    else
        return set_err(ctx, AVCER_EINVAL, "layernorm: c=%d unsupported", c);
    return AVCER_OK;
}
}  // namespace

// in_kind: storage of x / res (0 f32, 1 bf16, 2 sp32); yb_kind: storage of the operand copy yb (1 bf16, 2 sp32)
int k_layernorm(avcer_ctx* ctx, const void* x, const void* res, const float* g, const float* b, void* yf, void* yb,
                int64_t rows, int c, float eps, int act, int in_kind, int yb_kind, hipStream_t st) {
    int r = AVCER_OK;
    with_storage<bf16_t, sp32_t>(yb_kind, [&](auto ob) {
        with_storage(in_kind, [&](auto ti) {
            r = ln_launch<typename decltype(ti)::type, typename decltype(ob)::type>(ctx, x, res, g, b, yf, yb, rows, c, eps, act, st);
        });
    });
    if (r != AVCER_OK) return r;
    CHECK_LAUNCH(ctx, "layernorm");
    return AVCER_OK;
}

int k_add_pe(avcer_ctx* ctx, const float* x, const float* pe, float* yf, void* yb, int n, int s, int c, int yb_kind,
             hipStream_t st) {
    const long total4 = (long)n * s * c / 4;
    with_storage<bf16_t, sp32_t>(yb_kind, [&](auto tag) {
        using OB = typename decltype(tag)::type;
        add_pe_kernel<OB><<<cdiv(total4, 256), 256, 0, st>>>(x, pe, yf, (OB*)yb, total4, s, c, ctx->ovf);
    });
    CHECK_LAUNCH(ctx, "add_pe");
    return AVCER_OK;
}

int k_maxpool1d_relu(avcer_ctx* ctx, const float* x, float* y, void* y_sp32, int n, int t_in, int t_out, int c, int k, hipStream_t st) {
    if (y_sp32 && c % 32) return set_err(ctx, AVCER_EINVAL, "maxpool1d_relu: sp32 rows need c in whole groups of 32");
    maxpool1d_relu_kernel<<<cdiv((long)n * t_out * c, 256), 256, 0, st>>>(x, y, (sp32_t*)y_sp32, n, t_in, t_out, c, k, ctx->ovf);
    CHECK_LAUNCH(ctx, "maxpool1d_relu");
    return AVCER_OK;
}

int k_mean_time_relu(avcer_ctx* ctx, const float* x, float* y, int n, int t, int c, hipStream_t st) {
    mean_time_relu_kernel<<<cdiv((long)n * c, 256), 256, 0, st>>>(x, y, n, t, c);
    CHECK_LAUNCH(ctx, "mean_time_relu");
    return AVCER_OK;
}

int k_f32_to_bf16(avcer_ctx* ctx, const float* x, bf16_t* y, size_t n, hipStream_t st) {
    f32_to_bf16_kernel<<<cdiv((long)n, 256), 256, 0, st>>>(x, y, n);
    CHECK_LAUNCH(ctx, "f32_to_bf16");
    return AVCER_OK;
}

int k_frame_mean(avcer_ctx* ctx, const float* win_logits, const int32_t* lo, const int32_t* hi, int n_win, int c,
                 int n_frames, float* out, int32_t* count, hipStream_t st) {
    frame_mean_kernel<<<cdiv((long)n_frames * c, 128), 128, 0, st>>>(win_logits, lo, hi, n_win, c, n_frames, out, count);
    CHECK_LAUNCH(ctx, "frame_mean");
    return AVCER_OK;
}

static FuseParams fuse_params(const double* w, int has_w1, int cwt, int cmask) {
    FuseParams fp;
    for (int i = 0; i < 21; ++i) fp.w[i] = w ? w[i] : 1.0;
    // data/utils.py:228-236 with dict_weights of run.py:116-123 (Rule 2) or 1,1
    static const int dictw[7] = {0, 5, 6, 5, 6, 4, 2};
    static const int p1[7] = {3, 4, 5, 2, 1, 3, 1}, p2[7] = {6, 6, 6, 6, 6, 5, 5};
    for (int c = 0; c < 7; ++c) {
        if (cwt) {
            const double sw = (double)(dictw[p1[c]] + dictw[p2[c]]);
            fp.pair_w[2 * c] = dictw[p1[c]] / sw;
            fp.pair_w[2 * c + 1] = dictw[p2[c]] / sw;
        } else {
            fp.pair_w[2 * c] = 1.0;
            fp.pair_w[2 * c + 1] = 1.0;
        }
    }
    fp.has_w1 = has_w1;
    fp.cmask = cmask;
    return fp;
}

int k_fuse(avcer_ctx* ctx, const float* stat, const float* dyn, const float* aud, int n, int n_aud, int aud_c,
           const double* w, int has_w1, int cwt, int cmask, double* comp_prob, int32_t* comp_argmax, hipStream_t st) {
    const FuseParams fp = fuse_params(w, has_w1, cwt, cmask);
    fuse_kernel<<<cdiv(n, 64), 64, 0, st>>>(stat, dyn, aud, n, n_aud, aud_c, fp, comp_prob, comp_argmax);
    CHECK_LAUNCH(ctx, "fuse");
    return AVCER_OK;
}

int k_fuse_videos(avcer_ctx* ctx, const float* stat, const float* dyn, const float* win, const int32_t* lo, const int32_t* hi,
                  const int32_t* frame_off, const int32_t* win_off, const int32_t* n_aud, int n_videos, int n, int n_win, int c,
                  const double* w, int has_w1, int cwt, int cmask, float* aud_mean, int32_t* count, double* comp_prob,
                  int32_t* comp_argmax, hipStream_t st) {
    const FuseParams fp = fuse_params(w, has_w1, cwt, cmask);
    fuse_videos_kernel<<<cdiv(n, 64), 64, 0, st>>>(stat, dyn, win, lo, hi, frame_off, win_off, n_aud, n_videos, n, n_win, c, fp,
                                                   aud_mean, count, comp_prob, comp_argmax);
    CHECK_LAUNCH(ctx, "fuse_videos");
    return AVCER_OK;
}

int k_crop_tiles(avcer_ctx* ctx, const uint8_t* frames, int T, int H, int W, const int32_t* rects, int n, int swap_rb,
                 uint8_t* tiles, hipStream_t st) {
    crop_tiles_kernel<<<cdiv((long)n * 224 * 56, 256), 256, 0, st>>>(frames, T, H, W, rects, n, swap_rb, tiles);
    CHECK_LAUNCH(ctx, "crop_tiles");
    return AVCER_OK;
}

int k_face_pre(avcer_ctx* ctx, const uint8_t* frames, int n, int h, int w, int ph, int pw, int rgb, void* out, int bf16,
               hipStream_t st) {
    const long total = (long)n * ph * pw;
    with_storage<float, bf16_t>(bf16 ? KIND_BF16 : KIND_F32, [&](auto tag) {
        using T = typename decltype(tag)::type;
        face_pre_kernel<T><<<cdiv(total, 256), 256, 0, st>>>(frames, (T*)out, n, h, w, ph, pw, rgb);
    });
    CHECK_LAUNCH(ctx, "face_pre");
    return AVCER_OK;
}

int k_upsample_add(avcer_ctx* ctx, void* y, const void* coarse, int n, int h, int w, int ch, int cw, int c, int kind,
                   hipStream_t st) {
    const long total = (long)n * h * w * (c / 4);
    const int grid = cdiv(total, 256);
    with_storage(kind, [&](auto tag) {
        using T = typename decltype(tag)::type;
        upsample_add_kernel<T><<<grid, 256, 0, st>>>((T*)y, (const T*)coarse, n, h, w, ch, cw, c, ctx->ovf);
    });
    CHECK_LAUNCH(ctx, "upsample_add");
    return AVCER_OK;
}

int k_face_head(avcer_ctx* ctx, const float* hd, int ld, int n, int hw, int row0, int P, float* loc, float* conf,
                float* landms, hipStream_t st) {
    face_head_kernel<<<cdiv((long)n * hw * 2, 256), 256, 0, st>>>(hd, ld, n, hw, row0, P, loc, conf, landms);
    CHECK_LAUNCH(ctx, "face_head");
    return AVCER_OK;
}

int k_pack_nchw(avcer_ctx* ctx, const float* x, int n, void* out, int kind, hipStream_t st) {
    const long total = (long)n * PP * PP;
    if (kind == 3) pack_nchw_kernel<bf16_t, true><<<cdiv(total, 256), 256, 0, st>>>(x, (bf16_t*)out, (bf16_t*)out + total * 4, n, ctx->ovf);
    else with_storage<float, bf16_t>(kind, [&](auto tag) {
        using T = typename decltype(tag)::type;
        pack_nchw_kernel<T, false><<<cdiv(total, 256), 256, 0, st>>>(x, (T*)out, nullptr, n, nullptr);
    });
    CHECK_LAUNCH(ctx, "pack_nchw");
    return AVCER_OK;
}

int k_gather_windows(avcer_ctx* ctx, const float* feats, const int32_t* idx, int nwin, float* out, hipStream_t st) {
    const long total4 = (long)nwin * 10 * 128;
    gather_windows_kernel<<<cdiv(total4, 256), 256, 0, st>>>(feats, idx, out, total4);
    CHECK_LAUNCH(ctx, "gather_windows");
    return AVCER_OK;
}

int k_audio_chunks(avcer_ctx* ctx, const float* wav, const int32_t* starts, const int32_t* ends, int n, int window,
                   int mode, float* out, hipStream_t st) {
    audio_chunks_kernel<<<n, 512, 0, st>>>(wav, starts, ends, window, mode, out);
    CHECK_LAUNCH(ctx, "audio_chunks");
    return AVCER_OK;
}

int k_split_weight_rows(avcer_ctx* ctx, const float* w, bf16_t* out, int n, int k, hipStream_t st) {
    if (n % 32 || k % 32) return set_err(ctx, AVCER_EINVAL, "split_weight_rows: n=%d and k=%d must be multiples of 32", n, k);
    // trailer behind the split data: max |w| (word 1) -> the tensor's power-of-two scale; its inverse is left in word 0
    unsigned* trailer = reinterpret_cast<unsigned*>(out + (size_t)n * k * 2);
    HIP_TRY(ctx, hipMemsetAsync(trailer, 0, AVCER_SPLIT_TRAILER_BYTES, st));
    absmax_kernel<<<(int)std::min<long>(cdiv((long)n * k, 256 * 16), 2048), 256, 0, st>>>(w, (size_t)n * k, trailer + 1);
    split_weight_rows_kernel<<<cdiv((long)n * k, 256), 256, 0, st>>>(w, out, n, k);
    CHECK_LAUNCH(ctx, "split_weight_rows");
    return AVCER_OK;
}

int k_weight_frags(avcer_ctx* ctx, const bf16_t* rows, bf16_t* out, int n, int k, hipStream_t st) {
    if (n % 16 || k % 32) return set_err(ctx, AVCER_EINVAL, "weight_frags: n=%d must be a multiple of 16, k=%d of 32", n, k);
    weight_frags_kernel<<<cdiv((long)n * (k / 32) * 8, 256), 256, 0, st>>>((const uint4*)rows, (uint4*)out, n, k);
    CHECK_LAUNCH(ctx, "weight_frags");
    return AVCER_OK;
}

int k_split_weights(avcer_ctx* ctx, const float* w, bf16_t* out, size_t n, hipStream_t st) {
    split_weights_kernel<<<cdiv((long)n, 256), 256, 0, st>>>(w, out, n, ctx->ovf);
    CHECK_LAUNCH(ctx, "split_weights");
    return AVCER_OK;
}
