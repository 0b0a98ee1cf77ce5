// Internal declarations shared by the translation units of libavcer_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/avcer_hip.h"
#include "arena.h"
#include "gemm_forms.h"

typedef uint16_t bf16_t;  // raw bfloat16 bits

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

// the context's workspace slots (ws_reserve): one per pipeline, the second lanes of the two ResNets and two utilities
enum { WS_STATIC = 0, WS_DYNAMIC = 1, WS_AUDIO = 2, WS_FACE = 3, WS_NMS = 4, WS_CEILINGS = 5, WS_STATIC_LANE1 = 6, WS_FACE_LANE1 = 7,
       WS_GRU = 8, WS_JPEG = 9, WS_RESIZE = 10, WS_CHART = 11, WS_COUNT = 12 };

// storage of an activation tensor: a KIND_* of gemm_forms.h
struct Storage { int kind; size_t es; };  // es: bytes per element
// activation storage of a forward pass in `mode`: f32 / bf16 / sp32 pairs
inline Storage mode_storage(int mode) {
    return mode == AVCER_MODE_BF16 ? Storage{KIND_BF16, 2} : Storage{mode == AVCER_MODE_F16X3 ? KIND_SP32 : KIND_F32, 4};
}
// A kind as an element type, for the launchers: with_storage<Ts...>(kind, f) calls f(storage_tag<T>{}) with the T among Ts that
// stores `kind` (float / bf16_t / sp32_t of split_dev.h), so a launcher writes its launch expression once, on
// `typename decltype(tag)::type`.  Ts are the storages the kernel is built for; a launcher that takes fewer than three rejects
// the others in front, and any kind that is left goes to the first of Ts, as the last `else` of a hand-written chain did.
struct sp32_t;
template <typename T> struct storage_tag { using type = T; };
template <typename T> constexpr int storage_kind = std::is_same<T, bf16_t>::value ? KIND_BF16 : std::is_same<T, sp32_t>::value ? KIND_SP32 : KIND_F32;
template <typename T0, typename... Ts, typename F> void with_storage(int kind, F&& f) {
    if (!((kind == storage_kind<Ts> ? (f(storage_tag<Ts>{}), true) : false) || ...)) f(storage_tag<T0>{});
}
template <typename F> void with_storage(int kind, F&& f) { with_storage<float, bf16_t, sp32_t>(kind, f); }

// One packed tensor of a weight blob, resident on the device in f32 and (lazily) in bf16.
struct Tensor {
    float* f32 = nullptr;
    bf16_t* bf16 = nullptr;
    bf16_t* x3 = nullptr;  // split-fp16 copy (scaled hi/lo per 32-element K group + trailer, split_dev.h) for AVCER_MODE_F16X3
    bf16_t* x3f = nullptr; // the same in MFMA fragment order (conv_gemm dtype 7 / 8), where the shape allows it
    size_t numel = 0;
    int64_t dims[4] = {0, 0, 0, 0};
    int ndim = 0;
};

struct Model {
    bool loaded = false;
    std::map<std::string, Tensor> t;
    std::vector<void*> allocs;
};

struct avcer_ctx {
    int device = 0;
    char err[512] = {0};
    Model stat, dyn, aud, face;
    int face_kind = 0;        // the loaded detector (avcer_face_kind): 0 none, 1 RetinaFace-R50, 2 RetinaFace-MobileNet-0.25, 3 S3FD
    int aud_classes = 0;
    int aud_head = 0;         // head of the loaded audio model (avcer_audio_head_kind): 0 none, 1 GRU (ExprModelV1), 3 transformer (V2 / V3)
    int aud_max_tokens = 256; // longest audio window the forward accepts, in tokens (avcer_set_audio_max_tokens; reset by avcer_load_audio)
    int static_batch = 1024;  // frames per internal pass of the static CNN (4 GiB buffer-descriptor limit at f32)
    int static_back = 0;      // frames per back pass of the static CNN (0: two front passes; avcer_set_static_back_batch)
    int static_lanes = 2;     // calls of lane_min .. lane_max frames as two half-batches on two streams (avcer_set_static_lanes)
    bool skip_unread = true;  // the block in front of a strided last block stores the OUT rows that block reads alone (avcer_set_skip_unread_rows)
    int lane_min = 32, lane_max = 2048;  // avcer_set_static_lane_range (tools/two_lane_sweep.py: two lanes win from 16 to 2048 frames)
    hipStream_t lane_stream = nullptr;  // the second lane's stream, created on first use, and its fork / join events
    hipEvent_t lane_ev[2] = {nullptr, nullptr};
    int block_slots = 512;    // 2 x hipDeviceProp_t::multiProcessorCount: what gemm_forms.h grid_rounds() divides a grid by
    // grow-only workspace arenas (activations), one per WS_* slot
    DevBuf ws[WS_COUNT];
    // device counter of the x3 mode's range contract: += 1 per thread that split a finite |x| >= 65520 into an fp16 pair
    // (split_dev.h sp_commit); read and reset by avcer_x3_overflow_count
    unsigned* ovf = nullptr;
    int64_t gemm_launches = 0;
    double gemm_flops = 0.0;
    // live HIP-event timing of conv_gemm launches (avcer_profile_*): pairs of events on the launch stream
    bool prof = false;
    std::vector<hipEvent_t> prof_ev;
    std::vector<int> prof_fam;  // kernel family of every event pair (AVCER_FAM_*)
    struct ProfLaunch { double flops, bytes; long m, n, k; };
    std::vector<ProfLaunch> prof_log;  // per event pair: algorithmic FLOPs, compulsory bytes and the contraction's M, N, K
    size_t prof_used = 0;
    // per kernel family since the last avcer_profile_read*: launches, algorithmic FLOPs and compulsory HBM bytes
    int64_t fam_launches[8] = {0};
    double fam_flops[8] = {0};
    double fam_bytes[8] = {0};
    // one-shot debug tap (avcer_debug_tap): copy the named intermediate activation to a caller buffer
    std::string tap_name;
    void* tap_dst = nullptr;
    size_t tap_bytes = 0;
    int64_t tap_copied = -1;
};

int set_err(avcer_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return set_err((ctx), AVCER_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                           __FILE__, __LINE__);                                                    \
    } while (0)

#define TRY(expr)                  \
    do {                           \
        int _r = (expr);           \
        if (_r != AVCER_OK) return _r; \
    } while (0)

// right behind a kernel launch: a launch that failed returns "<name> launch: <HIP's message>" from the launcher
#define CHECK_LAUNCH(ctx, name)                                                                      \
    do {                                                                                             \
        hipError_t _e = hipGetLastError();                                                           \
        if (_e != hipSuccess) return set_err((ctx), AVCER_EHIP, name " launch: %s", hipGetErrorString(_e)); \
    } while (0)

// blocks of `b` items that cover `a` items, as a grid dimension: the quotient must fit an int (a < 2^31 * b), which no launcher checks
inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

int ws_reserve(avcer_ctx* ctx, int slot, size_t bytes, void** out);

// An allocation sized by its own layout (arena.h): `carve` is measured, alloc(bytes, &p) provides that many bytes, and `carve`
// runs again on exactly those -- so no size is stated twice, and a carving that differs between its two runs is an error.
// A carving that takes nothing allocates nothing.
template <class Alloc, class Carve>
int carve_measured(avcer_ctx* ctx, const char* what, const Alloc& alloc, const Carve& carve) {
    const size_t bytes = Arena().run(carve);
    void* p = nullptr;
    if (bytes) TRY(alloc(bytes, &p));
    return Arena(p, bytes).run(carve) == bytes ? AVCER_OK : set_err(ctx, AVCER_ENOMEM, "%s workspace arithmetic", what);
}

// The workspace of a forward pass: slot `slot` grown to what `carve` takes (ws_reserve's policy), then carved
template <class Carve>
int ws_carve(avcer_ctx* ctx, int slot, const char* what, const Carve& carve) {
    return carve_measured(ctx, what, [&](size_t bytes, void** p) { return ws_reserve(ctx, slot, bytes, p); }, carve);
}

// PIL's NEAREST resize to 224 (data/utils.py:34): the source index of output index `o` along an axis of `len` source pixels.
// The one statement of the rule: preprocess_kernel, crop_tiles_kernel (kernels.hip) and jpeg_tiles_kernel (jpeg_decode.hip) call it.
__device__ __forceinline__ int nearest_src(int o, int len) { return min((int)(((double)o + 0.5) * ((double)len / 224.0)), len - 1); }

// ---- gemm.hip
int launch_conv_gemm(avcer_ctx* ctx, const avcer_conv_desc& d, int dtype, const void* x, const void* w,
                     const float* scale, const float* bias, const void* residual, void* y, hipStream_t st,
                     const void* x2 = nullptr);

// kernel families of the MFMA launches (avcer_profile_read_families; include/avcer_hip.h AVCER_FAM_*)
enum { FAM_GEMM = 0, FAM_GEMM_WD = 1, FAM_CHAIN = 2, FAM_TAIL = 3, FAM_STEM = 4, FAM_SKINNY = 5, FAM_GRU = 6, FAM_COUNT = 7 };
// `flops` / `bytes`: algorithmic work and compulsory HBM traffic of the launch (operands read once + outputs written once)
int prof_begin(avcer_ctx* ctx, hipStream_t st, hipEvent_t* ev0, hipEvent_t* ev1, int family, double flops, double bytes, long M = 0,
               long N = 0, long K = 0);

// ---- fused.hip (split-fp16 mode only)
// planes: fp16 hi plane [n][230][230][4] followed plane_bytes later by the lo plane; y: sp32 [n][55][55][64]
int launch_stem_pool(avcer_ctx* ctx, const void* planes, size_t plane_bytes, const void* w_x3, const float* scale,
                     const float* bias, void* y, int n, hipStream_t st);
int launch_stem_pool_u8(avcer_ctx* ctx, const uint8_t* frames, int in_h, int in_w, const void* w_x3, const float* scale,
                        const float* bias9, void* y, int n, hipStream_t st);
int launch_stem_pool_face(avcer_ctx* ctx, const uint8_t* frames, int h, int w, int rgb, const void* w_x3, const float* scale,
                          const float* bias, void* y, int n, hipStream_t st);
// conv2 + conv3 (+ residual) of one bottleneck and conv1 of the next block (t1n / w1n null when there is none);
// ds_cin = 0: x [M][4 planes] is the residual; ds_cin = 64: x [M][64] is the downsample operand and w3 is [4 planes][planes + 64];
// all activations sp32, weights split-fp16 (scaled, row-permuted) with the BN scale folded in (packing.py: *.wf, c3d.w)
// w2_frags: the conv2 weights once more in MFMA fragment order (k_weight_frags), or null: selects the spatial-tile form
// where it applies (planes 64, 55 x 55 images, a next conv1)
// keep = 2 (needs t1n, no downsample, out_step 1): OUT is stored at the even (y, x) of every image alone, at its full-grid
// addresses -- for the block whose OUT only a strided last block reads; the other rows of `out` are left as they were
int launch_bneck(avcer_ctx* ctx, int planes, int nb, int h, int w, const void* t1, const void* x, int ds_cin, int out_step,
                 void* out, void* t1n, const void* w2, const float* b2, const void* w3, const float* b3, const void* w1n,
                 const float* b1n, hipStream_t st, const void* w2_frags = nullptr, int keep = 1);

// conv3 + residual + ReLU of a planes-256 bottleneck and conv1 of the next block in one launch (t2 = conv2 output [M][256]);
// keep = 2: as launch_bneck's, on M = whole images of h x w positions
int launch_bneck_tail(avcer_ctx* ctx, int planes, long M, const void* t2, const void* x, void* out, void* t1n, const void* w3,
                      const float* b3, const void* w1n, const float* b1n, hipStream_t st, int keep = 1, int h = 0, int w = 0);

// ---- gru.hip
// The recurrence of one GRU layer (hidden size 256) over S steps in one launch: xp [n, S, 768] f32 (input projections + b_ih,
// gates r, z, n), w = W_hh [768][256] as f32 (x3 = 0) or as the fragment-order split copy (x3 = 1), bhh [768] ->
// h_seq [n, S, 256] f32 and, x3 only, h_sp: the same as sp32 pairs (or null)
int launch_gru_layer(avcer_ctx* ctx, const float* xp, const void* w, int x3, const float* bhh, int n, int S, float* h_seq, void* h_sp,
                     hipStream_t st);

// ---- mnet.hip (the MobileNet-0.25 detector: plain NHWC f32 activations in both of its modes)
// u8 frames [n, h, w, 3] -> conv 3x3/2 (3 -> 8) of pixel - mean, BN, LeakyReLU(0.1): y [n, ceil(h/2), ceil(w/2), 8]; wt [27][8]
int launch_mnet_stem(avcer_ctx* ctx, const uint8_t* frames, int n, int h, int w, int rgb, const float* wt, const float* s, const float* b,
                     float* y, hipStream_t st);
// one conv_dw block (depthwise 3x3 at `stride` + BN + leaky, pointwise 1x1 + BN + leaky) in one launch: x [nb, h, w, cin] ->
// y [nb, ceil(h/stride), ceil(w/stride), cout]; dww [9][cin]; pw = the pointwise weights [ceil64(cout)][ceil32(cin)] (zero-padded)
// as f32 (x3 = 0) or as their split copy with its trailer (x3 = 1)
int launch_dwsep(avcer_ctx* ctx, int cin, int cout, int stride, int x3, const float* x, const float* dww, const float* dws,
                 const float* dwb, const void* pw, const float* pws, const float* pwb, float* y, int nb, int h, int w, hipStream_t st);
// direct ks x ks convolution (ks 1 or 3, stride 1, same padding) of the neck: wt [ks * ks * cin][cout], cout a multiple of 16;
// y[pos * y_ld + y_coff + c] = act(acc * s[c] + b[c]) (s null: 1); act 0 none, 1 ReLU, 4 LeakyReLU(0.1)
int launch_mnet_conv(avcer_ctx* ctx, int ks, const float* x, const float* wt, const float* s, const float* b, float* y, int n, int h, int w,
                     int cin, int cout, int y_ld, int y_coff, int act, hipStream_t st);

// ---- s3fd.hip (the S3FD detector; `kind` = KIND_F32 or KIND_SP32, the storage of the activations)
// u8 frames [n, h, w, 3] -> conv1_1 3x3 pad 1 (3 -> 64) of RGB pixel - (123, 117, 104) + bias + ReLU: y [n, h, w, 64]; wt [27][64]
int launch_s3fd_stem(avcer_ctx* ctx, const uint8_t* frames, int n, int h, int w, int rgb, const float* wt, const float* b, void* y, int kind,
                     hipStream_t st);
// one level's loc + conf 3x3 convolutions, max-out (n_out 8) and softmax: x [nb, h, w, c], wt [9][c][n_out], rows written at
// f * P + row0; inv: scratch for nb * h * w inverse L2 norms (the level is normalised) or null (it is not)
int launch_s3fd_head(avcer_ctx* ctx, const void* x, int kind, float* inv, const float* wt, const float* b, int nb, int h, int w, int c,
                     int n_out, int row0, int P, float* loc, float* conf, hipStream_t st);

// ---- detect_tail.hip (decode, order and NMS of both detectors)
// RetinaFace: loc / conf / landms [T, P, ..] -> dets [T, P, 15]; dets -> out [T, top_k, 15], out_n [T] (order [T, nms_top_k] and
// count [T] are scratch)
int k_face_decode(avcer_ctx*, const float* loc, const float* conf, const float* landms, const float* priors, int T, int P, int im_h,
                  int im_w, float var0, float var1, float* dets, hipStream_t);
int k_face_nms(avcer_ctx*, const float* dets, int T, int P, float conf_thresh, float nms_thresh, int nms_top_k, int top_k,
               float threshold, int32_t* order, int32_t* count, float* out, int32_t* out_n, hipStream_t);
// S3FD's Detect + the predictor's loop: decode, order, NMS; ws = s3fd_detect_ws_bytes(T, P, nms_top_k) bytes
size_t s3fd_detect_ws_bytes(int T, int P, int nms_top_k);
int launch_s3fd_detect(avcer_ctx* ctx, const float* loc, const float* conf, const float* priors, int T, int P, int im_h, int im_w, float var0,
                       float var1, float conf_thresh, float nms_thresh, int nms_top_k, int top_k, float threshold, void* ws, float* out,
                       int32_t* out_n, hipStream_t st);

int measure_ceilings(avcer_ctx* ctx, double* mfma_bf16_tflops, double* hbm_copy_tbs, hipStream_t st);

// ---- kernels.hip (element-wise / reduction kernels; `kind` / `*_kind` = KIND_F32, KIND_BF16 or KIND_SP32, the storage of the activations)
// u8 frames -> the zero-bordered image [n,230,230,4] of the stem; kind: KIND_F32 or KIND_BF16
int k_preprocess(avcer_ctx*, const uint8_t* frames, int n, int in_h, int in_w, void* out, int kind, hipStream_t);
// k x k / 2 max-pool with padding `pad` (0 or 1), NHWC: x [n, h, w, c] -> y [n, oh, ow, c], oh / ow the caller's (floor or ceil); a tap
// outside the input does not exist.  Built for what is called: k = 2 on f32 / sp32 (S3FD), k = 3 on f32 / bf16 (the two ResNet stems)
int k_maxpool(avcer_ctx*, const void* x, void* y, int n, int h, int w, int c, int k, int pad, int oh, int ow, int kind, hipStream_t);
int k_avgpool_hw(avcer_ctx*, const void* x, float* y, void* y_sp32, int n, int hw, int c, int kind, hipStream_t);
// Grad-CAM of layer 4 for all 7 classes (kernels.hip): x = layer 4's output [n,7,7,2048] in storage `kind`, probs [n,7],
// h = fc1's pre-ReLU output [n,512], w1 = fc1.w [512,2048], w2 = fc2.w [7,512], g = scratch f32 [n,7,2048] -> cam f32 [n,7,49]
int k_cam_maps(avcer_ctx*, const void* x, const float* probs, const float* h, const float* w1, const float* w2, float* g,
               float* cam, int n, int kind, hipStream_t);
int k_small_linear(avcer_ctx*, const float* x, const float* w, const float* b, float* logits, float* probs, int m,
                   int k, int n, int relu_in, hipStream_t);
int k_lstm_cell(avcer_ctx*, const float* xproj, int64_t xproj_ld, const float* hproj, float* c, float* h_out, void* h_sp,
                int64_t h_ld, int n, int hid, int first, hipStream_t);
int k_wav_normalize(avcer_ctx*, const float* x, float* y, int n, int t, hipStream_t);
int k_conv0_ln_gelu(avcer_ctx*, const float* x, const float* w, const float* b, const float* g, const float* beta,
                    void* y, int n, int t_in, int t_out, int kind, hipStream_t);
int k_layernorm(avcer_ctx*, const void* x, const void* res, const float* g, const float* b, void* yf, void* yb,
                int64_t rows, int c, float eps, int act, int in_kind, int yb_kind, hipStream_t);
int k_add_pe(avcer_ctx*, const float* x, const float* pe, float* yf, void* yb, int n, int s, int c, int yb_kind, hipStream_t);
// ---- attention.hip: softmax(q k^T * scale) v per (window, head); S <= 256: one head's K and V stay in LDS
int k_attention(avcer_ctx*, const void* qkv, void* out, int n, int s, int heads, int d, float scale, int in_kind,
                int out_kind, hipStream_t);
// the same for 1 <= s <= AVCER_AUDIO_MAX_TOKENS: key tiles streamed through LDS, running softmax
int k_attention_long(avcer_ctx*, const void* qkv, void* out, int n, int s, int heads, int d, float scale, int in_kind,
                int out_kind, hipStream_t);
// ---- kernels.hip again
int k_maxpool1d_relu(avcer_ctx*, const float* x, float* y, void* y_sp32, int n, int t_in, int t_out, int c, int k, hipStream_t);
int k_mean_time_relu(avcer_ctx*, const float* x, float* y, int n, int t, int c, hipStream_t);
int k_f32_to_bf16(avcer_ctx*, const float* x, bf16_t* y, size_t n, hipStream_t);
int k_frame_mean(avcer_ctx*, const float* win_logits, const int32_t* lo, const int32_t* hi, int n_win, int c,
                 int n_frames, float* out, int32_t* count, hipStream_t);
int k_fuse(avcer_ctx*, const float* stat, const float* dyn, const float* aud, int n, int n_aud, int aud_c,
           const double* w /*[21] device-side by value*/, int has_w1, int cwt, int cmask, double* comp_prob,
           int32_t* comp_argmax, hipStream_t);
int k_fuse_videos(avcer_ctx*, const float* stat, const float* dyn, const float* win, const int32_t* lo, const int32_t* hi,
                  const int32_t* frame_off, const int32_t* win_off, const int32_t* n_aud, int n_videos, int n, int n_win, int c,
                  const double* w, int has_w1, int cwt, int cmask, float* aud_mean, int32_t* count, double* comp_prob,
                  int32_t* comp_argmax, hipStream_t);
// the same image from a preprocessed f32 tensor [n,3,224,224]; kind: KIND_F32, KIND_BF16, or 3 = planar fp16 hi / lo (two
// [n,230,230,4] planes, the stem_pool input)
int k_pack_nchw(avcer_ctx*, const float* x, int n, void* out, int kind, hipStream_t);
int k_gather_windows(avcer_ctx*, const float* feats, const int32_t* idx, int nwin, float* out, hipStream_t);
int k_audio_chunks(avcer_ctx*, const float* wav, const int32_t* starts, const int32_t* ends, int n, int window, int mode,
                   float* out, hipStream_t);
int k_split_weights(avcer_ctx*, const float* w, bf16_t* out, size_t n, hipStream_t);
int k_split_weight_rows(avcer_ctx*, const float* w, bf16_t* out, int n, int k, hipStream_t);
int k_weight_frags(avcer_ctx*, const bf16_t* rows, bf16_t* out, int n, int k, hipStream_t);
int k_face_pre(avcer_ctx*, const uint8_t* frames, int n, int h, int w, int ph, int pw, int rgb, void* out, int bf16, hipStream_t);
int k_upsample_add(avcer_ctx*, void* y, const void* coarse, int n, int h, int w, int ch, int cw, int c, int kind, hipStream_t);
int k_face_head(avcer_ctx*, const float* hd, int ld, int n, int hw, int row0, int P, float* loc, float* conf, float* landms,
                hipStream_t);
int k_crop_tiles(avcer_ctx*, const uint8_t* frames, int T, int H, int W, const int32_t* rects, int n, int swap_rb,
                 uint8_t* tiles, hipStream_t);
