// Host-side declarations a network driver needs: a forward pass's Net, a tensor's operand pair, the contraction descriptors, the
// ResNet-50 body driver and the two-lane fork / join.  Included by api.hip (which defines Net's methods, the descriptors and the loaders),
// visual.hip (which defines run_bneck_stage), audio.hip and detect.hip only: host code, and no translation unit that holds a kernel sees it.
#pragma once

#include "common.h"

#include <algorithm>

// A tensor as f32 and once more in an operand storage (bf16, or sp32 pairs).  `op` is null where the pass keeps no such copy.
struct Pair { float* f; void* op; };
struct Operand { const void* p; int kind; };  // what a contraction reads, and the KIND_* to pass with it
// The copy of `t` that a reader of storage `kind` takes: the ONE place that chooses between a tensor's two copies
inline Operand operand(Pair t, int kind) { return {kind == KIND_F32 ? (const void*)t.f : t.op, kind}; }
// A tensor that exists once, in storage `kind` (a LayerNorm output that only a contraction reads): its other half is null, so it is
// read back with operand(., kind) of that same kind only
inline Pair only(void* p, int kind) { return kind == KIND_F32 ? Pair{(float*)p, nullptr} : Pair{nullptr, p}; }
// `t` from its element `elems` on; `es`: bytes per element of the operand storage
inline Pair advance(Pair t, size_t elems, size_t es) { return {t.f + elems, t.op ? (char*)t.op + elems * es : nullptr}; }
// Carves the operand half of a pair, of storage `kind`: the region is taken in every mode, but a kind that reads and writes f32 gets
// no `op`.  carve_pair: both halves, where they lie side by side; elsewhere `f` is carved on its own, where it always was
inline void* carve_op(Arena& ar, size_t bytes, int kind) {
    void* op = ar.get(bytes);
    return kind == KIND_F32 ? nullptr : op;
}
inline Pair carve_pair(Arena& ar, size_t f_bytes, size_t op_bytes, int kind) {
    float* f = ar.get<float>(f_bytes);
    return {f, carve_op(ar, op_bytes, kind)};
}
// device bytes of one split-fp16 weight copy: the data, its scale trailer (split_dev.h), rounded to 256 (api.hip)
size_t split_bytes(size_t numel);

// One forward pass of model `m` on stream `st`: looks tensors up by name, issues the contractions, keeps the first error
struct Net {
    avcer_ctx* ctx;
    Model& m;
    Storage act;  // activation storage, and with it the operand type of the MFMA contractions
    hipStream_t st;
    bool x3 = act.kind == KIND_SP32;  // f32-grade activations, split-fp16 MFMA (AVCER_MODE_F16X3)
    int err = AVCER_OK;

    const Tensor* T(const std::string& name);
    const float* F(const std::string& name) {
        const Tensor* t = T(name);
        return t ? t->f32 : nullptr;
    }
    // contraction with weights `wname`; akind / okind = storage of the activations read / written (KIND_*), which with the
    // shape selects the kernel instantiation (avcer_conv_gemm dtype: gemm_forms.h choose_gemm)
    void gemm(avcer_conv_desc d, const std::string& wname, const float* scale, const float* bias, const void* x,
              const void* res, void* y, int akind, int okind, const void* x2 = nullptr);
    void gemm(avcer_conv_desc d, const std::string& wname, const float* scale, const float* bias, Operand x, const void* res, void* y,
              int okind) { gemm(d, wname, scale, bias, x.p, res, y, x.kind, okind); }
    void chk(int r) { if (err == AVCER_OK && r != AVCER_OK) err = r; }
    // debug tap: raw copy of min(requested, available) bytes of an intermediate tensor
    void tap(const char* name, const void* src, size_t bytes);
};

avcer_conv_desc linear_desc(long m, int k, int n, int act);
avcer_conv_desc conv2d_desc(int nb, int h, int w, int c, int kh, int kw, int stride, int pad, int n, int act);
// The 7x7/2 stem of the fp32 / bf16 modes: 8 tap rows x (8 pixels x 4 channels) over a zero-bordered [nb, ph, pw, 4] image, stride 2
avcer_conv_desc stem_desc(int nb, int ph, int pw);
// Conv1d over a time-major [nb, len, c] tensor
avcer_conv_desc conv1d_desc(int nb, int len, int c, int k, int stride, int pad, int dil, int out_len, int n, int act);

// Stage-3 tails (conv3 + residual + the next block's conv1) of at most this many positions run as two contractions instead of
// the fused bneck_tail2_kernel: bit-identical, and faster up to 64 frames per call (0.66 vs 0.90 ms at one frame, 2.39 vs 2.42
// at 64, 3.51 vs 3.44 at 128: tools/tail_pair_probe.py, profiles/experiments/r05_tail_pair_probe.txt)
constexpr long kTailPairRows = 16384;
constexpr int kStages[4][3] = {{64, 3, 1}, {128, 4, 2}, {256, 6, 2}, {512, 3, 2}};  // video.py:105-108,165

// A packed weight blob -> model `m` on the device; frees what `m` held before, its lazy copies included
int load_blob(avcer_ctx* ctx, Model& m, const void* blob, size_t nbytes);

// What every forward pass (`who`) begins with: the mode's range, the device, the mode's lazy weight copies of model `m`
// (`bf16_form` = false: a pass that runs the bf16 mode on its f32 kernels and prepares no bf16 copies)
int begin_forward(avcer_ctx* ctx, const char* who, Model& m, int mode, bool bf16_form, hipStream_t st);

// The recognition CNN (visual.hip static_forward_lane) and the RetinaFace detector (detect.hip face_forward_lane) run the same
// ResNet-50 body on the same kernels.  Trunk is a body between stages: the activation X on an h x w grid of cin channels per
// frame, the ping-pong pair a block writes into (the one X does not occupy), the buffers of a block's conv1 / conv2 outputs, and
// the body's three properties (run_bneck_stage): where the stride lives, whether the chain gets the fragment-order conv2
// weights, the tap name prefix.
struct Trunk {
    void* X;
    void* pp[2];
    void* T1;
    void* T2;
    int h, w, cin;
    bool stride_last;
    bool w2_frags;
    const char* tap;
};

// Blocks [b_begin, b_end) of stage li (0-based) on nb frames; the last of them writes to `last_out` when given (visual.hip)
void run_bneck_stage(Net& net, Trunk& t, int li, int b_begin, int b_end, int nb, void* last_out, const std::string& end_tap);

// The two lanes of a call (static_forward_impl, face_forward_impl): lane(1, s) on the context's second stream s, forked from `st`
// by an event, then lane(0, st), then the join of s back into `st`.  The stream and its two events are created together on first
// use.  Once the fork is recorded the join is always attempted -- the caller's stream must not run ahead of the second lane -- and
// if the join itself fails, the host waits for the second lane instead.  Returns the first error.
template <class Lane>
int run_two_lanes(avcer_ctx* ctx, hipStream_t st, const Lane& lane) {
    auto hip = [ctx](hipError_t e, const char* what) {
        return e == hipSuccess ? AVCER_OK : set_err(ctx, AVCER_EHIP, "two lanes: %s failed: %s", what, hipGetErrorString(e));
    };
    if (!ctx->lane_stream) {
        hipStream_t s = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        int r = hip(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreateWithFlags");
        for (hipEvent_t& e : ev)
            if (r == AVCER_OK) r = hip(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreateWithFlags");
        if (r != AVCER_OK) {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
            if (s) (void)hipStreamDestroy(s);
            return r;
        }
        ctx->lane_stream = s;
        ctx->lane_ev[0] = ev[0];
        ctx->lane_ev[1] = ev[1];
    }
    hipStream_t s = ctx->lane_stream;
    // (a lane that has to grow its workspace synchronises the device first, ws_reserve: harmless here, both lanes only wait)
    TRY(hip(hipEventRecord(ctx->lane_ev[0], st), "fork hipEventRecord"));  // the inputs (and weight copies) are ready on `st`
    int r = hip(hipStreamWaitEvent(s, ctx->lane_ev[0], 0), "fork hipStreamWaitEvent");
    if (r == AVCER_OK) r = lane(1, s);
    if (r == AVCER_OK) r = lane(0, st);
    const hipError_t e = hipEventRecord(ctx->lane_ev[1], s);
    const int rj = hip(e == hipSuccess ? hipStreamWaitEvent(st, ctx->lane_ev[1], 0) : e, "join");
    if (rj != AVCER_OK) (void)hipStreamSynchronize(s);
    return r != AVCER_OK ? r : rj;
}
