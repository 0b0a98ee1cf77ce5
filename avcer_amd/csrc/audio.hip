// The audio model of libavcer_hip.so -- a wav2vec2 trunk under a GRU or a TransformerLayer head -- as a sequence of the kernels in
// gemm.hip / kernels.hip / attention.hip / gru.hip, and the C entries that run it (the loader and the aud_* getters and setters stay
// with the other loaders in api.hip).  Host code only.
#include "net.h"

#include <cmath>

// ------------------------------------------------------------------------------------------------ audio model
// ref: architectures/audio_8_cl.py:131-190; transformers 4.36.2 Wav2Vec2Model with feat_extract_norm="layer",
// do_stable_layer_norm=True (third party); architectures/attention_layers.py:221-267.
// Residual streams stay f32 in every mode; MFMA operand tensors (LN outputs, attention context, GELU'd FFN hidden,
// conv-extractor activations) are f32 / bf16 / sp32 pairs according to the mode.
//
// The head is what the loaded weights hold (avcer_load_audio): the two TransformerLayers of ExprModelV2 / V3, or the two-layer GRU of
// ExprModelV1 (ref: architectures/audio_8_cl.py:18-72, audio_7_cl.py:18-72) -- per layer one contraction for the input projections
// of all steps and ONE launch for the recurrence (gru.hip) -- in front of the same conv head at width 256 instead of 1024.
namespace {
const int ck[7] = {10, 3, 3, 3, 3, 2, 2}, cs[7] = {5, 2, 2, 2, 2, 2, 2};  // the extractor's kernels and strides
constexpr int C = 512, E = 1024, FF = 4096, GH = 256;                      // extractor, trunk and FFN widths; the GRU's hidden size

// One call of the audio model: its kinds, its shapes, the workspace of a pass, and the stages of a pass in the order they run
struct AudioPass {
    Net& net;
    avcer_ctx* const ctx = net.ctx;
    const hipStream_t st = net.st;
    const int act = net.act.kind;                               // storage of MFMA operand tensors: f32 / bf16 / sp32
    const int rk = net.x3 ? KIND_SP32 : KIND_F32;               // operands of the GRU and the conv head: the bf16 mode runs them as f32
    const int plain = act == KIND_BF16 ? KIND_BF16 : KIND_F32;  // storage of GEMM outputs read by LN / attention
    const size_t es = net.act.es;
    // GELU: the library erff in the f32 mode; the short Abramowitz-Stegun erf (gemm_dev.h gelu_fast, same 5e-7 bound as
    // the exact form's own f32 rounding) where the contractions around it are bf16 or split-fp16
    const int gelu = act == KIND_F32 ? 2 : 3;
    const bool gru = ctx->aud_head == 1;
    const int HE = gru ? GH : E;  // the head's width
    int len[8], S, L1, L2, L3, NB;  // samples (len[0]) and steps behind every extractor layer; tokens; the conv head's steps; windows per pass
    decltype(&k_attention) attention;
    int nb;  // windows of the pass under way, and its token rows: begin()
    long r;
    float *wn, *H, *O, *c1o, *c2o, *pooled, *gxp;
    void *EA, *EB, *TMP, *QKV, *FFB, *ATT;
    Pair X, Y, mp, gh[2];  // the operand copies of X and Y are of kind `act`, those of mp and the GRU layers' sequences of `rk`

    // ---- shapes of a call of n windows of t samples, and the windows per pass
    int shape(int n, int t) {
        len[0] = t;
        for (int i = 0; i < 7; ++i) {
            if (len[i] < ck[i]) return set_err(ctx, AVCER_EINVAL, "audio_forward: %d samples is too short", t);
            len[i + 1] = (len[i] - ck[i]) / cs[i] + 1;
        }
        S = len[7];
        if (S > ctx->aud_max_tokens)
            return set_err(ctx, AVCER_EINVAL, "audio_forward: %d tokens > %d (window longer than ~%.1f s; avcer_set_audio_max_tokens)", S,
                           ctx->aud_max_tokens, ctx->aud_max_tokens * 0.02 + 0.025);
        // up to 256 tokens a head's K and V fit LDS whole (k_attention); past that key tiles are streamed through it
        attention = S <= 256 ? k_attention : k_attention_long;
        L1 = (S - 2 * 4 - 1) / 3 + 1;  // Conv1d k5 s3 dil2
        L2 = L1 / 5;                   // MaxPool1d(5)
        L3 = L2 - 2;                   // Conv1d k3
        if (S < 9 || L2 < 3) return set_err(ctx, AVCER_EINVAL, "audio_forward: %d tokens is too short for the head", S);
        // Windows per pass: 128 up to 256 tokens; past that as many as keep a pass at the 32768 token rows of 128 x 256 (the carved
        // workspace stays what it was), and few enough that the pass's largest contraction operand -- the first extractor layer's
        // output, [nb, len[1], 512] -- stays inside the 4 GiB range of a buffer descriptor (conv_gemm refuses 0xFFFFFF00 bytes and up)
        NB = S <= 256 ? std::min(n, 128) : std::min(n, std::max(1, 128 * 256 / S));
        while (S > 256 && NB > 1 && (size_t)NB * len[1] * 512 * es >= (size_t)0xFFFFFF00u) --NB;
        return AVCER_OK;
    }
    void begin(int s0, int n) { nb = std::min(NB, n - s0); r = (long)nb * S; }  // ---- the pass that starts at window s0 of n
    // ---- the workspace of a pass of NB windows
    int carve() {
        const size_t rows = (size_t)NB * S, e0 = (size_t)NB * len[1] * C * es, e1 = (size_t)NB * len[2] * C * es;
        return ws_carve(ctx, WS_AUDIO, "audio", [&](Arena& ar) {
            wn = ar.get<float>((size_t)NB * len[0] * 4);
            EA = ar.get(e0);
            EB = ar.get(e1);
            TMP = ar.get(e1);
            H = ar.get<float>(rows * E * 4);  // residual stream
            O = ar.get<float>(rows * E * 4);
            X.f = ar.get<float>(rows * E * 4);
            Y.f = ar.get<float>(rows * E * 4);
            X.op = carve_op(ar, rows * E * es, act);  // operand-typed copies (bf16 or sp32) of f32 tensors
            Y.op = carve_op(ar, rows * E * es, act);
            QKV = ar.get(rows * 3 * E * es);
            FFB = ar.get(rows * FF * es);
            ATT = ar.get(rows * E * es);
            c1o = ar.get<float>((size_t)NB * L1 * HE * 4);
            mp = carve_pair(ar, (size_t)NB * L2 * HE * 4, (size_t)NB * L2 * HE * 4, rk);  // x3 mode: td4's operand as sp32 pairs
            c2o = ar.get<float>((size_t)NB * L3 * HE * 4);
            pooled = ar.get<float>((size_t)NB * HE * 4);
            // the GRU head: one layer's input projections at a time, and both layers' sequences as f32 (taps, the f32 modes'
            // operand) and as sp32 pairs (x3 mode: the operand of layer 2's projection and of td0)
            if (gru) gxp = ar.get<float>(rows * 3 * GH * 4);
            for (int l = 0; gru && l < 2; ++l) gh[l] = carve_pair(ar, rows * GH * 4, rows * GH * 4, rk);
        });
    }
    // LayerNorm `p` of `rows` rows of c channels, then activation `fn`, into whichever of y.f and y.op (in `act`) y has
    void ln(const void* x, int x_kind, const std::string& p, Pair y, long rows, int c, int fn) {
        net.chk(k_layernorm(ctx, x, nullptr, net.F(p + ".g"), net.F(p + ".b"), y.f, y.op, rows, c, 1e-5f, fn, x_kind, act, st));
        if (ctx->tap_dst) net.tap(("ln:" + p).c_str(), operand(y, act).p, (size_t)rows * c * es);
    }
    // ---- normalisation and the conv feature extractor, 7 x (Conv1d -> LN(512) -> GELU): returns its output [r, 512] in `act`
    const void* extract(const float* x0, int normalize) {
        if (normalize) {
            net.chk(k_wav_normalize(ctx, x0, wn, nb, len[0], st));
            x0 = wn;
        }
        net.chk(k_conv0_ln_gelu(ctx, x0, net.F("fe0.w"), net.F("fe0.cb"), net.F("fe0.ln.g"), net.F("fe0.ln.b"), EA, nb, len[0], len[1], act, st));
        net.tap("norm", x0, (size_t)nb * len[0] * 4);
        net.tap("conv0", EA, (size_t)nb * len[1] * C * es);
        void *cur = EA, *nxt = EB;
        for (int i = 1; i < 7; ++i) {
            const std::string p = "fe" + std::to_string(i);
            net.gemm(conv1d_desc(nb, len[i], C, ck[i], cs[i], 0, 1, len[i + 1], C, 0), p + ".w", nullptr, net.F(p + ".cb"), cur, nullptr, TMP, act, plain);
            ln(TMP, plain, p + ".ln", only(nxt, act), (long)nb * len[i + 1], C, gelu);
            std::swap(cur, nxt);
            if (i == 1) nxt = EA;  // EA (largest) is free once layer 1 has consumed it
        }
        net.tap("extract", cur, (size_t)r * C * es);
        return cur;
    }
    // ---- feature projection, LN(512) -> Linear 512 -> 1024, and the positional conv embedding added to it: returns the residual stream
    float* project(const void* feats) {
        ln(feats, act, "fp.ln", only(TMP, act), r, C, 0);
        net.gemm(linear_desc(r, C, E, 0), "fp.w", nullptr, net.F("fp.b"), TMP, nullptr, H, act, KIND_F32);
        net.tap("proj", H, (size_t)r * E * 4);
        const Pair pin{H, X.op};  // the pos-conv's operand: H itself, or its copy in X's (still free) operand half
        if (act == KIND_BF16) net.chk(k_f32_to_bf16(ctx, H, (bf16_t*)pin.op, (size_t)r * E, st));
        if (act == KIND_SP32) net.chk(k_split_weights(ctx, H, (bf16_t*)pin.op, (size_t)r * E, st));  // same sp32 layout as split weights
        net.tap("pos_in", operand(pin, act).p, (size_t)r * E * es);
        // k=128, groups=16, pad 64, drop last, GELU, then + H: 16 groups of 64 channels in ONE launch (grid.y = group)
        avcer_conv_desc d = conv1d_desc(nb, S, 64, 128, 1, 64, 1, S, 64, gelu);
        d.x_stride_b = (int64_t)S * E; d.x_stride_h = E; d.x_stride_w = E;
        d.y_ld = E; d.r_ld = E; d.res_after_act = 1; d.groups = 16;
        net.gemm(d, "pos.w", nullptr, net.F("pos.b"), operand(pin, act), H, O, KIND_F32);
        net.tap("posconv", O, (size_t)r * E * 4);
        return O;
    }
    // ---- pre-LN encoder layer l of the trunk, in place on the residual stream h
    void encoder_layer(int l, float* h) {
        const std::string p = "enc" + std::to_string(l);
        ln(h, KIND_F32, p + ".ln1", only(TMP, act), r, E, 0);
        net.gemm(linear_desc(r, E, 3 * E, 0), p + ".qkv.w", nullptr, net.F(p + ".qkv.b"), TMP, nullptr, QKV, act, plain);
        net.chk(attention(ctx, QKV, ATT, nb, S, 16, 64, 0.125f, plain, act, st));
        if (ctx->tap_dst) net.tap(("att:" + p).c_str(), ATT, (size_t)r * E * es);
        net.gemm(linear_desc(r, E, E, 0), p + ".o.w", nullptr, net.F(p + ".o.b"), ATT, h, h, act, KIND_F32);
        ln(h, KIND_F32, p + ".ln2", only(TMP, act), r, E, 0);
        net.gemm(linear_desc(r, E, FF, gelu), p + ".ff1.w", nullptr, net.F(p + ".ff1.b"), TMP, nullptr, FFB, act, act);
        net.gemm(linear_desc(r, FF, E, 0), p + ".ff2.w", nullptr, net.F(p + ".ff2.b"), FFB, h, h, act, KIND_F32);
        net.tap(("layer" + std::to_string(l)).c_str(), h, (size_t)r * E * 4);
    }
    // ---- ExprModelV1: two GRU layers over X (hidden 256; f32 state in every mode, f32 operands in the bf16 mode): returns gh[1] for td0
    Operand gru_head() {
        if (net.x3) net.chk(k_split_weights(ctx, X.f, (bf16_t*)X.op, (size_t)r * E, st));  // the trunk's output as sp32 pairs
        for (int l = 0; l < 2; ++l) {
            const std::string p = "gru" + std::to_string(l + 1);
            net.gemm(linear_desc(r, l ? GH : E, 3 * GH, 0), p + ".wih.w", nullptr, net.F(p + ".wih.b"), operand(l ? gh[0] : X, rk), nullptr, gxp, KIND_F32);
            const Tensor* whh = net.T(p + ".whh.w");
            const float* bhh = net.F(p + ".whh.b");
            if (net.err == AVCER_OK && net.x3 && !whh->x3f) net.err = set_err(ctx, AVCER_ESTATE, "%s.whh.w: split weights not prepared", p.c_str());
            if (net.err != AVCER_OK) break;
            // (the recurrent weight's copies, not a pair: f32, or the split copy in fragment order)
            net.chk(launch_gru_layer(ctx, gxp, net.x3 ? (const void*)whh->x3f : whh->f32, net.x3, bhh, nb, S, gh[l].f, gh[l].op, st));
            net.tap(p.c_str(), gh[l].f, (size_t)r * GH * 4);
        }
        return operand(gh[1], rk);
    }
    // ---- ExprModelV2 / V3: two first-party TransformerLayers (32 x 32 and 16 x 64 heads) over X: returns the conv head's operand, X
    Operand transformer_head() {
        for (int l = 1; l <= 2; ++l) {
            const std::string p = "tl" + std::to_string(l);
            const int heads = l == 1 ? 32 : 16, dh = E / heads;
            // x + PE is both the projections' operand (typed copy) and the residual (f32)
            net.chk(k_add_pe(ctx, X.f, net.F("pe"), Y.f, Y.op, nb, S, E, act, st));
            net.gemm(linear_desc(r, E, 3 * E, 0), p + ".qkv.w", nullptr, nullptr, operand(Y, act), nullptr, QKV, plain);
            net.chk(attention(ctx, QKV, ATT, nb, S, heads, dh, 1.0f / sqrtf((float)dh), plain, act, st));
            if (ctx->tap_dst) {
                net.tap(("att:" + p).c_str(), ATT, (size_t)r * E * es);
                net.tap(("pe:" + p).c_str(), operand(Y, act).p, (size_t)r * E * es);
            }
            net.gemm(linear_desc(r, E, E, 0), p + ".o.w", nullptr, nullptr, ATT, Y.f, H, act, KIND_F32);
            ln(H, KIND_F32, p + ".ln1", Y, r, E, 0);
            net.gemm(linear_desc(r, E, E, 1), p + ".ff1.w", nullptr, net.F(p + ".ff1.b"), operand(Y, act), nullptr, FFB, act);
            net.gemm(linear_desc(r, E, E, 0), p + ".ff2.w", nullptr, net.F(p + ".ff2.b"), FFB, Y.f, H, act, KIND_F32);
            ln(H, KIND_F32, p + ".ln2", X, r, E, 0);
            net.tap(p.c_str(), X.f, (size_t)r * E * 4);
        }
        return operand(X, act);
    }
    // ---- conv head on hx [nb, S, HE]: Conv1d k5 s3 dil2 + BN -> MaxPool(5) -> ReLU -> Conv1d k3 + BN -> mean -> ReLU -> Linear
    void conv_head(Operand hx, float* logits) {
        net.gemm(conv1d_desc(nb, S, HE, 5, 3, 0, 2, L1, HE, 0), "td0.w", net.F("td0.s"), net.F("td0.b"), hx, nullptr, c1o, KIND_F32);
        net.chk(k_maxpool1d_relu(ctx, c1o, mp.f, mp.op, nb, L1, L2, HE, 5, st));
        net.gemm(conv1d_desc(nb, L2, HE, 3, 1, 0, 1, L3, HE, 0), "td4.w", net.F("td4.s"), net.F("td4.b"), operand(mp, rk), nullptr, c2o, KIND_F32);
        net.tap("td0", c1o, (size_t)nb * L1 * HE * 4);
        net.tap("mp", mp.f, (size_t)nb * L2 * HE * 4);
        net.tap("td4", c2o, (size_t)nb * L3 * HE * 4);
        net.chk(k_mean_time_relu(ctx, c2o, pooled, nb, L3, HE, st));
        net.tap("pooled", pooled, (size_t)nb * HE * 4);
        net.chk(k_small_linear(ctx, pooled, net.F("fd.w"), net.F("fd.b"), logits, nullptr, nb, HE, ctx->aud_classes, 0, st));
    }
};
}  // namespace

// `features` (may be null): the pooled head activations [n, 256 or 1024], what the reference's get_features returns beside the logits.
extern "C" int avcer_audio_forward_features(avcer_ctx* ctx, const float* wav, int n, int t, int normalize, int mode,
                                            float* logits, float* features, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (!ctx->aud.loaded) return set_err(ctx, AVCER_ESTATE, "audio weights not loaded");
    if (!wav || !logits || n <= 0) return set_err(ctx, AVCER_EINVAL, "audio_forward: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    TRY(begin_forward(ctx, "audio_forward", ctx->aud, mode, true, st));
    Net net{ctx, ctx->aud, mode_storage(mode), st};
    AudioPass a{net};
    TRY(a.shape(n, t));
    TRY(a.carve());
    for (int s0 = 0; s0 < n; s0 += a.NB) {
        a.begin(s0, n);
        float* h = a.project(a.extract(wav + (size_t)s0 * t, normalize));
        for (int l = 0; l < 12; ++l) a.encoder_layer(l, h);
        net.chk(k_layernorm(ctx, h, nullptr, net.F("enc.ln.g"), net.F("enc.ln.b"), a.X.f, nullptr, a.r, E, 1e-5f, 0, 0, 0, st));
        net.tap("w2v", a.X.f, (size_t)a.r * E * 4);
        const Operand hx = a.gru ? a.gru_head() : a.transformer_head();
        if (net.err == AVCER_OK) a.conv_head(hx, logits + (size_t)s0 * ctx->aud_classes);  // (a head that lacks a weight has set it)
        if (net.err != AVCER_OK) return net.err;
        if (features) HIP_TRY(ctx, hipMemcpyAsync(features + (size_t)s0 * a.HE, a.pooled, (size_t)a.nb * a.HE * 4, hipMemcpyDeviceToDevice, st));
    }
    return net.err;
}

extern "C" int avcer_audio_forward(avcer_ctx* ctx, const float* wav, int n, int t, int normalize, int mode, float* logits, avcer_stream_t stream) {
    return avcer_audio_forward_features(ctx, wav, n, t, normalize, mode, logits, nullptr, stream);
}

// One GRU layer's recurrence on caller tensors (kernel-level tests; gru.hip): AVCER_MODE_F16X3 splits w_hh and puts it into
// fragment order here, in a workspace of its own; the other two modes run the f32 form
extern "C" int avcer_gru_layer(avcer_ctx* ctx, const float* xp, const float* w_hh, const float* b_hh, int n, int s, int h, int mode,
                               float* h_seq, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (!xp || !w_hh || !b_hh || !h_seq || n <= 0 || s <= 0) return set_err(ctx, AVCER_EINVAL, "gru_layer: bad arguments");
    if (h != 256) return set_err(ctx, AVCER_EINVAL, "gru_layer: hidden size %d (256 is what the kernel is built for)", h);
    if (mode < AVCER_MODE_FP32 || mode > AVCER_MODE_F16X3) return set_err(ctx, AVCER_EINVAL, "gru_layer: mode %d", mode);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (mode != AVCER_MODE_F16X3) return launch_gru_layer(ctx, xp, w_hh, 0, b_hh, n, s, h_seq, nullptr, st);
    bf16_t *rows, *frags;
    TRY(ws_carve(ctx, WS_GRU, "gru_layer", [&](Arena& ar) {
        rows = ar.get<bf16_t>(split_bytes((size_t)3 * h * h));
        frags = ar.get<bf16_t>(split_bytes((size_t)3 * h * h));
    }));
    TRY(k_split_weight_rows(ctx, w_hh, rows, 3 * h, h, st));
    TRY(k_weight_frags(ctx, rows, frags, 3 * h, h, st));
    return launch_gru_layer(ctx, xp, frags, 1, b_hh, n, s, h_seq, nullptr, st);
}
