// The visual models of libavcer_hip.so -- the recognition CNN (a ResNet-50 whose body driver the RetinaFace detector shares through
// net.h) and the LSTM over windows of its features -- as sequences of the kernels in gemm.hip / fused.hip / kernels.hip, and the
// C entries that run them.  Host code only.
#include "net.h"

// ------------------------------------------------------------------------------------------------ ResNet-50 bodies
// Blocks [b_begin, b_end) of stage li (0-based) of a Trunk (net.h) on nb frames; the last of them writes to `last_out` when given.
//
// Where the stride lives.  A block has one stride s: its conv2 is a 3x3 / stride s convolution and its shortcut is read at the
// same stride (the residual row of the even position, r_sub; the downsample operand, x2_stride).  torchvision, and so the
// detector, puts s on the FIRST block of stages 2-4.  The reference's recognition CNN strides that block's conv1 and downsample
// convolution instead: both 1x1, stride 2, no padding (video.py:12-19,140-149), so of the previous stage's output only the
// positions (2 oy, 2 ox) are ever read.  There (t.stride_last) the LAST block of stages 1-3 is evaluated at those positions alone
// and writes the compact [nb, oh, ow, 4 planes] tensor; the next stage's first block then reads it at stride 1.  Same values at
// every position anyone reads, 9.6 % fewer products per frame (0.74 of 7.67 GFLOP) and a quarter of that block's trunk bytes.
//
// x3 mode fuses the stride-1 blocks of stages 1-3 (fused.hip): in stages 1-2 a bneck_kernel chain computes conv2 -> conv3
// (+ x, or stage 1's 64 -> 256 downsample in registers) -> the next block's conv1; in stage 3 conv2 stays a conv_gemm launch and
// conv3 + residual + the next block's conv1 share bneck_tail2_kernel.  The first fused block of a stage (block 0 of stage 1,
// block 1 otherwise) runs its own conv1.  t.w2_frags: hand the chain the fragment-order conv2 copy, which selects the spatial-tile
// form on 55 x 55 grids.  Debug taps: t.tap + "l1b0_c1" / "l1b0_c2" / "l1b0", + "blk<stage>_<block>" (every block's output),
// + "chain_out:" / "chain_t1n:" / "tail_out:" / "tail_t1n:" + weight prefix (fused launches); `end_tap` after the stage's last block.
void run_bneck_stage(Net& net, Trunk& t, int li, int b_begin, int b_end, int nb, void* last_out, const std::string& end_tap) {
    avcer_ctx* ctx = net.ctx;
    const std::string tap = t.tap;
    const int act = net.act.kind;
    const size_t es = net.act.es;
    const int planes = kStages[li][0], blocks = kStages[li][1];
    const int fused_from = li == 0 ? 0 : 1;
    for (int b = b_begin; b < b_end; ++b) {
        const int s = t.stride_last ? (b == blocks - 1 && li < 3 ? kStages[li + 1][2] : 1) : (b == 0 ? kStages[li][2] : 1);
        const int h = t.h, w = t.w, oh = (h - 1) / s + 1, ow = (w - 1) / s + 1;
        const long M = (long)nb * h * w;
        const std::string p = "l" + std::to_string(li + 1) + "." + std::to_string(b) + ".",
                          pn = "l" + std::to_string(li + 1) + "." + std::to_string(b + 1) + ".";
        void* dst = (b == b_end - 1 && last_out) ? last_out : (t.X == t.pp[0] ? t.pp[1] : t.pp[0]);
        const bool fused = net.x3 && li < 3 && b >= fused_from, chain = fused && li < 2, next = b + 1 < blocks;
        // Work nobody reads: the block in front of the strided last one hands it OUT as the residual, which that block picks at
        // (2 oy, 2 ox) alone -- the fused launch stores those rows only (fused.hip KEEP).  A debug tap promises the whole tensor.
        const int keep = t.stride_last && li < 3 && kStages[li + 1][2] == 2 && b == blocks - 2 && fused && ctx->skip_unread && !ctx->tap_dst ? 2 : 1;
        if (!fused || b == fused_from)
            net.gemm(conv2d_desc(nb, h, w, t.cin, 1, 1, 1, 0, planes, 1), p + "c1.w", net.F(p + "c1.s"), net.F(p + "c1.b"), t.X,
                     nullptr, t.T1, act, act);
        if (chain) {
            const bool first = b == 0;
            const Tensor *w2 = net.T(p + "c2.wf"), *w3 = net.T(first ? p + "c3d.w" : p + "c3.wf"),
                         *w1n = next ? net.T(pn + "c1.wf") : nullptr;
            if (net.err != AVCER_OK) return;
            if (!w2->x3 || !w3->x3 || (next && !w1n->x3)) {
                net.err = set_err(ctx, AVCER_ESTATE, "%s: split chain weights not prepared", p.c_str());
                return;
            }
            net.chk(launch_bneck(ctx, planes, nb, h, w, t.T1, t.X, first ? t.cin : 0, s, dst, next ? t.T2 : nullptr, w2->x3,
                                 net.F(p + "c2.b"), w3->x3, net.F(first ? p + "c3d.b" : p + "c3.b"), next ? w1n->x3 : nullptr,
                                 next ? net.F(pn + "c1.b") : nullptr, net.st, t.w2_frags ? w2->x3f : nullptr, keep));
            if (ctx->tap_dst) {
                net.tap((tap + "chain_out:" + p).c_str(), dst, (size_t)nb * oh * ow * planes * 4 * es);
                if (next) net.tap((tap + "chain_t1n:" + p).c_str(), t.T2, (size_t)M * planes * es);
            }
            std::swap(t.T1, t.T2);  // the next block's T1 was written into T2; T2 holds this block's conv1 output
        } else {
            net.gemm(conv2d_desc(nb, h, w, planes, 3, 3, s, 1, planes, 1), p + "c2.w", net.F(p + "c2.s"), net.F(p + "c2.b"), t.T1,
                     nullptr, t.T2, act, act);
            avcer_conv_desc d3 = conv2d_desc(nb, oh, ow, planes, 1, 1, 1, 0, planes * 4, 1);
            if (fused && next && M <= kTailPairRows) {
                // few positions: the same two contractions (same folded weights, same arithmetic: bit-identical) as two
                // launches of the skinny / tiled forms -- the fused kernel's 128-row blocks leave the chip empty here
                net.gemm(d3, p + "c3.wf", nullptr, net.F(p + "c3.b"), t.T2, t.X, dst, act, act);
                net.gemm(conv2d_desc(nb, h, w, planes * 4, 1, 1, 1, 0, planes, 1), pn + "c1.wf", nullptr, net.F(pn + "c1.b"), dst,
                         nullptr, t.T1, act, act);
            } else if (fused && next) {
                const Tensor *w3 = net.T(p + "c3.wf"), *w1n = net.T(pn + "c1.wf");
                if (net.err != AVCER_OK) return;
                if (!w3->x3 || !w1n->x3) {
                    net.err = set_err(ctx, AVCER_ESTATE, "%s: split tail weights not prepared", p.c_str());
                    return;
                }
                net.chk(launch_bneck_tail(ctx, planes, M, t.T2, t.X, dst, t.T1, w3->x3, net.F(p + "c3.b"), w1n->x3,
                                          net.F(pn + "c1.b"), net.st, keep, h, w));
                if (ctx->tap_dst) {
                    net.tap((tap + "tail_out:" + p).c_str(), dst, (size_t)M * planes * 4 * es);
                    net.tap((tap + "tail_t1n:" + p).c_str(), t.T1, (size_t)M * planes * es);
                }
            } else if (b == 0) {
                // conv3 + downsample fused: K = [T2 (planes) | X at stride s (cin)], BN scales folded into the weights
                d3.x2_cin = t.cin; d3.x2_stride = s;
                d3.x2_stride_b = (int64_t)h * w * t.cin; d3.x2_stride_h = (int64_t)w * t.cin; d3.x2_stride_w = t.cin;
                net.gemm(d3, p + "c3d.w", nullptr, net.F(p + "c3d.b"), t.T2, nullptr, dst, act, act, t.X);
            } else {
                d3.r_sub = s; d3.r_h = h; d3.r_w = w;
                net.gemm(d3, p + "c3.w", net.F(p + "c3.s"), net.F(p + "c3.b"), t.T2, t.X, dst, act, act);
            }
        }
        t.X = dst;
        t.h = oh;
        t.w = ow;
        t.cin = planes * 4;
        const size_t out_bytes = (size_t)nb * oh * ow * t.cin * es;
        if (li == 0 && b == 0) {
            net.tap((tap + "l1b0_c1").c_str(), chain ? t.T2 : t.T1, (size_t)nb * oh * ow * planes * es);
            if (!chain) net.tap((tap + "l1b0_c2").c_str(), t.T2, (size_t)nb * oh * ow * planes * es);
            net.tap((tap + "l1b0").c_str(), t.X, out_bytes);
        }
        if (ctx->tap_dst) net.tap((tap + "blk" + std::to_string(li + 1) + "_" + std::to_string(b)).c_str(), t.X, out_bytes);
    }
    if (b_end == blocks) net.tap(end_tap.c_str(), t.X, (size_t)nb * t.h * t.w * t.cin * es);
}

// ------------------------------------------------------------------------------------------------ static CNN
// ref: architectures/video.py:93-166 (ResNet-50, stride on the first 1x1 of a bottleneck, BN eps 1e-3 folded into
// per-channel scale/bias by avcer_amd/packing.py), data/utils.py:19-39, get_prob_video.py:47-49,103-112.
// One LANE of the static CNN: `n` frames on stream `st`, activations in workspace slot `slot`.  Arguments validated and the
// mode's weight copies prepared by static_forward_impl below.
static int static_forward_lane(avcer_ctx* ctx, int slot, const uint8_t* frames, const float* nchw, int n, int in_h, int in_w, int mode,
                               float* logits, float* probs, float* feats, float* cam, hipStream_t st) {
    Net net{ctx, ctx->stat, mode_storage(mode), st};
    const int act = net.act.kind, bf = act == KIND_BF16;
    const size_t es = net.act.es;
    // Two granularities.  The FRONT (stem, stage 1, first block of stage 2: the 55x55 tensors) runs in passes of NB <= 1024
    // frames, the 4 GiB range of a buffer descriptor at 4 bytes per element.  The BACK (rest of stage 2, stages 3-4, tail)
    // runs once over NS = up to two front passes: its grids are small (stage 4: 1568 tiles per 1024 frames on 512 block
    // slots), and twice the rows per launch means a smaller last partial round (a tail of 0.06 rounds costs a whole one).
    const int NB = std::min(n, ctx->static_batch);
    const int NS = std::min(n, ctx->static_back > 0 ? ctx->static_back : 2 * NB);
    const size_t back_elems = (size_t)NS * 28 * 28 * 512;  // largest activation of the back (stage 2)
    if (back_elems * es >= 0xF0000000ull) return set_err(ctx, AVCER_EINVAL, "static_forward: %d frames per back pass", NS);
    const int kCamChunk = 256;
    const int hk = net.x3 ? KIND_SP32 : KIND_F32;  // fc1's operand: sp32 pairs in the x3 mode, f32 in the other two
    void *P, *buf[4], *bbuf[4];
    Pair pooled;
    float *feat_ws, *cam_g = nullptr;
    TRY(ws_carve(ctx, slot, "static", [&](Arena& ar) {
        P = ar.get((size_t)NB * 230 * 230 * 4 * es);
        for (auto& b : buf) b = ar.get((size_t)NB * 112 * 112 * 64 * es);  // largest activation of the front (stem output)
        for (auto& b : bbuf) b = ar.get(back_elems * es);
        pooled = carve_pair(ar, (size_t)NS * 2048 * 4, (size_t)NS * 2048 * 4, hk);
        feat_ws = ar.get<float>((size_t)NS * 512 * 4);
        // Grad-CAM (avcer_static_forward_cam): the per-class channel weights g of up to kCamChunk frames at a time, behind the rest
        if (cam) cam_g = ar.get<float>((size_t)std::min(NS, kCamChunk) * 7 * 2048 * 4);
    }));
    // stem + max-pool of `nb` frames starting at frame f0 of the call: -> B[1] (55x55x64), B[0] is scratch
    auto run_stem = [&](int f0, int nb, void** B) {
        if (net.x3) {
            // x3 mode: ONE kernel for conv 7x7/2 + BN + ReLU + max-pool 3x3/2 (fused.hip).  From u8 frames it also does the
            // preprocessing (raw pixels are exact in fp16: two MFMAs per product, the mean lives in the shift table stem.b9);
            // the preprocessed-tensor entry point carries arbitrary floats and goes through the planar fp16 hi / lo image.
            const Tensor* w = net.T("stem7.w");
            if (net.err != AVCER_OK) return;
            if (!w->x3) { net.err = set_err(ctx, AVCER_ESTATE, "stem7.w: split weights not prepared"); return; }
            if (frames) {
                net.chk(launch_stem_pool_u8(ctx, frames + (size_t)f0 * in_h * in_w * 3, in_h, in_w, w->x3, net.F("stem.s"),
                                            net.F("stem.b9"), B[1], nb, st));
                net.tap("stem", B[1], (size_t)nb * 55 * 55 * 64 * es);
                return;
            }
            net.chk(k_pack_nchw(ctx, nchw + (size_t)f0 * 3 * 224 * 224, nb, P, 3, st));
            net.chk(launch_stem_pool(ctx, P, (size_t)nb * 230 * 230 * 4 * 2, w->x3, net.F("stem.s"), net.F("stem.b"), B[1], nb, st));
            net.tap("stem", B[1], (size_t)nb * 55 * 55 * 64 * es);
            return;
        }
        if (frames) net.chk(k_preprocess(ctx, frames + (size_t)f0 * in_h * in_w * 3, nb, in_h, in_w, P, bf, st));
        else net.chk(k_pack_nchw(ctx, nchw + (size_t)f0 * 3 * 224 * 224, nb, P, bf, st));
        net.gemm(stem_desc(nb, 230, 230), "stem.w", net.F("stem.s"), net.F("stem.b"), P, nullptr, B[0], bf, act);  // P is f32 unless bf16
        net.tap("pre", P, (size_t)nb * 230 * 230 * 4 * es);
        net.tap("stem_conv", B[0], (size_t)nb * 112 * 112 * 64 * es);
        net.chk(k_maxpool(ctx, B[0], B[1], nb, 112, 112, 64, 3, 0, 55, 55, act, st));
        net.tap("stem", B[1], (size_t)nb * 55 * 55 * 64 * es);
    };
    for (int s0 = 0; s0 < n; s0 += NS) {
        const int nb = std::min(NS, n - s0);
        for (int c0 = 0; c0 < nb; c0 += NB) {  // front passes: stem, stage 1, first block of stage 2 -> bbuf[0]
            const int cn = std::min(NB, nb - c0);
            // the stride on the last block of a stage, the fragment-order conv2 copy for the chain, taps without a prefix
            Trunk t{buf[1], {buf[0], buf[1]}, buf[2], buf[3], 55, 55, 64, true, true, ""};
            run_stem(s0 + c0, cn, buf);
            run_bneck_stage(net, t, 0, 0, kStages[0][1], cn, nullptr, "layer1");
            run_bneck_stage(net, t, 1, 0, 1, cn, (char*)bbuf[0] + (size_t)c0 * 28 * 28 * 512 * es, "layer2");
        }
        Trunk t{bbuf[0], {bbuf[1], bbuf[0]}, bbuf[2], bbuf[3], 28, 28, 512, true, true, ""};
        for (int li = 1; li < 4; ++li)
            run_bneck_stage(net, t, li, li == 1 ? 1 : 0, kStages[li][1], nb, nullptr, "layer" + std::to_string(li + 1));
        // x3 mode: the pooled features once more as sp32 pairs, fc1's operand (the split fc1 did on the fly before)
        net.chk(k_avgpool_hw(ctx, t.X, pooled.f, pooled.op, nb, t.h * t.w, 2048, act, st));
        net.tap("avgpool", pooled.f, (size_t)nb * 2048 * 4);
        float* fo = feats ? feats + (size_t)s0 * 512 : feat_ws;
        {
            // fc1 in the mode's own arithmetic.  Rounds 2-3 ran it on the f32 MFMA in the x3 mode as well, because a bf16-pair
            // fc1 put 40 % on top of the pooled features' error; the fp16-pair contraction carries 7e-8 and costs a quarter
            // of the time of the f32 MFMA on this launch-latency-bound layer (16 tiles at batch 256: 114 -> ~30 us).
            avcer_conv_desc fd = linear_desc(nb, 2048, 512, 0);
            fd.tile_n = 64;  // 128 x 64 tiles: twice the blocks of a grid that does not fill the chip anyway
            net.gemm(fd, "fc1.w", nullptr, net.F("fc1.b"), operand(pooled, hk), nullptr, fo, KIND_F32);
        }
        if (logits || probs)
            net.chk(k_small_linear(ctx, fo, net.F("fc2.w"), net.F("fc2.b"), logits ? logits + (size_t)s0 * 7 : nullptr,
                                   probs ? probs + (size_t)s0 * 7 : nullptr, nb, 512, 7, 1, st));
        // Grad-CAM of every class from layer 4's output t.X (still in the workspace), fc1's pre-ReLU output and the probabilities
        for (int m0 = 0; cam && m0 < nb && net.err == AVCER_OK; m0 += kCamChunk) {
            const int mn = std::min(kCamChunk, nb - m0);
            net.chk(k_cam_maps(ctx, (const char*)t.X + (size_t)m0 * 49 * 2048 * es, probs + (size_t)(s0 + m0) * 7, fo + (size_t)m0 * 512,
                               net.F("fc1.w"), net.F("fc2.w"), cam_g, cam + (size_t)(s0 + m0) * 343, mn, act, st));
        }
        if (net.err != AVCER_OK) return net.err;
    }
    return net.err;
}

// Calls of 32-2048 frames (avcer_set_static_lane_range) run as TWO lanes: the halves of the batch on two HIP streams with a workspace
// each.  At those sizes the grids of stages 3-4 are a fraction of one round of block slots (256 frames: 448 tiles of 112 rows on 256
// CUs, the fullest CU holds 224 rows, the average 196) and no tile height removes that quantisation; two independent half-launches
// let the tail of one overlap the head of the other: -4 % at 32 frames, -8 ... -12 % at 48-192, -5 % at 256-512, -2 ... -3 % at 640-1536,
// -1.7 % at 2048 (tools/two_lane_sweep.py, profiles/r06_two_lane_sweep.txt; the full AV step, whose audio branch already runs beside
// the static CNN on its own stream, is unchanged by it).  A frame's result does not depend on the batch around it
// (tests/test_gpu_visual.py::test_static_batch_invariance_256), so the split never shows in a result.  Below 16 frames the launches
// are latency chains (the skinny forms) and halving them costs (+4 % at 8 frames).  SERIAL (one lane) whenever per-launch events
// are being recorded (avcer_profile_enable: overlapping kernels make event durations meaningless), a debug tap is armed, or
// avcer_set_static_lanes(ctx, 1) says so.
static int static_forward_impl(avcer_ctx* ctx, const uint8_t* frames, const float* nchw, int n, int in_h, int in_w, int mode,
                               float* logits, float* probs, float* feats, float* cam, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (!ctx->stat.loaded) return set_err(ctx, AVCER_ESTATE, "static weights not loaded");
    if ((!frames && !nchw) || n <= 0 || in_h <= 0 || in_w <= 0) return set_err(ctx, AVCER_EINVAL, "static_forward: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    TRY(begin_forward(ctx, "static_forward", ctx->stat, mode, true, st));
    const bool two = ctx->static_lanes >= 2 && n >= ctx->lane_min && n <= ctx->lane_max && !ctx->prof && !ctx->tap_dst;
    if (!two) return static_forward_lane(ctx, WS_STATIC, frames, nchw, n, in_h, in_w, mode, logits, probs, feats, cam, st);
    const int n0 = (n + 1) / 2;
    const size_t fstep = frames ? (size_t)in_h * in_w * 3 : 0;
    return run_two_lanes(ctx, st, [&](int lane, hipStream_t s) {
        const size_t f0 = lane ? n0 : 0;
        return static_forward_lane(ctx, lane ? WS_STATIC_LANE1 : WS_STATIC, frames ? frames + f0 * fstep : nullptr,
                                   nchw ? nchw + f0 * 3 * 224 * 224 : nullptr, lane ? n - n0 : n0, in_h, in_w, mode,
                                   logits ? logits + f0 * 7 : nullptr, probs ? probs + f0 * 7 : nullptr, feats ? feats + f0 * 512 : nullptr,
                                   cam ? cam + f0 * 343 : nullptr, s);
    });
}

extern "C" int avcer_static_forward(avcer_ctx* ctx, const uint8_t* frames, int n, int in_h, int in_w, int mode,
                                    float* logits, float* probs, float* feats, avcer_stream_t stream) {
    if (!frames) return ctx ? set_err(ctx, AVCER_EINVAL, "static_forward: null frames") : AVCER_EINVAL;
    return static_forward_impl(ctx, frames, nullptr, n, in_h, in_w, mode, logits, probs, feats, nullptr, stream);
}

extern "C" int avcer_static_forward_cam(avcer_ctx* ctx, const uint8_t* frames, int n, int in_h, int in_w, int mode,
                                        float* logits, float* probs, float* feats, float* cam, avcer_stream_t stream) {
    if (!frames || !probs || !cam)
        return ctx ? set_err(ctx, AVCER_EINVAL, "static_forward_cam: null frames, probs or cam") : AVCER_EINVAL;
    return static_forward_impl(ctx, frames, nullptr, n, in_h, in_w, mode, logits, probs, feats, cam, stream);
}

extern "C" int avcer_static_forward_nchw(avcer_ctx* ctx, const float* x, int n, int mode, float* logits, float* probs,
                                         float* feats, avcer_stream_t stream) {
    if (!x) return ctx ? set_err(ctx, AVCER_EINVAL, "static_forward_nchw: null input") : AVCER_EINVAL;
    return static_forward_impl(ctx, nullptr, x, n, 224, 224, mode, logits, probs, feats, nullptr, stream);
}

// ------------------------------------------------------------------------------------------------ dynamic LSTM
// ref: architectures/video.py:169-185.  Input projections of all 10 steps are one GEMM per layer; the recurrent
// part is one [n,H]x[H,4H] GEMM + one cell kernel per step (h_0 = c_0 = 0, so step 0 needs no GEMM).
constexpr int kSteps = 10;
// One layer of hidden size H on n windows: xp = its input projections [n, kSteps, 4H], hp = scratch of the recurrent projection,
// c = the cell state.  Step t writes h_t, as f32 and (x3 mode) as sp32 pairs, `h_step` elements behind h_{t-1} in rows `h_ld`
// apart: H and kSteps * H in an [n, kSteps, H] buffer that keeps the sequence, 0 and H where every step overwrites one [n, H] row.
static void lstm_layer(Net& net, const std::string& p, int H, const float* xp, float* hp, float* c, Pair h, int64_t h_ld, size_t h_step, int n) {
    avcer_conv_desc d = linear_desc(n, H, 4 * H, 0);
    d.x_stride_b = h_ld;  // rows of h_{t-1} inside the [n, kSteps, H] sequence buffer (H, linear_desc's own, where there is none)
    constexpr size_t sp32_bytes = 4;  // per element of h's operand half
    for (int t = 0; t < kSteps; ++t) {
        const Pair ht = advance(h, t * h_step, sp32_bytes);
        if (t > 0) net.gemm(d, p + ".whh.w", nullptr, nullptr, operand(advance(h, (t - 1) * h_step, sp32_bytes), net.act.kind), nullptr, hp, KIND_F32);
        net.chk(k_lstm_cell(net.ctx, xp + (size_t)t * 4 * H, (int64_t)kSteps * 4 * H, hp, c, ht.f, ht.op, h_ld, n, H, t == 0, net.st));
    }
}

extern "C" int avcer_dynamic_forward_mode(avcer_ctx* ctx, const float* windows, int n, int mode, float* logits, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (!ctx->dyn.loaded) return set_err(ctx, AVCER_ESTATE, "dynamic weights not loaded");
    if (!windows || !logits || n <= 0) return set_err(ctx, AVCER_EINVAL, "dynamic_forward: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    // the recurrence keeps f32 state in every mode; AVCER_MODE_F16X3 runs its ten dependent GEMMs per layer on the
    // split-fp16 MFMA (a 128-row tile of the f32 MFMA costs 5x the cycles, and these launches are pure latency);
    // the bf16 mode runs as f32
    TRY(begin_forward(ctx, "dynamic_forward", ctx->dyn, mode, false, st));
    Net net{ctx, ctx->dyn, mode_storage(mode == AVCER_MODE_F16X3 ? mode : AVCER_MODE_FP32), st};
    const int rk = net.act.kind;  // the pass's one operand kind: what reads h reads sp32 pairs in the x3 mode, f32 otherwise
    constexpr int T = kSteps, I = 512, H1 = 512, H2 = 256;
    float *xp1, *hp, *c1, *xp2, *c2;
    Pair h1, h2;
    TRY(ws_carve(ctx, WS_DYNAMIC, "dynamic", [&](Arena& ar) {
        xp1 = ar.get<float>((size_t)n * T * 4 * H1 * 4);
        hp = ar.get<float>((size_t)n * 4 * H1 * 4);
        h1.f = ar.get<float>((size_t)n * T * H1 * 4);
        c1 = ar.get<float>((size_t)n * H1 * 4);
        xp2 = ar.get<float>((size_t)n * T * 4 * H2 * 4);
        h2.f = ar.get<float>((size_t)n * H2 * 4);
        c2 = ar.get<float>((size_t)n * H2 * 4);
        // x3 mode: h of both layers once more as sp32 pairs, written by the cell kernel -- the operand of the next step's recurrent
        // contraction (and of layer 2's input projection), which then runs on the sp32 forms: at a window or a few hundred per call
        // that is the skinny one (9 us a step where the 128-row tile of the f32-operand form took 22)
        h1.op = carve_op(ar, (size_t)n * T * H1 * 4, rk);
        h2.op = carve_op(ar, (size_t)n * H2 * 4, rk);
    }));
    net.gemm(linear_desc((long)n * T, I, 4 * H1, 0), "lstm1.wih.w", nullptr, net.F("lstm1.b"), windows, nullptr, xp1, KIND_F32, KIND_F32);
    lstm_layer(net, "lstm1", H1, xp1, hp, c1, h1, (int64_t)T * H1, H1, n);  // the sequence is kept: layer 2's input
    net.tap("lstm_h1", h1.f, (size_t)n * T * H1 * 4);
    net.gemm(linear_desc((long)n * T, H1, 4 * H2, 0), "lstm2.wih.w", nullptr, net.F("lstm2.b"), operand(h1, rk), nullptr, xp2, KIND_F32);
    lstm_layer(net, "lstm2", H2, xp2, hp, c2, h2, H2, 0, n);  // only the last step is read
    net.tap("lstm_h2", h2.f, (size_t)n * H2 * 4);
    net.chk(k_small_linear(ctx, h2.f, net.F("fc.w"), net.F("fc.b"), logits, nullptr, n, H2, 7, 0, st));
    return net.err;
}

extern "C" int avcer_dynamic_forward(avcer_ctx* ctx, const float* windows, int n, float* logits, avcer_stream_t stream) {
    return avcer_dynamic_forward_mode(ctx, windows, n, AVCER_MODE_FP32, logits, stream);
}
