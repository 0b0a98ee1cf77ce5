// The three face detectors of libavcer_hip.so -- RetinaFace on a ResNet-50 body, RetinaFace on MobileNet-0.25, S3FD -- as
// sequences of the kernels in gemm.hip / fused.hip / kernels.hip / mnet.hip / s3fd.hip, and the C entries that load and run them.
// Host code only.
#include "net.h"

namespace {

// The detector's extents for H x W frames
struct FaceGeom {
    // extents behind conv1 7x7/2 (padding 3), of the zero-bordered image the 8x(8x4)-tap stem reads, behind max-pool 3x3/2 (padding 1)
    int OH, OW, PH, PW, MH, MW;
    int fh[5], fw[5];      // output extent of layer1..4 (index 1..4)
    int priors;            // two per position of layer2..4
    int max_frames;        // per pass: every gathered operand must stay below the 4 GiB buffer-descriptor range
};
FaceGeom face_geom(int H, int W) {
    FaceGeom g{};
    g.OH = (H - 1) / 2 + 1; g.OW = (W - 1) / 2 + 1;
    g.PH = 2 * (g.OH - 1) + 8; g.PW = 2 * (g.OW - 1) + 8;
    g.MH = (g.OH - 1) / 2 + 1; g.MW = (g.OW - 1) / 2 + 1;
    g.fh[1] = g.MH; g.fw[1] = g.MW;
    for (int li = 2; li <= 4; ++li) { g.fh[li] = (g.fh[li - 1] - 1) / 2 + 1; g.fw[li] = (g.fw[li - 1] - 1) / 2 + 1; }
    g.priors = 2 * (g.fh[2] * g.fw[2] + g.fh[3] * g.fw[3] + g.fh[4] * g.fw[4]);
    const size_t per_frame = std::max({(size_t)g.PH * g.PW * 4, (size_t)g.OH * g.OW * 64, (size_t)g.MH * g.MW * 256}) * 4;
    g.max_frames = (int)std::max<size_t>(1, (size_t)0xF0000000u / per_frame);
    return g;
}

// ------------------------------------------------------------------------------------------------ the RetinaFace neck
// FPN, SSH and the heads (retina_face_net.py:42-101, retina_face.py:101-113) are ONE sequence for both RetinaFace kinds, at two
// widths: C = 256 channels, ReLU and 64 head columns (32 + 32 padding) behind the ResNet-50 body, C = 64, LeakyReLU(0.1) and 32
// columns behind MobileNet-0.25.  How a convolution is issued differs too and stays with the lane (run_neck's two callables).
struct Neck {
    int C, hd_ld, act, fc[3];  // width, columns of a head row, activation code of the conv_bn layers (1 / 4), the body's channels
    void *feat[3], *pyr[3], *m1, *m2, *S, *t51, *t72;  // body outputs and FPN laterals, finest first; merged levels 1 and 2; SSH output and branches
    float* hd;                                         // a level's head rows
    // The buffers of passes of NB frames at `es` bytes per element.  own_m2 = false: the lane has a free buffer for m2
    void carve(Arena& ar, int NB, const int* fh, const int* fw, size_t es, bool own_m2) {
        const size_t lvl = (size_t)NB * fh[2] * fw[2];  // positions of the finest pyramid level
        for (int i = 0; i < 3; ++i) feat[i] = ar.get((size_t)NB * fh[i + 2] * fw[i + 2] * fc[i] * es);
        for (int i = 0; i < 3; ++i) pyr[i] = ar.get((size_t)NB * fh[i + 2] * fw[i + 2] * C * es);
        m1 = ar.get(lvl * C * es);
        if (own_m2) m2 = ar.get((size_t)NB * fh[3] * fw[3] * C * es);
        S = ar.get(lvl * C * es);
        t51 = ar.get(lvl * (C / 4) * es);
        t72 = ar.get(lvl * (C / 4) * es);
        hd = ar.get<float>(lvl * hd_ld * 4);
    }
};

// One pass of `nb` frames from the body's three outputs k.feat[i] (k.fc[i] channels on fh[i + 2] x fw[i + 2] positions, storage
// net.act) to the pass's rows of loc / conf / landms.  conv(ks, prefix, x, h, w, cin, cout, y, y_ld, y_coff, act) issues one
// ks x ks convolution with the weights named `prefix`, head(prefix, h, w) the head contraction S -> hd of one level.
// Debug taps: face_lat1..3 (the laterals, before the top-down adds overwrite levels 1 and 2), face_sum2 (merge2's input),
// face_fpn1..3 (the pyramid: the two merges and level 3's lateral, which no merge follows), face_ssh1.
template <class Conv, class Head>
void run_neck(Net& net, const Neck& k, int nb, const FaceGeom& g, float* loc, float* conf, float* landms, const Conv& conv, const Head& head) {
    avcer_ctx* ctx = net.ctx;
    const int C = k.C, kind = net.act.kind, *fh = g.fh, *fw = g.fw;
    auto tap = [&](const char* name, const void* x, int li) { net.tap(name, x, (size_t)nb * fh[li] * fw[li] * C * net.act.es); };
    // FPN (retina_face_net.py:87-101): laterals, then top-down nearest-upsample + add + 3x3 merge
    for (int i = 0; i < 3; ++i)
        conv(1, "fpn.o" + std::to_string(i + 1) + ".", k.feat[i], fh[i + 2], fw[i + 2], k.fc[i], C, k.pyr[i], C, 0, k.act);
    for (int i = 0; i < 3 && ctx->tap_dst; ++i) tap(("face_lat" + std::to_string(i + 1)).c_str(), k.pyr[i], i + 2);
    tap("face_fpn3", k.pyr[2], 4);
    net.chk(k_upsample_add(ctx, k.pyr[1], k.pyr[2], nb, fh[3], fw[3], fh[4], fw[4], C, kind, net.st));
    tap("face_sum2", k.pyr[1], 3);
    conv(3, "fpn.m2.", k.pyr[1], fh[3], fw[3], C, C, k.m2, C, 0, k.act);
    tap("face_fpn2", k.m2, 3);
    net.chk(k_upsample_add(ctx, k.pyr[0], k.m2, nb, fh[2], fw[2], fh[3], fw[3], C, kind, net.st));
    conv(3, "fpn.m1.", k.pyr[0], fh[2], fw[2], C, C, k.m1, C, 0, k.act);
    tap("face_fpn1", k.m1, 2);
    // SSH + heads per level (retina_face_net.py:59-73, retina_face.py:101-113): relu(cat(...)) = per-branch ReLU
    void* const lvl_in[3] = {k.m1, k.m2, k.pyr[2]};
    int row0 = 0;
    for (int i = 0; i < 3; ++i) {
        const int hh = fh[i + 2], ww = fw[i + 2];
        const std::string p = "ssh" + std::to_string(i + 1) + ".";
        conv(3, p + "c3.", lvl_in[i], hh, ww, C, C / 2, k.S, C, 0, 1);
        conv(3, p + "c51.", lvl_in[i], hh, ww, C, C / 4, k.t51, C / 4, 0, k.act);
        conv(3, p + "c52.", k.t51, hh, ww, C / 4, C / 4, k.S, C, C / 2, 1);
        conv(3, p + "c72.", k.t51, hh, ww, C / 4, C / 4, k.t72, C / 4, 0, k.act);
        conv(3, p + "c73.", k.t72, hh, ww, C / 4, C / 4, k.S, C, 3 * C / 4, 1);
        if (i == 0) tap("face_ssh1", k.S, 2);
        head("head" + std::to_string(i) + ".", hh, ww);
        net.chk(k_face_head(ctx, k.hd, k.hd_ld, nb, hh * ww, row0, g.priors, loc, conf, landms, net.st));
        row0 += hh * ww * 2;
    }
}

// ------------------------------------------------------------------------------------------------ RetinaFace-R50 (row f4)
// ref: data/face_detection/ibug/face_detection/retina_face/retina_face.py:46-115 (RetinaFace, test phase),
// retina_face_net.py:42-101 (SSH, FPN), torchvision ResNet-50 as the body (children conv1..layer4, return_layers
// layer2/3/4), retina_face_predictor.py:59-65 (mean subtraction).  Inference BatchNorm (eps 1e-5) is folded by
// avcer_amd/packing.py; the three 1x1 heads of a pyramid level are one GEMM with 32 (+32 padding) output channels.
// One LANE of the detector: `n` frames on stream `st`, activations in workspace slot `slot`, passes of at most `nb_cap` frames.
int face_forward_lane(avcer_ctx* ctx, int slot, int nb_cap, const uint8_t* frames, int n, int H, int W, int rgb, int mode, float* loc,
                      float* conf, float* landms, hipStream_t st) {
    Net net{ctx, ctx->face, mode_storage(mode), st};
    const int act = net.act.kind, bf = act == KIND_BF16;
    const size_t es = net.act.es;
    const FaceGeom g = face_geom(H, W);
    const int OH = g.OH, OW = g.OW, PH = g.PH, PW = g.PW, MH = g.MH, MW = g.MW, P = g.priors, *fh = g.fh, *fw = g.fw;
    const int NB = std::min({n, nb_cap, g.max_frames});
    // the largest activation: the stem output or layer1's output (equal for even extents, the latter larger for odd ones)
    const size_t big = (size_t)NB * std::max((size_t)OH * OW * 64, (size_t)MH * MW * 256);
    void *Pimg, *buf[4];
    Neck neck{256, 64, 1, {kStages[1][0] * 4, kStages[2][0] * 4, kStages[3][0] * 4}};
    TRY(ws_carve(ctx, slot, "face", [&](Arena& ar) {
        Pimg = ar.get((size_t)NB * PH * PW * 4 * es);
        for (auto& b : buf) b = ar.get(big * es);
        neck.carve(ar, NB, fh, fw, es, false);
    }));

    for (int s0 = 0; s0 < n; s0 += NB) {
        const int nb = std::min(NB, n - s0);
        if (net.x3) {
            // x3 mode (round 6): pixel - mean (integer means: exact in fp16), conv 7x7/2, BN, ReLU and the 3x3/2 max-pool in ONE launch
            // straight from the u8 frames (fused.hip stem_pool_u8_kernel<true>): no padded f32 image, no [n,180,320,64] stem map
            const Tensor* w7 = net.T("stem7.w");
            if (net.err != AVCER_OK) return net.err;
            if (!w7->x3) return set_err(ctx, AVCER_ESTATE, "face stem7.w: split weights not prepared");
            net.chk(launch_stem_pool_face(ctx, frames + (size_t)s0 * H * W * 3, H, W, rgb, w7->x3, net.F("stem.s"), net.F("stem.b"), buf[1],
                                          nb, st));
        } else {
            net.chk(k_face_pre(ctx, frames + (size_t)s0 * H * W * 3, nb, H, W, PH, PW, rgb, Pimg, bf, st));
            net.gemm(stem_desc(nb, PH, PW), "stem.w", net.F("stem.s"), net.F("stem.b"), Pimg, nullptr, buf[0], bf, act);
            net.tap("face_stem_conv", buf[0], (size_t)nb * OH * OW * 64 * es);
            net.chk(k_maxpool(ctx, buf[0], buf[1], nb, OH, OW, 64, 3, 1, MH, MW, act, st));
        }
        net.tap("face_pool", buf[1], (size_t)nb * MH * MW * 64 * es);
        // torchvision's stride on the first block of a stage; no fragment-order conv2 copy: a 217-220-pixel frame reaches 55 x 55 in
        // stage 1, where the copy would select the spatial-tile chain form, which was never measured on this body
        Trunk t{buf[1], {buf[0], buf[1]}, buf[2], buf[3], MH, MW, 64, false, false, "face_"};
        for (int li = 0; li < 4; ++li)  // stages 2-4 keep their outputs for the pyramid
            run_bneck_stage(net, t, li, 0, kStages[li][1], nb, li ? neck.feat[li - 1] : nullptr,
                            li ? "face_body" + std::to_string(li) : "face_layer1");
        if (net.err != AVCER_OK) return net.err;
        neck.m2 = t.T1;  // the ping-pong buffers of the body are free again
        // every contraction of the neck is net.gemm on the `*.w` weights, read and written in the mode's storage
        auto conv = [&](int ks, const std::string& p, const void* x, int hh, int ww, int cin, int cout, void* y, int y_ld, int y_coff, int relu) {
            avcer_conv_desc d = conv2d_desc(nb, hh, ww, cin, ks, ks, 1, ks / 2, cout, relu);
            d.y_ld = y_ld; d.y_coff = y_coff;
            net.gemm(d, p + "w", net.F(p + "s"), net.F(p + "b"), x, nullptr, y, act, act);
        };
        auto head = [&](const std::string& hp, int hh, int ww) {
            net.gemm(linear_desc((long)nb * hh * ww, 256, 64, 0), hp + "w", nullptr, net.F(hp + "b"), neck.S, nullptr, neck.hd, act, KIND_F32);
        };
        run_neck(net, neck, nb, g, loc + (size_t)s0 * P * 4, conf + (size_t)s0 * P * 2, landms + (size_t)s0 * P * 10, conv, head);
        if (net.err != AVCER_OK) return net.err;
    }
    return net.err;
}

// ------------------------------------------------------------------------------------------------ RetinaFace-MobileNet-0.25
// ref: retina_face.py:46-115 with cfg_mnet (config.py:3-20): MobileNetV1 body (retina_face_net.py:103-125, return_layers stage1/2/3 =
// 64 / 128 / 256 channels at strides 8 / 16 / 32), FPN and SSH at 64 channels with LeakyReLU(0.1), the same heads.  Kernels: mnet.hip.
// Every activation is NHWC f32 in both supported modes (AVCER_MODE_FP32, AVCER_MODE_F16X3); the priors, and with them decode, NMS and
// the tracker, are those of the R50 variant (same min_sizes / steps, same ceil(h/8), ceil(h/16), ceil(h/32) extents).
constexpr int kMnetBlocks[13][3] = {{8, 16, 1}, {16, 32, 2}, {32, 32, 1}, {32, 64, 2}, {64, 64, 1}, {64, 128, 2}, {128, 128, 1},
                                    {128, 128, 1}, {128, 128, 1}, {128, 128, 1}, {128, 128, 1}, {128, 256, 2}, {256, 256, 1}};
// frames per pass of the mnet lane: the two ping-pong buffers of the largest activation (block 1's output, 16 channels at half
// resolution) stay below 1.5 GiB each, and a launch's grid carries the frame in its y dimension
int face_mnet_max_frames(const FaceGeom& g) {
    return (int)std::max<size_t>(1, std::min<size_t>(65535, (size_t)0x60000000u / ((size_t)g.OH * g.OW * 16 * 4)));
}

int face_mnet_forward_lane(avcer_ctx* ctx, int slot, int nb_cap, const uint8_t* frames, int n, int H, int W, int rgb, int mode,
                           float* loc, float* conf, float* landms, hipStream_t st) {
    Net net{ctx, ctx->face, Storage{KIND_F32, 4}, st};
    const int x3 = mode == AVCER_MODE_F16X3;
    const FaceGeom g = face_geom(H, W);
    const int P = g.priors, *fh = g.fh, *fw = g.fw;
    const int NB = std::min({n, nb_cap, face_mnet_max_frames(g)});
    float* buf[2];
    Neck neck{64, 32, 4, {64, 128, 256}};
    TRY(ws_carve(ctx, slot, "face (mobilenet0.25)", [&](Arena& ar) {
        for (auto& b : buf) b = ar.get<float>((size_t)NB * g.OH * g.OW * 16 * 4);
        neck.carve(ar, NB, fh, fw, 4, true);
    }));
    for (int s0 = 0; s0 < n; s0 += NB) {
        const int nb = std::min(NB, n - s0);
        net.chk(launch_mnet_stem(ctx, frames + (size_t)s0 * H * W * 3, nb, H, W, rgb, net.F("stem.wt"), net.F("stem.s"), net.F("stem.b"), buf[0], st));
        // the thirteen conv_dw blocks; blocks 5, 11 and 13 end stages 1-3 and write the pyramid's inputs
        const float* X = buf[0];
        int h = g.OH, w = g.OW, pp = 1;
        for (int i = 0; i < 13 && net.err == AVCER_OK; ++i) {
            const int cin = kMnetBlocks[i][0], cout = kMnetBlocks[i][1], s = kMnetBlocks[i][2];
            const std::string p = "b" + std::to_string(i + 1) + ".";
            const Tensor* pw = net.T(p + "pw.w");
            if (net.err != AVCER_OK) break;
            if (x3 && !pw->x3) return set_err(ctx, AVCER_ESTATE, "face %spw.w: split weights not prepared", p.c_str());
            float* Y = i == 4 ? (float*)neck.feat[0] : i == 10 ? (float*)neck.feat[1] : i == 12 ? (float*)neck.feat[2] : buf[pp];
            net.chk(launch_dwsep(ctx, cin, cout, s, x3, X, net.F(p + "dw.w"), net.F(p + "dw.s"), net.F(p + "dw.b"),
                                 x3 ? (const void*)pw->x3 : (const void*)pw->f32, net.F(p + "pw.s"), net.F(p + "pw.b"), Y, nb, h, w, st));
            h = (h - 1) / s + 1; w = (w - 1) / s + 1;
            if (Y == buf[pp]) pp ^= 1;
            X = Y;
        }
        if (net.err != AVCER_OK) return net.err;
        for (int i = 0; i < 3; ++i)
            net.tap(("face_body" + std::to_string(i + 1)).c_str(), neck.feat[i], (size_t)nb * fh[i + 2] * fw[i + 2] * neck.fc[i] * 4);
        // every convolution of the neck is the direct kernel of mnet.hip on the `*.wt` weights, f32 in both modes
        auto conv = [&](int ks, const std::string& p, const void* x, int hh, int ww, int cin, int cout, void* y, int y_ld, int y_coff, int act) {
            net.chk(launch_mnet_conv(ctx, ks, (const float*)x, net.F(p + "wt"), net.F(p + "s"), net.F(p + "b"), (float*)y, nb, hh, ww, cin, cout, y_ld, y_coff, act, st));
        };
        auto head = [&](const std::string& hp, int hh, int ww) {
            net.chk(launch_mnet_conv(ctx, 1, (const float*)neck.S, net.F(hp + "wt"), nullptr, net.F(hp + "b"), neck.hd, nb, hh, ww, 64, 32, 32, 0, 0, st));
        };
        run_neck(net, neck, nb, g, loc + (size_t)s0 * P * 4, conf + (size_t)s0 * P * 2, landms + (size_t)s0 * P * 10, conv, head);
        if (net.err != AVCER_OK) return net.err;
    }
    return net.err;
}

// ------------------------------------------------------------------------------------------------ S3FD
// ref: s3fd/s3fd_net.py:28-171.  A VGG-16 trunk at full frame resolution (13 convolutions 3x3, five 2x2 max-pools, the third with
// ceil_mode), fc6 (3x3, dilation 6) and fc7 (1x1) at 1024 channels, four extras, six head levels with ONE anchor per position; the
// first three levels are L2-normalised (folded into the heads: packing.pack_face_s3fd, csrc/s3fd.hip).  No BatchNorm: every
// contraction runs with scale 1 and the convolution's own bias.  Activations are in the mode's storage (f32 / sp32); every
// contraction from conv1_2 on is net.gemm, so the x3 range contract counts at their epilogues.
struct S3fdGeom {
    int fh[6], fw[6];  // extents of the six head inputs: conv3_3, conv4_3, conv5_3, fc7, conv6_2, conv7_2
    int priors;        // one per position of the six
};
void s3fd_extents(int v, int* f) {
    f[0] = v / 2 / 2;            // two floor pools
    f[1] = (f[0] + 1) / 2;       // vgg.16: ceil_mode
    f[2] = f[1] / 2;
    f[3] = f[2] / 2;             // pool5; fc6 (dilation 6, padding 6) and fc7 keep the extent
    f[4] = (f[3] - 1) / 2 + 1;   // extras.1: 3x3 / 2, padding 1
    f[5] = (f[4] - 1) / 2 + 1;   // extras.3
}
S3fdGeom s3fd_geom(int H, int W) {
    S3fdGeom g{};
    s3fd_extents(H, g.fh);
    s3fd_extents(W, g.fw);
    for (int i = 0; i < 6; ++i) g.priors += g.fh[i] * g.fw[i];
    return g;
}
// frames per pass of the S3FD lane: the two ping-pong buffers hold conv1's maps -- 64 channels at FULL resolution, 59 MB per
// 640 x 360 frame at 4 bytes per element -- and stay below 1.5 GiB each (and with that inside the contraction's 4 GiB operand range)
int face_s3fd_max_frames(int H, int W) {
    return (int)std::max<size_t>(1, (size_t)0x60000000u / ((size_t)H * W * 64 * 4));
}

int face_s3fd_forward_lane(avcer_ctx* ctx, int slot, int nb_cap, const uint8_t* frames, int n, int H, int W, int rgb, int mode,
                           float* loc, float* conf, float*, hipStream_t st) {
    Net net{ctx, ctx->face, mode_storage(mode), st};
    const int act = net.act.kind;
    const size_t es = net.act.es;
    const S3fdGeom g = s3fd_geom(H, W);
    const int P = g.priors;
    const int NB = std::min({n, nb_cap, face_s3fd_max_frames(H, W)});
    void* buf[2];
    float* inv;
    TRY(ws_carve(ctx, slot, "face (s3fd)", [&](Arena& ar) {
        for (auto& b : buf) b = ar.get((size_t)NB * H * W * 64 * es);
        inv = ar.get<float>((size_t)NB * g.fh[0] * g.fw[0] * 4);  // inverse norms of the largest L2Norm level
    }));
    for (int s0 = 0; s0 < n; s0 += NB) {
        const int nb = std::min(NB, n - s0);
        float *lo = loc + (size_t)s0 * P * 4, *co = conf + (size_t)s0 * P * 2;
        int h = H, w = W, c = 64, cur = 0, row0 = 0, level = 0;
        auto conv = [&](const std::string& p, int cout, int k, int stride, int pad, int dil) {
            avcer_conv_desc d = conv2d_desc(nb, h, w, c, k, k, stride, pad, cout, 1);
            d.dil_h = d.dil_w = dil;
            d.out_h = (h + 2 * pad - dil * (k - 1) - 1) / stride + 1;
            d.out_w = (w + 2 * pad - dil * (k - 1) - 1) / stride + 1;
            net.gemm(d, p + ".w", nullptr, net.F(p + ".b"), buf[cur], nullptr, buf[cur ^ 1], act, act);
            cur ^= 1; h = d.out_h; w = d.out_w; c = cout;
        };
        auto pool = [&](int ceil_mode) {
            const int oh = ceil_mode ? (h + 1) / 2 : h / 2, ow = ceil_mode ? (w + 1) / 2 : w / 2;
            net.chk(k_maxpool(ctx, buf[cur], buf[cur ^ 1], nb, h, w, c, 2, 0, oh, ow, act, st));
            cur ^= 1; h = oh; w = ow;
        };
        auto tap = [&](const char* name) { net.tap(name, buf[cur], (size_t)nb * h * w * c * es); };
        // one level's loc / conf rows from the tensor just produced (the heads read it in place; `l2` = an L2Norm level)
        auto head = [&](bool l2) {
            const std::string p = "head" + std::to_string(level);
            if (net.err == AVCER_OK && (h != g.fh[level] || w != g.fw[level]))
                net.err = set_err(ctx, AVCER_ESTATE, "face_forward (s3fd): level %d is %d x %d, expected %d x %d", level, h, w, g.fh[level], g.fw[level]);
            if (net.err == AVCER_OK)
                net.chk(launch_s3fd_head(ctx, buf[cur], act, l2 ? inv : nullptr, net.F(p + ".wt"), net.F(p + ".b"), nb, h, w, c, level ? 6 : 8,
                                         row0, P, lo, co, st));
            row0 += h * w;
            ++level;
        };
        net.chk(launch_s3fd_stem(ctx, frames + (size_t)s0 * H * W * 3, nb, H, W, rgb, net.F("stem.wt"), net.F("stem.b"), buf[0], act, st));
        tap("s3fd_conv1");
        conv("vgg2", 64, 3, 1, 1, 1);
        pool(0);
        tap("s3fd_pool1");
        conv("vgg5", 128, 3, 1, 1, 1);
        conv("vgg7", 128, 3, 1, 1, 1);
        pool(0);
        tap("s3fd_pool2");
        conv("vgg10", 256, 3, 1, 1, 1);
        conv("vgg12", 256, 3, 1, 1, 1);
        conv("vgg14", 256, 3, 1, 1, 1);
        tap("s3fd_conv3_3");
        head(true);
        pool(1);  // vgg.16: ceil_mode
        tap("s3fd_pool3");
        conv("vgg17", 512, 3, 1, 1, 1);
        conv("vgg19", 512, 3, 1, 1, 1);
        conv("vgg21", 512, 3, 1, 1, 1);
        tap("s3fd_conv4_3");
        head(true);
        pool(0);
        tap("s3fd_pool4");
        conv("vgg24", 512, 3, 1, 1, 1);
        conv("vgg26", 512, 3, 1, 1, 1);
        conv("vgg28", 512, 3, 1, 1, 1);
        tap("s3fd_conv5_3");
        head(true);
        pool(0);
        tap("s3fd_pool5");
        conv("vgg31", 1024, 3, 1, 6, 6);  // fc6
        conv("vgg33", 1024, 1, 1, 0, 1);  // fc7
        tap("s3fd_fc7");
        head(false);
        conv("ex0", 256, 1, 1, 0, 1);
        conv("ex1", 512, 3, 2, 1, 1);
        tap("s3fd_ex1");
        head(false);
        conv("ex2", 128, 1, 1, 0, 1);
        conv("ex3", 256, 3, 2, 1, 1);
        tap("s3fd_ex3");
        head(false);
        if (net.err != AVCER_OK) return net.err;
    }
    return net.err;
}

// ------------------------------------------------------------------------------------------------ the detector kinds
// What face_forward_impl asks of the loaded detector, by avcer_ctx::face_kind - 1
struct FaceKind {
    const char* name;  // for messages
    int (*lane)(avcer_ctx* ctx, int slot, int nb_cap, const uint8_t* frames, int n, int H, int W, int rgb, int mode, float* loc,
                float* conf, float* landms, hipStream_t st);
    int (*max_frames)(int H, int W);  // frames per pass
    int (*priors)(int H, int W);
    bool landms, bf16;  // has landmarks: `landms` is not null (S3FD ignores its null one); AVCER_MODE_BF16 is supported
};
const FaceKind kFaceKinds[3] = {
    {"ResNet-50", face_forward_lane, [](int H, int W) { return face_geom(H, W).max_frames; },
     [](int H, int W) { return face_geom(H, W).priors; }, true, true},
    {"MobileNet-0.25", face_mnet_forward_lane, [](int H, int W) { return face_mnet_max_frames(face_geom(H, W)); },
     [](int H, int W) { return face_geom(H, W).priors; }, true, false},
    {"S3FD", face_s3fd_forward_lane, face_s3fd_max_frames, [](int H, int W) { return s3fd_geom(H, W).priors; }, false, false},
};

// Batches of at least 16 frames run as TWO lanes, like the static CNN (visual.hip static_forward_impl): the frames' halves on two
// streams with a workspace each, passes of equal size within a lane.  The detector's late grids are small too -- stage 4 is
// 12 x 20 positions per 640 x 360 frame, pyramid level 3 the same -- and a pass of 273 frames (the 4 GiB range of layer 1's output)
// leaves partial rounds that the other lane's launches fill.  Bit-identical (a frame's result does not depend on its batch:
// tests/test_gpu_retina.py); serial under profiling / debug taps / avcer_set_static_lanes(ctx, 1).  Every kind runs as two lanes
// under the same rule.
int face_forward_impl(avcer_ctx* ctx, const uint8_t* frames, int n, int H, int W, int rgb, int mode, float* loc, float* conf,
                      float* landms, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (!ctx->face.loaded) return set_err(ctx, AVCER_ESTATE, "face detector weights not loaded");
    const FaceKind& k = kFaceKinds[ctx->face_kind - 1];
    if (!frames || !loc || !conf || (k.landms ? !landms : landms != nullptr) || n <= 0 || H < 32 || W < 32)
        return k.landms ? set_err(ctx, AVCER_EINVAL, "face_forward: bad arguments (frames of at least 32x32)")
                        : set_err(ctx, AVCER_EINVAL, "face_forward: bad arguments (frames of at least 32x32; the %s detector takes landms = NULL)", k.name);
    hipStream_t st = (hipStream_t)stream;
    if (!k.bf16 && mode == AVCER_MODE_BF16)
        return set_err(ctx, AVCER_EINVAL, "face_forward: AVCER_MODE_BF16 is not supported by the %s detector "
                                          "(AVCER_MODE_FP32 and AVCER_MODE_F16X3 are)", k.name);
    TRY(begin_forward(ctx, "face_forward", ctx->face, mode, true, st));
    const bool two = ctx->static_lanes >= 2 && n >= 16 && !ctx->prof && !ctx->tap_dst;
    if (!two) return k.lane(ctx, WS_FACE, n, frames, n, H, W, rgb, mode, loc, conf, landms, st);
    const int n0 = (n + 1) / 2;
    // equal passes inside a lane: the pass limit (R50: 4 GiB of layer 1's output) would otherwise leave a short last pass
    const int max_frames = k.max_frames(H, W), passes = (n0 + max_frames - 1) / max_frames, nb_cap = (n0 + passes - 1) / passes, P = k.priors(H, W);
    return run_two_lanes(ctx, st, [&](int lane, hipStream_t s) {
        const size_t f0 = lane ? n0 : 0;
        return k.lane(ctx, lane ? WS_FACE_LANE1 : WS_FACE, nb_cap, frames + f0 * H * W * 3, lane ? n - n0 : n0, H, W, rgb, mode,
                      loc + f0 * P * 4, conf + f0 * P * 2, landms ? landms + f0 * P * 10 : nullptr, s);
    });
}

}  // namespace

extern "C" int avcer_load_face(avcer_ctx* ctx, const void* blob, size_t nbytes) {
    if (!ctx) return AVCER_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // load_blob frees the previous detector whole -- its weights and every lazy copy made from them -- before it installs this one
    const int r = load_blob(ctx, ctx->face, blob, nbytes);
    // the kind, as packing.pack_face records it: the tensor "mnet.kind" marks a MobileNet-0.25 blob, "s3fd.kind" an S3FD one
    ctx->face_kind = !ctx->face.loaded ? 0 : ctx->face.t.count("s3fd.kind") ? 3 : ctx->face.t.count("mnet.kind") ? 2 : 1;
    return r;
}

extern "C" int avcer_face_kind(const avcer_ctx* ctx) { return ctx && ctx->face.loaded ? ctx->face_kind : 0; }
extern "C" int avcer_face_num_priors(int h, int w) { return h < 1 || w < 1 ? 0 : face_geom(h, w).priors; }
extern "C" int avcer_s3fd_num_priors(int h, int w) { return h < 1 || w < 1 ? 0 : s3fd_geom(h, w).priors; }

extern "C" int avcer_face_forward(avcer_ctx* ctx, const uint8_t* frames, int n, int h, int w, int rgb, int mode, float* loc,
                                  float* conf, float* landms, avcer_stream_t stream) {
    return face_forward_impl(ctx, frames, n, h, w, rgb ? 1 : 0, mode, loc, conf, landms, stream);
}
