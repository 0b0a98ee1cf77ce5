// What avcer_conv_gemm's `dtype` means, which form of the contraction can take a shape and which form and tile is preferred: one
// statement for the launcher (gemm.hip) and the networks (net.h Net::gemm).  Host only, nothing of HIP (tests/gemm_forms_driver.cpp).
#pragma once
#include <algorithm>

#include "../../include/avcer_hip.h"

// how an activation tensor is stored (the `kind` / `act` arguments of the k_* launchers, Net::gemm's akind / okind, the kernels' OUT)
enum { KIND_F32 = 0, KIND_BF16 = 1, KIND_SP32 = 2 };
// the copy of the weights a dtype reads (common.h Tensor f32, bf16, x3 = split rows, x3f = the same in MFMA fragment order)
enum { W_F32 = 0, W_BF16 = 1, W_SPLIT = 2, W_FRAGS = 3 };
// the kernel: tiles through LDS (conv_gemm_kernel); 112 / 128 x 256 tiles, weight fragments direct from global memory
// (conv_gemm_wd_kernel); one wave per 16 / 32 / 64 x 16 tile, registers only, for a handful of positions (conv_gemm_skinny_kernel)
enum { FORM_STAGED = 0, FORM_DIRECT = 1, FORM_SKINNY = 2 };
// One row per dtype of the ABI.  mode: conv_gemm_kernel's MODE (0 f32, 1 bf16, 2 f32 split on the fly, 3 sp32)
struct GemmForm { int a_kind, o_kind, w_copy, form, mode; };
constexpr int kGemmForms = 11;
constexpr GemmForm kGemmForm[kGemmForms] = {
    {KIND_F32, KIND_F32, W_F32, FORM_STAGED, 0},      //  0
    {KIND_BF16, KIND_BF16, W_BF16, FORM_STAGED, 1},   //  1
    {KIND_BF16, KIND_F32, W_BF16, FORM_STAGED, 1},    //  2
    {KIND_F32, KIND_F32, W_SPLIT, FORM_STAGED, 2},    //  3
    {KIND_F32, KIND_SP32, W_SPLIT, FORM_STAGED, 2},   //  4
    {KIND_SP32, KIND_SP32, W_SPLIT, FORM_STAGED, 3},  //  5
    {KIND_SP32, KIND_F32, W_SPLIT, FORM_STAGED, 3},   //  6
    {KIND_SP32, KIND_SP32, W_FRAGS, FORM_DIRECT, 3},  //  7: 5 with the weights in fragment order
    {KIND_SP32, KIND_F32, W_FRAGS, FORM_DIRECT, 3},   //  8: 6 likewise
    {KIND_SP32, KIND_SP32, W_FRAGS, FORM_SKINNY, 3},  //  9: 7 for a handful of positions
    {KIND_SP32, KIND_F32, W_FRAGS, FORM_SKINNY, 3},   // 10: 8 likewise
};
// launch_conv_gemm's dispatch switch states its template arguments once more: each case asserts this of its row
template <int DTYPE, int FORM, int MODE, int OUT>
constexpr bool gemm_row_is = kGemmForm[DTYPE].form == FORM && kGemmForm[DTYPE].mode == MODE && kGemmForm[DTYPE].o_kind == OUT;
constexpr int gemm_in_bytes(int dtype) { return kGemmForm[dtype].a_kind == KIND_BF16 ? 2 : 4; }   // per element read (A and W)
constexpr int gemm_out_bytes(int dtype) { return kGemmForm[dtype].o_kind == KIND_BF16 ? 2 : 4; }  // per element written
constexpr int gemm_bk(int dtype) { return 128 / gemm_in_bytes(dtype); }  // elements per K-step: a 128-byte row (gemm_dev.h ROWB)
constexpr bool gemm_a_split(int dtype) { return kGemmForm[dtype].a_kind == KIND_SP32; }
// granularity of the output's leading dimension and offset: whole sp32 groups, else 16-byte vectors
constexpr int gemm_ovec(int dtype) { return kGemmForm[dtype].o_kind == KIND_SP32 ? 32 : 16 / gemm_out_bytes(dtype); }
constexpr int gemm_family(int dtype) {  // AVCER_FAM_* of the profile
    return kGemmForm[dtype].form == FORM_SKINNY ? AVCER_FAM_SKINNY : kGemmForm[dtype].form == FORM_DIRECT ? AVCER_FAM_GEMM_WD : AVCER_FAM_GEMM;
}
// The inverse: the dtype that reads a_kind, writes o_kind, with split-fp16 weights (x3) or not, on `form`; -1: there is none
constexpr int gemm_dtype(int a_kind, int o_kind, bool x3, int form) {
    for (int i = 0; i < kGemmForms; ++i)
        if (kGemmForm[i].a_kind == a_kind && kGemmForm[i].o_kind == o_kind && (kGemmForm[i].w_copy >= W_SPLIT) == x3 && kGemmForm[i].form == form) return i;
    return -1;
}

// ---- which form can take a shape
inline long gemm_m(const avcer_conv_desc& d) { return (long)d.batch * d.out_h * d.out_w; }
inline int gemm_groups(const avcer_conv_desc& d) { return d.groups > 1 ? d.groups : 1; }
// Fast gather: Cin a multiple of the K-step, no padding, and the last tap of the last output position inside the
// input -- true for every Linear, 1x1 convolution and un-padded Conv1d of both models.
inline bool gemm_fast_gather(const avcer_conv_desc& d, int bk) {
    return d.cin % bk == 0 && d.pad_h == 0 && d.pad_w == 0 && (long)(d.out_h - 1) * d.stride_h + (long)(d.kh - 1) * d.dil_h < d.in_h &&
           (long)(d.out_w - 1) * d.stride_w + (long)(d.kw - 1) * d.dil_w < d.in_w;
}
// Why the weights-direct / the skinny form cannot take a contraction of K inputs (x2: it has a second source; fast: its gather is
// gemm_fast_gather), or null: it can.  launch_conv_gemm refuses with the text, choose_gemm never picks a refused form.
inline const char* direct_cannot(const avcer_conv_desc& d, long K, bool x2, bool fast) {
    if (d.n % 256 || (K / 32) % 2 || gemm_groups(d) != 1 || d.tile_n == 64 || d.tile_n == 128) return "needs N % 256 == 0, an even number of K-steps, one group";
    return x2 && !fast ? "with a second source needs a pad-free gather" : nullptr;
}
// (the skinny kernel wants whole 32-channel K groups per tap and whole 32-channel output groups)
inline const char* skinny_cannot(const avcer_conv_desc& d, long /*K*/, bool x2, bool /*fast*/) {
    return x2 || d.cin % 32 || d.n % 32 || gemm_m(d) > 4096 ? "(skinny form) needs one source, cin % 32 == 0, n % 32 == 0, M <= 4096" : nullptr;
}
// The weights that get split copies on the first x3 call: [n][k] with whole K groups of 32 and whole 64-channel tiles
inline bool gemm_weight_splits(int ndim, long n, long k) { return ndim == 2 && k % 32 == 0 && n % 64 == 0; }

// ---- which form and tile is preferred
// Rounds a grid of 256-thread blocks takes on the chip's block slots (two per CU: `slots` = 2 x the CU count the context
// read from the device at creation, 512 on a whole MI355X), as the form / tile choices model them.
// Calibrated on tools/ab_layers.py (profiles/r03_ab_layers*.txt, 128- against 112-row tiles of the same layer): a grid of
// at most one block per CU runs in 0.62 of a round (a block alone on its CU is that much faster); behind whole rounds, a
// partial round that still fits one block per CU (fraction f <= 0.5) costs 0.25 + 0.7 f -- the whole rounds end ragged and
// absorb part of it --, a larger one a whole round (some CU runs two blocks from start to end).
inline double grid_rounds(long tiles, long slots) {
    const long whole = tiles / slots, rest = tiles % slots;
    if (whole == 0) return 2 * tiles <= slots ? 0.62 : 1.0;
    const double f = (double)rest / (double)slots;
    return (double)whole + (rest == 0 ? 0.0 : (2 * rest <= slots ? 0.25 + 0.7 * f : 1.0));
}
// cost of the weights-direct grid of `rows` x 256 tiles: rounds x rows per tile
inline double direct_cost(long M, int N, long slots, int rows) { return grid_rounds((M + rows - 1) / rows * (N / 256), slots) * rows; }
// 128 or 112 positions per weights-direct tile: whichever grid costs fewer; avcer_conv_desc.tile_m (`hint`) overrides
inline int direct_tile_m(long M, int N, long slots, int hint) {
    return hint == 112 || (hint == 0 && direct_cost(M, N, slots, 112) < 0.97 * direct_cost(M, N, slots, 128)) ? 112 : 128;
}
// Which form of the x3 contraction serves a layer of M positions, N channels: the weights-direct kernel (128 x 256 tiles,
// dtype 7 / 8) or the LDS-staged one (128 x 128, dtype 5 / 6).  Results are bit-identical, so this is speed only.  Model,
// calibrated on tools/ab_layers.py (profiles/r04_ab_layers*.txt; round 4's spread K loop moved it from 1.84-1.90): a 128 x 256
// tile costs 1.72 tiles of 128 x 128 (qkv 1.73, out-proj 1.75, ffn1 1.69, l3.x.c2 1.68, fe6 1.72), a 112 x 256 tile 7/8 of
// that, and the grid takes grid_rounds() rounds of the block slots.
inline bool prefer_weights_direct(long M, int N, long slots) {
    const double wd = std::min(direct_cost(M, N, slots, 128), direct_cost(M, N, slots, 112)) / 128.0;
    return wd * 1.72 < grid_rounds((M + 127) / 128 * (N / 128), slots);
}
// When the skinny form serves a launch: while its grid of 32-position x 16-channel wave tiles fits the chip's SIMDs in one
// round (n: all groups' channels).  tools/ab_layers.py --skinny at 1 / 4 / 16 / 64 frames and windows (profiles/r05_skinny_ab.txt):
// below that count it beats the better tiled form on every layer shape of both networks (by 1.05-3.8x), above it it loses.
inline bool prefer_skinny(long M, int n, int block_slots) {
    return M <= 4096 && ((M + 31) / 32) * (long)(n / 16) <= 2L * block_slots;
}
// Positions per skinny wave tile: the smallest tile whose grid still fits the chip in one round of one wave per SIMD.
// 16-position tiles while they leave half the SIMDs free (a wave is paced by its round trips -- the weights come from beyond
// the L2 once per launch -- so the smallest tile wins); past that the round trips lengthen with the load, and the 32-position
// tile moves 6 KiB per K-step where two 16s move 8 (tools/ab_layers.py --skinny, profiles/r05_skinny_ab.txt)
inline int skinny_tile_m(long M, int N, int groups, long slots, int hint) {
    const long simds = slots * 2, nt = N / 16 * groups;  // block slots = 2 per CU, 4 SIMDs per CU
    if (hint == 16 || (hint == 0 && (M + 15) / 16 * nt <= simds / 2)) return 16;
    return hint == 32 || (hint == 0 && (M + 31) / 32 * nt <= simds) ? 32 : 64;
}
// Width of the staged tile.  K <= 128: bandwidth-bound 1x1 convolutions, the 48 KiB 64-wide tile lets three blocks share a
// CU.  A grid of at most one block per two CUs (the LSTM's recurrent GEMMs, fc1, single-frame calls): twice the blocks at
// half the width.  avcer_conv_desc.tile_n (`hint`) overrides.
inline int staged_tile_n(long M, int N, long K, long slots, int hint) {
    const bool wide = K > 128 && (M + 127) / 128 * (N / 128) > slots / 4;
    return N % 128 == 0 && hint != 64 && (wide || hint == 128) ? 128 : 64;
}

// The dtype Net::gemm launches: activations read / written as a_kind / o_kind, `x3` the network's split-fp16 mode, `copies`
// bit W_* set where that copy of the weights exists, x2 a second source.  -1: no dtype serves the kinds with the copies there
// are.  Resets the tile hints of `d` for the skinny form: they are hints for the tiled forms and do not apply.
inline int choose_gemm(int a_kind, int o_kind, bool x3, unsigned copies, avcer_conv_desc& d, bool x2, int block_slots) {
    auto serves = [&](int dtype) { return dtype >= 0 && ((copies >> kGemmForm[dtype].w_copy) & 1); };
    int dtype = x3 ? gemm_dtype(a_kind, o_kind, true, FORM_STAGED) : -1;
    if (dtype >= 0 && gemm_a_split(dtype) && ((copies >> W_FRAGS) & 1)) {
        const long M = gemm_m(d), K = (long)d.kh * d.kw * d.cin + (x2 ? d.x2_cin : 0);
        const bool fast = gemm_fast_gather(d, gemm_bk(dtype));
        // sp32 activations: the weights-direct kernel wherever it is the cheaper grid (or asked for)
        if (!direct_cannot(d, K, x2, fast) && (d.tile_n == 256 || (d.tile_n == 0 && prefer_weights_direct(M, d.n, block_slots))))
            dtype = gemm_dtype(a_kind, o_kind, true, FORM_DIRECT);
        // a handful of positions (a frame or a window per call through the mirrors; the deep layers of a small batch):
        // bit-identical to the tiled forms, so the choice by M does not show in any result
        if (!skinny_cannot(d, K, x2, fast) && prefer_skinny(M, d.n * gemm_groups(d), block_slots)) {
            dtype = gemm_dtype(a_kind, o_kind, true, FORM_SKINNY);
            d.tile_n = d.tile_m = 0;
        }
    }
    if (!serves(dtype)) dtype = gemm_dtype(a_kind, o_kind, false, FORM_STAGED);  // no split copy of this tensor: exact f32
    return serves(dtype) ? dtype : -1;
}
