// The recurrence of one torch.nn.GRU layer (hidden size 256) as ONE launch with the time loop inside it: the GRU head of the
// audio model ExprModelV1 (ref: architectures/audio_8_cl.py:18-72, audio_7_cl.py:18-72; two layers, 99 steps for a 2 s window
// and 199 for a 4 s one).  The input projections of all steps (x W_ih^T + b_ih: [n, S, 768], gate order r, z, n) come from an
// ordinary contraction in front of this launch; what is left per step is
//     g = W_hh h_{t-1}                        [768] per window
//     r = sigmoid(xp_r + g_r + b_hr),  z = sigmoid(xp_z + g_z + b_hz),  n = tanh(xp_n + r (g_n + b_hn)),
//     h_t = (1 - z) n + z h_{t-1},  h_0 = 0   (b_hn sits inside the r product: the two bias vectors cannot be merged)
// and it depends on the step before: the LSTM's way (one contraction + one cell launch per step, visual.hip) would be ~800 dependent
// launches per call here.
//
// Work split.  Windows are independent, so a block owns a tile of 16 windows -- the N of the 16 x 16 MFMA with the weights as
// the A operand, as everywhere in this library -- and walks t = 0 .. S-1 itself.  Blocks never wait for one another.  The
// block's 8 waves split the 256 hidden units: wave w holds units 32 w .. 32 w + 31 of ALL THREE gates (six 16-row fragment
// tiles), so the r, z and n pre-activations of a (window, unit) pair meet in one lane's accumulators and the gate arithmetic
// needs no exchange; that lane also keeps the unit's h as f32 state in a register for the whole sequence.  Only the B operand
// of the next step -- all 256 h values of a window -- crosses waves: every step ends with the new h written to one of two LDS
// tiles (16 rows, padded against bank conflicts) and ONE barrier; the other tile is what the step has been reading.
//
// W_hh is 768 KiB in either arithmetic -- more than a CU's LDS (160 KiB) or what its register file can spare -- so it is
// streamed from the L2 every step.  It does not depend on h: each wave keeps a register ring of RING fragments that runs ahead
// ACROSS step boundaries (the slot a product has just consumed is refilled with the fragment 12 positions further on, modulo
// the step), so the start of a step never waits for memory; hipcc's own counted vmcnt waits pace the ring, and the step's
// barrier (no LDS-DMA in flight) does not drain it.
//
//   X3 = 1 (AVCER_MODE_F16X3): the split-fp16 contraction ah.wh + ah.wl + al.wh on v_mfma_f32_16x16x32_f16, weights from the
//     fragment-order split copy (k_weight_frags), h split into an fp16 pair when it is written to LDS.  |h| < 1, so the
//     range contract of the split (split_dev.h) cannot break here and nothing is counted.
//   X3 = 0 (AVCER_MODE_FP32, and the bf16 mode, which runs the recurrence as f32 like the LSTM): v_mfma_f32_16x16x4_f32 on the
//     f32 weights as packed.  A lane fetches 16 bytes of a weight row at a time, so lane group g supplies K elements
//     16 q + 4 g + j to MFMA j of group q -- for A and B alike, which is all the K order of an MFMA has to satisfy.
//
// A tile with fewer than 16 valid windows computes the last valid window again in its spare columns (columns of an MFMA do not
// mix) and stores nothing for them: a window's values do not depend on its position or on its neighbours.
#include "common.h"
#include "gemm_dev.h"
#include "split_dev.h"

namespace {

constexpr int GRU_H = 256;          // hidden size
constexpr int GRU_THREADS = 512;    // 8 waves x 32 hidden units
constexpr int GRU_ROW = 1024 + 16;  // bytes of one window's h in LDS (256 x 4 bytes in either storage), + 16 against bank conflicts
constexpr int GRU_RING = 12;        // weight fragments in flight per wave (8 registers each); divides the 48 of a step
constexpr int GRU_ITEMS = 48;       // 8 K chunks x 6 fragment tiles per wave and step

struct GruParams {
    const float* xp;    // [n, S, 768] input projections + b_ih
    const char* w;      // X3: fragment-order split copy of W_hh [768][256] (+ trailer); else the f32 matrix
    unsigned w_bytes;   // bytes of the matrix without its trailer
    const float* bhh;   // [768]
    float* hseq;        // [n, S, 256] f32
    char* hsp;          // the same as sp32 pairs, or null
    int n, S;
};

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

template <int X3>
__global__ void __launch_bounds__(GRU_THREADS) gru_layer_kernel(const GruParams p) {
    __shared__ __attribute__((aligned(16))) char hs[2][16 * GRU_ROW];
    __shared__ __attribute__((aligned(16))) float bs[3 * GRU_H];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l15 = lane & 15;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int win = blockIdx.x * 16 + l15;
    const bool ok = win < p.n;
    const long wrow = (long)(ok ? win : p.n - 1) * p.S;  // first row of this lane's window in xp / the outputs
    // this lane's hidden units: c0[u] .. c0[u] + 3 for its two tiles per gate.  X3: the stored rows of a fragment tile are
    // permuted (kernels.hip split_weight_rows_kernel) so that the two tiles of a 32-unit group leave a lane 8 consecutive units
    int c0[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) c0[u] = X3 ? 32 * wv + 8 * g + 4 * u : 32 * wv + 16 * u + 4 * g;
    // weights: one lane-varying offset, everything else scalar.  Item i of a step = K chunk i / 6 (32 elements), tile i % 6
    // (gate (i % 6) / 2, half u = i % 2); its two 16-byte pieces: X3 hi / lo fragment, else K elements 16 g' + 4 g .. of g' = 2 k, 2 k + 1
    const auto wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.w), (short)0, (int)p.w_bytes, 0x00020000);
    const unsigned w_v = X3 ? (unsigned)lane * 16u : (unsigned)l15 * 1024u + (unsigned)g * 16u;
    const unsigned w_s = X3 ? (unsigned)wv * (2u * 8u * 2048u) : (unsigned)wv * (32u * 1024u);
    constexpr unsigned W_GATE = X3 ? 16u * 8u * 2048u : 256u * 1024u;  // 16 tiles of 8 K-steps / 256 rows
    constexpr unsigned W_HALF = X3 ? 8u * 2048u : 16u * 1024u;
    constexpr unsigned W_K = X3 ? 2048u : 128u, W_SEC = X3 ? 1024u : 64u;
    u32x4_t ring[GRU_RING][2];
#define AVCER_GRU_ISSUE(SLOT, ITEM)                                                                                      \
    do {                                                                                                                 \
        constexpr unsigned so_ = (unsigned)(((ITEM) % 6) / 2) * W_GATE + (unsigned)((ITEM) % 2) * W_HALF + (unsigned)((ITEM) / 6) * W_K; \
        ring[SLOT][0] = __builtin_amdgcn_raw_buffer_load_b128(wrs, w_v, w_s + so_, 0);                                   \
        ring[SLOT][1] = __builtin_amdgcn_raw_buffer_load_b128(wrs, w_v, w_s + so_ + W_SEC, 0);                           \
    } while (0)
    float wmul = 1.f;
    if constexpr (X3) wmul = split_wmul(p.w, p.w_bytes);
    // b_hh into LDS (read back at gate time: 24 registers less to keep alive); h_0 = 0 in the tile step 0 reads and in the registers
    for (int i = tid; i < 3 * GRU_H; i += GRU_THREADS) bs[i] = p.bhh[i];
    for (int i = tid; i < 16 * GRU_ROW / 16; i += GRU_THREADS) reinterpret_cast<uint4*>(hs[1])[i] = make_uint4(0u, 0u, 0u, 0u);
    float h[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[u][r] = 0.f;
    // the ring's first fill
    AVCER_GRU_ISSUE(0, 0);
    AVCER_GRU_ISSUE(1, 1);
    AVCER_GRU_ISSUE(2, 2);
    AVCER_GRU_ISSUE(3, 3);
    AVCER_GRU_ISSUE(4, 4);
    AVCER_GRU_ISSUE(5, 5);
    AVCER_GRU_ISSUE(6, 6);
    AVCER_GRU_ISSUE(7, 7);
    AVCER_GRU_ISSUE(8, 8);
    AVCER_GRU_ISSUE(9, 9);
    AVCER_GRU_ISSUE(10, 10);
    AVCER_GRU_ISSUE(11, 11);
    static_assert(GRU_RING == 12 && GRU_ITEMS % GRU_RING == 0, "the ring's slots are static: 48 items in 12 slots");
    __syncthreads();
    for (int t = 0; t < p.S; ++t) {
        const char* hb = hs[(t + 1) & 1] + l15 * GRU_ROW + g * 16;  // h_{t-1}: this lane's column of the B operand
        char* hn = hs[t & 1] + l15 * GRU_ROW;
        const float* xr = p.xp + (wrow + t) * (3 * GRU_H);
        f32x4_t acc[6], x[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const u32x4_t b0 = *reinterpret_cast<const u32x4_t*>(hb + k * 128), b1 = *reinterpret_cast<const u32x4_t*>(hb + k * 128 + 64);
            if (k == 4) {
                // this step's input projections, requested in the middle of the step: behind the ring in the memory queue, and
                // four K chunks ahead of their use
#pragma unroll
                for (int j = 0; j < 6; ++j) x[j] = *reinterpret_cast<const f32x4_t*>(xr + (j >> 1) * GRU_H + c0[j & 1]);
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int i = k * 6 + j, slot = i % GRU_RING;
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (X3) {
                    const spx8_t whi = __builtin_bit_cast(spx8_t, ring[slot][0]), wlo = __builtin_bit_cast(spx8_t, ring[slot][1]);
                    const spx8_t bhi = __builtin_bit_cast(spx8_t, b0), blo = __builtin_bit_cast(spx8_t, b1);
                    acc[j] = mfma_sp(wlo, bhi, acc[j]);
                    acc[j] = mfma_sp(whi, blo, acc[j]);
                    acc[j] = mfma_sp(whi, bhi, acc[j]);
                } else {
                    const f32x4_t w0 = __builtin_bit_cast(f32x4_t, ring[slot][0]), w1 = __builtin_bit_cast(f32x4_t, ring[slot][1]);
                    const f32x4_t h0 = __builtin_bit_cast(f32x4_t, b0), h1 = __builtin_bit_cast(f32x4_t, b1);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[q], h0[q], acc[j], 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[q], h1[q], acc[j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                // the slot just consumed: the fragment RING positions further on, which past the step's end is the next step's
                // (same matrix every step; the last step's look-ahead is requested and never used)
                switch ((i + GRU_RING) % GRU_ITEMS) {
#define AVCER_GRU_CASE(I) case I: AVCER_GRU_ISSUE((I) % GRU_RING, I); break;
                    AVCER_GRU_CASE(0) AVCER_GRU_CASE(1) AVCER_GRU_CASE(2) AVCER_GRU_CASE(3) AVCER_GRU_CASE(4) AVCER_GRU_CASE(5)
                    AVCER_GRU_CASE(6) AVCER_GRU_CASE(7) AVCER_GRU_CASE(8) AVCER_GRU_CASE(9) AVCER_GRU_CASE(10) AVCER_GRU_CASE(11)
                    AVCER_GRU_CASE(12) AVCER_GRU_CASE(13) AVCER_GRU_CASE(14) AVCER_GRU_CASE(15) AVCER_GRU_CASE(16) AVCER_GRU_CASE(17)
                    AVCER_GRU_CASE(18) AVCER_GRU_CASE(19) AVCER_GRU_CASE(20) AVCER_GRU_CASE(21) AVCER_GRU_CASE(22) AVCER_GRU_CASE(23)
                    AVCER_GRU_CASE(24) AVCER_GRU_CASE(25) AVCER_GRU_CASE(26) AVCER_GRU_CASE(27) AVCER_GRU_CASE(28) AVCER_GRU_CASE(29)
                    AVCER_GRU_CASE(30) AVCER_GRU_CASE(31) AVCER_GRU_CASE(32) AVCER_GRU_CASE(33) AVCER_GRU_CASE(34) AVCER_GRU_CASE(35)
                    AVCER_GRU_CASE(36) AVCER_GRU_CASE(37) AVCER_GRU_CASE(38) AVCER_GRU_CASE(39) AVCER_GRU_CASE(40) AVCER_GRU_CASE(41)
                    AVCER_GRU_CASE(42) AVCER_GRU_CASE(43) AVCER_GRU_CASE(44) AVCER_GRU_CASE(45) AVCER_GRU_CASE(46) AVCER_GRU_CASE(47)
#undef AVCER_GRU_CASE
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // gates (torch.nn.GRU, order r, z, n), f32
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x4_t br = *reinterpret_cast<const f32x4_t*>(bs + c0[u]), bz = *reinterpret_cast<const f32x4_t*>(bs + GRU_H + c0[u]),
                          bn = *reinterpret_cast<const f32x4_t*>(bs + 2 * GRU_H + c0[u]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float gr = gru_sigmoid(x[u][r] + (acc[u][r] * wmul + br[r]));
                const float gz = gru_sigmoid(x[2 + u][r] + (acc[2 + u][r] * wmul + bz[r]));
                const float gn = tanhf(x[4 + u][r] + gr * (acc[4 + u][r] * wmul + bn[r]));
                h[u][r] = (1.f - gz) * gn + gz * h[u][r];
            }
        }
        // h_t: to the sequence (f32, and sp32 pairs for the next contraction that reads it) and to the LDS tile of the next step
        uint4 hi, lo;
        if constexpr (X3) {
            const float h8[8] = {h[0][0], h[0][1], h[0][2], h[0][3], h[1][0], h[1][1], h[1][2], h[1][3]};
            float hmax = 0.f;  // never read: |h_t| <= 1
            sp_split8(h8, hmax, hi, lo);
            // units 32 wv + 8 g .. + 7: K group wv of the sp32 row, 16 bytes of its hi half and of its lo half
            *reinterpret_cast<uint4*>(hn + wv * 128 + g * 16) = hi;
            *reinterpret_cast<uint4*>(hn + wv * 128 + g * 16 + 64) = lo;
        } else {
#pragma unroll
            for (int u = 0; u < 2; ++u)
                *reinterpret_cast<float4*>(hn + c0[u] * 4) = make_float4(h[u][0], h[u][1], h[u][2], h[u][3]);
        }
        if (ok) {
            float* ho = p.hseq + (wrow + t) * GRU_H;
#pragma unroll
            for (int u = 0; u < 2; ++u) *reinterpret_cast<float4*>(ho + c0[u]) = make_float4(h[u][0], h[u][1], h[u][2], h[u][3]);
            if constexpr (X3) {
                if (p.hsp) {
                    char* so = p.hsp + (wrow + t) * (GRU_H * 4) + wv * 128 + g * 16;
                    *reinterpret_cast<uint4*>(so) = hi;
                    *reinterpret_cast<uint4*>(so + 64) = lo;
                }
            }
        }
        __syncthreads();  // h_t is in its tile for every wave; every wave is done reading h_{t-1}, which step t + 1 overwrites
    }
#undef AVCER_GRU_ISSUE
}

}  // namespace

// One GRU layer's recurrence over S steps for n windows.  xp [n, S, 768] f32; w: the fragment-order split copy of W_hh (x3) or
// the f32 matrix; bhh [768]; h_seq [n, S, 256] f32; h_sp: the same as sp32 pairs (x3 only) or null.
int launch_gru_layer(avcer_ctx* ctx, const float* xp, const void* w, int x3, const float* bhh, int n, int S, float* h_seq, void* h_sp,
                     hipStream_t st) {
    if (!xp || !w || !bhh || !h_seq || n <= 0 || S <= 0) return set_err(ctx, AVCER_EINVAL, "gru_layer: bad arguments");
    if (h_sp && !x3) return set_err(ctx, AVCER_EINVAL, "gru_layer: sp32 output in the f32 arithmetic");
    GruParams p;
    p.xp = xp; p.w = (const char*)w; p.w_bytes = 3u * GRU_H * GRU_H * 4u; p.bhh = bhh;
    p.hseq = h_seq; p.hsp = (char*)h_sp; p.n = n; p.S = S;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // per step and window 2 x 768 x 256 FLOPs; compulsory bytes: xp and the sequence once, the matrix once
    TRY(prof_begin(ctx, st, &ev0, &ev1, FAM_GRU, 2.0 * n * S * 3.0 * GRU_H * GRU_H,
                   (double)n * S * (3.0 + 1.0 + (h_sp ? 1.0 : 0.0)) * GRU_H * 4 + 3.0 * GRU_H * GRU_H * 4, (long)n * S, 3 * GRU_H, GRU_H));
    const dim3 grid((n + 15) / 16);
    if (x3) gru_layer_kernel<1><<<grid, GRU_THREADS, 0, st>>>(p);
    else gru_layer_kernel<0><<<grid, GRU_THREADS, 0, st>>>(p);
    if (ev1) (void)hipEventRecord(ev1, st);
    CHECK_LAUNCH(ctx, "gru_layer");
    return AVCER_OK;
}
