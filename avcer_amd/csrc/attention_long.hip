// softmax(q k^T * scale) v for any number of tokens up to AVCER_AUDIO_MAX_TOKENS (gfx950): the attention of audio windows longer
// than the 256 tokens whose K and V the whole-head kernels of kernels.hip keep in LDS.
//   ref: architectures/attention_layers.py:10-38,80-144; transformers Wav2Vec2Attention (eager): no length limit of their own.
//
// One workgroup (8 waves) per (window, head, block of ATL_QB = 128 queries): a single 100 s window of 16 heads is 640 workgroups,
// not 16.  Keys pass through LDS in tiles of ATL_KT = 128 (one tile's K and V image; the f32 form: 66 KiB, the x3 form: 66.5 KiB),
// and every query row keeps a running maximum m, a running denominator l and accumulators that are multiplied by exp(m_old - m_new)
// whenever a tile raises the maximum (the textbook order: the factor is applied to O and l BEFORE the tile's exponentials, which
// are taken against m_new, are added; a tile's P V sum is formed on its own and then added: blocked summation).  Keys of the
// tail tile past s are masked: their score is -inf, their weight exactly 0.
// Every loop is counted (ceil(s / 128) tiles), and no workgroup waits for another.
//
// The three arithmetic forms are those of the whole-head kernels:
//   attention_long_f32_kernel    f32 in, f32 out, exact f32 on the VALU: a wave takes one query at a time, lanes over the tile's keys
//   attention_long_mfma_kernel   X3 = 0: bf16 in, bf16 out, bf16 operands on the MFMA
//                                X3 = 1: f32 in, sp32 out, every product as hi.hi + hi.lo + lo.hi of fp16 pairs (split_dev.h)
// The MFMA form is attention_mfma_kernel's tile arithmetic (swapped operands: a lane holds ONE query's scores, so the row
// statistics are in-lane plus two shuffles, and the exponentiated accumulators are the B operand of the P V product) with the
// key loop around it; the next tile's global loads are in flight while the present one is computed.
#include "attention_dev.h"

#include <cmath>

namespace {

constexpr int ATL_WAVES = 8;
constexpr int ATL_THREADS = 64 * ATL_WAVES;
constexpr int ATL_KT = AVCER_ATT_LONG_KT;  // keys per tile
constexpr int ATL_QB = AVCER_ATT_LONG_QB;  // queries per workgroup
static_assert(ATL_KT == 128 && ATL_QB == 16 * ATL_WAVES, "eight 16-key MFMA tiles per key tile; one 16-query MFMA tile per wave");

// the factor that brings sums taken against the maximum m_old to the maximum m_new >= m_old.  m_old == m_new also covers
// -inf == -inf (nothing seen yet, or only NaN scores: fmaxf skips them), where exp(m_old - m_new) would be exp(NaN)
__device__ __forceinline__ float atl_rescale(float m_old, float m_new) { return m_old == m_new ? 1.f : expf(m_old - m_new); }

// ---- exact f32 on the VALU
// LDS: K tile (rows padded by 4 floats: conflict-free b128 row reads), V tile, the block's 128 pre-scaled query rows, their
// unnormalised outputs (64 floats a query: d = 64 one per lane, d = 32 the two half-waves' partial sums), one row of weights per wave.
// Wave w owns queries w, w + 8, ... of the block (16 of them); lane i of the wave keeps m and l of the wave's i-th query.
template <int D>
__global__ void __launch_bounds__(ATL_THREADS) attention_long_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int s,
                                                                          int heads, int nqb, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int KP = D + 4;
    constexpr int QW = ATL_QB / ATL_WAVES;                    // queries per wave
    float* ks = reinterpret_cast<float*>(smem_raw);           // [ATL_KT][KP]
    float* vs = ks + ATL_KT * KP;                             // [ATL_KT][D]
    float* qs = vs + ATL_KT * D;                              // [ATL_QB][D]
    float* os = qs + ATL_QB * D;                              // [ATL_QB][64]
    float* ps = os + ATL_QB * 64;                             // [ATL_WAVES][ATL_KT]
    const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
    const int b = bh / heads, h = bh % heads;
    const int e = heads * D;
    const long rowstride = 3L * e;
    const float* base = qkv + (long)b * s * rowstride + h * D;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int q0 = qb * ATL_QB;
    for (int i = tid; i < ATL_QB * (D / 4); i += ATL_THREADS) {
        const int r = i / (D / 4), c4 = (i % (D / 4)) * 4;
        float qv[4] = {0.f, 0.f, 0.f, 0.f};
        if (q0 + r < s) ld4<float>(base, (long)(q0 + r) * rowstride + c4, qv);
        *reinterpret_cast<float4*>(qs + r * D + c4) = make_float4(qv[0] * scale, qv[1] * scale, qv[2] * scale, qv[3] * scale);
    }
    for (int i = tid; i < ATL_QB * 64; i += ATL_THREADS) os[i] = 0.f;
    float m_all = -INFINITY, l_all = 0.f;
    float* pw = ps + wv * ATL_KT;
    const int nkt = (s + ATL_KT - 1) / ATL_KT;
    for (int kt = 0; kt < nkt; ++kt) {
        const int k0 = kt * ATL_KT;
        const int kn = min(ATL_KT, s - k0);                   // keys of this tile
        __syncthreads();                                      // the tile before has been read by every wave
        for (int i = tid; i < kn * (D / 4); i += ATL_THREADS) {
            const int r = i / (D / 4), c4 = (i % (D / 4)) * 4;
            float kv[4], vv[4];
            ld4<float>(base, (long)(k0 + r) * rowstride + e + c4, kv);
            ld4<float>(base, (long)(k0 + r) * rowstride + 2 * e + c4, vv);
            *reinterpret_cast<float4*>(ks + r * KP + c4) = make_float4(kv[0], kv[1], kv[2], kv[3]);
            *reinterpret_cast<float4*>(vs + r * D + c4) = make_float4(vv[0], vv[1], vv[2], vv[3]);
        }
        __syncthreads();
        for (int i = 0; i < QW; ++i) {
            const int ql = wv + ATL_WAVES * i;
            if (q0 + ql >= s) break;                          // wave-uniform
            const float* qw = qs + ql * D;
            float sc[ATL_KT / 64];
            float mx = -INFINITY;
#pragma unroll
            for (int jj = 0; jj < ATL_KT / 64; ++jj) {
                const int j = jj * 64 + lane;
                float a = -INFINITY;
                if (j < kn) {
                    a = 0.f;
#pragma unroll
                    for (int c = 0; c < D; c += 4) {
                        const float4 kk = *reinterpret_cast<const float4*>(ks + j * KP + c);
                        const float4 qq = *reinterpret_cast<const float4*>(qw + c);
                        a += qq.x * kk.x + qq.y * kk.y + qq.z * kk.z + qq.w * kk.w;
                    }
                }
                sc[jj] = a;
                mx = fmaxf(mx, a);
            }
            mx = wave_max(mx);
            const float m_old = __shfl(m_all, i, 64);
            const float m_new = fmaxf(m_old, mx);
            const float alpha = atl_rescale(m_old, m_new);
            float den = 0.f;
#pragma unroll
            for (int jj = 0; jj < ATL_KT / 64; ++jj) {
                const int j = jj * 64 + lane;
                const float pv = j < kn ? expf(sc[jj] - m_new) : 0.f;
                pw[j] = pv;
                den += pv;
            }
            den = wave_sum(den);
            if (lane == i) {
                m_all = m_new;
                l_all = l_all * alpha + den;
            }
            __builtin_amdgcn_wave_barrier();
            // the tile's sum on its own, then into the running one: blocked summation, as a BLAS contraction over 5000 keys is
            // (one accumulator over all keys read 1.4e-6 rel rms at 5000 keys, 1.6 x the reference's own float32 error)
            float o = 0.f;
            if constexpr (D == 64) {
                for (int j = 0; j < kn; ++j) o += pw[j] * vs[j * D + lane];
            } else {
                const int c = lane & 31, half = lane >> 5;
                for (int j = half; j < kn; j += 2) o += pw[j] * vs[j * D + c];
            }
            os[ql * 64 + lane] = os[ql * 64 + lane] * alpha + o;
            __builtin_amdgcn_wave_barrier();
        }
    }
    for (int i = 0; i < QW; ++i) {
        const int ql = wv + ATL_WAVES * i;
        if (q0 + ql >= s) break;
        const float den = __shfl(l_all, i, 64);
        float o = os[ql * 64 + lane];
        if constexpr (D == 32) o += __shfl_xor(o, 32, 64);
        if (lane < D) stf<float>(out, ((long)b * s + q0 + ql) * e + h * D + lane, o / den);
    }
}

// ---- 16-bit MFMA: bf16 (X3 = 0) or fp16 pairs (X3 = 1)
// LDS per tile as in attention_mfma_kernel at 8 key tiles: K rows of 128 bytes (GEMM swizzle), V transposed and key-permuted
// (k-index 8g+e <-> key 32b + 16(e>>2) + 4g + (e&3) of the tile), hi planes and, in the split form, lo planes.
template <typename T, typename TO, int X3, int D>
__global__ void __launch_bounds__(ATL_THREADS) attention_long_mfma_kernel(const T* __restrict__ qkv, TO* __restrict__ out, int s, int heads,
                                                                           int nqb, float scale, unsigned* ovf) {
    static_assert(D == 64 || D == 32, "head dimension 64 (wav2vec2 layers, tl2) or 32 (tl1)");
    using Op = AttOp<X3>;
    using frag_t = typename Op::frag_t;
    using elem_t = typename Op::elem_t;
    constexpr int NKT = ATL_KT / 16;         // 16-key MFMA tiles per key tile
    constexpr int KS = D / 32;               // 32-wide K-steps of Q.K^T
    constexpr int TV = D / 16;               // 16-row tiles of V^T / O^T
    constexpr int VROW = ATL_KT * 2 + 16;    // bytes per V^T row (16-byte pad against bank conflicts)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* khi = smem_raw;                    // [ATL_KT][128 B]
    char* klo = khi + ATL_KT * 128;
    char* vhi = klo + (X3 ? ATL_KT * 128 : 0);  // [D][VROW]
    char* vlo = vhi + D * VROW;
    const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
    const int b = bh / heads, h = bh % heads;
    const int e = heads * D;
    const long rowstride = 3L * e;
    const T* base = qkv + (long)b * s * rowstride + h * D;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = lane >> 4, q16 = lane & 15;
    const int qrow = qb * ATL_QB + wv * 16 + q16;
    const bool wave_live = qb * ATL_QB + wv * 16 < s;  // wave-uniform: a wave without queries still stages tiles and meets the barriers
    float amax = 0.f;  // largest finite magnitude this thread split into an fp16 pair

    // ---- Q fragments (B operand): this lane's query row, head-dim 32ks + 8g .. +7, pre-scaled
    frag_t qh[KS], ql[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        float qv[8];
        if (qrow < s) {
            ld4<T>(base, (long)qrow * rowstride + 32 * ks + 8 * g, qv);
            ld4<T>(base, (long)qrow * rowstride + 32 * ks + 8 * g + 4, qv + 4);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) qv[j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) qv[j] *= scale;
        if constexpr (X3) {
            sp_split8(qv, amax, qh[ks], ql[ks]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) qh[ks][j] = (elem_t)qv[j];
        }
    }

    constexpr int ITEMS = ATL_KT * (D / 8), PASSES = ITEMS / ATL_THREADS;
    static_assert(ITEMS % ATL_THREADS == 0, "whole staging passes");
    float kvb[PASSES][8], vvb[PASSES][8];
    // the raw rows of key tile `kt` into registers (rows past s: zeros)
    auto fetch = [&](int kt) {
#pragma unroll
        for (int u = 0; u < PASSES; ++u) {
            const int it = u * ATL_THREADS + tid;
            const int r = kt * ATL_KT + it / (D / 8), c = it % (D / 8);
            if (r < s) {
                ld4<T>(base, (long)r * rowstride + e + 8 * c, kvb[u]);
                ld4<T>(base, (long)r * rowstride + e + 8 * c + 4, kvb[u] + 4);
                ld4<T>(base, (long)r * rowstride + 2 * e + 8 * c, vvb[u]);
                ld4<T>(base, (long)r * rowstride + 2 * e + 8 * c + 4, vvb[u] + 4);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) { kvb[u][j] = 0.f; vvb[u][j] = 0.f; }
            }
        }
    };

    float m = -INFINITY, l = 0.f;  // m: of the query's row (equal in its four lanes); l: this lane's part of the denominator
    att_f32x4_t oc[TV];
#pragma unroll
    for (int tv = 0; tv < TV; ++tv) oc[tv] = att_f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int nkt = (s + ATL_KT - 1) / ATL_KT;
    fetch(0);
    for (int kt = 0; kt < nkt; ++kt) {
        const int k0 = kt * ATL_KT;
        __syncthreads();  // the tile before has been read by every wave
        // ---- stage K (row-major) and V (transposed + permuted) as 16-bit planes
#pragma unroll
        for (int u = 0; u < PASSES; ++u) {
            const int it = u * ATL_THREADS + tid;
            const int r = it / (D / 8), c = it % (D / 8);   // key row of the tile, chunk of 8 head-dim elements (K rows keep a 128-byte pitch)
            const int kpos = (r >> 5) * 32 + ((r & 15) >> 2) * 8 + ((r >> 4) & 1) * 4 + (r & 3);
            if constexpr (X3) {  // fp16 pairs (split_dev.h); amax: their range contract
                uint4 hw, lw;
                sp_split8(kvb[u], amax, hw, lw);
                *reinterpret_cast<uint4*>(khi + att_swz(r, c)) = hw;
                *reinterpret_cast<uint4*>(klo + att_swz(r, c)) = lw;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    uint16_t hv, lv;
                    sp_split1(vvb[u][j], amax, hv, lv);
                    *reinterpret_cast<uint16_t*>(vhi + (8 * c + j) * VROW + kpos * 2) = hv;
                    *reinterpret_cast<uint16_t*>(vlo + (8 * c + j) * VROW + kpos * 2) = lv;
                }
            } else {
                uint32_t hw[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) hw[j] = (uint32_t)Op::bits(kvb[u][2 * j]) | ((uint32_t)Op::bits(kvb[u][2 * j + 1]) << 16);
                *reinterpret_cast<uint4*>(khi + att_swz(r, c)) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
#pragma unroll
                for (int j = 0; j < 8; ++j) *reinterpret_cast<uint16_t*>(vhi + (8 * c + j) * VROW + kpos * 2) = Op::bits(vvb[u][j]);
            }
        }
        __syncthreads();
        if (kt + 1 < nkt) fetch(kt + 1);  // in flight while this tile is computed
        if (!wave_live) continue;
        // ---- scores^T: key tiles x this query tile
        att_f32x4_t sc[NKT];
#pragma unroll
        for (int t = 0; t < NKT; ++t) {
            sc[t] = att_f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int off = att_swz(t * 16 + q16, ks * 4 + g);
                const frag_t kh = *reinterpret_cast<const frag_t*>(khi + off);
                if (X3) {
                    const frag_t kl = *reinterpret_cast<const frag_t*>(klo + off);
                    sc[t] = Op::mfma(kl, qh[ks], sc[t]);
                    sc[t] = Op::mfma(kh, ql[ks], sc[t]);
                }
                sc[t] = Op::mfma(kh, qh[ks], sc[t]);
            }
        }
        // ---- running softmax (register r of tile t is key k0 + 16t + 4g + r); keys past s contribute nothing
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NKT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (k0 + 16 * t + 4 * g + r >= s) sc[t][r] = -INFINITY;
                mx = fmaxf(mx, sc[t][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);
        const float alpha = atl_rescale(m, m_new);
        m = m_new;
        float den = 0.f;
#pragma unroll
        for (int t = 0; t < NKT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = (k0 + 16 * t + 4 * g + r < s) ? expf(sc[t][r] - m_new) : 0.f;
                sc[t][r] = pv;
                den += pv;
            }
        l = l * alpha + den;
        // ---- this tile's O^T = V^T . P^T over key blocks of 32, in accumulators of its own: blocked summation over the key
        // tiles, as in the f32 form
        att_f32x4_t ot[TV];
#pragma unroll
        for (int tv = 0; tv < TV; ++tv) ot[tv] = att_f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < NKT / 2; ++kb) {
            frag_t ph, pl;
            float pmax = 0.f;  // never read: probabilities are at most 1
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (X3) {
                    spe_t hh, ll;
                    sp_split1(sc[2 * kb + (j >> 2)][j & 3], pmax, hh, ll);
                    ph[j] = hh;
                    pl[j] = ll;
                } else {
                    ph[j] = (elem_t)sc[2 * kb + (j >> 2)][j & 3];
                }
            }
#pragma unroll
            for (int tv = 0; tv < TV; ++tv) {
                const int off = (tv * 16 + q16) * VROW + (kb * 4 + g) * 16;
                const frag_t vh = *reinterpret_cast<const frag_t*>(vhi + off);
                if (X3) {
                    const frag_t vl = *reinterpret_cast<const frag_t*>(vlo + off);
                    ot[tv] = Op::mfma(vl, ph, ot[tv]);
                    ot[tv] = Op::mfma(vh, pl, ot[tv]);
                }
                ot[tv] = Op::mfma(vh, ph, ot[tv]);
            }
        }
#pragma unroll
        for (int tv = 0; tv < TV; ++tv)
#pragma unroll
            for (int r = 0; r < 4; ++r) oc[tv][r] = oc[tv][r] * alpha + ot[tv][r];
    }
    // ---- normalise and store: registers of tile tv are head-dim 16tv + 4g + r of query lane&15
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (qrow < s) {
        const float inv = 1.f / l;
#pragma unroll
        for (int tv = 0; tv < TV; ++tv) {
            float o4[4] = {oc[tv][0] * inv, oc[tv][1] * inv, oc[tv][2] * inv, oc[tv][3] * inv};
            st4<TO>(out, ((long)b * s + qrow) * e + h * D + 16 * tv + 4 * g, o4, ovf);
        }
    }
    if (X3) sp_count_now(ovf, amax);
}

}  // namespace

// in_kind: storage of qkv (0 f32, 1 bf16); out_kind: storage of the context vectors (0 f32, 1 bf16, 2 sp32)
int k_attention_long(avcer_ctx* ctx, const void* qkv, void* out, int n, int s, int heads, int d, float scale, int in_kind,
                     int out_kind, hipStream_t st) {
    if (s > AVCER_AUDIO_MAX_TOKENS || s < 1) return set_err(ctx, AVCER_EINVAL, "attention_long: S=%d outside [1,%d]", s, AVCER_AUDIO_MAX_TOKENS);
    if (d != 32 && d != 64) return set_err(ctx, AVCER_EINVAL, "attention_long: head dim %d", d);
    if (in_kind == 2 || (in_kind == 1) != (out_kind == 1))
        return set_err(ctx, AVCER_EINVAL, "attention_long: unsupported storage combination %d -> %d", in_kind, out_kind);
    const int nqb = cdiv(s, ATL_QB);
    const long blocks = (long)n * heads * nqb;
    if (blocks > 2147483647L) return set_err(ctx, AVCER_EINVAL, "attention_long: %ld workgroups: split the batch", blocks);
    const int grid = (int)blocks;
    if (in_kind == 1 || out_kind == 2) {
        const int x3 = out_kind == 2;
        const size_t lds_m = (size_t)ATL_KT * 128 * (x3 ? 2 : 1) + (size_t)d * (ATL_KT * 2 + 16) * (x3 ? 2 : 1);
#define ATLM(T, TO, X3, D)                                                                                                        \
    do {                                                                                                                          \
        TRY((big_lds_once<attention_long_mfma_kernel<T, TO, X3, D>>(ctx)));                                                       \
        attention_long_mfma_kernel<T, TO, X3, D><<<grid, ATL_THREADS, lds_m, st>>>((const T*)qkv, (TO*)out, s, heads, nqb, scale, ctx->ovf); \
    } while (0)
        if (x3) { if (d == 64) ATLM(float, sp32_t, 1, 64); else ATLM(float, sp32_t, 1, 32); }
        else { if (d == 64) ATLM(bf16_t, bf16_t, 0, 64); else ATLM(bf16_t, bf16_t, 0, 32); }
#undef ATLM
        CHECK_LAUNCH(ctx, "attention_long_mfma");
        return AVCER_OK;
    }
    const size_t lds = ((size_t)ATL_KT * (d + 4) + (size_t)ATL_KT * d + (size_t)ATL_QB * d + (size_t)ATL_QB * 64 + ATL_WAVES * ATL_KT) * sizeof(float);
    if (d == 64) {
        TRY(big_lds_once<attention_long_f32_kernel<64>>(ctx));
        attention_long_f32_kernel<64><<<grid, ATL_THREADS, lds, st>>>((const float*)qkv, (float*)out, s, heads, nqb, scale);
    } else {
        TRY(big_lds_once<attention_long_f32_kernel<32>>(ctx));
        attention_long_f32_kernel<32><<<grid, ATL_THREADS, lds, st>>>((const float*)qkv, (float*)out, s, heads, nqb, scale);
    }
    CHECK_LAUNCH(ctx, "attention_long");
    return AVCER_OK;
}
