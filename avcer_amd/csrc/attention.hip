// softmax(q k^T * scale) v of the AVCER hot path (gfx950): the whole-head kernels (S <= 256: one head's K and V stay in LDS) and the
// streamed-key kernels (any S up to AVCER_AUDIO_MAX_TOKENS: key tiles pass through LDS under a running softmax).
//   ref: wav2vec2 encoder self-attention (16 x 64) and architectures/attention_layers.py:10-38,80-144 (32 x 32, 16 x 64);
//        transformers Wav2Vec2Attention (eager): no length limit of their own.
//
// Three arithmetic forms, each with a whole-head and a streamed kernel:
//   attention_kernel / attention_long_f32_kernel     f32 in, f32 out, exact f32 on the VALU
//   attention_mfma_kernel / attention_long_mfma_kernel
//                                X3 = 0: bf16 in, bf16 out, bf16 operands on the MFMA
//                                X3 = 1: f32 in, sp32 out, every product as hi.hi + hi.lo + lo.hi of fp16 pairs (f32-grade, as
//                                conv_gemm MODE 2/3; split_dev.h: scores and exponentials are O(1), nothing here needs a scale)
// The two MFMA kernels share the operand types, the K swizzle, the V row pitch, the LDS size, the score contraction (att_scores)
// and the epilogue (att_store).  Their Q fragments, K / V fetch and staging, masked softmax and P V blocks, and the scores,
// exponentials and P V loop of the two f32 kernels, are still the SAME TEXT TWICE (marked "twin:" below; change both): moved
// into functions, each MFMA block changes what hipcc makes of attention_mfma_kernel -- the x3 d64 form at 16 key tiles goes from
// 123 VGPRs to 167-182 and from 4 waves per SIMD to 3 or 2, its SGPR spills from 97 to 101-198 --, and the f32 functions made
// attention_long_f32_kernel<64> 8-9 % slower at every length ("One attention source").
// What differs by design is how keys reach LDS and what surrounds a tile: the whole-head kernels issue every global load of the
// block before the first wait and loop over query tiles; the streamed ones prefetch the next key tile and carry a running
// maximum, denominator and rescaled accumulators.
#include "act_io.h"

#include <cmath>
#include <type_traits>

namespace {

// More than 64 KiB of dynamic LDS is an attribute of the kernel PER DEVICE: raised to the chip's 160 KiB before KERNEL's first
// launch on the context's device (one bit per device index), then the launch
template <auto KERNEL, typename... A>
int att_launch(avcer_ctx* ctx, int grid, int threads, size_t lds, hipStream_t st, A... args) {
    static uint64_t done = 0;
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (!(done & bit)) {
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        done |= bit;
    }
    KERNEL<<<grid, threads, lds, st>>>(args...);
    return AVCER_OK;
}

// ================================================================================================ exact f32 on the VALU
// K rows are padded by 4 floats (conflict-free b128 row reads); a wave takes one query at a time, lanes over the keys.
// twin: the scores, the exponentials into the wave's weight row and the P V loop of attention_kernel and attention_long_f32_kernel

// ---- whole head: one (batch, head) per workgroup; S <= 256
// K and V live in LDS as f32; each wave owns query rows.
// 8 waves share one head's K/V image (~105 KiB f32 at S=199): two waves per SIMD hide the LDS latency of the score loop
constexpr int ATT_WAVES = 8;
constexpr int ATT_THREADS = ATT_WAVES * 64;
template <int D>
__global__ void __launch_bounds__(ATT_THREADS) attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, int s, int heads,
                                                      float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int KP = D + 4;
    float* ks = reinterpret_cast<float*>(smem_raw);           // [s][KP]
    float* vs = ks + (long)s * KP;                            // [s][D]
    float* ps = vs + (long)s * D;                             // [ATT_WAVES][256]
    float* qs = ps + ATT_WAVES * 256;                         // [ATT_WAVES][D]
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int e = heads * D;
    const long rowstride = 3L * e;
    const float* base = qkv + (long)b * s * rowstride + h * D;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < s * (D / 4); i += ATT_THREADS) {
        const int r = i / (D / 4), c4 = (i % (D / 4)) * 4;
        float kv[4], vv[4];
        ld4<float>(base, (long)r * rowstride + e + c4, kv);
        ld4<float>(base, (long)r * rowstride + 2 * e + c4, vv);
        *reinterpret_cast<float4*>(ks + r * KP + c4) = make_float4(kv[0], kv[1], kv[2], kv[3]);
        *reinterpret_cast<float4*>(vs + r * D + c4) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    }
    __syncthreads();
    float* pw = ps + wv * 256;
    float* qw = qs + wv * D;
    for (int qi = wv; qi < s; qi += ATT_WAVES) {
        if (lane < D) qw[lane] = ldf<float>(base, (long)qi * rowstride + lane) * scale;
        __builtin_amdgcn_wave_barrier();
        float sc[4];
        float mx = -INFINITY;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = jj * 64 + lane;
            float a = -INFINITY;
            if (j < s) {
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
        float den = 0.f;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = jj * 64 + lane;
            const float pv = j < s ? expf(sc[jj] - mx) : 0.f;
            pw[j] = pv;
            den += pv;
        }
        den = wave_sum(den);
        __builtin_amdgcn_wave_barrier();
        float o = 0.f;
        if constexpr (D == 64) {
            for (int j = 0; j < s; ++j) o += pw[j] * vs[j * D + lane];
        } else {
            const int c = lane & 31, half = lane >> 5;
            for (int j = half; j < s; j += 2) o += pw[j] * vs[j * D + c];
            o += __shfl_xor(o, 32, 64);
        }
        if (lane < D) stf<float>(out, ((long)b * s + qi) * e + h * D + lane, o / den);
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- streamed keys: one workgroup (8 waves) per (window, head, block of ATL_QB = 128 queries): a single 100 s window of 16 heads
// is 640 workgroups, not 16.  Keys pass through LDS in tiles of ATL_KT = 128 (one tile's K and V image; the f32 form: 66 KiB,
// the x3 form: 66.5 KiB), and every query row keeps a running maximum m, a running denominator l and accumulators that are
// multiplied by exp(m_old - m_new) whenever a tile raises the maximum (the textbook order: the factor is applied to O and l
// BEFORE the tile's exponentials, which are taken against m_new, are added; a tile's P V sum is formed on its own and then
// added: blocked summation).  Keys of the tail tile past s are masked: their score is -inf, their weight exactly 0.
// Every loop is counted (ceil(s / 128) tiles), and no workgroup waits for another.
constexpr int ATL_WAVES = 8;
constexpr int ATL_THREADS = 64 * ATL_WAVES;
constexpr int ATL_KT = AVCER_ATT_LONG_KT;  // keys per tile
constexpr int ATL_QB = AVCER_ATT_LONG_QB;  // queries per workgroup
static_assert(ATL_KT == 128 && ATL_QB == 16 * ATL_WAVES, "eight 16-key MFMA tiles per key tile; one 16-query MFMA tile per wave");

// the factor that brings sums taken against the maximum m_old to the maximum m_new >= m_old.  m_old == m_new also covers
// -inf == -inf (nothing seen yet, or only NaN scores: fmaxf skips them), where exp(m_old - m_new) would be exp(NaN)
__device__ __forceinline__ float atl_rescale(float m_old, float m_new) { return m_old == m_new ? 1.f : expf(m_old - m_new); }

// LDS: K tile, V tile, the block's 128 pre-scaled query rows, their unnormalised outputs (64 floats a query: d = 64 one per lane,
// d = 32 the two half-waves' partial sums), one row of weights per wave.
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

// ================================================================================================ 16-bit MFMA
// K is kept in LDS as 16-bit rows of 128 bytes (GEMM swizzle; fp16 in the x3 form, bf16 else), V transposed and key-permuted,
// both as hi (+ lo in the split mode) planes, for NKT 16-key tiles.  Each wave takes 16-query tiles:
//   S^T tile = K . Q^T   (swapped operands: a lane then holds, for ONE query lane&15, the keys 16t + 4(lane>>4) + r)
//   softmax over keys     in-lane over its registers + 2 shuffles across the four lane groups
//   O^T tile = V^T . P^T  the exponentiated accumulators of key tiles (2b, 2b+1) ARE the B operand of the PV MFMA for
//                         key block b once V^T is stored with k-index 8g+e <-> key 32b + 16(e>>2) + 4g + (e&3)
// Throughout: g = lane >> 4, q16 = lane & 15; amax: the largest finite magnitude this thread split into an fp16 pair (the
// range contract of split_dev.h).
typedef __attribute__((ext_vector_type(8))) __bf16 att_bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float att_f32x4_t;
// operand element by arithmetic: the split type (fp16) in the x3 form, bf16 in the plain form
template <int X3> struct AttOp {
    typedef spe_t elem_t;
    typedef spx8_t frag_t;
    static __device__ __forceinline__ att_f32x4_t mfma(const frag_t a, const frag_t b, const att_f32x4_t c) { return mfma_sp(a, b, c); }
};
template <> struct AttOp<0> {
    typedef __bf16 elem_t;
    typedef att_bf16x8_t frag_t;
    static __device__ __forceinline__ uint16_t bits(float f) { return f2bf(f); }
    static __device__ __forceinline__ att_f32x4_t mfma(const frag_t a, const frag_t b, const att_f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

// byte offset of 16-byte chunk `chunk` of key row `row` in a K plane
__device__ __forceinline__ int att_swz(int row, int chunk) {
    return row * 128 + ((chunk ^ (int)((0x32765410u >> (((row >> 1) & 7) * 4)) & 7u)) << 4);
}
// bytes per V^T row of an image of NKT key tiles (16-byte pad against bank conflicts)
constexpr int att_vrow(int nkt) { return nkt * 32 + 16; }
// bytes of the K and V planes of `keys` keys (a multiple of 16): what the kernels below carve, what their launchers ask for
constexpr size_t att_mfma_lds(int keys, int d, int x3) { return ((size_t)keys * 128 + (size_t)d * att_vrow(keys / 16)) * (x3 ? 2 : 1); }

// scores^T: the image's key tiles x this lane's query; register r of tile t is key 16t + 4g + r of the image
template <int X3, int D, int NKT>
__device__ __forceinline__ void att_scores(const char* khi, const char* klo, const typename AttOp<X3>::frag_t (&qh)[D / 32],
                                           const typename AttOp<X3>::frag_t (&ql)[D / 32], int q16, int g, att_f32x4_t (&sc)[NKT]) {
    using Op = AttOp<X3>;
    using frag_t = typename Op::frag_t;
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
        sc[t] = att_f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < D / 32; ++ks) {
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
}

// normalise and store: registers of tile tv are head-dim 16tv + 4g + r of query lane&15, whose row of `out` starts at `row`
template <typename TO, int D>
__device__ __forceinline__ void att_store(TO* out, long row, const att_f32x4_t (&o)[D / 16], float den, int g, unsigned* ovf) {
    const float inv = 1.f / den;
#pragma unroll
    for (int tv = 0; tv < D / 16; ++tv) {
        float o4[4] = {o[tv][0] * inv, o[tv][1] * inv, o[tv][2] * inv, o[tv][3] * inv};
        st4<TO>(out, row + 16 * tv + 4 * g, o4, ovf);
    }
}

// ---- whole head: one workgroup (8 waves) per (window, head), an image of NKT * 16 >= s keys
constexpr int ATTM_WAVES = 8;  // one query tile per wave at 99 tokens (7 tiles): the four-wave form ran two rounds of 2 / 2 / 2 / 1
template <typename T, typename TO, int NKT, int X3, int D>
__global__ void __launch_bounds__(64 * ATTM_WAVES) attention_mfma_kernel(const T* __restrict__ qkv, TO* __restrict__ out, int s, int heads,
                                                           float scale, unsigned* ovf) {
    static_assert(D == 64 || D == 32, "head dimension 64 (wav2vec2 layers, tl2) or 32 (tl1)");
    using Op = AttOp<X3>;
    using frag_t = typename Op::frag_t;
    using elem_t = typename Op::elem_t;
    constexpr int KS = D / 32;               // 32-wide K-steps of Q.K^T
    constexpr int TV = D / 16;               // 16-row tiles of V^T / O^T
    constexpr int SP = NKT * 16;             // padded key count
    constexpr int VROW = att_vrow(NKT);      // bytes per V^T row
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* khi = smem_raw;                    // [SP][128 B]
    char* klo = khi + SP * 128;
    char* vhi = klo + (X3 ? SP * 128 : 0);   // [D][VROW]
    char* vlo = vhi + D * VROW;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int e = heads * D;
    const long rowstride = 3L * e;
    const T* base = qkv + (long)b * s * rowstride + h * D;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = lane >> 4, q16 = lane & 15;

    // Every global load of the block is issued before the first one is needed: a block is a chain of HBM round trips
    // otherwise (four staging passes, then one per query tile: ~6 x 2.5 us against ~4 us of arithmetic -- the launch ran at
    // a third of its present speed).  First the query rows of this wave's tiles (tile wv, wv + 8, ...), raw; then K / V in
    // batches of up to four staging passes.
    const int nqt = (s + 15) >> 4;
    constexpr int NTHR = 64 * ATTM_WAVES;
    constexpr int QI = NKT / ATTM_WAVES;     // query tiles per wave
    float qraw[QI][KS][8];
#pragma unroll
    for (int qi = 0; qi < QI; ++qi) {
        const int qrow = (wv + ATTM_WAVES * qi) * 16 + q16;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (qrow < s) {
                ld4<T>(base, (long)qrow * rowstride + 32 * ks + 8 * g, qraw[qi][ks]);
                ld4<T>(base, (long)qrow * rowstride + 32 * ks + 8 * g + 4, qraw[qi][ks] + 4);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) qraw[qi][ks][j] = 0.f;
            }
        }
    }
    // ---- (twin: attention_long_mfma_kernel's fetch and staging) stage K (row-major) and V (transposed + permuted) as 16-bit planes
    constexpr int ITEMS = SP * (D / 8), PASSES = ITEMS / NTHR, UB = PASSES < 4 ? PASSES : 4;
    static_assert(ITEMS % NTHR == 0 && PASSES % UB == 0 && NKT % ATTM_WAVES == 0, "whole staging passes, whole batches");
    float amax = 0.f;  // largest finite magnitude this thread split into an fp16 pair
    for (int p0 = 0; p0 < PASSES; p0 += UB) {
    float kvb[UB][8], vvb[UB][8];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
        const int it = (p0 + u) * NTHR + tid;
        const int r = it / (D / 8), c = it % (D / 8);
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
#pragma unroll
    for (int u = 0; u < UB; ++u) {
        const int it = (p0 + u) * NTHR + tid;
        const int r = it / (D / 8), c = it % (D / 8);   // key row, chunk of 8 head-dim elements (K rows keep a 128-byte pitch)
        // V^T: key r sits at k-position (r>>5)*32 + ((r&15)>>2)*8 + ((r>>4)&1)*4 + (r&3) of every head-dim row
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
    }
    __syncthreads();

#pragma unroll
    for (int qi = 0; qi < QI; ++qi) {
        const int tq = wv + ATTM_WAVES * qi;
        if (tq >= nqt) break;
        const int qrow = tq * 16 + q16;
        // ---- Q fragments (B operand): this lane's query row, head-dim 32ks + 8g .. +7, pre-scaled (twin: attention_long_mfma_kernel)
        frag_t qh[KS], ql[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            float qv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) qv[j] = qraw[qi][ks][j] * scale;
            if constexpr (X3) {
                sp_split8(qv, amax, qh[ks], ql[ks]);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) qh[ks][j] = (elem_t)qv[j];
            }
        }
        // ---- scores^T: key tiles x this query tile
        att_f32x4_t sc[NKT];
        att_scores<X3, D>(khi, klo, qh, ql, q16, g, sc);
        // ---- (twin: attention_long_mfma_kernel) softmax over keys (register r of tile t is key 16t + 4g + r); padded keys contribute nothing
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NKT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (16 * t + 4 * g + r >= s) sc[t][r] = -INFINITY;
                mx = fmaxf(mx, sc[t][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float den = 0.f;
#pragma unroll
        for (int t = 0; t < NKT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = (16 * t + 4 * g + r < s) ? expf(sc[t][r] - mx) : 0.f;
                sc[t][r] = pv;
                den += pv;
            }
        den += __shfl_xor(den, 16, 64);
        den += __shfl_xor(den, 32, 64);
        // ---- (twin: attention_long_mfma_kernel) O^T = V^T . P^T over key blocks of 32
        att_f32x4_t oc[TV];
#pragma unroll
        for (int tv = 0; tv < TV; ++tv) oc[tv] = att_f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < NKT / 2; ++kb) {
            frag_t ph, pl;
            // element by element from the accumulators: through a float[8] copy and sp_split8 the 16-key-tile forms need 27 / 58
            // more VGPRs and lose an occupancy step
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
                    oc[tv] = Op::mfma(vl, ph, oc[tv]);
                    oc[tv] = Op::mfma(vh, pl, oc[tv]);
                }
                oc[tv] = Op::mfma(vh, ph, oc[tv]);
            }
        }
        if (qrow < s) att_store<TO, D>(out, ((long)b * s + qrow) * e + h * D, oc, den, g, ovf);
    }
    if (X3) sp_count_now(ovf, amax);
}

// ---- streamed keys: the workgroups and the running softmax of attention_long_f32_kernel, one key tile's image (NKT = 8) at a
// time; the next tile's global loads are in flight while the present one is computed.
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
    constexpr int VROW = att_vrow(NKT);      // bytes per V^T row
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

    // ---- Q fragments (B operand): this lane's query row, head-dim 32ks + 8g .. +7, pre-scaled (twin: attention_mfma_kernel)
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
        // ---- (twin: attention_mfma_kernel) stage K (row-major) and V (transposed + permuted) as 16-bit planes
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
        att_scores<X3, D>(khi, klo, qh, ql, q16, g, sc);
        // ---- (twin: attention_mfma_kernel) running softmax (register r of tile t is key k0 + 16t + 4g + r); keys past s contribute nothing
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
        // ---- (twin: attention_mfma_kernel) this tile's O^T = V^T . P^T over key blocks of 32, in accumulators of its own: blocked summation over the key
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
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (qrow < s) att_store<TO, D>(out, ((long)b * s + qrow) * e + h * D, oc, l, g, ovf);
    if (X3) sp_count_now(ovf, amax);
}

// ================================================================================================ launchers
// what k_attention and k_attention_long require alike; `who` prefixes the message
int att_check(avcer_ctx* ctx, const char* who, int s, int s_max, int d, int in_kind, int out_kind) {
    if (s > s_max || s < 1) return set_err(ctx, AVCER_EINVAL, "%s: S=%d outside [1,%d]", who, s, s_max);
    if (d != 32 && d != 64) return set_err(ctx, AVCER_EINVAL, "%s: head dim %d", who, d);
    if (in_kind == 2 || (in_kind == 1) != (out_kind == 1))
        return set_err(ctx, AVCER_EINVAL, "%s: unsupported storage combination %d -> %d", who, in_kind, out_kind);
    return AVCER_OK;
}

// f(T, TO, X3, D) with the template arguments of an MFMA kernel as values: input and output element, arithmetic, head dimension
template <typename F>
int att_mfma_dispatch(int x3, int d, F&& f) {
    const auto with_d = [&](auto t, auto to, auto x) {
        return d == 64 ? f(t, to, x, std::integral_constant<int, 64>{}) : f(t, to, x, std::integral_constant<int, 32>{});
    };
    return x3 ? with_d(float{}, sp32_t{}, std::integral_constant<int, 1>{}) : with_d(bf16_t{}, bf16_t{}, std::integral_constant<int, 0>{});
}

}  // namespace

// in_kind: storage of qkv (0 f32, 1 bf16); out_kind: storage of the context vectors (0 f32, 1 bf16, 2 sp32)
int k_attention(avcer_ctx* ctx, const void* qkv, void* out, int n, int s, int heads, int d, float scale, int in_kind,
                int out_kind, hipStream_t st) {
    TRY(att_check(ctx, "attention", s, 256, d, in_kind, out_kind));
    const int grid = n * heads;
    // bf16 / split-fp16 modes: QK^T and PV on the MFMA, 64- and 32-wide heads (the f32 mode keeps exact f32 arithmetic)
    if (in_kind == 1 || out_kind == 2) {
        const int x3 = out_kind == 2, nkt = s <= 128 ? 8 : 16;
        const size_t lds_m = att_mfma_lds(nkt * 16, d, x3);
        TRY(att_mfma_dispatch(x3, d, [&](auto t, auto to, auto X3, auto D) {
            using T = decltype(t);
            using TO = decltype(to);
            if (nkt == 8)
                return att_launch<attention_mfma_kernel<T, TO, 8, X3(), D()>>(ctx, grid, 64 * ATTM_WAVES, lds_m, st, (const T*)qkv, (TO*)out,
                                                                              s, heads, scale, ctx->ovf);
            return att_launch<attention_mfma_kernel<T, TO, 16, X3(), D()>>(ctx, grid, 64 * ATTM_WAVES, lds_m, st, (const T*)qkv, (TO*)out, s,
                                                                           heads, scale, ctx->ovf);
        }));
        CHECK_LAUNCH(ctx, "attention_mfma");
        return AVCER_OK;
    }
    const size_t lds = ((size_t)s * (d + 4) + (size_t)s * d + ATT_WAVES * 256 + ATT_WAVES * d) * sizeof(float);
    if (d == 64) TRY(att_launch<attention_kernel<64>>(ctx, grid, ATT_THREADS, lds, st, (const float*)qkv, (float*)out, s, heads, scale));
    else TRY(att_launch<attention_kernel<32>>(ctx, grid, ATT_THREADS, lds, st, (const float*)qkv, (float*)out, s, heads, scale));
    CHECK_LAUNCH(ctx, "attention");
    return AVCER_OK;
}

int k_attention_long(avcer_ctx* ctx, const void* qkv, void* out, int n, int s, int heads, int d, float scale, int in_kind,
                     int out_kind, hipStream_t st) {
    TRY(att_check(ctx, "attention_long", s, AVCER_AUDIO_MAX_TOKENS, d, in_kind, out_kind));
    const int nqb = cdiv(s, ATL_QB);
    const long blocks = (long)n * heads * nqb;
    if (blocks > 2147483647L) return set_err(ctx, AVCER_EINVAL, "attention_long: %ld workgroups: split the batch", blocks);
    const int grid = (int)blocks;
    if (in_kind == 1 || out_kind == 2) {
        const int x3 = out_kind == 2;
        TRY(att_mfma_dispatch(x3, d, [&](auto t, auto to, auto X3, auto D) {
            using T = decltype(t);
            using TO = decltype(to);
            return att_launch<attention_long_mfma_kernel<T, TO, X3(), D()>>(ctx, grid, ATL_THREADS, att_mfma_lds(ATL_KT, d, x3), st,
                                                                            (const T*)qkv, (TO*)out, s, heads, nqb, scale, ctx->ovf);
        }));
        CHECK_LAUNCH(ctx, "attention_long_mfma");
        return AVCER_OK;
    }
    const size_t lds = ((size_t)ATL_KT * (d + 4) + (size_t)ATL_KT * d + (size_t)ATL_QB * d + (size_t)ATL_QB * 64 + ATL_WAVES * ATL_KT) * sizeof(float);
    if (d == 64) TRY(att_launch<attention_long_f32_kernel<64>>(ctx, grid, ATL_THREADS, lds, st, (const float*)qkv, (float*)out, s, heads, nqb, scale));
    else TRY(att_launch<attention_long_f32_kernel<32>>(ctx, grid, ATL_THREADS, lds, st, (const float*)qkv, (float*)out, s, heads, nqb, scale));
    CHECK_LAUNCH(ctx, "attention_long");
    return AVCER_OK;
}
