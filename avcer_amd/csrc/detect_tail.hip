// The tail of the two face detectors, RetinaFace (retina_face_predictor.py:70-108 with box_utils.py:210-249 and py_cpu_nms.py:11-39)
// and S3FD (s3fd/utils.py:6-24, :94-171 with s3fd_predictor.py:56-64): decode every prior's box, order the candidates by score,
// greedy NMS, top-k, final threshold.  gfx950 only.  The two tails differ in the width of a row (RetinaFace 15 floats: box in pixels,
// score, five landmarks; S3FD 5: box in NORMALISED coordinates, score), in the "+1 pixel" of RetinaFace's widths and areas, and in
// S3FD's scaling to pixels on the way out; everything else is stated once here.  f32 arithmetic in torch's / numpy's evaluation order
// with contraction off, so only expf may differ (<= 2 ulp) and the keep decisions are the reference's.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ decode
// box_utils.py:210-228 = utils.py:6-24: a prior (cx, cy, w, h) and its regression -> the corners x0, y0, x1, y1 in normalised coordinates
__device__ __forceinline__ float4 decode_box(float4 pr, float4 l, float var0, float var1) {
#pragma clang fp contract(off)
    const float cx = pr.x + (l.x * var0) * pr.z;
    const float cy = pr.y + (l.y * var0) * pr.w;
    const float w = pr.z * expf(l.z * var1);
    const float h = pr.w * expf(l.w * var1);
    const float x0 = cx - w / 2.0f, y0 = cy - h / 2.0f;
    return make_float4(x0, y0, w + x0, h + y0);
}

// every prior's box, score and five landmarks in pixels -> dets [T, P, 15]; grid.y = frame, the priors are shared
__global__ void face_decode_kernel(const float* __restrict__ loc, const float* __restrict__ conf,
                                   const float* __restrict__ landms, const float* __restrict__ priors, int P, float im_w,
                                   float im_h, float var0, float var1, float* __restrict__ dets) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    {
        const long f = blockIdx.y;
        loc += f * P * 4; conf += f * P * 2; landms += f * P * 10; dets += f * P * 15;
    }
    const float4 pr = *reinterpret_cast<const float4*>(priors + 4L * i);
    const float4 b = decode_box(pr, *reinterpret_cast<const float4*>(loc + 4L * i), var0, var1);
    float* o = dets + 15L * i;
    o[0] = b.x * im_w;
    o[1] = b.y * im_h;
    o[2] = b.z * im_w;
    o[3] = b.w * im_h;
    o[4] = conf[2L * i + 1];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        o[5 + 2 * k] = (pr.x + (landms[10L * i + 2 * k] * var0) * pr.z) * im_w;
        o[6 + 2 * k] = (pr.y + (landms[10L * i + 2 * k + 1] * var0) * pr.w) * im_h;
    }
}

// every prior's normalised box and its score -> dets [T, P, 5]
__global__ void s3fd_decode_kernel(const float* __restrict__ loc, const float* __restrict__ conf, const float* __restrict__ priors, int P,
                                   float var0, float var1, float* __restrict__ dets) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const long r = (long)blockIdx.y * P + i;
    const float4 b = decode_box(*reinterpret_cast<const float4*>(priors + 4L * i), *reinterpret_cast<const float4*>(loc + r * 4), var0, var1);
    float* o = dets + r * 5;
    o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w;
    o[4] = conf[r * 2 + 1];
}

// ------------------------------------------------------------------------------------------------ order
// The visiting order of py_cpu_nms / nms_np (`scores.argsort()[: -top_k - 1 : -1]`: an ascending sort read backwards, so wherever
// that sort keeps tied scores in index order -- numpy's default does on short arrays, `kind="stable"` always -- ties are visited
// HIGHER prior index first; that is the rule here) of the candidates `score > conf_thresh` (strict in both references):
// order [T, nms_top_k] = prior index by rank, count [T] = candidates.
//
// A candidate's key: the score's bits made monotone (sign flip) in the high word, prior index + 1 in the low word, so descending
// keys are that order, every key is distinct, and 0 is no key (it pads a sort and sinks).
__device__ __forceinline__ unsigned long long score_key(float score, int prior) {
    unsigned v = __float_as_uint(score);
    if (v == 0x80000000u) v = 0u;  // -0.0 == +0.0 is a tie for numpy and for the counting kernel: index order decides, not the sign bit
    v = (v & 0x80000000u) ? ~v : (v | 0x80000000u);
    return ((unsigned long long)v << 32) | (unsigned)(prior + 1);
}
__device__ __forceinline__ int key_prior(unsigned long long key) { return (int)(unsigned)(key & 0xffffffffu) - 1; }

constexpr int ORDER_THREADS = 1024;
constexpr int ORDER_LDS = 16384;  // keys held in LDS (128 KiB)

// Bitonic sort, descending, of N keys in LDS (N a power of two, 64 .. ORDER_LDS).  NPT > 0: N = 2048 NPT, NPT compare-exchanges per
// thread and pass, fully unrolled and branch-free, so that a pass is NPT pairs of LDS reads in flight at once instead of a chain of
// dependent round trips.  NPT = 0: N = n < 2048, the threads below N / 2 take one exchange each.
template <int NPT>
__device__ __forceinline__ void bitonic_desc(unsigned long long* key, int n, int tid) {
    constexpr int U = NPT ? NPT : 1;
    const int N = NPT ? 2 * ORDER_THREADS * NPT : n;
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (NPT || tid < N / 2) {
                unsigned long long ka[U], kb[U];
                int ia[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int t = tid + u * ORDER_THREADS;
                    ia[u] = 2 * t - (t & (j - 1));
                    ka[u] = key[ia[u]];
                    kb[u] = key[ia[u] + j];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    // descending runs where bit k of the position is clear: the whole array at k = N
                    const bool sw = ((ia[u] & k) == 0) ? ka[u] < kb[u] : ka[u] > kb[u];
                    key[ia[u]] = sw ? kb[u] : ka[u];
                    key[ia[u] + j] = sw ? ka[u] : kb[u];
                }
            }
            __syncthreads();
        }
    }
}

// One workgroup per frame; dets [T, P, ROW] with the score in column 4.  The candidates' keys are compacted in arrival order (what
// follows fixes the order) -- a real detector leaves a few dozen priors above the confidence floor -- into LDS when P <= ORDER_LDS,
// where they cannot overflow it, else into `keys` [T, P] in memory (null when P <= ORDER_LDS).  Up to ORDER_LDS of them are sorted in
// LDS, padded to the next power of two of THEIR number; more are ranked by counting from memory (the keys are distinct, so the ranks
// are a permutation).  LDS: min(max(64, next power of two of P), ORDER_LDS) keys.
template <int ROW>
__global__ void __launch_bounds__(ORDER_THREADS) order_kernel(const float* __restrict__ dets, int P, float conf_thresh, int nms_top_k,
                                                               unsigned long long* __restrict__ keys, int32_t* __restrict__ order,
                                                               int32_t* __restrict__ count) {
    extern __shared__ __align__(16) unsigned long long order_keys[];
    unsigned long long* key = order_keys;
    __shared__ int cnt;
    const int f = blockIdx.x, tid = threadIdx.x;
    const float* d = dets + (long)f * P * ROW;
    const bool spill = P > ORDER_LDS;
    unsigned long long* gk = keys + (long)f * P;  // read and written only where `spill`
    int32_t* ord = order + (long)f * nms_top_k;
    if (tid == 0) cnt = 0;
    __syncthreads();
    for (int i0 = 0; i0 < P; i0 += 4 * ORDER_THREADS) {  // four loads in flight
        float sc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * ORDER_THREADS + tid;
            sc[u] = i < P ? d[(long)ROW * i + 4] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * ORDER_THREADS + tid;
            if (i < P && sc[u] > conf_thresh) {
                const int slot = atomicAdd(&cnt, 1);
                if (spill) gk[slot] = score_key(sc[u], i);
                else key[slot] = score_key(sc[u], i);
            }
        }
    }
    __syncthreads();
    const int c = cnt;
    if (tid == 0) count[f] = c;
    if (c <= ORDER_LDS) {
        int N = 64;
        while (N < c) N <<= 1;
        if (spill)
            for (int i = tid; i < c; i += ORDER_THREADS) key[i] = gk[i];
        for (int i = c + tid; i < N; i += ORDER_THREADS) key[i] = 0ull;  // padding sinks to the end of a descending sort
        __syncthreads();
        switch (N / (2 * ORDER_THREADS)) {
            case 0: bitonic_desc<0>(key, N, tid); break;
            case 1: bitonic_desc<1>(key, N, tid); break;
            case 2: bitonic_desc<2>(key, N, tid); break;
            case 4: bitonic_desc<4>(key, N, tid); break;
            default: bitonic_desc<8>(key, N, tid); break;
        }
        for (int r = tid; r < min(c, nms_top_k); r += ORDER_THREADS) ord[r] = key_prior(key[r]);
    } else {
        for (int i = tid; i < c; i += ORDER_THREADS) {
            const unsigned long long ki = gk[i];
            int rank = 0;
            for (int j = 0; j < c; ++j) rank += gk[j] > ki;
            if (rank < nms_top_k) ord[rank] = key_prior(ki);
        }
    }
}

// The same order of RetinaFace's rows by counting on the scores themselves, many blocks per frame (count [T] zeroed by the caller):
// k_face_nms takes it where a frame has more than ORDER_LDS priors.  It survives beside order_kernel's counting branch because that
// branch is ONE workgroup per frame: on a 1080p frame with every prior a candidate it would do the work of some 330 of these blocks.
__global__ void face_rank_kernel(const float* __restrict__ dets, int P, float conf_thresh, int nms_top_k,
                                 int32_t* __restrict__ order, int32_t* __restrict__ count) {
    const int f = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float* d = dets + (long)f * P * 15;
    __shared__ float sc[256];
    const float si = i < P ? d[15L * i + 4] : 0.f;
    const bool cand = i < P && si > conf_thresh;
    int rank = 0;
    for (int j0 = 0; j0 < P; j0 += 256) {
        __syncthreads();
        const int jj = j0 + threadIdx.x;
        sc[threadIdx.x] = jj < P ? d[15L * jj + 4] : -1.f;
        __syncthreads();
        if (cand) {
            const int lim = min(256, P - j0);
            for (int k = 0; k < lim; ++k) {
                const float sj = sc[k];
                rank += (sj > conf_thresh) && (sj > si || (sj == si && j0 + k > i));
            }
        }
    }
    if (cand) {
        atomicAdd(count + f, 1);
        if (rank < nms_top_k) order[(long)f * nms_top_k + rank] = i;
    }
}

// order_kernel<ROW> on T frames; keys: [T, P] spill, or null where P <= ORDER_LDS
template <int ROW>
int launch_order(avcer_ctx* ctx, const float* dets, int T, int P, float conf_thresh, int nms_top_k, unsigned long long* keys, int32_t* order,
                 int32_t* count, hipStream_t st) {
    static uint64_t attr_dev = 0;  // of this instance: devices that have the attribute
    if (!((attr_dev >> (ctx->device & 63)) & 1)) {
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)order_kernel<ROW>, hipFuncAttributeMaxDynamicSharedMemorySize, ORDER_LDS * 8));
        attr_dev |= 1ull << (ctx->device & 63);
    }
    int N = 64;  // LDS for the worst case the sort takes (every prior a candidate); the kernel sorts the next power of two of ITS count
    while (N < P && N < ORDER_LDS) N <<= 1;
    order_kernel<ROW><<<T, ORDER_THREADS, (size_t)N * 8, st>>>(dets, P, conf_thresh, nms_top_k, keys, order, count);
    return AVCER_OK;
}

// ------------------------------------------------------------------------------------------------ NMS
constexpr int NMS_THREADS = 1024;
constexpr int NMS_MAX = 6144;  // API bound on avcer_face_nms's nms_top_k (the kernel itself does not hold all boxes at once)

// What the two tails do differently: the row width, the "+1 pixel" of py_cpu_nms's widths and areas (nms_np has none), and column c
// of a reported row.
struct RetinaTail {
    static constexpr int ROW = 15;
    static constexpr bool PLUS1 = true;
    static __device__ __forceinline__ float out(const float* row, int c, float, float) { return row[c]; }
};
struct S3fdTail {
    static constexpr int ROW = 5;
    static constexpr bool PLUS1 = false;
    // the normalised corners times (w, h, w, h), the score as it is (s3fd_predictor.py:62-64)
    static __device__ __forceinline__ float out(const float* row, int c, float im_w, float im_h) {
        return c == 4 ? row[c] : row[c] * ((c & 1) ? im_h : im_w);
    }
};

template <bool PLUS1>
__device__ __forceinline__ float box_area(float4 b) {
#pragma clang fp contract(off)
    if constexpr (PLUS1) return (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f);
    else return (b.z - b.x) * (b.w - b.y);
}

// does kept box a (area aar) suppress box b (area bar)?  `!(ovr <= thresh)`: a NaN overlap suppresses, as `ovr <= thresh` keeps
template <bool PLUS1>
__device__ __forceinline__ bool suppresses(float4 a, float aar, float4 b, float bar, float nms_thresh) {
#pragma clang fp contract(off)
    float w = fminf(a.z, b.z) - fmaxf(a.x, b.x), h = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    if constexpr (PLUS1) { w = w + 1.0f; h = h + 1.0f; }
    w = fmaxf(0.0f, w);
    h = fmaxf(0.0f, h);
    const float inter = w * h;
    const float ovr = inter / (aar + bar - inter);
    return !(ovr <= nms_thresh);
}

// Greedy NMS of one frame per workgroup, in CHUNKS of 1024 boxes of the visiting order.  The references keep every survivor and then
// take keep[:top_k] (retina_face_predictor.py:96-100, utils.py:167); boxes are visited in score order, so the first top_k kept ones
// ARE that prefix and nothing behind the chunk that completes them is ever looked at.  Per chunk: every thread owns one box; it is
// first tested against the boxes kept from earlier chunks (their corners sit in LDS), then the chunk is walked in order with one
// barrier per kept box and at most ONE IoU per thread and kept box.  (A first form held all nms_top_k boxes in 126 KiB of LDS, one
// block per CU, and tested every later box against every kept one: with every prior a candidate 4.4-6.7 ms per 750 RetinaFace
// frames; here the walk ends inside the first chunk and three blocks share a CU.)  out [T, top_k, ROW]: rows [0, out_n[f]) of frame f.
template <class Tail>
__global__ void __launch_bounds__(NMS_THREADS) nms_kernel(const float* __restrict__ dets, int P, const int32_t* __restrict__ order,
                                                           const int32_t* __restrict__ count, int nms_top_k, float nms_thresh, int top_k,
                                                           float threshold, float im_w, float im_h, float* __restrict__ out,
                                                           int32_t* __restrict__ out_n) {
    constexpr int ROW = Tail::ROW;
    __shared__ float cx1[NMS_THREADS], cy1[NMS_THREADS], cx2[NMS_THREADS], cy2[NMS_THREADS], car[NMS_THREADS];  // the chunk
    __shared__ float kx1[1024], ky1[1024], kx2[1024], ky2[1024], kar[1024];                                       // kept so far
    __shared__ unsigned char cdead[NMS_THREADS];
    __shared__ int kept[1024];  // position in the visiting order of every kept box (beyond top_k they are never reported)
    __shared__ int out_rows;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(count[f], nms_top_k);
    const float* d = dets + (long)f * P * ROW;
    const int32_t* ord = order + (long)f * nms_top_k;
    const int cap = min(top_k, 1024);
    int nkept = 0;  // uniform across the block
    for (int c0 = 0; c0 < n && nkept < cap; c0 += NMS_THREADS) {
        const int cn = min(NMS_THREADS, n - c0);
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        float ar = 0.f;
        bool dead = tid >= cn;
        if (!dead) {
            const float* r = d + (long)ROW * ord[c0 + tid];
            b = make_float4(r[0], r[1], r[2], r[3]);
            ar = box_area<Tail::PLUS1>(b);
            for (int k = 0; k < nkept; ++k)  // boxes kept from earlier chunks all precede this one in the order
                if (suppresses<Tail::PLUS1>(make_float4(kx1[k], ky1[k], kx2[k], ky2[k]), kar[k], b, ar, nms_thresh)) { dead = true; break; }
        }
        __syncthreads();  // the previous chunk's arrays are free (every thread has left its walk)
        cx1[tid] = b.x; cy1[tid] = b.y; cx2[tid] = b.z; cy2[tid] = b.w; car[tid] = ar;
        cdead[tid] = dead ? 1 : 0;
        __syncthreads();
        for (int a = 0; a < cn; ++a) {
            if (cdead[a]) continue;  // uniform: every thread reads the same flag behind the previous barrier
            const float4 ab = make_float4(cx1[a], cy1[a], cx2[a], cy2[a]);
            const float aar = car[a];
            if (tid == 0) {
                kept[nkept] = c0 + a;
                kx1[nkept] = ab.x; ky1[nkept] = ab.y; kx2[nkept] = ab.z; ky2[nkept] = ab.w; kar[nkept] = aar;
            }
            if (++nkept >= cap) break;
            if (tid > a && !dead && suppresses<Tail::PLUS1>(ab, aar, b, ar, nms_thresh)) { dead = true; cdead[tid] = 1; }
            __syncthreads();
        }
        __syncthreads();  // tid 0's last kept entry is visible before the next chunk tests against it
    }
    // keep[:top_k], then the rows with score >= threshold: RetinaFace filters them (retina_face_predictor.py:102-108), S3FD's loop
    // stops at the first below (s3fd_predictor.py:56-64).  One form serves both: the kept boxes come in descending key order, along
    // which the score does not rise (-0.0 and +0.0, one key, compare alike), so `score >= threshold` holds on a prefix and the filter
    // selects exactly that prefix.
    __syncthreads();
    const int nk = min(nkept, cap);
    if (tid == 0) {
        int m = 0;
        while (m < nk && d[(long)ROW * ord[kept[m]] + 4] >= threshold) { kept[m] = ord[kept[m]]; ++m; }
        out_rows = m;
        out_n[f] = m;
    }
    __syncthreads();
    for (int e = tid; e < out_rows * ROW; e += NMS_THREADS)
        out[((long)f * top_k + e / ROW) * ROW + e % ROW] = Tail::out(d + (long)ROW * kept[e / ROW], e % ROW, im_w, im_h);
}

}  // namespace

int k_face_decode(avcer_ctx* ctx, const float* loc, const float* conf, const float* landms, const float* priors, int T, int P,
                  int im_h, int im_w, float var0, float var1, float* dets, hipStream_t st) {
    face_decode_kernel<<<dim3(cdiv(P, 256), T), 256, 0, st>>>(loc, conf, landms, priors, P, (float)im_w, (float)im_h, var0, var1, dets);
    CHECK_LAUNCH(ctx, "face_decode");
    return AVCER_OK;
}

int k_face_nms(avcer_ctx* ctx, const float* dets, int T, int P, float conf_thresh, float nms_thresh, int nms_top_k, int top_k,
               float threshold, int32_t* order, int32_t* count, float* out, int32_t* out_n, hipStream_t st) {
    if (nms_top_k > NMS_MAX) return set_err(ctx, AVCER_EINVAL, "face_nms: nms_top_k %d exceeds %d", nms_top_k, NMS_MAX);
    if (P <= ORDER_LDS) {
        TRY(launch_order<15>(ctx, dets, T, P, conf_thresh, nms_top_k, nullptr, order, count, st));
        CHECK_LAUNCH(ctx, "face_sort");
    } else {
        if (hipMemsetAsync(count, 0, (size_t)T * 4, st) != hipSuccess) return set_err(ctx, AVCER_EHIP, "face_nms: memset failed");
        face_rank_kernel<<<dim3(cdiv(P, 256), T), 256, 0, st>>>(dets, P, conf_thresh, nms_top_k, order, count);
        CHECK_LAUNCH(ctx, "face_rank");
    }
    nms_kernel<RetinaTail><<<T, NMS_THREADS, 0, st>>>(dets, P, order, count, nms_top_k, nms_thresh, top_k, threshold, 0.f, 0.f, out, out_n);
    CHECK_LAUNCH(ctx, "face_nms");
    return AVCER_OK;
}

size_t s3fd_detect_ws_bytes(int T, int P, int nms_top_k) {
    return (size_t)T * P * 5 * 4 + (size_t)T * P * 8 + ((size_t)T * nms_top_k + T) * 4 + 768;
}

int launch_s3fd_detect(avcer_ctx* ctx, const float* loc, const float* conf, const float* priors, int T, int P, int im_h, int im_w, float var0,
                       float var1, float conf_thresh, float nms_thresh, int nms_top_k, int top_k, float threshold, void* ws, float* out,
                       int32_t* out_n, hipStream_t st) {
    // the workspace, in the order of s3fd_detect_ws_bytes: keys (8-byte aligned first), dets, order, count
    unsigned long long* keys = (unsigned long long*)ws;
    float* dets = (float*)(keys + (size_t)T * P);
    int32_t* order = (int32_t*)(dets + (size_t)T * P * 5);
    int32_t* count = order + (size_t)T * nms_top_k;
    s3fd_decode_kernel<<<dim3(cdiv(P, 256), T), 256, 0, st>>>(loc, conf, priors, P, var0, var1, dets);
    CHECK_LAUNCH(ctx, "s3fd_decode");
    TRY(launch_order<5>(ctx, dets, T, P, conf_thresh, nms_top_k, keys, order, count, st));
    CHECK_LAUNCH(ctx, "s3fd_order");
    nms_kernel<S3fdTail><<<T, NMS_THREADS, 0, st>>>(dets, P, order, count, nms_top_k, nms_thresh, top_k, threshold, (float)im_w, (float)im_h,
                                                    out, out_n);
    CHECK_LAUNCH(ctx, "s3fd_nms");
    return AVCER_OK;
}
