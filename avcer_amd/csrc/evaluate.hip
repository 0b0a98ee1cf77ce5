// Dataset evaluation: the per-video loops of get_abaw_pred / get_afew_pred (get_pred_av.py:77-195, get_pred_audio.py:64-141) and
// get_metrics' prediction and confusion matrix (get_pred_av.py:35-45, get_pred_audio.py:30-34), each for a whole file list in one
// call.  Definitions: include/avcer_hip.h avcer_eval_tables, avcer_eval_confusion; stated in numpy by avcer_amd/evaluate.py
// (evaluate_numpy), which referees tests/test_gpu_evaluate.py.  All arithmetic is float64.
//
// avcer_eval_tables.  The audio CSV has one row per (window, frame) pair in no order, and the reference's groupby numbers the
// distinct frames in ascending order.  Nothing is sorted here: the caller states the key range of each video, a video owns that
// many SLOTS of the workspace (slot = key - key_lo), and
//   eval_extent_kernel   one thread per row: counts its slot's rows and, per column, the finite values and their largest exponent;
//   eval_sum_kernel      one thread per row: adds each finite value to its (slot, column) sum as a 96-bit fixed-point integer
//                        scaled by that exponent (two 64-bit integer atomics), so the sum is the same whatever the order;
//   eval_scan_*          the inclusive scan of "slot has rows" over all slots: a slot's scan value - 1 is its GROUP NUMBER
//                        counted from the first video, and the difference over a video's slots its group count;
//   eval_groups_kernel   one thread per slot: the mean of a slot with rows, written to row `group number` of the group table;
//   eval_rows_kernel     one thread per OUTPUT row (a wave owns 64 of them): its video, the kept position it shows (the last
//                        surviving one behind them), the row's softmax;
//   eval_video_kernel    video-level mode, one block per video: 256 partial sums over the video's groups and a fixed tree.
// A video of a million rows is a million threads in the first two kernels and 4096 rows per thread in the last.
// Without keys a row is its own group and only one of the last two kernels runs.
//
// Every index array comes from device memory, so every index derived from one is clamped or checked against the sizes that were
// passed by value before it addresses anything.
//
// Every product and every sum rounds on its own, as numpy's do: contraction is off for this whole file (see search.hip).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_COLS = 7;
constexpr int EV_SCAN_ITEMS = 4;                         // slots per thread of eval_scan_blocks
constexpr int EV_SCAN_TILE = EV_THREADS * EV_SCAN_ITEMS;  // slots per block
constexpr int EV_CM_MAX_BLOCKS = 2048;

struct EvalWs {
    double* groups;            // [n_slots][7]  group means, row = group number
    unsigned long long* hi;    // [n_slots][7]  sum of the terms' upper parts (two's complement)
    unsigned long long* lo;    // [n_slots][7]  sum of the terms' lower 32 bits
    int32_t* cnt;              // [n_slots][7]  finite values
    int32_t* emax;             // [n_slots][7]  their largest biased exponent
    int32_t* flags;            // [n_slots][7]  1: a +inf, 2: a -inf
    int32_t* rows;             // [n_slots]     rows of the slot
    int32_t* rank;             // [n_slots]     inclusive scan of (rows > 0)
    int32_t* tiles;            // [tiles + 1]   per scan tile: its count, then the count of all tiles before it
    size_t zero_from, bytes;
};

EvalWs eval_ws(void* base, long n_slots) {
    EvalWs w;
    char* p = (char*)base;
    const size_t cells = (size_t)n_slots * EV_COLS;
    const size_t n_tiles = ((size_t)n_slots + EV_SCAN_TILE - 1) / EV_SCAN_TILE + 1;
    w.groups = (double*)p; p += cells * 8;
    w.zero_from = (size_t)(p - (char*)base);
    w.hi = (unsigned long long*)p; p += cells * 8;
    w.lo = (unsigned long long*)p; p += cells * 8;
    w.cnt = (int32_t*)p; p += cells * 4;
    w.emax = (int32_t*)p; p += cells * 4;
    w.flags = (int32_t*)p; p += cells * 4;
    w.rows = (int32_t*)p; p += (size_t)n_slots * 4;
    w.rank = (int32_t*)p; p += (size_t)n_slots * 4;
    w.tiles = (int32_t*)p; p += n_tiles * 4;
    w.bytes = ((size_t)(p - (char*)base) + 255) / 256 * 256;
    return w;
}

__device__ __forceinline__ int clampi(int x, long lo, long hi) { return x < lo ? (int)lo : (x > hi ? (int)hi : x); }

// the video v of [0, n_videos) with off[v] <= i < off[v + 1]; videos without items are passed over
__device__ __forceinline__ int find_video(const int32_t* __restrict__ off, int n_videos, long i) {
    int a = 0, b = n_videos - 1;
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (off[mid + 1] > i) b = mid; else a = mid + 1;
    }
    return a;
}

// the slot of row i, or -1: its key lies outside its video's range, or its video's range outside the workspace
__device__ __forceinline__ long row_slot(const int32_t* __restrict__ keys, const int32_t* __restrict__ row_off,
                                         const int32_t* __restrict__ key_lo, const int32_t* __restrict__ key_off, int n_videos,
                                         long n_slots, long i) {
    const int v = find_video(row_off, n_videos, i);
    if (i < row_off[v] || i >= row_off[v + 1]) return -1;  // offsets that do not cover row i
    const long d = (long)keys[i] - (long)key_lo[v];
    const long s0 = key_off[v], s1 = key_off[v + 1];
    if (d < 0 || s0 < 0 || s1 > n_slots || s0 + d >= s1) return -1;
    return s0 + d;
}

__global__ void __launch_bounds__(EV_THREADS) eval_extent_kernel(const double* __restrict__ rows, const int32_t* __restrict__ keys,
                                                                 long n_rows, int c, const int32_t* __restrict__ row_off,
                                                                 const int32_t* __restrict__ key_lo,
                                                                 const int32_t* __restrict__ key_off, int n_videos, long n_slots,
                                                                 EvalWs w) {
    const long i = (long)blockIdx.x * EV_THREADS + threadIdx.x;
    if (i >= n_rows) return;
    const long s = row_slot(keys, row_off, key_lo, key_off, n_videos, n_slots, i);
    if (s < 0) return;
    atomicAdd(&w.rows[s], 1);
#pragma unroll
    for (int k = 0; k < EV_COLS; ++k) {
        const double x = rows[i * c + k];
        if (x != x) continue;  // skipna
        const int e = (int)((__double_as_longlong(x) >> 52) & 0x7ff);
        if (e == 0x7ff) { atomicOr(&w.flags[s * EV_COLS + k], x > 0 ? 1 : 2); continue; }
        atomicAdd(&w.cnt[s * EV_COLS + k], 1);
        atomicMax(&w.emax[s * EV_COLS + k], e);
    }
}

// The grid of a (slot, column): 2^(E - 60), where 2^E <= the column's largest magnitude < 2^(E + 1) (E = -1022 for subnormals and
// zeros).  A term scaled by 2^(60 - E) is below 2^61 in magnitude, the largest keeps all its 53 bits, and 2^28 terms sum to
// less than 2^61 in the upper part and 2^60 in the lower.
__device__ __forceinline__ int grid_shift(int emax_biased) { return 60 - ((emax_biased > 0 ? emax_biased : 1) - 1023); }

__global__ void __launch_bounds__(EV_THREADS) eval_sum_kernel(const double* __restrict__ rows, const int32_t* __restrict__ keys,
                                                              long n_rows, int c, const int32_t* __restrict__ row_off,
                                                              const int32_t* __restrict__ key_lo,
                                                              const int32_t* __restrict__ key_off, int n_videos, long n_slots,
                                                              EvalWs w) {
    const long i = (long)blockIdx.x * EV_THREADS + threadIdx.x;
    if (i >= n_rows) return;
    const long s = row_slot(keys, row_off, key_lo, key_off, n_videos, n_slots, i);
    if (s < 0) return;
#pragma unroll
    for (int k = 0; k < EV_COLS; ++k) {
        const double x = rows[i * c + k];
        const int e = (int)((__double_as_longlong(x) >> 52) & 0x7ff);
        if (x != x || e == 0x7ff) continue;
        const long long q = __double2ll_rn(ldexp(x, grid_shift(w.emax[s * EV_COLS + k])));
        atomicAdd(&w.hi[s * EV_COLS + k], (unsigned long long)(q >> 32));
        atomicAdd(&w.lo[s * EV_COLS + k], (unsigned long long)(q & 0xffffffffLL));
    }
}

// inclusive scan of 256 values, one per thread, through LDS; returns this thread's value and leaves the total in buf[255]
__device__ __forceinline__ int block_scan(int x, int* buf) {
    const int t = threadIdx.x;
    buf[t] = x;
    __syncthreads();
    for (int d = 1; d < EV_THREADS; d <<= 1) {
        const int y = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += y;
        __syncthreads();
    }
    return buf[t];
}

__global__ void __launch_bounds__(EV_THREADS) eval_scan_blocks(long n_slots, EvalWs w) {
    __shared__ int buf[EV_THREADS];
    const long s0 = ((long)blockIdx.x * EV_THREADS + threadIdx.x) * EV_SCAN_ITEMS;
    int has[EV_SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int j = 0; j < EV_SCAN_ITEMS; ++j) {
        has[j] = s0 + j < n_slots && w.rows[s0 + j] > 0;
        sum += has[j];
    }
    int run = block_scan(sum, buf) - sum;
#pragma unroll
    for (int j = 0; j < EV_SCAN_ITEMS; ++j) {
        run += has[j];
        if (s0 + j < n_slots) w.rank[s0 + j] = run;
    }
    if (threadIdx.x == EV_THREADS - 1) w.tiles[blockIdx.x] = buf[EV_THREADS - 1];
}

// one block: the tiles' counts become the counts of all tiles before each
__global__ void __launch_bounds__(EV_THREADS) eval_scan_tiles(int n_tiles, EvalWs w) {
    __shared__ int buf[EV_THREADS];
    int carry = 0;
    for (int base = 0; base < n_tiles; base += EV_THREADS) {
        const int i = base + threadIdx.x;
        const int x = i < n_tiles ? w.tiles[i] : 0;
        const int incl = block_scan(x, buf);
        const int total = buf[EV_THREADS - 1];
        if (i < n_tiles) w.tiles[i] = carry + incl - x;
        carry += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(EV_THREADS) eval_groups_kernel(long n_slots, EvalWs w) {
    const long s = (long)blockIdx.x * EV_THREADS + threadIdx.x;
    if (s >= n_slots) return;
    const int r = w.rank[s] + w.tiles[s / EV_SCAN_TILE];
    w.rank[s] = r;  // groups of all slots up to and including s
    if (w.rows[s] <= 0 || r < 1 || r > n_slots) return;
#pragma unroll
    for (int k = 0; k < EV_COLS; ++k) {
        const long cell = s * EV_COLS + k;
        const int fl = w.flags[cell], n = w.cnt[cell];
        double mean;
        if (fl) mean = fl == 1 ? INFINITY : (fl == 2 ? -INFINITY : NAN);
        else if (n == 0) mean = NAN;
        else {
            const unsigned long long lo = w.lo[cell];
            const long long up = (long long)w.hi[cell] + (long long)(lo >> 32);
            // exact while |up| < 2^53 (some 2^24 terms); beyond, one more rounding of the upper part
            const double sum = (double)up * 4294967296.0 + (double)(lo & 0xffffffffULL);
            mean = ldexp(sum, -grid_shift(w.emax[cell])) / (double)n;
        }
        w.groups[(long)(r - 1) * EV_COLS + k] = mean;
    }
}

// where video v's groups lie: rows of `rows` (no keys) or of the group table
struct Span {
    const double* src;
    int ld;
    long first, count;
};

__device__ __forceinline__ Span video_span(const double* __restrict__ rows, long n_rows, int c, const int32_t* __restrict__ row_off,
                                           const int32_t* __restrict__ key_off, long n_slots, const EvalWs& w, bool keyed, int v) {
    Span sp;
    if (keyed) {
        const int s0 = clampi(key_off[v], 0, n_slots), s1 = clampi(key_off[v + 1], s0, n_slots);
        const long g0 = s0 > 0 ? w.rank[s0 - 1] : 0, g1 = s1 > 0 ? w.rank[s1 - 1] : 0;
        sp.src = w.groups; sp.ld = EV_COLS; sp.first = g0; sp.count = g1 - g0;
        if (g0 < 0 || g1 > n_slots || g1 < g0) sp.count = 0;
    } else {
        const int r0 = clampi(row_off[v], 0, n_rows), r1 = clampi(row_off[v + 1], r0, n_rows);
        sp.src = rows; sp.ld = c; sp.first = r0; sp.count = r1 - r0;
    }
    return sp;
}

// data/utils.py:125-127 on one row; a NaN anywhere makes np.max, and with it every element, NaN
__device__ __forceinline__ void load_row(const double* __restrict__ p, bool softmax, double* x) {
#pragma unroll
    for (int k = 0; k < EV_COLS; ++k) x[k] = p[k];
    if (!softmax) return;
    double mx = x[0];
    bool nan = x[0] != x[0];
#pragma unroll
    for (int k = 1; k < EV_COLS; ++k) { mx = x[k] > mx ? x[k] : mx; nan |= x[k] != x[k]; }
    double den = 0.0;
#pragma unroll
    for (int k = 0; k < EV_COLS; ++k) { x[k] = exp(x[k] - mx); den = den + x[k]; }
#pragma unroll
    for (int k = 0; k < EV_COLS; ++k) x[k] = nan ? NAN : x[k] / den;
}

__global__ void __launch_bounds__(EV_THREADS) eval_rows_kernel(const double* __restrict__ rows, long n_rows, int c,
                                                               const int32_t* __restrict__ row_off,
                                                               const int32_t* __restrict__ key_off, long n_slots,
                                                               const int32_t* __restrict__ need, long n_need,
                                                               const int32_t* __restrict__ need_off,
                                                               const int32_t* __restrict__ out_off, int n_videos, long n_out,
                                                               int softmax, bool keyed, EvalWs w, double* __restrict__ out) {
    const long p = (long)blockIdx.x * EV_THREADS + threadIdx.x;
    if (p >= n_out) return;
    double x[EV_COLS];
#pragma unroll
    for (int k = 0; k < EV_COLS; ++k) x[k] = NAN;
    const int v = find_video(out_off, n_videos, p);
    const long j = p - out_off[v];
    if (j >= 0 && p < out_off[v + 1]) {
        const Span sp = video_span(rows, n_rows, c, row_off, key_off, n_slots, w, keyed, v);
        // kept positions below the group count: `need` ascends, so they are a prefix
        const long nb = clampi(need_off[v], 0, n_need), ne = clampi(need_off[v + 1], nb, n_need);
        long a = nb, b = ne;
        while (a < b) {
            const long mid = a + ((b - a) >> 1);
            if (need[mid] < sp.count) a = mid + 1; else b = mid;
        }
        const long kept = a - nb;
        if (kept > 0) {
            const long g = need[nb + (j < kept ? j : kept - 1)];
            if (g >= 0 && g < sp.count) load_row(sp.src + (sp.first + g) * sp.ld, softmax != 0, x);
        }
    }
#pragma unroll
    for (int k = 0; k < EV_COLS; ++k) out[p * EV_COLS + k] = x[k];
}

__global__ void __launch_bounds__(EV_THREADS) eval_video_kernel(const double* __restrict__ rows, long n_rows, int c,
                                                                const int32_t* __restrict__ row_off,
                                                                const int32_t* __restrict__ key_off, long n_slots, int softmax,
                                                                bool keyed, EvalWs w, double* __restrict__ out) {
    __shared__ double part[EV_THREADS][EV_COLS];
    const int v = blockIdx.x, t = threadIdx.x;
    const Span sp = video_span(rows, n_rows, c, row_off, key_off, n_slots, w, keyed, v);
    double acc[EV_COLS];
#pragma unroll
    for (int k = 0; k < EV_COLS; ++k) acc[k] = 0.0;
    for (long g = t; g < sp.count; g += EV_THREADS) {
        double x[EV_COLS];
        load_row(sp.src + (sp.first + g) * sp.ld, softmax != 0, x);
#pragma unroll
        for (int k = 0; k < EV_COLS; ++k) acc[k] = acc[k] + x[k];
    }
#pragma unroll
    for (int k = 0; k < EV_COLS; ++k) part[t][k] = acc[k];
    __syncthreads();
    for (int d = EV_THREADS / 2; d >= 1; d >>= 1) {
        if (t < d)
#pragma unroll
            for (int k = 0; k < EV_COLS; ++k) part[t][k] = part[t][k] + part[t + d][k];
        __syncthreads();
    }
    if (t < EV_COLS) out[(long)v * EV_COLS + t] = sp.count > 0 ? part[0][t] / (double)sp.count : NAN;
}

// ------------------------------------------------------------------------------------------------ confusion matrix
struct CmParams {
    double w1[AVCER_EVAL_MAX_MODELS][EV_COLS];
    double w2[AVCER_EVAL_MAX_MODELS];
    double u1[EV_COLS], u2[EV_COLS];
    int compound, mask;
};

template <int M>
__global__ void __launch_bounds__(EV_THREADS) eval_confusion_kernel(const double* __restrict__ tables,
                                                                    const int32_t* __restrict__ labels, long n, CmParams cp,
                                                                    int32_t* __restrict__ pred, unsigned long long* __restrict__ cm) {
    __shared__ unsigned int hist[EV_COLS * EV_COLS];
    if (threadIdx.x < EV_COLS * EV_COLS) hist[threadIdx.x] = 0;
    __syncthreads();
    const int p1[7] = {3, 4, 5, 2, 1, 3, 1}, p2[7] = {6, 6, 6, 6, 6, 5, 5};  // get_pred_audio.py:202-210, audio class order
    for (long i = (long)blockIdx.x * EV_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * EV_THREADS) {
        double f[EV_COLS];
#pragma unroll
        for (int k = 0; k < EV_COLS; ++k) f[k] = (tables[i * EV_COLS + k] * cp.w1[0][k]) * cp.w2[0];
#pragma unroll
        for (int m = 1; m < M; ++m)
#pragma unroll
            for (int k = 0; k < EV_COLS; ++k) f[k] = f[k] + (tables[((long)m * n + i) * EV_COLS + k] * cp.w1[m][k]) * cp.w2[m];
        if (cp.compound) {
            double q[EV_COLS];
#pragma unroll
            for (int k = 0; k < EV_COLS; ++k) q[k] = cp.mask ? (f[k] > 1.0 / 7.0 ? f[k] : 0.0) : f[k];
#pragma unroll
            for (int k = 0; k < EV_COLS; ++k) f[k] = q[p1[k]] * cp.u1[k] + q[p2[k]] * cp.u2[k];
        }
        // np.argmax: the first index of the maximum; the first NaN wins and nothing displaces it
        double best = f[0];
        int am = 0;
#pragma unroll
        for (int k = 1; k < EV_COLS; ++k) {
            const bool take = !(f[k] <= best) && best == best;
            best = take ? f[k] : best;
            am = take ? k : am;
        }
        if (pred) pred[i] = am;
        if (cm) {
            const int lab = labels[i];
            if (lab >= 0 && lab < EV_COLS) atomicAdd(&hist[lab * EV_COLS + am], 1u);
        }
    }
    __syncthreads();
    if (cm && threadIdx.x < EV_COLS * EV_COLS && hist[threadIdx.x]) atomicAdd(&cm[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

}  // namespace

extern "C" int64_t avcer_eval_tables_workspace(int64_t n_slots) {
    if (n_slots <= 0 || n_slots > AVCER_EVAL_MAX_ROWS) return 0;
    return (int64_t)eval_ws(nullptr, (long)n_slots).bytes;
}

extern "C" int avcer_eval_tables(avcer_ctx* ctx, const double* rows, const int32_t* keys, int64_t n_rows, int c,
                                 const int32_t* row_off, const int32_t* key_lo, const int32_t* key_off, int64_t n_slots,
                                 const int32_t* need, int64_t n_need, const int32_t* need_off, const int32_t* out_off, int n_videos,
                                 int64_t n_out, int softmax, int video_level, double* out, void* ws, int64_t ws_bytes, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (n_videos < 1 || n_videos > AVCER_EVAL_MAX_VIDEOS || c < 7 || c > 8 || n_rows < 0 || n_rows > AVCER_EVAL_MAX_ROWS ||
        n_out < 0 || n_out > AVCER_EVAL_MAX_ROWS || n_need < 0 || n_need > AVCER_EVAL_MAX_ROWS || n_slots < 0 || n_slots > AVCER_EVAL_MAX_ROWS)
        return set_err(ctx, AVCER_EINVAL, "eval tables: %d videos (1..%d), %d columns (7..8), %lld rows, %lld key slots, %lld output "
                       "rows (0..%lld each)", n_videos, AVCER_EVAL_MAX_VIDEOS, c, (long long)n_rows, (long long)n_slots,
                       (long long)n_out, (long long)AVCER_EVAL_MAX_ROWS);
    if (video_level && n_out != n_videos)
        return set_err(ctx, AVCER_EINVAL, "eval tables: video level writes one row per video, %lld rows for %d videos", (long long)n_out,
                       n_videos);
    if (!row_off || !out_off || (n_rows && !rows) || (n_out && !out) || (!video_level && (!need_off || (n_need && !need))))
        return set_err(ctx, AVCER_EINVAL, "eval tables: null buffer");
    const bool keyed = keys != nullptr;
    if (keyed && (!key_lo || !key_off)) return set_err(ctx, AVCER_EINVAL, "eval tables: keys without key_lo / key_off");
    if (!keyed) n_slots = 0;
    EvalWs w = eval_ws(ws, (long)n_slots);
    if (keyed && n_slots && (!ws || ws_bytes < (int64_t)w.bytes))
        return set_err(ctx, AVCER_EINVAL, "eval tables: workspace of %lld bytes, %lld key slots need %lld", (long long)ws_bytes,
                       (long long)n_slots, (long long)w.bytes);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (keyed && n_slots) {
        HIP_TRY(ctx, hipMemsetAsync((char*)ws + w.zero_from, 0, w.bytes - w.zero_from, st));
        if (n_rows) {
            const int gr = cdiv(n_rows, EV_THREADS);
            eval_extent_kernel<<<gr, EV_THREADS, 0, st>>>(rows, keys, (long)n_rows, c, row_off, key_lo, key_off, n_videos, (long)n_slots, w);
            eval_sum_kernel<<<gr, EV_THREADS, 0, st>>>(rows, keys, (long)n_rows, c, row_off, key_lo, key_off, n_videos, (long)n_slots, w);
        }
        const int n_tiles = cdiv(n_slots, EV_SCAN_TILE);
        eval_scan_blocks<<<n_tiles, EV_THREADS, 0, st>>>((long)n_slots, w);
        eval_scan_tiles<<<1, EV_THREADS, 0, st>>>(n_tiles, w);
        eval_groups_kernel<<<cdiv(n_slots, EV_THREADS), EV_THREADS, 0, st>>>((long)n_slots, w);
        CHECK_LAUNCH(ctx, "eval groups");
    }
    if (video_level)
        eval_video_kernel<<<n_videos, EV_THREADS, 0, st>>>(rows, (long)n_rows, c, row_off, key_off, (long)n_slots, softmax, keyed, w, out);
    else if (n_out)
        eval_rows_kernel<<<cdiv(n_out, EV_THREADS), EV_THREADS, 0, st>>>(rows, (long)n_rows, c, row_off, key_off, (long)n_slots, need,
                                                                        (long)n_need, need_off, out_off, n_videos, (long)n_out, softmax, keyed, w, out);
    CHECK_LAUNCH(ctx, "eval tables");
    return AVCER_OK;
}

extern "C" int avcer_eval_confusion(avcer_ctx* ctx, const double* tables, const int32_t* labels, int64_t n, int m,
                                    const double* w1_host, const double* w2_host, int compound, int32_t* pred, int64_t* cm,
                                    avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (m < 1 || m > AVCER_EVAL_MAX_MODELS || n < 1 || n > AVCER_EVAL_MAX_ROWS)
        return set_err(ctx, AVCER_EINVAL, "eval confusion: %d tables (1..%d), %lld rows (1..%lld)", m, AVCER_EVAL_MAX_MODELS, (long long)n,
                       (long long)AVCER_EVAL_MAX_ROWS);
    if (!tables || (!pred && !cm) || (cm && !labels)) return set_err(ctx, AVCER_EINVAL, "eval confusion: null buffer");
    if (compound & ~(AVCER_EVAL_COMPOUND | AVCER_EVAL_CE_WEIGHTS | AVCER_EVAL_CE_MASK))
        return set_err(ctx, AVCER_EINVAL, "eval confusion: compound flags 0x%x", compound);
    CmParams cp;
    for (int q = 0; q < AVCER_EVAL_MAX_MODELS; ++q) {
        for (int k = 0; k < EV_COLS; ++k) cp.w1[q][k] = (w1_host && q < m) ? w1_host[q * EV_COLS + k] : 1.0;
        cp.w2[q] = (w2_host && q < m) ? w2_host[q] : 1.0;
    }
    const int p1[7] = {3, 4, 5, 2, 1, 3, 1}, p2[7] = {6, 6, 6, 6, 6, 5, 5};
    const double cw[7] = {0, 5, 6, 5, 6, 4, 2};  // dict_weights, get_pred_audio.py:212-219
    for (int k = 0; k < EV_COLS; ++k) {
        const double s = cw[p1[k]] + cw[p2[k]];
        cp.u1[k] = (compound & AVCER_EVAL_CE_WEIGHTS) ? cw[p1[k]] / s : 1.0;
        cp.u2[k] = (compound & AVCER_EVAL_CE_WEIGHTS) ? cw[p2[k]] / s : 1.0;
    }
    cp.compound = compound & AVCER_EVAL_COMPOUND;
    cp.mask = (compound & AVCER_EVAL_CE_MASK) != 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (cm) HIP_TRY(ctx, hipMemsetAsync(cm, 0, EV_COLS * EV_COLS * sizeof(int64_t), st));
    long blocks = ((long)n + EV_THREADS - 1) / EV_THREADS;
    if (blocks > EV_CM_MAX_BLOCKS) blocks = EV_CM_MAX_BLOCKS;
    unsigned long long* cmu = (unsigned long long*)cm;
    switch (m) {
        case 1: eval_confusion_kernel<1><<<(int)blocks, EV_THREADS, 0, st>>>(tables, labels, (long)n, cp, pred, cmu); break;
        case 2: eval_confusion_kernel<2><<<(int)blocks, EV_THREADS, 0, st>>>(tables, labels, (long)n, cp, pred, cmu); break;
        case 3: eval_confusion_kernel<3><<<(int)blocks, EV_THREADS, 0, st>>>(tables, labels, (long)n, cp, pred, cmu); break;
        case 4: eval_confusion_kernel<4><<<(int)blocks, EV_THREADS, 0, st>>>(tables, labels, (long)n, cp, pred, cmu); break;
    }
    CHECK_LAUNCH(ctx, "eval confusion");
    return AVCER_OK;
}
