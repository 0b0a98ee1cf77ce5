// The traces of the prediction timeline chart (run.py:272-296, visualization/visualize.py:175-215): the class tables of a batch of
// charts rasterised where they lie, so that tables -> traces -> text -> JPEG never brings a table or a pixel to the host.
//
// The kernels restate avcer_amd/chart.py (line_runs, series_numpy) pixel for pixel, and that restates PIL's ImageDraw.line(width=1):
// integer arithmetic only.  Two launches:
//   envelope  per (chart, series, column) the rows its segments cover in that column, as ONE interval;
//   paint     a thread per plot pixel tests the interval of the one series the thinning rule lets paint it.
//
// Why one interval is enough.  A segment covers one contiguous run of rows in each column it touches, and it covers both its end
// points.  A column that holds the frames f .. l is touched by the segments f-1 -> f, ..., l -> l+1; each run contains one of the
// points (column, row of frame i), f <= i <= l, and consecutive segments share such a point, so the union of the runs is connected:
// min .. max over the rows of the frames f .. l, of the join from frame f-1 and of the join to frame l+1.  A column that holds no
// frame lies strictly between two consecutive frames and is crossed by that one segment.  So the bound is 1 interval per (series,
// column) for every T, below the 4 a column could hold were its runs disjoint (two joins, the column's own frames, a crossing).
#include "common.h"

namespace {

constexpr int CH_THREADS = 256;       // four waves: wave s of a block is series s of the block's column
constexpr int CH_TILE_W = 64, CH_TILE_H = 4;
constexpr uint32_t CH_EMPTY = 0x0000ffffu;  // lo = 65535, hi = 0: no row passes lo - 1 <= y <= hi + 1

struct Colours { uint32_t rgb[AVCER_CHART_MAX_SERIES]; };  // r | g << 8 | b << 16

template <class E> __device__ __forceinline__ int cls(const E* __restrict__ row, long i) {
    const long v = (long)row[i];
    return (int)(v < 0 ? 0 : v > AVCER_CHART_CLASSES - 1 ? AVCER_CHART_CLASSES - 1 : v);  // the host refused such a value; no table index leaves yc
}

// The smallest frame whose column ((2i + 1) * pw) / (2T) is at least c, in 64 bits
__device__ __forceinline__ long first_frame(long c, long T, long pw) {
    const long a = 2 * T * c - pw;
    return a <= 0 ? 0 : (a + 2 * pw - 1) / (2 * pw);
}

__device__ __forceinline__ int column_of(long i, long T, long pw) { return (int)(((2 * i + 1) * pw) / (2 * T)); }

// The rows lo .. hi that the line from (xa, ya) to (xb, yb), xa <= x <= xb, covers in column x (chart.py line_runs; the sides are
// at most AVCER_CHART_MAX_SIDE = 2^14, so every product stays below 2^30)
__device__ __forceinline__ void seg_rows(int xa, int ya, int xb, int yb, int x, int& lo, int& hi) {
    const int dx = xb - xa, dy = yb > ya ? yb - ya : ya - yb, ys = yb > ya ? 1 : -1, m = x - xa;
    int a, b;
    if (dx > dy) {
        a = b = (2 * dy * m + dx) / (2 * dx);
    } else if (dx == 0) {
        a = 0; b = dy;
    } else {
        a = m == 0 ? 0 : (dy * (2 * m - 1) + 2 * dx - 1) / (2 * dx);
        b = min(dy, (dy * (2 * m + 1) + 2 * dx - 1) / (2 * dx) - 1);
    }
    const int p = ya + ys * a, q = ya + ys * b;
    lo = min(lo, min(p, q));
    hi = max(hi, max(p, q));
}

// One wave per (column, series, chart).  T >= pw: the column holds T / pw frames or more, read with a stride of 64 (coalesced) and
// reduced over the wave -- the one loop whose trip count depends on T.  T < pw: at most one frame, no reduction.
template <class E>
__global__ void __launch_bounds__(CH_THREADS) chart_envelope_kernel(const E* __restrict__ table, long stride, int series,
                                                                    const avcer_chart_plan* __restrict__ plans, int pw_max,
                                                                    uint32_t* __restrict__ env) {
    const int c = blockIdx.x, v = blockIdx.y, s = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (s >= series) return;  // a whole wave; the kernel has no barrier
    const avcer_chart_plan* p = plans + v;
    const long T = p->length, off = p->offset;
    const int pw = p->pw;
    if (c >= pw || pw > pw_max || T < 1 || off < 0 || off + T > stride) return;
    const E* row = table + (long)s * stride + off;
    const long f = first_frame(c, T, pw), l = min(first_frame((long)c + 1, T, pw), T) - 1;
    int lo = INT32_MAX, hi = -1;
    if (f <= l) {
        int cmin = AVCER_CHART_CLASSES - 1, cmax = 0;
        if (T >= pw) {
#pragma unroll 4
            for (long i = f + lane; i <= l; i += 64) {
                const int k = cls(row, i);
                cmin = min(cmin, k);
                cmax = max(cmax, k);
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                cmin = min(cmin, __shfl_xor(cmin, d, 64));
                cmax = max(cmax, __shfl_xor(cmax, d, 64));
            }
        } else {
            cmin = cmax = cls(row, f);  // f == l
        }
        lo = p->yc[cmax];  // class 0 is the lowest row of the picture: the largest y
        hi = p->yc[cmin];
        if (f >= 1) seg_rows(column_of(f - 1, T, pw), p->yc[cls(row, f - 1)], c, p->yc[cls(row, f)], c, lo, hi);
        if (l < T - 1) seg_rows(c, p->yc[cls(row, l)], column_of(l + 1, T, pw), p->yc[cls(row, l + 1)], c, lo, hi);
    } else if (f >= 1 && f <= T - 1) {  // between frame f - 1 and frame f
        seg_rows(column_of(f - 1, T, pw), p->yc[cls(row, f - 1)], column_of(f, T, pw), p->yc[cls(row, f)], c, lo, hi);
    }
    if (lane == 0) env[((long)v * series + s) * pw_max + c] = lo > hi ? CH_EMPTY : (uint32_t)lo | (uint32_t)hi << 16;
}

// A thread per plot pixel: the thinning rule names the one series that may paint it, whose interval, widened by one row each way,
// decides.  Uncovered pixels are neither read nor written.
__global__ void __launch_bounds__(CH_THREADS) chart_paint_kernel(const uint32_t* __restrict__ env, int series,
                                                                 const avcer_chart_plan* __restrict__ plans, int pw_max,
                                                                 uint8_t* __restrict__ out, int h, int w, Colours colours) {
    const int v = blockIdx.z;
    const avcer_chart_plan* p = plans + v;
    const int x = blockIdx.x * CH_TILE_W + (threadIdx.x & 63), y = blockIdx.y * CH_TILE_H + (threadIdx.x >> 6);
    if (x >= p->pw || y >= p->ph || p->pw > pw_max) return;
    const int X = p->x0 + x, Y = p->y0 + y;
    if (X < 0 || X >= w || Y < 0 || Y >= h) return;  // nothing outside the picture is ever addressed
    const int s = (X + Y) & 3;
    if (s >= series) return;
    const uint32_t e = env[((long)v * series + s) * pw_max + x];
    const int lo = (int)(e & 0xffffu), hi = (int)(e >> 16);
    if (Y < lo - 1 || Y > hi + 1) return;
    uint8_t* px = out + (((long)v * h + Y) * w + X) * 3;
    const uint32_t ink = colours.rgb[s];
    px[0] = (uint8_t)ink; px[1] = (uint8_t)(ink >> 8); px[2] = (uint8_t)(ink >> 16);
}

}  // namespace

extern "C" int avcer_chart_path(int64_t frames, int pw) {
    if (frames < 1 || pw < 1 || pw > AVCER_CHART_MAX_SIDE) return AVCER_EINVAL;
    return frames >= pw ? AVCER_CHART_REDUCE : AVCER_CHART_SEGMENT;
}

extern "C" int avcer_chart_series(avcer_ctx* ctx, const void* table, int elem_bytes, int series, int64_t stride,
                                  const avcer_chart_plan* plans_host, const avcer_chart_plan* plans, int n_charts, uint8_t* out, int h,
                                  int w, const uint8_t* colours, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (!table || !plans_host || !plans || !out || !colours) return set_err(ctx, AVCER_EINVAL, "chart_series: null pointer");
    if ((elem_bytes != 4 && elem_bytes != 8) || series < 1 || series > AVCER_CHART_MAX_SERIES || stride < 1 || n_charts < 0 || h < 1 ||
        w < 1 || h > AVCER_CHART_MAX_SIDE || w > AVCER_CHART_MAX_SIDE)
        return set_err(ctx, AVCER_EINVAL, "chart_series: %d charts of %d x %d, %d series of %d-byte classes, stride %lld", n_charts, w, h,
                       series, elem_bytes, (long long)stride);
    int pw_max = 0, ph_max = 0;
    for (int v = 0; v < n_charts; ++v) {
        const avcer_chart_plan& p = plans_host[v];
        bool ok = p.x0 >= 0 && p.y0 >= 0 && p.pw >= 1 && p.ph >= 1 && (long)p.x0 + p.pw <= w && (long)p.y0 + p.ph <= h && p.length >= 1 &&
                  p.length <= (1L << 44) /* (2i + 1) * pw and 2 * T * c stay far inside 64 bits */ && p.offset >= 0 && p.offset <= stride && p.length <= stride - p.offset;
        for (int c = 0; ok && c < AVCER_CHART_CLASSES; ++c) ok = p.yc[c] >= p.y0 && p.yc[c] < p.y0 + p.ph;
        if (!ok)
            return set_err(ctx, AVCER_EINVAL, "chart_series: chart %d: plot rectangle (%d, %d, %d x %d), %lld frames at %lld of %lld, or a row "
                           "centre outside the rectangle", v, p.x0, p.y0, p.pw, p.ph, (long long)p.length, (long long)p.offset, (long long)stride);
        pw_max = p.pw > pw_max ? p.pw : pw_max;
        ph_max = p.ph > ph_max ? p.ph : ph_max;
    }
    if (n_charts == 0) return AVCER_OK;
    if (n_charts > 65535) return set_err(ctx, AVCER_EINVAL, "chart_series: %d charts in one call (at most 65535)", n_charts);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint32_t* env = nullptr;
    TRY(ws_carve(ctx, WS_CHART, "chart_series", [&](Arena& a) { env = a.get<uint32_t>((size_t)n_charts * series * pw_max); }));
    Colours ink;
    for (int s = 0; s < AVCER_CHART_MAX_SERIES; ++s)
        ink.rgb[s] = s < series ? (uint32_t)colours[3 * s] | (uint32_t)colours[3 * s + 1] << 8 | (uint32_t)colours[3 * s + 2] << 16 : 0;
    const dim3 eg(pw_max, n_charts);
    if (elem_bytes == 4)
        chart_envelope_kernel<int32_t><<<eg, CH_THREADS, 0, st>>>((const int32_t*)table, (long)stride, series, plans, pw_max, env);
    else
        chart_envelope_kernel<int64_t><<<eg, CH_THREADS, 0, st>>>((const int64_t*)table, (long)stride, series, plans, pw_max, env);
    CHECK_LAUNCH(ctx, "chart_envelope");
    chart_paint_kernel<<<dim3(cdiv(pw_max, CH_TILE_W), cdiv(ph_max, CH_TILE_H), n_charts), CH_THREADS, 0, st>>>(env, series, plans, pw_max,
                                                                                                               out, h, w, ink);
    CHECK_LAUNCH(ctx, "chart_paint");
    return AVCER_OK;
}
