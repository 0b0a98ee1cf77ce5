// PIL's Image.resize of a batch of RGB frames (Pillow's Resample.c, the 8 bits-per-channel path) for its convolution filters, bit for
// bit.  Definition and table layout: include/avcer_hip.h avcer_resize_frames; the coefficient tables are built on the host in
// double (avcer_amd/resize.py resize_plan), the CPU statement of the same arithmetic is resize_numpy there.
//
// The arithmetic.  Two separable passes with a u8 value between them, horizontal first.  Per axis and output index o:
//   out = clip(((1 << 21) + sum_{j < count[o]} in[first[o] + j] * kk[o][j]) >> 22, 0, 255)       (int32, arithmetic shift)
// The sums are integer, so no tiling or summation order changes a bit: the two forms below agree by construction.
//
// Shape.  A row is treated as 3 * width BYTES; output byte b belongs to pixel b / 3, channel b % 3.  The unit of work is a DWORD
// of four consecutive output bytes, so that the value between the passes is written to LDS, and the result to the frame, four
// bytes at a time (a wave stores 256 contiguous bytes of one row; a row that does not start on a 4-byte address, and the cut last
// dword of a row, go out as byte stores).
//   h_dwords: four output bytes of RS_RR source rows at once -- a tap is loaded once for RS_RR products per byte.
//   v_dword:  four output bytes of one output row from a column of dwords, one per source row.
// Fused form (one launch, the source is read from HBM once, nothing between the passes touches HBM): a block owns a tile of
// RS_TH output rows x RS_TB output bytes of one frame.  It runs h_dwords over exactly the source rows its vertical taps read --
// rows [lo, hi) with lo = min first, hi = max first + count over the tile's output rows --, leaves them in LDS as u8 rows of RS_TB
// bytes, and runs v_dword out of LDS.  LDS per block = (hi - lo) * RS_TB bytes; the host sizes the launch by the largest tile of
// the vertical table and takes this form when that is at most RS_FUSED_LDS (three blocks per CU of 160 KiB).  The detector's
// downscales: 4 x bilinear needs 73 rows (18.3 KiB, eight blocks per CU by LDS), 3 x lanczos 67 rows.
// General form (any table within the documented limits): the same two device functions as two launches, through a u8
// intermediate [n, H, w2, 3] carved from the context's WS_RESIZE slot; an unchanged axis is skipped, as PIL skips it.
#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TB = 256;                 // output bytes of a row per tile: 64 dwords, one per lane of a wave
constexpr int RS_TD = RS_TB / 4;           // dword columns of a tile
constexpr int RS_TH = 16;                  // output rows per tile
constexpr int RS_RR = 4;                   // source rows per thread that share a horizontal tap
constexpr int RS_FUSED_LDS = 48 * 1024;    // the fused form's LDS limit per block
constexpr int RS_PREC = 22;                // PIL's PRECISION_BITS = 32 - 8 - 2

// One axis' table on the device: first[out], count[out], kk[out][k], back to back (include/avcer_hip.h)
struct Axis {
    const int32_t* first;
    const int32_t* count;
    const int32_t* kk;
    int in, out, k;
};

inline Axis axis_of(const int32_t* tab, int in, int out, int k) { return Axis{tab, tab + out, tab + 2 * (size_t)out, in, out, k}; }

// clip(acc >> 22, 0, 255), written as clamp first, shift second (the same value: a negative sum gives 0, one from 256 << 22 on gives
// 255).  Shift-then-clamp of two neighbours packed into one word is what hipcc turns into gfx950's v_ashr_pk_u8_i32 and then ORs
// with the other two bytes as if the instruction had cleared the word's upper half; on the MI355X it had not, and bytes 2 and 3 of
// every vertically resized dword came out with stray bits set.  This order keeps the packing in plain shifts and ORs.
__device__ __forceinline__ int clip8(int acc) { return min(max(acc, 0), (256 << RS_PREC) - 1) >> RS_PREC; }

// Four bytes to p: one dword store where p is 4-byte aligned and all four belong to the row, else byte stores of the first `valid`
__device__ __forceinline__ void store4(uint8_t* p, uint32_t v, int valid) {
    if (valid >= 4 && ((uintptr_t)p & 3) == 0) {
        *(uint32_t*)p = v;
    } else {
        for (int i = 0; i < valid && i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
    }
}

// Horizontal pass: output bytes [ob, ob + 4) of RS_RR rows.  rows[r]: the source rows (3 * ax.in bytes each; the caller passes a
// valid row for every r, repeating one where it has fewer).  Bytes at or behind 3 * ax.out come back 0.  The source pixel index is
// clamped to the row: a table that breaks first + count <= in gives wrong numbers, never a read outside the row.
__device__ __forceinline__ void h_dwords(const Axis& ax, const uint8_t* const (&rows)[RS_RR], int ob, uint32_t (&out)[RS_RR]) {
#pragma unroll
    for (int r = 0; r < RS_RR; ++r) out[r] = 0;
    const int row_bytes = 3 * ax.out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = ob + i;
        if (b >= row_bytes) break;
        const int px = b / 3, c = b - 3 * px;
        const int f = ax.first[px], cnt = min(ax.count[px], ax.k);
        const int32_t* kk = ax.kk + (long)px * ax.k;
        int acc[RS_RR];
#pragma unroll
        for (int r = 0; r < RS_RR; ++r) acc[r] = 1 << (RS_PREC - 1);
        for (int j = 0; j < cnt; ++j) {
            const int t = kk[j];
            const int s = min(max(f + j, 0), ax.in - 1) * 3 + c;
#pragma unroll
            for (int r = 0; r < RS_RR; ++r) acc[r] += (int)rows[r][s] * t;
        }
#pragma unroll
        for (int r = 0; r < RS_RR; ++r) out[r] |= (uint32_t)clip8(acc[r]) << (8 * i);
    }
}

// Vertical pass: four output bytes of output row oy.  load(r): the dword of those four byte columns in source row r (r already
// relative to what `load` addresses, clamped by the caller's `rows`): LDS in the fused form, the intermediate in the general one.
template <class Load>
__device__ __forceinline__ uint32_t v_dword(const Axis& ay, int oy, int row0, int rows, const Load& load) {
    const int f = ay.first[oy] - row0, cnt = min(ay.count[oy], ay.k);
    const int32_t* kk = ay.kk + (long)oy * ay.k;
    int a0 = 1 << (RS_PREC - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int j = 0; j < cnt; ++j) {
        const int t = kk[j];
        const uint32_t v = load(min(max(f + j, 0), rows - 1));
        a0 += (int)(v & 255) * t;
        a1 += (int)((v >> 8) & 255) * t;
        a2 += (int)((v >> 16) & 255) * t;
        a3 += (int)(v >> 24) * t;
    }
    return (uint32_t)clip8(a0) | ((uint32_t)clip8(a1) << 8) | ((uint32_t)clip8(a2) << 16) | ((uint32_t)clip8(a3) << 24);
}

// Fused form.  Grid: tiles_x * tiles_y * n blocks; lds_rows: the rows of RS_TB bytes the launch has LDS for.
__global__ void __launch_bounds__(RS_THREADS) resize_fused_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n, Axis ax,
                                                                  Axis ay, int tiles_x, int tiles_y, int lds_rows) {
    extern __shared__ uint32_t mid[];  // [rows][RS_TD]: the horizontally resized source rows lo .. hi of the tile's byte columns
    const int W = ax.in, H = ay.in, w2 = ax.out, h2 = ay.out;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, fr = blockIdx.x / (tiles_x * tiles_y);
    if (fr >= n) return;
    const int d = threadIdx.x % RS_TD, rl = threadIdx.x / RS_TD;  // a wave = the 64 dword columns of one row
    const int oy0 = ty * RS_TH, oyn = min(RS_TH, h2 - oy0);
    int lo = H, hi = 0;  // uniform over the block: scalar loads
    for (int i = 0; i < oyn; ++i) {
        const int f = ay.first[oy0 + i];
        lo = min(lo, f);
        hi = max(hi, f + ay.count[oy0 + i]);
    }
    lo = min(max(lo, 0), H - 1);
    const int rows = min(max(hi - lo, 1), lds_rows);  // a table the host did not size the launch for: clamped, wrong numbers
    const uint8_t* const frame = src + (long)fr * H * W * 3;
    const int ob = tx * RS_TB + 4 * d;
    for (int rb = rl * RS_RR; rb < rows; rb += (RS_THREADS / RS_TD) * RS_RR) {
        const uint8_t* rp[RS_RR];
#pragma unroll
        for (int r = 0; r < RS_RR; ++r) rp[r] = frame + (long)min(lo + rb + r, H - 1) * W * 3;
        uint32_t v[RS_RR];
        h_dwords(ax, rp, ob, v);
#pragma unroll
        for (int r = 0; r < RS_RR; ++r)
            if (rb + r < rows) mid[(rb + r) * RS_TD + d] = v[r];
    }
    __syncthreads();
    const int valid = 3 * w2 - ob;
    if (valid <= 0) return;
    for (int i = rl; i < oyn; i += RS_THREADS / RS_TD) {
        const uint32_t v = v_dword(ay, oy0 + i, lo, rows, [&](int r) { return mid[r * RS_TD + d]; });
        store4(dst + ((long)fr * h2 + oy0 + i) * w2 * 3 + ob, v, valid);
    }
}

// General form, horizontal: `rows` rows of 3 * ax.in bytes -> rows of 3 * ax.out bytes.  A block: RS_TD dword columns x 16 rows.
__global__ void __launch_bounds__(RS_THREADS) resize_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long rows, Axis ax,
                                                              int tiles_x) {
    const int tx = blockIdx.x % tiles_x;
    const long r0 = (long)(blockIdx.x / tiles_x) * (RS_THREADS / RS_TD) * RS_RR + (threadIdx.x / RS_TD) * RS_RR;
    const int ob = tx * RS_TB + 4 * (threadIdx.x % RS_TD);
    const int valid = 3 * ax.out - ob;
    if (r0 >= rows || valid <= 0) return;
    const uint8_t* rp[RS_RR];
#pragma unroll
    for (int r = 0; r < RS_RR; ++r) rp[r] = src + min(r0 + r, rows - 1) * ax.in * 3;
    uint32_t v[RS_RR];
    h_dwords(ax, rp, ob, v);
#pragma unroll
    for (int r = 0; r < RS_RR; ++r)
        if (r0 + r < rows) store4(dst + (r0 + r) * ax.out * 3 + ob, v[r], valid);
}

// General form, vertical: n images of ay.in rows of `row_bytes` bytes -> ay.out rows.  One thread per output dword.
__global__ void __launch_bounds__(RS_THREADS) resize_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n, Axis ay,
                                                              int row_bytes, int tiles_x) {
    const int tx = blockIdx.x % tiles_x;
    const long orow = (long)(blockIdx.x / tiles_x) * (RS_THREADS / RS_TD) + threadIdx.x / RS_TD;  // fr * out + oy
    const int ob = tx * RS_TB + 4 * (threadIdx.x % RS_TD);
    const int valid = row_bytes - ob;
    if (orow >= (long)n * ay.out || valid <= 0) return;
    const int oy = (int)(orow % ay.out);
    const uint8_t* const col = src + (orow / ay.out) * ay.in * row_bytes + ob;
    const uint32_t v = v_dword(ay, oy, 0, ay.in, [&](int r) {
        const uint8_t* p = col + (long)r * row_bytes;
        uint32_t w = 0;
        for (int i = 0; i < 4 && i < valid; ++i) w |= (uint32_t)p[i] << (8 * i);
        return w;
    });
    store4(dst + orow * row_bytes + ob, v, valid);
}

// The source rows the largest fused tile of a vertical table reads (first / count on the host)
int fused_rows(const int32_t* ytab, int h2) {
    int most = 1;
    for (int oy0 = 0; oy0 < h2; oy0 += RS_TH) {
        int lo = INT32_MAX, hi = 0;
        for (int i = oy0; i < oy0 + RS_TH && i < h2; ++i) {
            lo = ytab[i] < lo ? ytab[i] : lo;
            hi = ytab[i] + ytab[h2 + i] > hi ? ytab[i] + ytab[h2 + i] : hi;
        }
        most = hi - lo > most ? hi - lo : most;
    }
    return most;
}

// first >= 0, 0 <= count <= k, first + count <= in for every output
bool table_ok(const int32_t* tab, int in, int out, int k) {
    for (int o = 0; o < out; ++o) {
        const long f = tab[o], c = tab[out + o];
        if (f < 0 || c < 0 || c > k || f + c > in) return false;
    }
    return true;
}

}  // namespace

extern "C" int avcer_resize_form(const int32_t* ytab_host, int h2) {
    if (!ytab_host || h2 < 1 || h2 > AVCER_RESIZE_MAX_SIDE) return AVCER_EINVAL;
    return (size_t)fused_rows(ytab_host, h2) * RS_TB <= (size_t)RS_FUSED_LDS ? AVCER_RESIZE_FUSED : AVCER_RESIZE_TWO_PASS;
}

extern "C" int avcer_resize_frames(avcer_ctx* ctx, const uint8_t* src, int n, int h, int w, uint8_t* dst, int h2, int w2,
                                   const int32_t* xtab_host, const int32_t* xtab, int xk, const int32_t* ytab_host, const int32_t* ytab,
                                   int yk, int form, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (!src || !dst || !xtab_host || !xtab || !ytab_host || !ytab) return set_err(ctx, AVCER_EINVAL, "resize_frames: null pointer");
    const int M = AVCER_RESIZE_MAX_SIDE;
    if (n < 0 || h < 1 || w < 1 || h2 < 1 || w2 < 1 || h > M || w > M || h2 > M || w2 > M || xk < 1 || yk < 1)
        return set_err(ctx, AVCER_EINVAL, "resize_frames: %d frames of %d x %d -> %d x %d (width x height): sides must be in 1..%d", n, w, h, w2,
                       h2, M);
    if (form != AVCER_RESIZE_CHOOSE && form != AVCER_RESIZE_FUSED && form != AVCER_RESIZE_TWO_PASS)
        return set_err(ctx, AVCER_EINVAL, "resize_frames: form %d", form);
    if (!table_ok(xtab_host, w, w2, xk) || !table_ok(ytab_host, h, h2, yk))
        return set_err(ctx, AVCER_EINVAL, "resize_frames: a table entry with first < 0, count > ksize or first + count behind the source");
    if (n == 0) return AVCER_OK;
    const int rows = fused_rows(ytab_host, h2);
    const bool fits = (size_t)rows * RS_TB <= (size_t)RS_FUSED_LDS;
    if (form == AVCER_RESIZE_FUSED && !fits)
        return set_err(ctx, AVCER_EINVAL, "resize_frames: a tile reads %d source rows, the fused form holds %d", rows, RS_FUSED_LDS / RS_TB);
    if (form == AVCER_RESIZE_CHOOSE) form = fits ? AVCER_RESIZE_FUSED : AVCER_RESIZE_TWO_PASS;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const Axis ax = axis_of(xtab, w, w2, xk), ay = axis_of(ytab, h, h2, yk);
    const int tiles_x = cdiv(3L * w2, RS_TB);
    if (form == AVCER_RESIZE_FUSED) {
        const int tiles_y = cdiv(h2, RS_TH);
        const long grid = (long)tiles_x * tiles_y * n;
        if (grid > 0x7fffffffL) return set_err(ctx, AVCER_EINVAL, "resize_frames: too many tiles");
        resize_fused_kernel<<<(unsigned)grid, RS_THREADS, (size_t)rows * RS_TB, st>>>(src, dst, n, ax, ay, tiles_x, tiles_y, rows);
        CHECK_LAUNCH(ctx, "resize_fused");
        return AVCER_OK;
    }
    // two launches through the workspace; an axis that keeps its size is skipped (PIL skips that pass)
    const bool do_h = w != w2, do_v = h != h2 || !do_h;
    uint8_t* mid = nullptr;
    if (do_h && do_v) TRY(ws_carve(ctx, WS_RESIZE, "resize_frames", [&](Arena& a) { mid = a.get<uint8_t>((size_t)n * h * w2 * 3); }));
    if (do_h) {
        const long rows_all = (long)n * h;
        const long grid = (long)tiles_x * ((rows_all + 15) / 16);
        if (grid > 0x7fffffffL) return set_err(ctx, AVCER_EINVAL, "resize_frames: too many tiles");
        resize_h_kernel<<<(unsigned)grid, RS_THREADS, 0, st>>>(src, do_v ? mid : dst, rows_all, ax, tiles_x);
        CHECK_LAUNCH(ctx, "resize_h");
    }
    if (do_v) {
        const long grid = (long)tiles_x * (((long)n * h2 + 3) / 4);
        if (grid > 0x7fffffffL) return set_err(ctx, AVCER_EINVAL, "resize_frames: too many tiles");
        resize_v_kernel<<<(unsigned)grid, RS_THREADS, 0, st>>>(do_h ? mid : src, dst, n, ay, 3 * w2, tiles_x);
        CHECK_LAUNCH(ctx, "resize_v");
    }
    return AVCER_OK;
}
