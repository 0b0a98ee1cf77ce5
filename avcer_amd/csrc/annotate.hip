// The drawing of the result video (video/functions/get_visualization.py:40-118): face boxes, label backdrops and text masks drawn
// into the frame batch where it lies, so that decode -> draw -> encode never brings a pixel to the host.
//
// The kernel restates avcer_amd/annotate.py draw_numpy pixel for pixel, and that restates PIL's ImageDraw (rectangle with outline
// and width, bitmap with a fill colour): integer arithmetic only, one rounding per blend.  A frame's items are drawn one after
// another in list order; the unit of parallelism is therefore the PIXEL, never the item: one thread owns one pixel of the frame's
// covered area, walks that frame's items in order and keeps the pixel in registers in between, so two items never race for it.
#include "common.h"

namespace {

constexpr int TILE_W = 64, TILE_H = 4;  // one wave per row of 64 pixels = 192 contiguous bytes per wave access
constexpr int WORK_INTS = 8;            // a row of the work table, see avcer_annotate_frames in include/avcer_hip.h

// Coverage 0..255 of pixel (x, y) by one item.  All sums in 64 bits: no item, however far off the frame, wraps.
__device__ __forceinline__ int item_coverage(const avcer_draw_item& it, int x, int y, const uint8_t* __restrict__ masks, long masks_bytes,
                                             const int32_t* __restrict__ table, int n_masks) {
    const long x0 = it.x0, y0 = it.y0, x1 = it.x1, y1 = it.y1, a = it.arg;
    if (a < 1) return 0;
    if (it.kind == AVCER_DRAW_OUTLINE) {
        // ImagingDrawRectangle without fill: per border line i < a the rows y0 + i and y1 - i over x0..x1, and the columns x0 + i
        // and x1 - i from row y0 + a towards row y1 - a + 1, the far end not drawn (Draw.c line8/line32, vertical case)
        if (x1 < x0 || y1 < y0) return 0;
        const bool rows = x >= x0 && x <= x1 && ((y >= y0 && y <= y0 + a - 1) || (y >= y1 - a + 1 && y <= y1));
        const long p = y0 + a, q = y1 - a + 1;
        const long lo = p < q ? p : q + 1, hi = p < q ? q - 1 : p;
        const bool cols = ((x >= x0 && x <= x0 + a - 1) || (x >= x1 - a + 1 && x <= x1)) && y >= lo && y <= hi;
        return rows || cols ? 255 : 0;
    }
    if (it.kind == AVCER_DRAW_FILL) return (a <= 255 && x >= x0 && x <= x1 && y >= y0 && y <= y1) ? (int)a : 0;
    if (it.kind == AVCER_DRAW_MASK) {
        if (it.mask < 0 || it.mask >= n_masks) return 0;
        const long off = table[3 * it.mask], w = table[3 * it.mask + 1], h = table[3 * it.mask + 2];
        if (off < 0 || w <= 0 || h <= 0 || off + w * h > masks_bytes) return 0;
        const long dx = x - x0, dy = y - y0;
        if (dx < 0 || dy < 0 || dx >= a * w || dy >= a * h) return 0;
        return masks[off + (dy / a) * w + dx / a];
    }
    return 0;
}

// PIL's BLEND8 (ImagingUtils.h): the SUM of both products divided by 255 with one rounding, the MULDIV255 shift form
__device__ __forceinline__ int blend8(int cov, int dst, int ink) {
    const int t = dst * (255 - cov) + ink * cov + 128;
    return ((t >> 8) + t) >> 8;
}

__global__ void __launch_bounds__(TILE_W * TILE_H) annotate_kernel(uint8_t* __restrict__ frames, int n, int H, int W,
                                                                   const avcer_draw_item* __restrict__ items, int m,
                                                                   const uint8_t* __restrict__ masks, long masks_bytes,
                                                                   const int32_t* __restrict__ table, int n_masks,
                                                                   const int32_t* __restrict__ work, int n_work) {
    const int b = blockIdx.x;
    int lo = 0, hi = n_work - 1;  // the last row whose first tile is <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (work[mid * WORK_INTS + 6] <= b) lo = mid; else hi = mid - 1;
    }
    const int32_t* wr = work + (long)lo * WORK_INTS;
    const int f = wr[0], i0 = wr[1], i1 = wr[2], tiles_x = wr[5], t = b - wr[6];
    if (f < 0 || f >= n || i0 < 0 || i1 > m || tiles_x <= 0 || t < 0) return;
    const long x = (long)wr[3] + (long)(t % tiles_x) * TILE_W + (threadIdx.x % TILE_W);
    const long y = (long)wr[4] + (long)(t / tiles_x) * TILE_H + (threadIdx.x / TILE_W);
    if (x < 0 || x >= W || y < 0 || y >= H) return;  // nothing outside the frame is ever addressed
    uint8_t* px = frames + (((long)f * H + y) * W + x) * 3;
    int v0 = 0, v1 = 0, v2 = 0;
    bool loaded = false;
    for (int i = i0; i < i1; ++i) {
        const avcer_draw_item& it = items[i];
        if (it.frame != f) continue;
        const int cov = item_coverage(it, (int)x, (int)y, masks, masks_bytes, table, n_masks);
        if (cov == 0) continue;
        if (!loaded) {
            v0 = px[0]; v1 = px[1]; v2 = px[2];
            loaded = true;
        }
        v0 = blend8(cov, v0, it.colour[0] & 255);
        v1 = blend8(cov, v1, it.colour[1] & 255);
        v2 = blend8(cov, v2, it.colour[2] & 255);
    }
    if (loaded) {  // byte stores: a frame of odd byte size starts at an odd address
        px[0] = (uint8_t)v0; px[1] = (uint8_t)v1; px[2] = (uint8_t)v2;
    }
}

}  // namespace

extern "C" int avcer_annotate_frames(avcer_ctx* ctx, uint8_t* frames, int n, int h, int w, const avcer_draw_item* items, int m,
                                     const uint8_t* masks, int64_t masks_bytes, const int32_t* table, int n_masks, const int32_t* work,
                                     int n_work, int64_t n_tiles, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (!frames || n <= 0 || h <= 0 || w <= 0 || m < 0 || n_masks < 0 || masks_bytes < 0 || n_work < 0 || n_tiles < 0 ||
        n_tiles > 0x7fffffffL || (m > 0 && !items) || (n_masks > 0 && (!masks || !table)) || (n_work > 0 && !work))
        return set_err(ctx, AVCER_EINVAL, "annotate_frames: bad arguments");
    if (m == 0 || n_work == 0 || n_tiles == 0) return AVCER_OK;  // nothing to draw: nothing is launched
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    annotate_kernel<<<(int)n_tiles, TILE_W * TILE_H, 0, (hipStream_t)stream>>>(frames, n, h, w, items, m, masks, (long)masks_bytes, table,
                                                                             n_masks, work, n_work);
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}
