// Uncompressed video frames of an AVI file (BI_RGB device-independent bitmaps, 24 or 32 bits a pixel) unpacked into the frame batch
// [n, H, W, 3] the detector and the crop kernels read.  Definition: include/avcer_hip.h avcer_dib_frames; the CPU statement of the
// same bytes is avcer_amd/dib.py unpack_numpy (PIL's BMP reader, tolerance zero).
//
// There is no arithmetic: every output byte is one source byte.  A source frame is H rows of `stride` = (W * bits / 8 + 3) & ~3
// bytes, the last row of the picture first when bottom-up, B G R (X) per pixel; the output drops the row padding and the fourth
// byte, turns the rows over and, for RGB order, swaps the first and third byte of every pixel.
//
// Shape.  As jpeg_frames_kernel: a thread owns one 16-byte ALIGNED piece of one output row (rows are 3 W bytes and start wherever
// that leaves them; the first and last piece of a row are cut to the row and go out as byte stores, every piece between as one
// 16-byte store, a wave stores 1 KiB of one row).  The source bytes of a piece are a window of 16 (24-bit, same order), 20 (24-bit,
// swapped: two bytes on either side) or 24 bytes (32-bit: six pixels) at an address of ANY alignment -- chunk data in an AVI file
// are 2-byte aligned, the span may start anywhere, and a row of 3 W output bytes moves against its source row.  The window is read
// as the two or three aligned 16-byte chunks it touches and shifted into place in registers (whole dwords by selects, the rest by
// a funnel shift).
// Bounds.  A chunk is read with one wide load only where all 16 bytes lie inside the uploaded span; where it straddles an end of
// the span, the bytes inside are read one by one and the others are taken as zero: nothing outside [span, span + span_bytes) is
// read, whatever the offset table holds.  A frame whose offset does not leave stride * H bytes inside the span is written as zeros.
#include "common.h"

namespace {

constexpr int DIB_THREADS = 256;

// The 16 bytes at span[pos, pos + 16) (span + pos is 16-byte aligned); bytes outside [0, n) read as zero and are not touched
__device__ __forceinline__ void span16(const uint8_t* __restrict__ span, long pos, long n, uint32_t* q) {
    if (pos >= 0 && pos + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(span + pos);
        q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
        return;
    }
    q[0] = q[1] = q[2] = q[3] = 0;
    for (int j = 0; j < 16; ++j)
        if (pos + j >= 0 && pos + j < n) q[j >> 2] |= (uint32_t)span[pos + j] << (8 * (j & 3));
}

// w[0 .. 5] = the 24 bytes span[p, p + 24), of which the caller uses the first NEED (16, 20 or 24); p of any alignment and sign
template <int NEED>
__device__ __forceinline__ void window(const uint8_t* __restrict__ span, long p, long n, uint32_t (&w)[6]) {
    const int m = (int)(((uintptr_t)span + (uintptr_t)p) & 15);  // two's complement: right for p < 0 as well
    const long a = p - m;
    uint32_t q[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) q[i] = 0;
    span16(span, a, n, q);
    if (m + NEED > 16) span16(span, a + 16, n, q + 4);
    if (m + NEED > 32) span16(span, a + 32, n, q + 8);
    // down by m bytes: m / 4 whole dwords in two select stages, then m % 4 bytes across neighbouring dwords
    uint32_t r[9], s[7];
#pragma unroll
    for (int i = 0; i < 9; ++i) r[i] = (m & 8) ? q[i + 2] : q[i];
#pragma unroll
    for (int i = 0; i < 7; ++i) s[i] = (m & 4) ? r[i + 1] : r[i];
    const int sh = 8 * (m & 3);
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = (uint32_t)((((uint64_t)s[i + 1] << 32) | s[i]) >> sh);
}

// The bytes b of a dword with (b + s) % 3 == 0, s in 0 .. 2
__device__ __forceinline__ uint32_t every_third(int s) { return s == 0 ? 0xFF0000FFu : s == 1 ? 0x00FF0000u : 0x0000FF00u; }

template <int BITS, bool SWAP>
__global__ void __launch_bounds__(DIB_THREADS) dib_frames_kernel(const uint8_t* __restrict__ span, long span_bytes,
                                                                 const int64_t* __restrict__ offsets, int n, int H, int W, int per_row,
                                                                 int bottom_up, uint8_t* __restrict__ frames) {
    const long idx = (long)blockIdx.x * DIB_THREADS + threadIdx.x;
    if (idx >= (long)n * H * per_row) return;
    const int piece = (int)(idx % per_row);
    const long row = idx / per_row;  // t * H + y
    const int y = (int)(row % H), t = (int)(row / H);
    uint8_t* const out = frames + row * 3L * W;
    // the piece in bytes of the row: [wb, wb + 16), wb < 0 where the row starts inside its first aligned piece
    const int wb = 16 * piece - (int)((uintptr_t)out & 15);
    if (wb >= 3 * W) return;
    const long stride = ((long)W * (BITS / 8) + 3) & ~3L;
    const long off = offsets[t];
    uint32_t o4[4] = {0, 0, 0, 0};
    if (off >= 0 && off <= span_bytes - stride * H) {
        const long src = off + (long)(bottom_up ? H - 1 - y : y) * stride;  // the source row, from the span's first byte
        uint32_t w[6];
        if (BITS == 24 && !SWAP) {
            window<16>(span, src + wb, span_bytes, w);
#pragma unroll
            for (int d = 0; d < 4; ++d) o4[d] = w[d];
        } else if (BITS == 24) {
            // output byte j of channel c = (wb + j) % 3 is source byte wb + j + 2 - 2 c of the row: of the window that starts at
            // row byte wb - 2, the 16 bytes from 4 on (c = 0), from 2 on (c = 1) or from 0 on (c = 2)
            window<20>(span, src + wb - 2, span_bytes, w);
            const int c0 = ((wb % 3) + 3) % 3;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const uint32_t mid = (w[d] >> 16) | (w[d + 1] << 16);
                o4[d] = (w[d + 1] & every_third((c0 + d) % 3)) | (mid & every_third((c0 + d + 2) % 3)) | (w[d] & every_third((c0 + d + 1) % 3));
            }
        } else {
            // the piece holds bytes of the six pixels from k0 = floor(wb / 3) on: 24 source bytes, 18 packed, 16 of those from byte wb - 3 k0
            const int k0 = wb >= 0 ? wb / 3 : -((2 - wb) / 3);
            window<24>(span, src + 4L * k0, span_bytes, w);
            uint32_t px[6];
#pragma unroll
            for (int i = 0; i < 6; ++i)
                px[i] = SWAP ? ((w[i] & 0x0000FF00u) | ((w[i] >> 16) & 0xFFu) | ((w[i] & 0xFFu) << 16)) : (w[i] & 0x00FFFFFFu);
            uint32_t d[5];
            d[0] = px[0] | (px[1] << 24);
            d[1] = (px[1] >> 8) | (px[2] << 16);
            d[2] = (px[2] >> 16) | (px[3] << 8);
            d[3] = px[4] | (px[5] << 24);
            d[4] = px[5] >> 8;
            const int sh = 8 * (wb - 3 * k0);
#pragma unroll
            for (int k = 0; k < 4; ++k) o4[k] = (uint32_t)((((uint64_t)d[k + 1] << 32) | d[k]) >> sh);
        }
    }
    if (wb >= 0 && wb + 16 <= 3 * W) {
        *reinterpret_cast<uint4*>(out + wb) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
    } else {  // a row's first or last piece: only the bytes that are the row's
#pragma unroll
        for (int m = 0; m < 16; ++m)
            if (wb + m >= 0 && wb + m < 3 * W) out[wb + m] = (uint8_t)(o4[m >> 2] >> (8 * (m & 3)));
    }
}

}  // namespace

extern "C" int avcer_dib_frames(avcer_ctx* ctx, const uint8_t* span, int64_t span_bytes, const int64_t* offsets, int n, uint8_t* frames,
                                int H, int W, int bits, int bottom_up, int bgr, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (n < 0 || span_bytes < 0 || (n > 0 && (!span || !offsets || !frames))) return set_err(ctx, AVCER_EINVAL, "dib_frames: null pointer or negative size");
    if (bits != 24 && bits != 32) return set_err(ctx, AVCER_EINVAL, "dib_frames: %d bits a pixel (24 or 32)", bits);
    if (H <= 0 || W <= 0 || H > 65535 || W > 65535 || (long)n * H * W >= (1L << 36))
        return set_err(ctx, AVCER_EINVAL, "dib_frames: frames %d x %d x %d (1..65535 a side, fewer than 2^36 pixels)", n, H, W);
    if (n == 0) return AVCER_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int per_row = (3 * W + 15) / 16 + 1;  // aligned 16-byte pieces a row of 3 W bytes can touch
    const long total = (long)n * H * per_row;
    const long grid = (total + DIB_THREADS - 1) / DIB_THREADS;
    if (grid > 0x7fffffffL) return set_err(ctx, AVCER_EINVAL, "dib_frames: too many pieces");
    const bool up = bottom_up != 0;
    if (bits == 24 && bgr)
        dib_frames_kernel<24, false><<<(unsigned)grid, DIB_THREADS, 0, st>>>(span, (long)span_bytes, offsets, n, H, W, per_row, up, frames);
    else if (bits == 24)
        dib_frames_kernel<24, true><<<(unsigned)grid, DIB_THREADS, 0, st>>>(span, (long)span_bytes, offsets, n, H, W, per_row, up, frames);
    else if (bgr)
        dib_frames_kernel<32, false><<<(unsigned)grid, DIB_THREADS, 0, st>>>(span, (long)span_bytes, offsets, n, H, W, per_row, up, frames);
    else
        dib_frames_kernel<32, true><<<(unsigned)grid, DIB_THREADS, 0, st>>>(span, (long)span_bytes, offsets, n, H, W, per_row, up, frames);
    CHECK_LAUNCH(ctx, "dib_frames");
    return AVCER_OK;
}
