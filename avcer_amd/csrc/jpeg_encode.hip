// JPEG encoding, the mirror image of jpeg_decode.hip: the device computes the quantised coefficients of every image straight from the
// decoded frames
// (avcer_jpeg_forward: one launch per batch), the host writes the files (avcer_jpeg_write_batch: headers and Huffman coding, a
// small thread pool, files are independent) -- or the device does that as well (avcer_jpeg_pack, jpeg_pack.hip: a wave per block,
// prefix sums for the bit and byte positions; whole files leave the device, and the host writer is its oracle).  All of it restates
// libjpeg(-turbo)'s compressor with the parameters PIL's
// Image.save(f, "JPEG", quality=q, subsampling=s) gives it -- jccolor.c, jcsample.c, jcprepct.c's edges, jfdctint.c ("islow"),
// jcdctmgr.c's quantisation, jccoefct.c's dummy blocks, jcmarker.c, jchuff.c with the standard tables -- and the contract is
// byte-identity with the file PIL writes (tests/test_jpeg_encode_host.py holds the numpy statement of the kernel,
// avcer_amd/jpeg.py forward_numpy, and the writer to PIL; tests/test_gpu_jpeg_encode.py holds the kernel to both).
//
// Dummy blocks (those that only pad a component to whole MCUs; with chroma at 1 x 1 only luma has any) get their final value in
// the KERNEL: zero AC and the DC of the block libjpeg codes before them in the MCU.  The writer codes what it is given.
#include "jpeg.h"

namespace {

// ------------------------------------------------------------------------------------------------ host: tables and headers
// jcparam.c: the standard's two example tables, natural order
const uint8_t kStdLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                              80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72,
                              92, 95, 98, 112, 100, 103, 99};
const uint8_t kStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// code and length of every symbol of one DHT segment (jpeg_make_c_derived_tbl: canonical codes in the order of the values)
struct EncTable {
    uint16_t code[256];
    uint8_t size[256];
    explicit EncTable(const uint8_t* seg) {
        memset(code, 0, sizeof(code));
        memset(size, 0, sizeof(size));
        const uint8_t* bits = seg + 5;   // counts of lengths 1..16
        const uint8_t* vals = seg + 21;
        int c = 0, p = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < bits[l - 1]; ++i, ++p, ++c) {
                code[vals[p]] = (uint16_t)c;
                size[vals[p]] = (uint8_t)l;
            }
            c <<= 1;
        }
    }
};

void quant_tables(int quality, uint16_t qt[2][64]) {
    const int q = std::min(std::max(quality, 1), 100);          // jpeg_quality_scaling
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int k = 0; k < 64; ++k) {                              // jpeg_add_quant_table, force_baseline
        qt[0][k] = (uint16_t)std::min(std::max((kStdLuma[k] * scale + 50) / 100, 1), 255);
        qt[1][k] = (uint16_t)std::min(std::max((kStdChroma[k] * scale + 50) / 100, 1), 255);
    }
}

// jcmarker.c for PIL's call: SOI, JFIF 1.01 (no units, 1 : 1), DQT 0 and 1 (zigzag order), SOF0, the four standard DHT, SOS
uint8_t* write_header(const Desc& d, uint8_t* p) {
    static const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    memcpy(p, app0, sizeof(app0));
    p += sizeof(app0);
    for (int t = 0; t < 2; ++t) {
        *p++ = 0xFF; *p++ = 0xDB; *p++ = 0; *p++ = 67; *p++ = (uint8_t)t;
        for (int k = 0; k < 64; ++k) *p++ = (uint8_t)d.qt[t][kNatural[k]];
    }
    const uint8_t sof[19] = {0xFF, 0xC0, 0, 17, 8, (uint8_t)(d.height >> 8), (uint8_t)d.height, (uint8_t)(d.width >> 8), (uint8_t)d.width, 3,
                             1, (uint8_t)((d.hs << 4) | d.vs), 0, 2, 0x11, 1, 3, 0x11, 1};
    memcpy(p, sof, sizeof(sof));
    p += sizeof(sof);
    memcpy(p, kDhtDc0, sizeof(kDhtDc0)); p += sizeof(kDhtDc0);
    memcpy(p, kDhtAc0, sizeof(kDhtAc0)); p += sizeof(kDhtAc0);
    memcpy(p, kDhtDc1, sizeof(kDhtDc1)); p += sizeof(kDhtDc1);
    memcpy(p, kDhtAc1, sizeof(kDhtAc1)); p += sizeof(kDhtAc1);
    static const uint8_t sos[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    memcpy(p, sos, sizeof(sos));
    return p + sizeof(sos);
}

// ------------------------------------------------------------------------------------------------ host: entropy-coded segment
// jchuff.c's bit buffer: bits leave from the top, a 0xFF byte is followed by a stuffed zero.  put() takes at most 16 bits and
// leaves fewer than 8 behind, so the 64-bit accumulator never loses one.
struct BitWriter {
    uint8_t* p;
    uint64_t acc = 0;
    int n = 0;
    inline void put(uint32_t bits, int size) {
        acc = (acc << size) | bits;
        n += size;
        while (n >= 8) {
            const uint8_t b = (uint8_t)(acc >> (n - 8));
            *p++ = b;
            if (b == 0xFF) *p++ = 0;
            n -= 8;
        }
    }
    inline void flush() { put(0x7F, 7); n = 0; }  // the last byte filled up with ones
};

inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// The most one block can take: a DC code (<= 9 bits) and 11 value bits, 63 AC codes (<= 16 bits) with 10 value bits each, all of
// it 0xFF bytes that double: 2 * ceil((20 + 63 * 26) / 8) = 416 bytes.  The writer keeps this much room, the final byte and EOI
// (BLOCK_ROOM) free before every block, so put() never checks.
constexpr size_t BLOCK_ROOM = 416 + 2 + 2;

// encode_one_block.  false: a coefficient the standard tables have no code for (more than 11 bits of DC difference, 10 of AC)
inline bool encode_block(BitWriter& bw, const int16_t* blk, int& pred, const EncTable& dc, const EncTable& ac) {
    int t = blk[0] - pred, t2 = t;
    pred = blk[0];
    if (t < 0) { t = -t; --t2; }
    int nb = bit_length((unsigned)t);
    if (nb > 11) return false;
    bw.put(dc.code[nb], dc.size[nb]);
    if (nb) bw.put((uint32_t)t2 & ((1u << nb) - 1), nb);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        t = blk[kNatural[k]];
        if (t == 0) { ++run; continue; }
        for (; run > 15; run -= 16) bw.put(ac.code[0xF0], ac.size[0xF0]);
        t2 = t;
        if (t < 0) { t = -t; --t2; }
        nb = bit_length((unsigned)t);
        if (nb > 10) return false;
        const int sym = (run << 4) | nb;
        bw.put(ac.code[sym], ac.size[sym]);
        bw.put((uint32_t)t2 & ((1u << nb) - 1), nb);
        run = 0;
    }
    if (run) bw.put(ac.code[0], ac.size[0]);
    return true;
}

// One file into `buf` (grown as needed): its length in *len.  Returns a reason.
int write_file(const int16_t* coeffs, const Desc& d, std::vector<uint8_t>& buf, size_t* len) {
    static const EncTable dc0(kDhtDc0), ac0(kDhtAc0), dc1(kDhtDc1), ac1(kDhtAc1);
    *len = 0;
    if (!plan_consistent(d)) return R_ENC_DESC;
    if (buf.size() < HEADER_BYTES + BLOCK_ROOM) buf.resize(HEADER_BYTES + BLOCK_ROOM + 4096);
    BitWriter bw;
    bw.p = write_header(d, buf.data());
    const int mx = d.bw[1], my = d.bh[1];
    const int ch[3] = {d.hs, 1, 1}, cv[3] = {d.vs, 1, 1};
    const int64_t base[3] = {0, (int64_t)d.bw[0] * d.bh[0], (int64_t)d.bw[0] * d.bh[0] + (int64_t)d.bw[1] * d.bh[1]};
    const int16_t* blocks = coeffs + 64 * d.coef_block;
    int pred[3] = {0, 0, 0};
    for (int y = 0; y < my; ++y)
        for (int x = 0; x < mx; ++x) {
            const size_t at = (size_t)(bw.p - buf.data());
            if (buf.size() - at < BLOCK_ROOM * (size_t)(d.hs * d.vs + 2)) {
                buf.resize(2 * buf.size() + BLOCK_ROOM * 6);
                bw.p = buf.data() + at;
            }
            for (int c = 0; c < 3; ++c)
                for (int v = 0; v < cv[c]; ++v)
                    for (int u = 0; u < ch[c]; ++u) {
                        const int64_t b = base[c] + (int64_t)(y * cv[c] + v) * d.bw[c] + (x * ch[c] + u);
                        if (!encode_block(bw, blocks + 64 * b, pred[c], c ? dc1 : dc0, c ? ac1 : ac0)) return R_RANGE;
                    }
        }
    bw.flush();
    *bw.p++ = 0xFF;
    *bw.p++ = 0xD9;
    *len = (size_t)(bw.p - buf.data());
    return R_OK;
}

// ------------------------------------------------------------------------------------------------ device
// libjpeg's jfdctint.c (jpeg_fdct_islow), one 1-D pass over 8 values.  FIRST: the row pass, results scaled up by 2^PASS1_BITS;
// else the column pass, which takes that factor out again (the factor 8 of the 2-D transform stays: the quantiser divides by 8 q).
//
// Range: 32-bit integers hold it.  Samples are within +-128, so the row pass leaves at most 8 * 128 * 4 = 4096 in d[0] / d[4] and
// (a 1-D DCT with libjpeg's scaling has gain < 8 * sqrt(2) / 2) < 4100 elsewhere.  In the column pass a difference tmp4..7 is then
// < 8200, z3 + z4 < 32800, the largest product 32800 * 9633 < 3.2e8 and the largest sum of products
// 8200 * (25172 + 2 * 20995 + 2 * 16069) + 3.2e8 < 1.2e9 < 2^31.  The first pass is smaller by the factor 4100 / 128.
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(int (&d)[8]) {
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int SH = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    const auto descale = [](int x) { return (x + (1 << (SH - 1))) >> SH; };
    if (FIRST) {
        d[0] = (tmp10 + tmp11) << PASS1_BITS;
        d[4] = (tmp10 - tmp11) << PASS1_BITS;
    } else {
        d[0] = (tmp10 + tmp11 + (1 << (PASS1_BITS - 1))) >> PASS1_BITS;
        d[4] = (tmp10 - tmp11 + (1 << (PASS1_BITS - 1))) >> PASS1_BITS;
    }
    int z1 = (tmp12 + tmp13) * 4433;
    d[2] = descale(z1 + tmp13 * 6270);
    d[6] = descale(z1 + tmp12 * -15137);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    tmp4 *= 2446;
    tmp5 *= 16819;
    tmp6 *= 25172;
    tmp7 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = descale(tmp4 + z1 + z3);
    d[5] = descale(tmp5 + z2 + z4);
    d[3] = descale(tmp6 + z2 + z3);
    d[1] = descale(tmp7 + z1 + z4);
}

// One component sample of a source pixel: libjpeg's jccolor.c, 16-bit fixed point (Cb and Cr carry 128 and round with 32767)
__device__ __forceinline__ int ycc_at(const uint8_t* __restrict__ px, int c, int bgr) {
    const int r = px[bgr ? 2 : 0], g = px[1], b = px[bgr ? 0 : 2];
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

constexpr int FWD_THREADS = 256;  // 4 waves, 8 blocks each

// the descriptor's three components are grids of blocks that fill its n_blocks, inside the storage: what a store into the
// component planes relies on (a descriptor avcer_jpeg_plan wrote passes; the full check is plan_consistent)
__device__ __forceinline__ bool planes_fit(const Desc& d, long n_blocks) {
    if (d.bw[0] < 1 || d.bw[1] < 1 || d.bw[2] < 1 || d.bh[0] < 1 || d.bh[1] < 1 || d.bh[2] < 1 || d.bw[0] > 16384 || d.bw[1] > 16384 ||
        d.bw[2] > 16384 || d.bh[0] > 16384 || d.bh[1] > 16384 || d.bh[2] > 16384)
        return false;
    const long all = (long)d.bw[0] * d.bh[0] + (long)d.bw[1] * d.bh[1] + (long)d.bw[2] * d.bh[2];
    return d.coef_block >= 0 && d.n_blocks == all && all <= n_blocks - d.coef_block;
}

// The forward kernel, shaped like jpeg_idct_kernel.  A wave takes 8 consecutive blocks of the coefficient storage; lane = 8 *
// block + j.  Lane j fetches the source pixels of ROW j of its block -- 8 for luma and for chroma at 1 x 1, 16 under 4:2:2, two
// rows of 16 under 4:2:0 -- straight from the rectangle of the frame (single-byte loads: a row starts at any byte), converts
// them, averages for chroma and runs the row pass in registers; the column pass and the way back to rows go through LDS.  Then
// it quantises row j (the table row is one 16-byte load) and stores it with one 16-byte store, natural order.
// LDS rows are 9 dwords and blocks 72.  Row access (after pass 1, and the final read) is dword 72 b + 9 j + k, column access
// (pass 2) 72 b + 9 r + j; all are 4-byte accesses, served per 32-lane half (b = 0..3) over 32 banks: 8 b + 9 j mod 32 takes 32
// different values for b < 4, j < 8 (9 j mod 32 = 0, 9, 18, 27, 4, 13, 22, 31, and 8 b shifts them into the gaps), and so does
// 8 b + j: neither order has a bank conflict.  A lane's pass-2 writes go where its own reads came from, so two barriers suffice.
//
// Edges (jcprepct.c): columns repeat the last pixel; luma rows repeat the last row; chroma rows under 4:2:0 repeat the last
// input row only to make the height even, and the last DOWNSAMPLED row from there down.  A dummy block runs on the pixels of the
// block whose DC it inherits -- a real row's dummy on its left neighbour, a dummy row's on the last block of the row above in its
// MCU -- and keeps the DC alone.  Frame, slot and coordinates are clamped to the tensor: a wrong rectangle reads wrong pixels,
// never outside `src`.
//
// PLANES (avcer_jpeg_roundtrip_*): the lane does not stop at row j of the quantised block.  It multiplies it by the table row it
// has just divided by, leaves the products where it read the row from (its own dwords of LDS: no barrier) and goes on as kernel A
// of the decoder does behind its dequantisation (idct_block_store): the block's samples reach the component planes without the
// coefficients having left the chip.  `coeffs` may then be null; given, they are stored as well, dummy blocks included.
template <bool PLANES>
__device__ __forceinline__ void forward_block(int (&ws)[FWD_THREADS / 64][8 * 8 * WS_LD], const uint8_t* __restrict__ src, int N, int H,
                                              int W, const int32_t* __restrict__ rects, const Desc* __restrict__ desc, int n, int bgr,
                                              int16_t* __restrict__ coeffs, long n_blocks, uint8_t* __restrict__ planes,
                                              int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane >> 3, j = lane & 7;
    const long g = ((long)blockIdx.x * (FWD_THREADS / 64) + wave) * 8 + b;
    int* w = ws[wave] + b * 8 * WS_LD;
    bool live = false, dummy = false, wild = false;
    const uint16_t* qrow = nullptr;
    uint8_t* dst = nullptr;  // PLANES: row j of the block in its component plane; null where the descriptor's geometry has no room for it
    int v[8], i = 0;
    if (g < n_blocks) {
        i = image_of_block(desc, n, g);
        const Desc* d = desc + i;
        const long r = g - d->coef_block;
        if (d->status == AVCER_JPEG_OK && r >= 0 && r < d->n_blocks) {
            live = true;
            const long c0 = (long)d->bw[0] * d->bh[0], c1 = c0 + (long)d->bw[1] * d->bh[1];
            const int c = r < c0 ? 0 : (r < c1 ? 1 : 2);
            const long rr = r - (c == 0 ? 0 : (c == 1 ? c0 : c1));
            int by = (int)(rr / d->bw[c]), bx = (int)(rr % d->bw[c]);
            const int wd = d->width, ht = d->height;
            if (PLANES && planes_fit(*d, n_blocks) && rr < (long)d->bw[c] * d->bh[c])
                dst = planes + 64 * (d->coef_block + (r - rr)) + ((long)by * 8 + j) * (d->bw[c] * 8) + bx * 8;  // as jpeg_idct_kernel
            const int hs = c ? d->hs : 1, vs = c ? d->vs : 1;  // source pixels per sample of this component
            if (c == 0) {
                const int wb = (wd + 7) >> 3, hb = (ht + 7) >> 3;
                if (by >= hb) {
                    by -= 1;
                    bx = bx / d->hs * d->hs + d->hs - 1;
                    dummy = true;
                }
                if (bx >= wb) {
                    bx = wb - 1;
                    dummy = true;
                }
            }
            qrow = d->qt[c] + 8 * j;
            const int slot = min(max(rects[5 * i], 0), N - 1), x0 = rects[5 * i + 1], y0 = rects[5 * i + 2];
            const uint8_t* frame = src + (long)slot * H * W * 3;
            const int row = min(8 * by + j, (ht + vs - 1) / vs - 1);  // the sample row, the last one repeated
            const int bias = hs == 1 ? 0 : (vs == 1 ? 0 : 1), shift = hs + vs - 2;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int acc = hs == 1 ? 0 : bias + (k & 1);  // jcsample.c: 0, 1, 0, 1 (h2v1) and 1, 2, 1, 2 (h2v2) along a row
                for (int dy = 0; dy < vs; ++dy) {
                    const int y = min(max(y0 + min(row * vs + dy, ht - 1), 0), H - 1);
                    for (int dx = 0; dx < hs; ++dx) {
                        const int x = min(max(x0 + min((8 * bx + k) * hs + dx, wd - 1), 0), W - 1);
                        acc += ycc_at(frame + ((long)y * W + x) * 3, c, bgr);
                    }
                }
                v[k] = (acc >> shift) - 128;
            }
            fdct_1d<true>(v);
#pragma unroll
            for (int k = 0; k < 8; ++k) w[j * WS_LD + k] = v[k];
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = w[r * WS_LD + j];
        fdct_1d<false>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) w[r * WS_LD + j] = v[r];
    }
    __syncthreads();
    if (live) {
        const int4 qv = *reinterpret_cast<const int4*>(qrow);
        const int qw[4] = {qv.x, qv.y, qv.z, qv.w};
        uint32_t o[4];
        int dq[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            // jcdctmgr.c: divide by 8 q, halves away from zero
            const int x = w[j * WS_LD + k];
            const uint32_t q8 = ((k & 1) ? (uint32_t)qw[k >> 1] >> 16 : (uint32_t)qw[k >> 1] & 0xffff) << 3;
            const uint32_t a = ((uint32_t)abs(x) + (q8 >> 1)) / q8;
            int q = x < 0 ? -(int)a : (int)a;
            if (dummy && (j | k)) q = 0;
            if (k & 1) o[k >> 1] |= (uint32_t)q << 16; else o[k >> 1] = (uint32_t)q & 0xffff;
            dq[k] = (int)(int16_t)q * (int)(q8 >> 3);  // what the decoder multiplies: the int16 it would read, and q
        }
        if (!PLANES || coeffs) *reinterpret_cast<uint4*>(coeffs + 64 * g + 8 * j) = make_uint4(o[0], o[1], o[2], o[3]);
        if (PLANES) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                w[j * WS_LD + k] = dq[k];
                wild = wild || abs(dq[k]) > IDCT_PAIR_MAX;
            }
        }
    }
    if (PLANES) idct_block_store(w, j, live && dst, wild, dst, flags + i);
}

__global__ void __launch_bounds__(FWD_THREADS) jpeg_forward_kernel(const uint8_t* __restrict__ src, int N, int H, int W,
                                                                   const int32_t* __restrict__ rects, const Desc* __restrict__ desc, int n,
                                                                   int bgr, int16_t* __restrict__ coeffs, long n_blocks) {
    __shared__ int ws[FWD_THREADS / 64][8 * 8 * WS_LD];
    forward_block<false>(ws, src, N, H, W, rects, desc, n, bgr, coeffs, n_blocks, nullptr, nullptr);
}

__global__ void __launch_bounds__(FWD_THREADS) jpeg_roundtrip_kernel(const uint8_t* __restrict__ src, int N, int H, int W,
                                                                     const int32_t* __restrict__ rects, const Desc* __restrict__ desc, int n,
                                                                     int bgr, int16_t* __restrict__ coeffs, long n_blocks,
                                                                     uint8_t* __restrict__ planes, int32_t* __restrict__ flags) {
    __shared__ int ws[FWD_THREADS / 64][8 * 8 * WS_LD];
    forward_block<true>(ws, src, N, H, W, rects, desc, n, bgr, coeffs, n_blocks, planes, flags);
}

// The flags of avcer_jpeg_roundtrip_*, before the kernel above runs: 0, or 1 for a descriptor avcer_jpeg_plan did not write or
// whose blocks leave the storage -- kernel B reads the planes through the descriptor's geometry, so it must not see such an image
__global__ void roundtrip_check_kernel(const Desc* __restrict__ desc, int n, long n_blocks, int32_t* __restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Desc& d = desc[i];
    flags[i] = d.status == AVCER_JPEG_OK && !(plan_consistent(d) && d.n_blocks <= n_blocks - d.coef_block) ? 1 : 0;
}

// avcer_jpeg_roundtrip_*: arguments, workspace, the flags and the fused kernel; *planes is what kernel B then reads
int jpeg_roundtrip_planes(avcer_ctx* ctx, const char* what, const uint8_t* src, int N, int H, int W, const int32_t* rects, const Desc* desc,
                          int n, int bgr, int16_t* coeffs, int64_t n_blocks, int32_t* flags, const void* out, uint8_t** planes,
                          hipStream_t st) {
    const int frames[3] = {N, H, W};
    TRY(coeff_args(ctx, what, coeffs, true, n_blocks, desc, n,
                   src && rects && flags && out && N > 0 && H > 0 && W > 0 && !((uintptr_t)rects & 3) && !((uintptr_t)flags & 3), frames));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TRY(jpeg_plane_ws(ctx, n_blocks, planes));
    LAUNCH(ctx, roundtrip_check_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(desc, n, (long)n_blocks, flags));
    const long per = FWD_THREADS / 64 * 8;
    LAUNCH(ctx, jpeg_roundtrip_kernel<<<(unsigned)((n_blocks + per - 1) / per), FWD_THREADS, 0, st>>>(
                    src, N, H, W, rects, desc, n, bgr ? 1 : 0, coeffs, (long)n_blocks, *planes, flags));
    return AVCER_OK;
}

}  // namespace

extern "C" int avcer_jpeg_quant_tables(int quality, uint16_t qt[2][64]) {
    if (!qt || quality < 1 || quality > 100) return AVCER_EINVAL;
    quant_tables(quality, qt);
    return AVCER_OK;
}

extern "C" int avcer_jpeg_plan(const int32_t* sizes, int n, int subsampling, int quality, avcer_jpeg_desc* desc, int64_t* blocks_needed) {
    if (n < 0 || (n && (!sizes || !desc)) || subsampling < 0 || subsampling > 2 || quality < 1 || quality > 100) return AVCER_EINVAL;
    uint16_t qt[2][64];
    quant_tables(quality, qt);
    const int hs = subsampling ? 2 : 1, vs = subsampling == 2 ? 2 : 1;
    int64_t used = 0;
    for (int i = 0; i < n; ++i) {
        Desc& d = desc[i];
        memset(&d, 0, sizeof(d));
        d.width = sizes[2 * i];
        d.height = sizes[2 * i + 1];
        d.ncomp = 3;
        d.hs = hs;
        d.vs = vs;
        d.coef_block = used;
        if (d.width < 1 || d.width > 65535 || d.height < 1 || d.height > 65535) {
            not_handled(d, R_ENC_SIZE);
            continue;
        }
        const int mx = (d.width + 8 * hs - 1) / (8 * hs), my = (d.height + 8 * vs - 1) / (8 * vs);
        d.bw[0] = mx * hs;
        d.bh[0] = my * vs;
        d.bw[1] = d.bw[2] = mx;
        d.bh[1] = d.bh[2] = my;
        d.tq[1] = d.tq[2] = 1;
        memcpy(d.qt[0], qt[0], sizeof(qt[0]));
        memcpy(d.qt[1], qt[1], sizeof(qt[1]));
        memcpy(d.qt[2], qt[1], sizeof(qt[1]));
        d.n_blocks = (int64_t)mx * my * (hs * vs + 2);
        used += d.n_blocks;
    }
    if (blocks_needed) *blocks_needed = used;
    return AVCER_OK;
}

extern "C" int avcer_jpeg_write_batch(avcer_ctx* ctx, const int16_t* coeffs, avcer_jpeg_desc* desc, int n, uint8_t* out, int64_t cap_bytes,
                                      int64_t* offsets, int threads, int64_t* bytes_needed) {
    // ctx may be NULL (host-only call, no device needed): errors then come back as the code alone
    if (n < 0 || (n && (!coeffs || !desc)) || !offsets || cap_bytes < 0 || (cap_bytes && !out))
        return set_err(ctx, AVCER_EINVAL, "jpeg_write_batch: bad arguments");
    try {
        // every file into a buffer of its own, in parallel; then, in file order, each takes the next free bytes of `out` (a file
        // that does not fit is not written and takes nothing), and the copies run in parallel again
        std::vector<std::vector<uint8_t>> files((size_t)n);
        std::vector<size_t> lens((size_t)n, 0);
        const int nt = threads_for(threads, n);
        each_index(n, nt, [&](int i) {
            if (desc[i].status != AVCER_JPEG_OK) return;
            const int r = write_file(coeffs, desc[i], files[i], &lens[i]);
            if (r != R_OK) {
                lens[i] = 0;
                not_handled(desc[i], r);
            }
        });
        // bytes, not blocks, and an offset for every file and one behind the last: not place_blocks
        int64_t used = 0, needed = 0;
        for (int i = 0; i < n; ++i) {
            offsets[i] = used;
            if (desc[i].status != AVCER_JPEG_OK) continue;
            needed += (int64_t)lens[i];
            if ((int64_t)lens[i] > cap_bytes - used) {
                not_handled(desc[i], R_NO_SPACE);
                lens[i] = 0;
            }
            used += (int64_t)lens[i];
        }
        offsets[n] = used;
        if (bytes_needed) *bytes_needed = needed;
        each_index(n, nt, [&](int i) {
            if (lens[i]) memcpy(out + offsets[i], files[i].data(), lens[i]);
        });
    } catch (...) {
        return set_err(ctx, AVCER_ENOMEM, "jpeg_write_batch: out of host memory");
    }
    return AVCER_OK;
}

extern "C" int avcer_jpeg_forward(avcer_ctx* ctx, const uint8_t* src, int N, int H, int W, const int32_t* rects, const avcer_jpeg_desc* desc,
                                  int n, int bgr, int16_t* coeffs, int64_t n_blocks, avcer_stream_t stream) {
    const int frames[3] = {N, H, W};
    TRY(coeff_args(ctx, "jpeg_forward", coeffs, false, n_blocks, desc, n,
                   src && rects && N > 0 && H > 0 && W > 0 && !((uintptr_t)rects & 3), frames));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const long per = FWD_THREADS / 64 * 8;
    LAUNCH(ctx, jpeg_forward_kernel<<<(unsigned)((n_blocks + per - 1) / per), FWD_THREADS, 0, (hipStream_t)stream>>>(
                    src, N, H, W, rects, desc, n, bgr ? 1 : 0, coeffs, (long)n_blocks));
    return AVCER_OK;
}

extern "C" int avcer_jpeg_roundtrip_tiles(avcer_ctx* ctx, const uint8_t* src, int N, int H, int W, const int32_t* rects,
                                          const avcer_jpeg_desc* desc, int n, int bgr, int16_t* coeffs, int64_t n_blocks, int32_t* flags,
                                          uint8_t* tiles, avcer_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    uint8_t* planes = nullptr;
    TRY(jpeg_roundtrip_planes(ctx, "jpeg_roundtrip_tiles", src, N, H, W, rects, desc, n, bgr, coeffs, n_blocks, flags, tiles, &planes, st));
    return launch_jpeg_tiles(ctx, planes, desc, flags, n, tiles, st);
}

extern "C" int avcer_jpeg_roundtrip_rgb(avcer_ctx* ctx, const uint8_t* src, int N, int H, int W, const int32_t* rects,
                                        const avcer_jpeg_desc* desc, int n, int bgr, int16_t* coeffs, int64_t n_blocks, int32_t* flags,
                                        uint8_t* canvas, int hmax, int wmax, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    TRY(canvas_args(ctx, "jpeg_roundtrip_rgb", n, hmax, wmax));
    hipStream_t st = (hipStream_t)stream;
    uint8_t* planes = nullptr;
    TRY(jpeg_roundtrip_planes(ctx, "jpeg_roundtrip_rgb", src, N, H, W, rects, desc, n, bgr, coeffs, n_blocks, flags, canvas, &planes, st));
    return launch_jpeg_canvas(ctx, planes, desc, flags, n, hmax, wmax, canvas, st);
}
