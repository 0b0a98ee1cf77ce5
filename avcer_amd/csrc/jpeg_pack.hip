// JPEG entropy coding on the device.
// avcer_jpeg_pack: write_file / encode_block / BitWriter of jpeg_encode.hip on the device, byte for byte.  A WAVE codes one 8 x 8
// block, lane k
// the coefficient at zigzag position k: a ballot of the non-zero ACs gives every lane its zero run (the distance to the set bit
// below it), so each lane knows its own bits -- up to three ZRL codes, the run / size code, the value bits: 59 at the most,
// one 64-bit register -- and a prefix sum over the wave's lengths says where they go.  Lane 0 codes the DC difference against the
// block libjpeg codes before it in the same component (read straight from the coefficients: the prediction needs no scan),
// lane 63 the EOB when the last coefficient is zero.  Seven launches, none of them waits for the host:
//   check   one workgroup: plan_consistent and the storage bounds of every descriptor; valid files take consecutive WORK ITEMS
//           (one per block, in scan order) by a prefix sum over their n_blocks -- ascending whatever order coef_block has;
//   count   a wave per item: the block's bit count (and status 16 for a coefficient without a code);
//   scan    a workgroup per file: exclusive prefix sum of the bit counts along the scan -> every block's bit offset in its file
//           (32 bits; the 64-bit total decides whether they hold, else status 17), and zeros where the file's bits will land;
//   emit    a wave per item: the bits again, merged in LDS into whole 32-bit words, stored MSB first into the file's UNSTUFFED
//           scan -- plain stores for the words a block owns, vector atomic ORs for the two it may share with its neighbours;
//   stuff   a workgroup per file: the 0xFF bytes of that scan (its last byte filled with ones) -> the file's length;
//   place   one workgroup: files take the next free bytes of `out` in file order, one that does not fit takes none (status 12);
//   write   a workgroup per file: header, the scan with a zero behind every 0xFF (a second prefix sum, over the 0xFF counts), EOI.
// The bytes of a file depend on its descriptor and coefficients alone: bit offsets are relative to the file, items are found by
// search and not by launch geometry, and no file reads another's scratch.
#include "jpeg.h"

namespace {

constexpr int BLOCK_WORDS = 52;                      // an unstuffed block: ceil((20 + 63 * 26) / 8) = 208 bytes at the most
constexpr int64_t PACK_MAX_BITS = (1LL << 32) - 64;  // of one file's scan: bit offsets inside a file are 32 bits wide

struct PackTables {
    uint32_t dc[2][12];   // size << 16 | code of a DC category; [0] luma, [1] chroma
    uint32_t ac[2][256];  // ... of an AC run / size symbol
    uint8_t nat[64];      // kNatural
    uint8_t head[624];    // write_header's bytes; tables, size and sampling are patched in (HEAD_*)
};
constexpr int HEAD_QT0 = 25, HEAD_QT1 = 94, HEAD_SOF = 158;  // offsets of the two tables' 64 bytes and of the SOF0 segment

// EncTable, packed
constexpr void pack_codes(uint32_t* t, int count, const uint8_t* seg) {
    const uint8_t* bits = seg + 5;
    const uint8_t* vals = seg + 21;
    int c = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++p, ++c)
            if (vals[p] < count) t[vals[p]] = ((uint32_t)l << 16) | (uint32_t)c;
        c <<= 1;
    }
}

constexpr PackTables make_pack_tables() {
    PackTables t{};
    pack_codes(t.dc[0], 12, kDhtDc0);
    pack_codes(t.ac[0], 256, kDhtAc0);
    pack_codes(t.dc[1], 12, kDhtDc1);
    pack_codes(t.ac[1], 256, kDhtAc1);
    for (int k = 0; k < 64; ++k) t.nat[k] = kNatural[k];
    const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    const uint8_t sof[19] = {0xFF, 0xC0, 0, 17, 8, 0, 0, 0, 0, 3, 1, 0, 0, 2, 0x11, 1, 3, 0x11, 1};
    const uint8_t sos[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    int p = 0;
    for (int i = 0; i < 20; ++i) t.head[p++] = app0[i];
    for (int q = 0; q < 2; ++q) {
        t.head[p++] = 0xFF; t.head[p++] = 0xDB; t.head[p++] = 0; t.head[p++] = 67; t.head[p++] = (uint8_t)q;
        p += 64;
    }
    for (int i = 0; i < 19; ++i) t.head[p++] = sof[i];
    for (int i = 0; i < 33; ++i) t.head[p++] = kDhtDc0[i];
    for (int i = 0; i < 183; ++i) t.head[p++] = kDhtAc0[i];
    for (int i = 0; i < 33; ++i) t.head[p++] = kDhtDc1[i];
    for (int i = 0; i < 183; ++i) t.head[p++] = kDhtAc1[i];
    for (int i = 0; i < 14; ++i) t.head[p++] = sos[i];
    return t;
}
static_assert(make_pack_tables().head[HEAD_SOF + 1] == 0xC0 && make_pack_tables().head[HEADER_BYTES - 2] == 63, "header layout");
__device__ const PackTables kPack = make_pack_tables();

// the file that holds work item w: the last one that starts at or before it (wb ascends; a file without items starts where the
// next one does and is never the last such)
__device__ __forceinline__ int file_of_item(const int64_t* __restrict__ wb, int n, int64_t w) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (wb[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Block s of a file's scan (write_file's loops: MCU after MCU, hs * vs luma blocks, Cb, Cr): its place among the file's
// coefficient blocks, the block coded before it in its component (-1: it is the first) and its table set (0 luma, 1 chroma)
struct ScanAt { int64_t b, prev; int tb; };
__device__ __forceinline__ ScanAt scan_block(const Desc* __restrict__ d, int64_t s) {
    const int nl = d->hs * d->vs, per = nl + 2;
    const int64_t mcu = s / per;
    const int k = (int)(s % per);
    ScanAt a;
    if (k < nl) {
        const int mx = d->bw[1];
        const auto luma = [&](int64_t m, int kk) {
            return ((m / mx) * d->vs + kk / d->hs) * (int64_t)d->bw[0] + (m % mx) * d->hs + kk % d->hs;
        };
        a.b = luma(mcu, k);
        a.prev = k > 0 ? luma(mcu, k - 1) : (mcu > 0 ? luma(mcu - 1, nl - 1) : -1);
        a.tb = 0;
    } else {
        const int64_t y = (int64_t)d->bw[0] * d->bh[0], c = (int64_t)d->bw[1] * d->bh[1];
        a.b = y + (k - nl) * c + mcu;  // chroma blocks are one per MCU, in MCU order
        a.prev = mcu > 0 ? a.b - 1 : -1;
        a.tb = 1;
    }
    return a;
}

// encode_block, the part of lane `lane`: its bits (right-aligned, first bit on top) and their count; bad: no code for the value
struct Code { uint64_t bits; int len; bool bad; };
__device__ __forceinline__ Code lane_code(const int16_t* __restrict__ blocks, const ScanAt& at, int lane) {
    int t = blocks[64 * at.b + kPack.nat[lane]];
    const uint64_t nz = __ballot(lane > 0 && t != 0);
    Code r = {0, 0, false};
    if (lane == 0) {
        t -= at.prev >= 0 ? (int)blocks[64 * at.prev] : 0;
        int t2 = t;
        if (t < 0) { t = -t; --t2; }
        const int nb = t ? 32 - __clz(t) : 0;
        if (nb > 11) {
            r.bad = true;
        } else {
            const uint32_t e = kPack.dc[at.tb][nb];
            r.bits = ((uint64_t)(e & 0xffff) << nb) | ((uint32_t)t2 & ((1u << nb) - 1));
            r.len = (int)(e >> 16) + nb;
        }
    } else if (t != 0) {
        const uint64_t below = nz & ((1ULL << lane) - 1);
        const int run = below ? lane - 1 - (63 - __clzll((long long)below)) : lane - 1;
        int t2 = t;
        if (t < 0) { t = -t; --t2; }
        const int nb = 32 - __clz(t);
        if (nb > 10) {
            r.bad = true;
        } else {
            const uint32_t zrl = kPack.ac[at.tb][0xF0], e = kPack.ac[at.tb][((run & 15) << 4) | nb];
            for (int z = run >> 4; z > 0; --z) {
                r.bits = (r.bits << (zrl >> 16)) | (zrl & 0xffff);
                r.len += (int)(zrl >> 16);
            }
            r.bits = (((r.bits << (e >> 16)) | (e & 0xffff)) << nb) | ((uint32_t)t2 & ((1u << nb) - 1));
            r.len += (int)(e >> 16) + nb;
        }
    } else if (lane == 63) {
        const uint32_t e = kPack.ac[at.tb][0];
        r.bits = e & 0xffff;
        r.len = (int)(e >> 16);
    }
    return r;
}

__global__ void __launch_bounds__(PACK_THREADS) pack_check_kernel(const Desc* __restrict__ desc, int n, int64_t blocks, int64_t* __restrict__ wb,
                                                                  int32_t* __restrict__ status, int32_t* __restrict__ range) {
    __shared__ int64_t tot[PACK_WAVES];
    int64_t carry = 0;
    for (int c0 = 0; c0 < n; c0 += PACK_THREADS) {
        const int i = c0 + (int)threadIdx.x;
        int64_t nb = 0;
        int st = R_OK;
        if (i < n) {
            const Desc& d = desc[i];
            if (d.status != AVCER_JPEG_OK) st = d.reason ? d.reason : R_ENC_DESC;
            else if (!plan_consistent(d) || d.n_blocks > blocks || d.coef_block > blocks - d.n_blocks) st = R_ENC_DESC;
            else nb = d.n_blocks;
        }
        int64_t total;
        const int64_t end = carry + block_scan(nb, tot, &total);
        if (i < n) {
            if (nb && end > blocks) st = R_ENC_DESC;  // the files of a call share no blocks: together they fit the storage
            wb[i] = end - nb;
            status[i] = st;
            range[i] = 0;
        }
        carry += total;
    }
    if (threadIdx.x == 0) wb[n] = carry;
}

// the item of this wave: false when there is none (past the last file's items, or in a file that is not coded)
__device__ __forceinline__ bool pack_item(const Desc* __restrict__ desc, int n, const int64_t* __restrict__ wb, int64_t blocks,
                                          const int32_t* __restrict__ status, int64_t* w, int* i, ScanAt* at) {
    *w = (int64_t)blockIdx.x * PACK_WAVES + (threadIdx.x >> 6);
    if (*w >= blocks || *w >= wb[n]) return false;
    *i = file_of_item(wb, n, *w);
    const int64_t s = *w - wb[*i];
    if (status[*i] != R_OK || s >= desc[*i].n_blocks) return false;
    *at = scan_block(desc + *i, s);
    return true;
}

__global__ void __launch_bounds__(PACK_THREADS) pack_count_kernel(const int16_t* __restrict__ coeffs, const Desc* __restrict__ desc, int n,
                                                                  const int64_t* __restrict__ wb, int64_t blocks,
                                                                  const int32_t* __restrict__ status, int32_t* __restrict__ range,
                                                                  uint32_t* __restrict__ nbits) {
    const int lane = threadIdx.x & 63;
    int64_t w;
    int i;
    ScanAt at;
    if (!pack_item(desc, n, wb, blocks, status, &w, &i, &at)) return;  // the whole wave
    const Code c = lane_code(coeffs + 64 * desc[i].coef_block, at, lane);
    const bool bad = __any(c.bad);
    const int sum = wave_scan(c.len, lane);
    if (lane == 63) {
        nbits[w] = bad ? 0u : (uint32_t)sum;
        if (bad) range[i] = 1;  // every wave that sees one stores the same 1
    }
}

__global__ void __launch_bounds__(PACK_THREADS) pack_scan_kernel(const int64_t* __restrict__ wb, const int32_t* __restrict__ range,
                                                                 int32_t* __restrict__ status, uint32_t* __restrict__ nbits,
                                                                 int64_t* __restrict__ fbits, uint32_t* __restrict__ stream) {
    __shared__ uint32_t tot[PACK_WAVES];
    const int i = blockIdx.x, t = threadIdx.x;
    int st = status[i];
    if (st == R_OK && range[i]) st = R_RANGE;
    __syncthreads();  // every thread has read the status thread 0 is going to overwrite
    const int64_t base = wb[i], nb = st == R_OK ? wb[i + 1] - base : 0;
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < nb; c0 += PACK_THREADS) {
        const uint32_t v = c0 + t < nb ? nbits[base + c0 + t] : 0u;
        uint32_t total;
        const uint32_t incl = block_scan(v, tot, &total);
        if (c0 + t < nb) nbits[base + c0 + t] = (uint32_t)carry + incl - v;  // wraps only in a file that is then not written
        carry += total;
    }
    if (st == R_OK && carry > PACK_MAX_BITS) st = R_SIZE;
    if (st != R_OK) carry = 0;
    if (t == 0) {
        status[i] = st;
        fbits[i] = carry;
    }
    // every word the file's bits touch (and one more, where the storage has it)
    const int64_t words = min((carry + 31) / 32 + 1, BLOCK_WORDS * nb);
    uint32_t* fs = stream + BLOCK_WORDS * base;
    for (int64_t j = t; j < words; j += PACK_THREADS) fs[j] = 0u;
}

__global__ void __launch_bounds__(PACK_THREADS) pack_emit_kernel(const int16_t* __restrict__ coeffs, const Desc* __restrict__ desc, int n,
                                                                 const int64_t* __restrict__ wb, int64_t blocks,
                                                                 const int32_t* __restrict__ status, const uint32_t* __restrict__ bitoff,
                                                                 uint32_t* __restrict__ stream) {
    __shared__ uint32_t buf[PACK_WAVES][BLOCK_WORDS + 4];  // a block's bits behind up to 31 of its predecessor's: 53 words
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t w;
    int i = 0;
    ScanAt at;
    const bool live = pack_item(desc, n, wb, blocks, status, &w, &i, &at);  // the same for the whole wave
    Code c = {0, 0, false};
    if (live) c = lane_code(coeffs + 64 * desc[i].coef_block, at, lane);
    if (lane < BLOCK_WORDS + 4) buf[wave][lane] = 0u;
    __syncthreads();
    const int incl = wave_scan(c.len, lane);
    const uint32_t at_bit = live ? bitoff[w] : 0u;
    const int lead = (int)(at_bit & 31);
    if (c.len) {
        const int rel = lead + incl - c.len, sh = rel & 31;
        const uint64_t v = c.bits << (64 - c.len);
        const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
        uint32_t* p = buf[wave] + (rel >> 5);
        atomicOr(p, hi >> sh);
        const uint32_t w1 = sh ? (hi << (32 - sh)) | (lo >> sh) : lo, w2 = sh ? lo << (32 - sh) : 0u;
        if (w1) atomicOr(p + 1, w1);
        if (w2) atomicOr(p + 2, w2);
    }
    __syncthreads();
    const int words = (lead + __shfl(incl, 63, 64) + 31) >> 5;
    if (live && lane < words) {
        const uint32_t x = buf[wave][lane];
        uint32_t* dst = stream + BLOCK_WORDS * wb[i] + (at_bit >> 5) + lane;
        if (lane == 0 || lane == words - 1) {
            if (x) atomicOr(dst, x);  // a word the neighbouring block may write as well
        } else {
            *dst = x;
        }
    }
}

// Word j of a file's unstuffed scan as it is written: byte k is x >> (24 - 8 k), the first *valid of them belong to the scan,
// and the scan's last byte is filled up with ones (BitWriter::flush)
__device__ __forceinline__ uint32_t scan_word(const uint32_t* __restrict__ fs, int64_t j, int64_t bits, int* valid) {
    const int64_t nbytes = (bits + 7) >> 3;
    const int v = (int)min((int64_t)4, nbytes - 4 * j);
    uint32_t x = fs[j];
    if (4 * j + v == nbytes && (bits & 7)) x |= (0xFFu >> (bits & 7)) << (24 - 8 * (v - 1));
    *valid = v;
    return x;
}

__device__ __forceinline__ uint32_t count_ff(uint32_t x, int valid) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += k < valid && ((x >> (24 - 8 * k)) & 0xFF) == 0xFF;
    return c;
}

__global__ void __launch_bounds__(PACK_THREADS) pack_stuff_kernel(const int64_t* __restrict__ wb, const int32_t* __restrict__ status,
                                                                  const int64_t* __restrict__ fbits, const uint32_t* __restrict__ stream,
                                                                  int64_t* __restrict__ flen) {
    __shared__ uint32_t tot[PACK_WAVES];
    const int i = blockIdx.x, t = threadIdx.x;
    const bool live = status[i] == R_OK;
    const int64_t bits = live ? fbits[i] : 0, nbytes = (bits + 7) >> 3, words = (nbytes + 3) >> 2;
    const uint32_t* fs = stream + BLOCK_WORDS * wb[i];
    uint32_t c = 0;
    for (int64_t j = t; j < words; j += PACK_THREADS) {
        int valid;
        const uint32_t x = scan_word(fs, j, bits, &valid);
        c += count_ff(x, valid);
    }
    uint32_t total;
    block_scan(c, tot, &total);
    if (t == 0) flen[i] = live ? (int64_t)HEADER_BYTES + nbytes + total + 2 : 0;
}

// avcer_jpeg_write_batch's loop over the files: in file order, one that fits takes the next free bytes.  What a file takes
// depends on every file before it, so one thread walks them, PACK_THREADS at a time out of LDS (n is hundreds to thousands).
__global__ void __launch_bounds__(PACK_THREADS) pack_place_kernel(const int64_t* __restrict__ flen, int n, int64_t cap, int64_t* __restrict__ offsets,
                                                                  int32_t* __restrict__ status, int64_t* __restrict__ need) {
    __shared__ int64_t len[PACK_THREADS];
    __shared__ int32_t st[PACK_THREADS];
    const int t = threadIdx.x;
    int64_t used = 0, needed = 0;
    for (int c0 = 0; c0 < n; c0 += PACK_THREADS) {
        if (c0 + t < n) {
            len[t] = flen[c0 + t];
            st[t] = status[c0 + t];
        }
        __syncthreads();
        if (t == 0)
            for (int k = 0; k < min(PACK_THREADS, n - c0); ++k) {
                offsets[c0 + k] = used;
                if (st[k] != R_OK) continue;
                needed += len[k];
                if (len[k] > cap - used) status[c0 + k] = R_NO_SPACE; else used += len[k];
            }
        __syncthreads();
    }
    if (t == 0) {
        offsets[n] = used;
        *need = needed;
    }
}

__global__ void __launch_bounds__(PACK_THREADS) pack_write_kernel(const Desc* __restrict__ desc, const int64_t* __restrict__ wb,
                                                                  const int32_t* __restrict__ status, const int64_t* __restrict__ fbits,
                                                                  const int64_t* __restrict__ flen, const uint32_t* __restrict__ stream,
                                                                  const int64_t* __restrict__ offsets, uint8_t* __restrict__ out) {
    __shared__ uint32_t tot[PACK_WAVES];
    const int i = blockIdx.x, t = threadIdx.x;
    if (status[i] != R_OK) return;  // the whole workgroup
    const Desc& d = desc[i];
    uint8_t* file = out + offsets[i];
    for (int k = t; k < (int)HEADER_BYTES; k += PACK_THREADS) {
        uint8_t b = kPack.head[k];
        if (k >= HEAD_QT0 && k < HEAD_QT0 + 64) b = (uint8_t)d.qt[0][kPack.nat[k - HEAD_QT0]];
        else if (k >= HEAD_QT1 && k < HEAD_QT1 + 64) b = (uint8_t)d.qt[1][kPack.nat[k - HEAD_QT1]];
        else if (k == HEAD_SOF + 5) b = (uint8_t)(d.height >> 8);
        else if (k == HEAD_SOF + 6) b = (uint8_t)d.height;
        else if (k == HEAD_SOF + 7) b = (uint8_t)(d.width >> 8);
        else if (k == HEAD_SOF + 8) b = (uint8_t)d.width;
        else if (k == HEAD_SOF + 11) b = (uint8_t)((d.hs << 4) | d.vs);
        file[k] = b;
    }
    const int64_t bits = fbits[i], nbytes = (bits + 7) >> 3, words = (nbytes + 3) >> 2;
    const uint32_t* fs = stream + BLOCK_WORDS * wb[i];
    int64_t carry = 0;  // 0xFF bytes in front of this round's words
    for (int64_t j0 = 0; j0 < words; j0 += PACK_THREADS) {
        const int64_t j = j0 + t;
        int valid = 0;
        const uint32_t x = j < words ? scan_word(fs, j, bits, &valid) : 0u;
        const uint32_t c = count_ff(x, valid);
        uint32_t total;
        const uint32_t incl = block_scan(c, tot, &total);
        uint8_t* q = file + HEADER_BYTES + 4 * j + carry + (incl - c);
        for (int k = 0; k < valid; ++k) {
            const uint8_t b = (uint8_t)(x >> (24 - 8 * k));
            *q++ = b;
            if (b == 0xFF) *q++ = 0;
        }
        carry += total;
    }
    if (t == 0) {
        file[flen[i] - 2] = 0xFF;
        file[flen[i] - 1] = 0xD9;
    }
}

}  // namespace

extern "C" int avcer_jpeg_pack(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const avcer_jpeg_desc* desc, int n, uint8_t* out,
                               int64_t cap_bytes, int64_t* offsets, int32_t* status, int64_t* bytes_needed, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (!coeffs || !desc || !offsets || !status || !bytes_needed || n <= 0 || n_blocks <= 0 || n_blocks >= (1LL << 31) || cap_bytes < 0 ||
        (cap_bytes && !out) || ((uintptr_t)desc & 15) || ((uintptr_t)offsets & 7) || ((uintptr_t)bytes_needed & 7) || ((uintptr_t)status & 3))
        return set_err(ctx, AVCER_EINVAL, "jpeg_pack: bad arguments (n %d, %lld blocks < 2^31, %lld bytes; descriptors 16-byte aligned)", n,
                       (long long)n_blocks, (long long)cap_bytes);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    int64_t *wb = nullptr, *fbits = nullptr, *flen = nullptr;
    int32_t* range = nullptr;
    uint32_t *nbits = nullptr, *bits = nullptr;
    TRY(ws_carve(ctx, WS_JPEG, "jpeg_pack", [&](Arena& a) {
        wb = a.get<int64_t>(sizeof(int64_t) * ((size_t)n + 1));      // first work item of every file, and the end of the last
        fbits = a.get<int64_t>(sizeof(int64_t) * (size_t)n);         // bits of every file's scan
        flen = a.get<int64_t>(sizeof(int64_t) * (size_t)n);          // bytes of every file
        range = a.get<int32_t>(sizeof(int32_t) * (size_t)n);         // a coefficient without a code was seen
        nbits = a.get<uint32_t>(sizeof(uint32_t) * (size_t)n_blocks);  // per item: its bit count, then its bit offset in the file
        bits = a.get<uint32_t>(sizeof(uint32_t) * BLOCK_WORDS * (size_t)n_blocks);  // the unstuffed scans, BLOCK_WORDS per item
    }));
    const unsigned per_item = (unsigned)((n_blocks + PACK_WAVES - 1) / PACK_WAVES);
    LAUNCH(ctx, pack_check_kernel<<<1, PACK_THREADS, 0, st>>>(desc, n, n_blocks, wb, status, range));
    LAUNCH(ctx, pack_count_kernel<<<per_item, PACK_THREADS, 0, st>>>(coeffs, desc, n, wb, n_blocks, status, range, nbits));
    LAUNCH(ctx, pack_scan_kernel<<<(unsigned)n, PACK_THREADS, 0, st>>>(wb, range, status, nbits, fbits, bits));
    LAUNCH(ctx, pack_emit_kernel<<<per_item, PACK_THREADS, 0, st>>>(coeffs, desc, n, wb, n_blocks, status, nbits, bits));
    LAUNCH(ctx, pack_stuff_kernel<<<(unsigned)n, PACK_THREADS, 0, st>>>(wb, status, fbits, bits, flen));
    LAUNCH(ctx, pack_place_kernel<<<1, PACK_THREADS, 0, st>>>(flen, n, cap_bytes, offsets, status, bytes_needed));
    LAUNCH(ctx, pack_write_kernel<<<(unsigned)n, PACK_THREADS, 0, st>>>(desc, wb, status, fbits, flen, bits, offsets, out));
    return AVCER_OK;
}
