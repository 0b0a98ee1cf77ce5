// JPEG face crops (`<faces>/<track>/NNNNNN.jpg`, get_prob_video.py:79-100 + data/utils.py:34) without a decoder library:
//   host   -- marker parsing and Huffman decoding, serial bit-stream work: one native call per batch of files, files spread over a
//             small thread pool (avcer_jpeg_probe, avcer_jpeg_entropy_batch; ctx may be NULL, no device is touched);
//   device -- everything behind the coefficients (avcer_jpeg_tiles, avcer_jpeg_rgb): kernel A dequantises and runs the inverse
//             DCT into u8 component planes, kernel B computes exactly the output pixels asked for (the 224 x 224 NEAREST tile or
//             the full-size canvas) from them: chroma upsampling at that pixel, YCbCr -> RGB.
// All of it is integer arithmetic and restates what libjpeg(-turbo) computes with its defaults (JDCT_ISLOW, fancy upsampling):
// the contract is bit-identity with PIL's decode (tests/test_jpeg_host.py holds the numpy statement of kernels A and B,
// avcer_amd/jpeg.py pixels_numpy, to PIL; tests/test_gpu_jpeg.py holds the kernels to goldens PIL wrote).
// A file outside the supported subset (include/avcer_hip.h) is REPORTED as not handled and never guessed at; the caller then
// decodes it with PIL as before.
// The Huffman decoding runs on the device as well when asked to (avcer_jpeg_scan_batch + avcer_jpeg_unpack, jpeg_unpack.hip:
// the host then parses headers only, with parse_header below); the host pass above is its oracle.
#include "jpeg.h"

namespace {

// ------------------------------------------------------------------------------------------------ host: markers
// libjpeg's jpeg_make_d_derived_tbl: canonical codes from the counts; a count list that over-subscribes a length is an error there
void derive(Huff& t) {
    t.ok = t.dc_ok = false;
    int size[257], code[257], n = 0;
    for (int l = 1; l <= 16; ++l) {
        if (n + t.bits[l] > 256) return;
        for (int i = 0; i < t.bits[l]; ++i) size[n++] = l;
    }
    int c = 0, si = n ? size[0] : 0, p = 0;
    while (p < n) {
        while (p < n && size[p] == si) code[p++] = c++;
        if (c > (1 << si)) return;
        c <<= 1;
        ++si;
    }
    p = 0;
    memset(t.look, 0, sizeof(t.look));
    for (int l = 1; l <= 16; ++l) {
        if (t.bits[l]) {
            t.valoff[l] = p - code[p];
            if (l <= 9)
                for (int i = 0; i < t.bits[l]; ++i) {
                    const int first = code[p + i] << (9 - l);
                    for (int k = 0; k < (1 << (9 - l)); ++k) t.look[first + k] = (uint16_t)((l << 8) | t.vals[p + i]);
                }
            p += t.bits[l];
            t.maxcode[l] = code[p - 1];
        } else {
            t.maxcode[l] = -1;
            t.valoff[l] = 0;
        }
    }
    t.ok = true;
    t.dc_ok = true;
    for (int i = 0; i < n; ++i) t.dc_ok = t.dc_ok && t.vals[i] <= 15;
}

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// One annex-K table into `t`, from its DHT segment (jpeg.h: marker, length, class / id, 16 counts, the symbols)
void assume_std(Huff& t, const uint8_t* seg, int count) {
    t.bits[0] = 0;
    memcpy(t.bits + 1, seg + 5, 16);
    memset(t.vals, 0, sizeof(t.vals));
    memcpy(t.vals, seg + 21, (size_t)count);
    t.defined = true;
    derive(t);
}

}  // namespace

// Everything up to the first entropy-coded byte.  Returns a reason; on R_OK h.d holds the geometry and the tables of the scan.
// std_tables (AVCER_JPEG_STD_TABLES): a table 0 or 1 the scan references and no DHT segment of the file defined is the standard's
// annex-K table of that class and id -- what libjpeg-turbo (jdhuff.c, std_huff_tables) and ffmpeg's mjpeg2jpeg assume for Motion-JPEG
// frames.  A table the file defines is the file's; ids 2 and 3 have no standard table and stay R_TABLE.
int parse_header(const uint8_t* s, size_t len, Header& h, bool std_tables) {
    h = Header();  // a worker reuses one Header for all its files: no table, id or restart interval of the last one survives
    Desc& d = h.d;
    memset(&d, 0, sizeof(d));
    if (!s || len < 4 || s[0] != 0xFF || s[1] != 0xD8) return R_NO_SOI;
    size_t p = 2;
    bool sof = false, jfif = false, adobe = false;
    int adobe_transform = -1;
    for (;;) {
        if (p + 2 > len) return R_TRUNCATED;
        if (s[p] != 0xFF) return R_MARKER;  // bytes between segments: libjpeg skips them with a warning, this decoder does not guess
        while (p < len && s[p] == 0xFF) ++p;  // fill bytes
        if (p >= len) return R_TRUNCATED;
        const int m = s[p++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return R_MARKER;  // stuffing, TEM, RSTn, SOI, EOI: not in a header
        if (p + 2 > len) return R_TRUNCATED;
        const int L = be16(s + p);
        if (L < 2 || p + (size_t)L > len) return R_TRUNCATED;
        const uint8_t* b = s + p + 2;
        const int n = L - 2;
        p += (size_t)L;
        if (m == 0xC0 || m == 0xC1) {
            if (sof || n < 6) return R_MARKER;
            sof = true;
            if (b[0] != 8) return R_PRECISION;
            d.height = be16(b + 1);
            d.width = be16(b + 3);
            d.ncomp = b[5];
            if (d.height == 0 || d.width == 0) return R_SIZE;  // height 0: a DNL segment would follow
            if (d.ncomp != 1 && d.ncomp != 3) return R_COMPONENTS;
            if (n != 6 + 3 * d.ncomp) return R_MARKER;
            for (int c = 0; c < d.ncomp; ++c) {
                h.comp_id[c] = b[6 + 3 * c];
                h.comp_h[c] = b[7 + 3 * c] >> 4;
                h.comp_v[c] = b[7 + 3 * c] & 15;
                d.tq[c] = b[8 + 3 * c];
                if (h.comp_h[c] < 1 || h.comp_h[c] > 4 || h.comp_v[c] < 1 || h.comp_v[c] > 4 || d.tq[c] > 3) return R_SAMPLING;
            }
            d.hs = h.comp_h[0];
            d.vs = h.comp_v[0];
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4) {
            return R_SOF_KIND;  // progressive, lossless, differential, arithmetic (SOF2..15, DAC, JPG)
        } else if (m == 0xC4) {
            int o = 0;
            while (o < n) {
                if (o + 17 > n) return R_TABLE;
                const int tc = b[o] >> 4, th = b[o] & 15;
                if (tc > 1 || th > 3) return R_TABLE;
                Huff& t = tc ? h.ac[th] : h.dc[th];
                int count = 0;
                t.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) count += (t.bits[l] = b[o + l]);
                if (count > 256 || o + 17 + count > n) return R_TABLE;
                memset(t.vals, 0, sizeof(t.vals));
                memcpy(t.vals, b + o + 17, (size_t)count);
                t.defined = true;
                derive(t);
                o += 17 + count;
            }
        } else if (m == 0xDB) {
            int o = 0;
            while (o < n) {
                const int pq = b[o] >> 4, tq = b[o] & 15;
                if (pq != 0) return R_TABLE;  // 16-bit tables
                if (tq > 3 || o + 65 > n) return R_TABLE;
                for (int k = 0; k < 64; ++k) h.q[tq][kNatural[k]] = b[o + 1 + k];
                h.q_def[tq] = true;
                o += 65;
            }
        } else if (m == 0xDD) {
            if (n != 2) return R_MARKER;
            h.restart = be16(b);
        } else if (m == 0xE0) {
            if (n >= 14 && memcmp(b, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(b, "Adobe", 5) == 0) {
                adobe = true;
                adobe_transform = b[11];
            }
        } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE) {
            // APPn / COM: skipped
        } else if (m == 0xDA) {
            if (!sof) return R_MARKER;
            if (n < 1 || b[0] != d.ncomp || n != 1 + 2 * d.ncomp + 3) return R_SCAN;  // a scan of fewer components: more scans follow
            for (int c = 0; c < d.ncomp; ++c) {
                if (b[1 + 2 * c] != h.comp_id[c]) return R_SCAN;
                h.td[c] = b[2 + 2 * c] >> 4;
                h.ta[c] = b[2 + 2 * c] & 15;
                if (h.td[c] > 3 || h.ta[c] > 3) return R_SCAN;
            }
            const uint8_t* e = b + 1 + 2 * d.ncomp;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return R_SCAN;
            h.scan = p;
            break;
        } else {
            return R_MARKER;  // DNL, DHP, EXP, JPGn, reserved
        }
    }
    // colour: one component is grey; three are YCbCr where libjpeg says so (jdapimin.c default_decompress_parms)
    if (d.ncomp == 3) {
        if (jfif) {
        } else if (adobe) {
            if (adobe_transform != 1) return R_COLOUR;
        } else if (!(h.comp_id[0] == 1 && h.comp_id[1] == 2 && h.comp_id[2] == 3)) {
            return R_COLOUR;
        }
        if (!((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2))) return R_SAMPLING;
        if (h.comp_h[1] != 1 || h.comp_v[1] != 1 || h.comp_h[2] != 1 || h.comp_v[2] != 1) return R_SAMPLING;
        const int mx = (d.width + 8 * d.hs - 1) / (8 * d.hs), my = (d.height + 8 * d.vs - 1) / (8 * d.vs);
        d.bw[0] = mx * d.hs;
        d.bh[0] = my * d.vs;
        d.bw[1] = d.bw[2] = mx;
        d.bh[1] = d.bh[2] = my;
    } else {  // a one-component scan is not interleaved: its MCU is one block whatever the sampling factors say
        d.bw[0] = (d.width + 7) / 8;
        d.bh[0] = (d.height + 7) / 8;
    }
    d.n_blocks = 0;
    if (std_tables)
        for (int c = 0; c < d.ncomp; ++c) {
            if (h.td[c] < 2 && !h.dc[h.td[c]].defined) assume_std(h.dc[h.td[c]], h.td[c] ? kDhtDc1 : kDhtDc0, (int)sizeof(kDhtDc0) - 21);
            if (h.ta[c] < 2 && !h.ac[h.ta[c]].defined) assume_std(h.ac[h.ta[c]], h.ta[c] ? kDhtAc1 : kDhtAc0, (int)sizeof(kDhtAc0) - 21);
        }
    for (int c = 0; c < d.ncomp; ++c) {
        if (!h.q_def[d.tq[c]]) return R_TABLE;
        if (!h.dc[h.td[c]].defined || !h.dc[h.td[c]].dc_ok || !h.ac[h.ta[c]].defined || !h.ac[h.ta[c]].ok) return R_TABLE;
        memcpy(d.qt[c], h.q[d.tq[c]], sizeof(d.qt[c]));
        d.n_blocks += (int64_t)d.bw[c] * d.bh[c];
    }
    // a block costs at least two bits (a DC code and an end-of-block code, one bit each at the least): a file whose header claims
    // more blocks than its bytes can hold is cut short, and is refused here, before anybody reserves storage for its claim
    if (d.n_blocks > 4 * (int64_t)(len - h.scan)) return R_TRUNCATED;
    return R_OK;
}

namespace {

// ------------------------------------------------------------------------------------------------ host: entropy-coded segment
// Bits of the entropy-coded segment, 0xFF00 unstuffed.  A marker or the end of the file stops the supply: bits past it read
// as zero but cannot be CONSUMED (`bad`), so a stream that ends early is an error and never a picture.
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;
    int n = 0;
    bool stop = false, bad = false;
    void fill() {
        while (n <= 48 && !stop) {
            if (p >= end) { stop = true; break; }
            const uint8_t b = *p;
            if (b == 0xFF) {
                if (p + 1 >= end || p[1] != 0) { stop = true; break; }
                p += 2;
            } else {
                ++p;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    inline int peek(int k) {
        if (n < k) fill();
        return (int)((n >= k ? acc >> (n - k) : acc << (k - n)) & ((1u << k) - 1));
    }
    inline void skip(int k) {
        if (k > n) { bad = true; n = 0; } else n -= k;
    }
    inline int symbol(const Huff& t) {
        const int e = t.look[peek(9)];
        if (e) { skip(e >> 8); return e & 255; }
        const int w = peek(16);
        for (int l = 10; l <= 16; ++l) {
            const int c = w >> (16 - l);
            if (c <= t.maxcode[l]) { skip(l); return t.vals[(c + t.valoff[l]) & 255]; }
        }
        bad = true;  // a code the table does not define
        return 0;
    }
    inline int receive_extend(int s) {
        const int v = peek(s);
        skip(s);
        return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    }
    // the end of an interval: pad bits dropped, then the marker (0xFF, fill bytes, code); -1 when there is none
    int marker() {
        if (n >= 8) return -1;  // whole unread bytes in front of the marker
        n = 0;
        acc = 0;
        stop = false;
        if (p >= end || *p != 0xFF) return -1;
        while (p < end && *p == 0xFF) ++p;
        return p < end ? *p++ : -1;
    }
};

// One 8 x 8 block into `blk` (natural order, not dequantised).  `q`: the component's table, for the range check alone.
int decode_block(Bits& br, const Huff& dc, const Huff& ac, const uint16_t* q, int& pred, int16_t* blk) {
    memset(blk, 0, 64 * sizeof(int16_t));
    const int s = br.symbol(dc);
    if (br.bad) return R_CODE;
    if (s) pred += br.receive_extend(s);
    // libjpeg-turbo's SIMD dequantises in 16 bits: a product outside int16 has no defined picture
    if (pred < -32768 || pred > 32767 || pred * (int)q[0] < -32768 || pred * (int)q[0] > 32767) return R_RANGE;
    blk[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        const int rs = br.symbol(ac);
        if (br.bad) return R_CODE;
        const int r = rs >> 4, z = rs & 15;
        if (z) {
            k += r;
            if (k > 63) return R_INDEX;
            const int v = br.receive_extend(z), nat = kNatural[k];
            if (v * (int)q[nat] < -32768 || v * (int)q[nat] > 32767) return R_RANGE;
            blk[nat] = (int16_t)v;
            ++k;
        } else if (r == 15) {
            k += 16;
            if (k > 64) return R_INDEX;
        } else {
            break;
        }
    }
    return br.bad ? R_TRUNCATED : R_OK;
}

int decode_scan(const uint8_t* s, size_t len, const Header& h, int16_t* out) {
    const Desc& d = h.d;
    Bits br;
    br.p = s + h.scan;
    br.end = s + len;
    int pred[3] = {0, 0, 0};
    const bool inter = d.ncomp == 3;
    const int mx = inter ? d.bw[1] : d.bw[0], my = inter ? d.bh[1] : d.bh[0];
    const int ch[3] = {inter ? d.hs : 1, 1, 1}, cv[3] = {inter ? d.vs : 1, 1, 1};
    int64_t base[3] = {0, (int64_t)d.bw[0] * d.bh[0], (int64_t)d.bw[0] * d.bh[0] + (int64_t)d.bw[1] * d.bh[1]};
    int left = h.restart, next_rst = 0;
    for (int y = 0; y < my; ++y)
        for (int x = 0; x < mx; ++x) {
            if (h.restart && left == 0) {
                if (br.marker() != 0xD0 + next_rst) return R_RESTART;
                next_rst = (next_rst + 1) & 7;
                left = h.restart;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < d.ncomp; ++c)
                for (int v = 0; v < cv[c]; ++v)
                    for (int u = 0; u < ch[c]; ++u) {
                        const int64_t b = base[c] + (int64_t)(y * cv[c] + v) * d.bw[c] + (x * ch[c] + u);
                        const int r = decode_block(br, h.dc[h.td[c]], h.ac[h.ta[c]], d.qt[c], pred[c], out + 64 * b);
                        if (r != R_OK) return r;
                    }
            --left;
        }
    return br.marker() == 0xD9 ? R_OK : R_NO_EOI;  // anything else behind the scan: another scan, DNL, a cut file
}

// ------------------------------------------------------------------------------------------------ device
constexpr int IDCT_THREADS = 256;  // 4 waves, 8 blocks each

// Kernel A (its 1-D pass, its range guard and all behind the dequantisation: jpeg.h).  A wave takes 8 consecutive blocks; lane =
// 8 * block + j.  Lane j loads ROW j of its block's coefficients and of the
// quantisation table (16 bytes each: the wave reads 1 KiB of coefficients in one instruction), multiplies and leaves the
// products in LDS; then takes COLUMN j (pass 1), then ROW j (pass 2) and stores that row's 8 samples with one 8-byte store.
// LDS rows are 9 dwords and blocks 72, so within a 32-lane half both the column access (bank 8 b + j + 9 r) and the row access
// (bank 8 b + 9 j + k) touch 32 distinct banks: neither pass has a bank conflict.
__global__ void __launch_bounds__(IDCT_THREADS) jpeg_idct_kernel(const int16_t* __restrict__ coeffs, const Desc* __restrict__ desc,
                                                                 int n, long n_blocks, uint8_t* __restrict__ planes,
                                                                 int32_t* __restrict__ flags) {
    __shared__ int ws[IDCT_THREADS / 64][8 * 8 * WS_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane >> 3, j = lane & 7;
    const long g = ((long)blockIdx.x * (IDCT_THREADS / 64) + wave) * 8 + b;
    int* w = ws[wave] + b * 8 * WS_LD;
    bool live = false, wild = false;
    uint8_t* dst = nullptr;
    int ld = 0, i = 0;
    if (g < n_blocks) {
        i = image_of_block(desc, n, g);
        const Desc* d = desc + i;
        const long r = g - d->coef_block;
        if (d->status == AVCER_JPEG_OK && r >= 0 && r < d->n_blocks) {
            live = true;
            const long c0 = (long)d->bw[0] * d->bh[0], c1 = c0 + (long)d->bw[1] * d->bh[1];
            const int c = r < c0 ? 0 : (r < c1 ? 1 : 2);
            const long rr = r - (c == 0 ? 0 : (c == 1 ? c0 : c1));
            ld = d->bw[c] * 8;
            const int by = (int)(rr / d->bw[c]), bx = (int)(rr % d->bw[c]);
            // the plane mirrors the coefficient storage: 64 bytes per block, component after component
            dst = planes + 64 * (d->coef_block + (r - rr)) + ((long)by * 8 + j) * ld + bx * 8;
            const int4 cv = *reinterpret_cast<const int4*>(coeffs + 64 * g + 8 * j);
            const int4 qv = *reinterpret_cast<const int4*>(d->qt[c] + 8 * j);
            const int cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                w[j * WS_LD + 2 * k] = (int)(int16_t)(cw[k] & 0xffff) * (qw[k] & 0xffff);
                w[j * WS_LD + 2 * k + 1] = (cw[k] >> 16) * (int)((uint32_t)qw[k] >> 16);
                wild = wild || abs(w[j * WS_LD + 2 * k]) > IDCT_PAIR_MAX || abs(w[j * WS_LD + 2 * k + 1]) > IDCT_PAIR_MAX;
            }
        }
    }
    idct_block_store(w, j, live, wild, dst, flags + i);
}

// what kernel B needs of one image
struct Planes {
    const uint8_t* y;
    const uint8_t* cb;
    const uint8_t* cr;
    int ldy, ldc, w, h, dw, dh, hs, vs, ncomp;
};

__device__ __forceinline__ bool planes_of(const Desc* __restrict__ d, const uint8_t* __restrict__ planes, int flag, Planes& p) {
    if (d->status != AVCER_JPEG_OK || flag) return false;
    p.w = d->width;
    p.h = d->height;
    p.ncomp = d->ncomp;
    p.hs = p.ncomp == 3 ? d->hs : 1;
    p.vs = p.ncomp == 3 ? d->vs : 1;
    p.dw = (p.w + p.hs - 1) / p.hs;  // libjpeg's downsampled_width / _height of the chroma components
    p.dh = (p.h + p.vs - 1) / p.vs;
    p.ldy = d->bw[0] * 8;
    p.ldc = d->bw[1] * 8;
    p.y = planes + 64 * d->coef_block;
    p.cb = p.y + 64L * d->bw[0] * d->bh[0];
    p.cr = p.cb + 64L * d->bw[1] * d->bh[1];
    return true;
}

// One chroma sample at full-resolution position (x, y): libjpeg-turbo's jdsample.c evaluated at that pixel.  h2v1 fancy: the 3:1
// triangle, rounding +1 towards the left neighbour and +2 towards the right; h2v2 fancy: 3:1 between the nearer and the farther
// row, then 3:1 between the column sums, +8 / +7, >> 4.  Edge rows and columns replicate (which reproduces libjpeg's special
// first / last columns exactly).  A component of at most two columns is replicated, not filtered (jinit_upsampler's
// `downsampled_width > 2`), in both directions.
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int ld, const Planes& g, int x, int y) {
    if (g.hs == 1) return p[(long)y * ld + x];
    const int s = x >> 1;
    if (g.dw <= 2) return p[(long)(g.vs == 2 ? y >> 1 : y) * ld + s];
    const int sn = (x & 1) ? min(s + 1, g.dw - 1) : max(s - 1, 0);
    if (g.vs == 1) {
        const uint8_t* r = p + (long)y * ld;
        return (3 * r[s] + r[sn] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int t = y >> 1, tn = (y & 1) ? min(t + 1, g.dh - 1) : max(t - 1, 0);
    const uint8_t* r0 = p + (long)t * ld;
    const uint8_t* r1 = p + (long)tn * ld;
    const int cs = 3 * r0[s] + r1[s], cn = 3 * r0[sn] + r1[sn];
    return (3 * cs + cn + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// RGB of source pixel (x, y) as r | g << 8 | b << 16: libjpeg's jdcolor.c, 16-bit fixed point, one half added before the shift,
// the Cb and Cr terms of green combined before it; grey is replicated (PIL's convert("RGB") of mode L)
__device__ __forceinline__ uint32_t rgb_at(const Planes& g, int x, int y) {
    const int Y = g.y[(long)y * g.ldy + x];
    if (g.ncomp == 1) return (uint32_t)Y * 0x010101u;
    const int cb = chroma_at(g.cb, g.ldc, g, x, y) - 128, cr = chroma_at(g.cr, g.ldc, g, x, y) - 128;
    const int r = clamp255(Y + ((91881 * cr + 32768) >> 16));
    const int gg = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    const int bl = clamp255(Y + ((116130 * cb + 32768) >> 16));
    return (uint32_t)r | ((uint32_t)gg << 8) | ((uint32_t)bl << 16);
}

// Kernel B, tiles: tile pixel (y, x) = the decoded image at nearest_src (the rule of avcer_crop_tiles); one thread per 4 tile
// pixels, three 4-byte stores.  An image that was not decoded yields a zero tile.
__global__ void jpeg_tiles_kernel(const uint8_t* __restrict__ planes, const Desc* __restrict__ desc, const int32_t* __restrict__ flags,
                                  int n, uint8_t* __restrict__ tiles) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n * 224 * 56) return;
    const int xq = idx % 56;
    const int y = (idx / 56) % 224;
    const int t = idx / (56L * 224);
    uint32_t px[4] = {0, 0, 0, 0};
    Planes g;
    if (planes_of(desc + t, planes, flags[t], g)) {
        const int sy = nearest_src(y, g.h);
#pragma unroll
        for (int j = 0; j < 4; ++j) px[j] = rgb_at(g, nearest_src(xq * 4 + j, g.w), sy);
    }
    uint32_t* o = reinterpret_cast<uint32_t*>(tiles + ((long)t * 224 + y) * 224 * 3 + xq * 12);
    o[0] = px[0] | (px[1] << 24);
    o[1] = (px[1] >> 8) | (px[2] << 16);
    o[2] = (px[2] >> 16) | (px[3] << 8);
}

// Kernel B, canvas: the image itself at (0, 0) of its [hmax, wmax] slot, zeros around it; one thread per pixel
__global__ void jpeg_canvas_kernel(const uint8_t* __restrict__ planes, const Desc* __restrict__ desc, const int32_t* __restrict__ flags,
                                   int n, int hmax, int wmax, uint8_t* __restrict__ canvas) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n * hmax * wmax) return;
    const int x = idx % wmax;
    const int y = (idx / wmax) % hmax;
    const int t = idx / ((long)wmax * hmax);
    uint32_t px = 0;
    Planes g;
    if (planes_of(desc + t, planes, flags[t], g) && x < g.w && y < g.h) px = rgb_at(g, x, y);
    uint8_t* o = canvas + idx * 3;
    o[0] = (uint8_t)px;
    o[1] = (uint8_t)(px >> 8);
    o[2] = (uint8_t)(px >> 16);
}

// Kernel B, frames: whole video frames [n, H, W, 3], every image exactly W x H, channel order as asked.  Shaped by the store: a
// thread owns one 16-byte ALIGNED piece of one output row (rows are 3 W bytes and start wherever that leaves them, so the pieces
// are counted from the row's first aligned address down; the first and last piece of a row are cut to the row and go out as byte
// stores, every piece between as one 16-byte store).  A piece holds bytes of at most 6 pixels; they lie inside the 8 pixels
// [e, e + 8), e even, which are 4 horizontal chroma pairs: with 2 x subsampling the thread reads the 6 chroma columns s - 1 .. s + 4
// ONCE (for 2 x 2: both rows, folded into the column sums 3 near + far), and every pair takes its two outputs from three of them
// -- jdsample.c's h2v1 / h2v2 fancy upsampling, the arithmetic of chroma_at.  Columns and pixels past the picture's edge are
// clamped (the clamp IS libjpeg's edge rule for the columns; pixels out there belong to no byte of the row and are dropped).
constexpr int FRAME_THREADS = 256;

__device__ __forceinline__ uint32_t frame_px(int Y, int cb, int cr, bool bgr) {
    const int r = clamp255(Y + ((91881 * cr + 32768) >> 16));
    const int g = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    const int b = clamp255(Y + ((116130 * cb + 32768) >> 16));
    return (uint32_t)(bgr ? b : r) | ((uint32_t)g << 8) | ((uint32_t)(bgr ? r : b) << 16);
}

__global__ void frames_size_kernel(const Desc* __restrict__ desc, int n, int H, int W, int32_t* __restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && desc[i].status == AVCER_JPEG_OK && (desc[i].width != W || desc[i].height != H)) flags[i] = 2;
}

__global__ void __launch_bounds__(FRAME_THREADS) jpeg_frames_kernel(const uint8_t* __restrict__ planes, const Desc* __restrict__ desc,
                                                                    const int32_t* __restrict__ flags, int n, int H, int W, int per_row,
                                                                    int bgr, uint8_t* __restrict__ frames) {
    const long idx = (long)blockIdx.x * FRAME_THREADS + threadIdx.x;
    if (idx >= (long)n * H * per_row) return;
    const int piece = (int)(idx % per_row);
    const long row = idx / per_row;  // t * H + y
    const int y = (int)(row % H), t = (int)(row / H);
    uint8_t* const out = frames + row * 3L * W;
    // the piece in bytes of the row: [wb, wb + 16), wb < 0 where the row starts inside its first aligned piece
    const int wb = 16 * piece - (int)((uintptr_t)out & 15);
    if (wb >= 3 * W) return;
    uint32_t o4[4] = {0, 0, 0, 0};
    Planes g;
    if (planes_of(desc + t, planes, flags[t], g)) {  // flag 2 (another size) included: such a frame is zero
        const int x0 = wb >= 0 ? wb / 3 : -((2 - wb) / 3);  // floor
        const int e = x0 & ~1;
        int cb[8], cr[8];
        if (g.ncomp == 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) cb[j] = cr[j] = 0;
        } else if (g.hs == 2 && g.dw > 2) {
            const int s0 = (e >> 1) - 1;
            int colb[6], colr[6];
            int bias_even, bias_odd, shift;
            if (g.vs == 2) {
                const int ty = y >> 1, tn = (y & 1) ? min(ty + 1, g.dh - 1) : max(ty - 1, 0);
                const long r0 = (long)ty * g.ldc, r1 = (long)tn * g.ldc;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const int s = min(max(s0 + k, 0), g.dw - 1);
                    colb[k] = 3 * g.cb[r0 + s] + g.cb[r1 + s];
                    colr[k] = 3 * g.cr[r0 + s] + g.cr[r1 + s];
                }
                bias_even = 8, bias_odd = 7, shift = 4;
            } else {
                const long r0 = (long)y * g.ldc;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const int s = min(max(s0 + k, 0), g.dw - 1);
                    colb[k] = g.cb[r0 + s];
                    colr[k] = g.cr[r0 + s];
                }
                bias_even = 1, bias_odd = 2, shift = 2;
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {  // pair p: chroma column s0 + 1 + p, its left neighbour for the even pixel, its right for the odd
                cb[2 * p] = ((3 * colb[p + 1] + colb[p] + bias_even) >> shift) - 128;
                cb[2 * p + 1] = ((3 * colb[p + 1] + colb[p + 2] + bias_odd) >> shift) - 128;
                cr[2 * p] = ((3 * colr[p + 1] + colr[p] + bias_even) >> shift) - 128;
                cr[2 * p + 1] = ((3 * colr[p + 1] + colr[p + 2] + bias_odd) >> shift) - 128;
            }
        } else {  // chroma at full width, or a component of at most two columns (replicated, not filtered): the sample of that pixel
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int x = min(max(e + j, 0), g.w - 1);
                cb[j] = chroma_at(g.cb, g.ldc, g, x, y) - 128;
                cr[j] = chroma_at(g.cr, g.ldc, g, x, y) - 128;
            }
        }
        uint32_t px[8];
        const uint8_t* yr = g.y + (long)y * g.ldy;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int Y = yr[min(max(e + j, 0), g.w - 1)];
            px[j] = g.ncomp == 1 ? (uint32_t)Y * 0x010101u : frame_px(Y, cb[j], cr[j], bgr != 0);
        }
        // the 24 bytes of the 8 pixels, then the 16 of them that start at byte wb - 3 e (0 .. 5)
        uint32_t d[7];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            d[3 * q] = px[4 * q] | (px[4 * q + 1] << 24);
            d[3 * q + 1] = (px[4 * q + 1] >> 8) | (px[4 * q + 2] << 16);
            d[3 * q + 2] = (px[4 * q + 2] >> 16) | (px[4 * q + 3] << 8);
        }
        d[6] = 0;
        const int off = wb - 3 * e, sh = 8 * (off & 3);
        const bool up = off >= 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t lo = up ? d[k + 1] : d[k], hi = up ? d[k + 2] : d[k + 1];
            o4[k] = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
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

// Kernel A into the component planes
int jpeg_planes(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const Desc* desc, int n, int32_t* flags, uint8_t** planes,
                hipStream_t st) {
    uint8_t* p = nullptr;
    TRY(jpeg_plane_ws(ctx, n_blocks, &p));
    HIP_TRY(ctx, hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)n, st));
    const long per = IDCT_THREADS / 64 * 8;
    LAUNCH(ctx,
           jpeg_idct_kernel<<<(unsigned)((n_blocks + per - 1) / per), IDCT_THREADS, 0, st>>>(coeffs, desc, n, (long)n_blocks, p, flags));
    *planes = p;
    return AVCER_OK;
}

}  // namespace

// The component planes in the context's JPEG workspace, sized by their own carving (one byte per coefficient)
int jpeg_plane_ws(avcer_ctx* ctx, int64_t n_blocks, uint8_t** planes) {
    return ws_carve(ctx, WS_JPEG, "jpeg", [&](Arena& a) { *planes = a.get<uint8_t>(64 * (size_t)n_blocks); });
}

int launch_jpeg_tiles(avcer_ctx* ctx, const uint8_t* planes, const Desc* desc, const int32_t* flags, int n, uint8_t* tiles,
                      hipStream_t st) {
    const long total = (long)n * 224 * 56;
    LAUNCH(ctx, jpeg_tiles_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(planes, desc, flags, n, tiles));
    return AVCER_OK;
}

int canvas_args(avcer_ctx* ctx, const char* what, int n, int hmax, int wmax) {
    if (hmax <= 0 || wmax <= 0 || n <= 0 || (long)n * hmax * wmax >= (1L << 38))
        return set_err(ctx, AVCER_EINVAL, "%s: canvas %d x %d x %d", what, n, hmax, wmax);
    return AVCER_OK;
}

int launch_jpeg_canvas(avcer_ctx* ctx, const uint8_t* planes, const Desc* desc, const int32_t* flags, int n, int hmax, int wmax,
                       uint8_t* canvas, hipStream_t st) {
    const long total = (long)n * hmax * wmax;
    LAUNCH(ctx, jpeg_canvas_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(planes, desc, flags, n, hmax, wmax, canvas));
    return AVCER_OK;
}

int coeff_args(avcer_ctx* ctx, const char* what, const void* coeffs, bool null_ok, int64_t n_blocks, const void* desc, int n, bool own,
               const int* frames) {
    if (!ctx) return AVCER_EINVAL;
    if (own && (coeffs || null_ok) && desc && n > 0 && n_blocks > 0 && n_blocks < (1LL << 34) && !((uintptr_t)coeffs & 15) &&
        !((uintptr_t)desc & 15))
        return AVCER_OK;
    char fr[64] = "";
    if (frames) snprintf(fr, sizeof(fr), "frames %d x %d x %d, ", frames[0], frames[1], frames[2]);
    return set_err(ctx, AVCER_EINVAL, "%s: bad arguments (n %d, %s%lld blocks; coefficients and descriptors 16-byte aligned)", what, n, fr,
                   (long long)n_blocks);
}

extern "C" int avcer_jpeg_probe(const uint8_t* bytes, size_t len, avcer_jpeg_desc* info) {
    if (!info) return AVCER_EINVAL;
    try {
        Header* h = new Header();
        const int r = parse_header(bytes, len, *h);
        *info = h->d;
        info->reason = r;
        info->status = r == R_OK ? AVCER_JPEG_OK : AVCER_JPEG_NOT_HANDLED;
        delete h;
    } catch (...) {
        return AVCER_ENOMEM;
    }
    return AVCER_OK;
}

extern "C" int avcer_jpeg_entropy_batch(avcer_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, int16_t* coeffs,
                                        int64_t cap_blocks, avcer_jpeg_desc* desc, int threads, int64_t* blocks_needed) {
    return avcer_jpeg_entropy_batch_ex(ctx, files, lens, n, coeffs, cap_blocks, desc, threads, 0, blocks_needed);
}

extern "C" int avcer_jpeg_entropy_batch_ex(avcer_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, int16_t* coeffs,
                                           int64_t cap_blocks, avcer_jpeg_desc* desc, int threads, int hflags, int64_t* blocks_needed) {
    const bool std_tables = (hflags & AVCER_JPEG_STD_TABLES) != 0;
    // ctx may be NULL (host-only call, no device needed): errors then come back as the code alone
    if (n < 0 || (n && (!files || !lens || !desc)) || cap_blocks < 0 || (cap_blocks && !coeffs) || (hflags & ~AVCER_JPEG_STD_TABLES))
        return set_err(ctx, AVCER_EINVAL, "jpeg_entropy_batch: bad arguments");
    try {
        const int nt = threads_for(threads, n);
        // headers first, every thread with its one Header; then the storage (place_blocks): a file that does not fit takes nothing
        each_index<Header>(n, nt, [&](int i, Header& h) {
            const int r = parse_header(files[i], lens[i] < 0 ? 0 : (size_t)lens[i], h, std_tables);  // no bytes: R_NO_SOI
            desc[i] = h.d;
            desc[i].reason = r;
        });
        const int64_t needed = place_blocks(desc, n, [&](int, const Desc& d, int64_t used) { return d.n_blocks <= cap_blocks - used; });
        if (blocks_needed) *blocks_needed = needed;
        // the scans: independent.  The header is parsed again (some hundred bytes) rather than kept for every file of the batch
        each_index<Header>(n, nt, [&](int i, Header& h) {
            if (desc[i].status != AVCER_JPEG_OK) return;
            int r = parse_header(files[i], (size_t)lens[i], h, std_tables);
            if (r == R_OK) r = decode_scan(files[i], (size_t)lens[i], h, coeffs + 64 * desc[i].coef_block);
            if (r != R_OK) not_handled(desc[i], r);
        });
    } catch (...) {
        return set_err(ctx, AVCER_ENOMEM, "jpeg_entropy_batch: out of host memory");
    }
    return AVCER_OK;
}

extern "C" int avcer_jpeg_tiles(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const avcer_jpeg_desc* desc, int n,
                                int32_t* flags, uint8_t* tiles, avcer_stream_t stream) {
    TRY(coeff_args(ctx, "jpeg_tiles", coeffs, false, n_blocks, desc, n, flags && tiles));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint8_t* planes = nullptr;
    TRY(jpeg_planes(ctx, coeffs, n_blocks, desc, n, flags, &planes, st));
    return launch_jpeg_tiles(ctx, planes, desc, flags, n, tiles, st);
}

extern "C" int avcer_jpeg_rgb(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const avcer_jpeg_desc* desc, int n,
                              int32_t* flags, uint8_t* canvas, int hmax, int wmax, avcer_stream_t stream) {
    TRY(coeff_args(ctx, "jpeg_rgb", coeffs, false, n_blocks, desc, n, flags && canvas));
    TRY(canvas_args(ctx, "jpeg_rgb", n, hmax, wmax));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint8_t* planes = nullptr;
    TRY(jpeg_planes(ctx, coeffs, n_blocks, desc, n, flags, &planes, st));
    return launch_jpeg_canvas(ctx, planes, desc, flags, n, hmax, wmax, canvas, st);
}

extern "C" int avcer_jpeg_frames(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const avcer_jpeg_desc* desc, int n,
                                 int32_t* flags, uint8_t* frames, int H, int W, int bgr, avcer_stream_t stream) {
    TRY(coeff_args(ctx, "jpeg_frames", coeffs, false, n_blocks, desc, n, flags && frames));
    if (H <= 0 || W <= 0 || H > 65535 || W > 65535 || (long)n * H * W >= (1L << 36))
        return set_err(ctx, AVCER_EINVAL, "jpeg_frames: frames %d x %d x %d (1..65535 a side, fewer than 2^36 pixels)", n, H, W);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint8_t* planes = nullptr;
    TRY(jpeg_planes(ctx, coeffs, n_blocks, desc, n, flags, &planes, st));
    LAUNCH(ctx, frames_size_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(desc, n, H, W, flags));
    const int per_row = (3 * W + 15) / 16 + 1;  // aligned 16-byte pieces a row of 3 W bytes can touch
    const long total = (long)n * H * per_row;
    LAUNCH(ctx, jpeg_frames_kernel<<<(unsigned)((total + FRAME_THREADS - 1) / FRAME_THREADS), FRAME_THREADS, 0, st>>>(
                    planes, desc, flags, n, H, W, per_row, bgr, frames));
    return AVCER_OK;
}
