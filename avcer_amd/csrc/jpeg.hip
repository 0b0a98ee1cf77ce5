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
// The Huffman decoding runs on the device as well when asked to (avcer_jpeg_scan_batch + avcer_jpeg_unpack, at the end of this file:
// the host then parses headers only); the host pass above is its oracle.
#include "common.h"
#include "jpeg_sync_dev.h"

#include <algorithm>
#include <atomic>
#include <memory>
#include <new>
#include <thread>

namespace {

typedef avcer_jpeg_desc Desc;

// ------------------------------------------------------------------------------------------------ host: markers
enum {  // Desc::reason: why a file is not handled (0 = it is)
    R_OK = 0, R_NO_SOI = 1, R_MARKER = 2, R_SOF_KIND = 3, R_PRECISION = 4, R_COMPONENTS = 5, R_SAMPLING = 6, R_COLOUR = 7, R_TABLE = 8,
    R_SCAN = 9, R_TRUNCATED = 10, R_CODE = 11, R_NO_SPACE = 12, R_INDEX = 13, R_RESTART = 14, R_NO_EOI = 15, R_RANGE = 16, R_SIZE = 17,
    R_ENC_SIZE = 18, R_ENC_DESC = 19  // encoding: an image of no or of more than 65535 pixels a side; a descriptor avcer_jpeg_plan did not write
};

constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// The four DHT segments as libjpeg writes them (the standard's tables K.3 - K.6), marker and length included: DC 0, AC 0, DC 1, AC 1.
// The ONE statement of these tables: the writer emits them (encoding, below), and the reader assumes them for a table a scan
// references and no DHT segment defined when AVCER_JPEG_STD_TABLES asks for it (MJPEG frames, parse_header)
constexpr uint8_t kDhtDc0[33] = {255, 196, 0, 31, 0, 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kDhtDc1[33] = {255, 196, 0, 31, 1, 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kDhtAc0[183] = {
    255, 196, 0,   181, 16,  0,   2,   1,   3,   3,   2,   4,   3,   5,   5,   4,   4,   0,   0,   1,   125, 1,   2,   3,   0,   4,   17,
    5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177, 193, 21,  82,  209, 240, 36,
    51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,  56,  57,  58,  67,  68,  69,
    70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120,
    121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169,
    170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217,
    218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250};
constexpr uint8_t kDhtAc1[183] = {
    255, 196, 0,   181, 17,  0,   2,   1,   2,   4,   4,   3,   4,   7,   5,   4,   4,   0,   1,   2,   119, 0,   1,   2,   3,   17,  4,
    5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193, 9,   35,  51,  82,  240, 21,
    98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,  55,  56,  57,  58,  67,  68,
    69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119,
    120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
    168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215,
    216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250};
struct Huff {
    bool defined = false;
    uint8_t bits[17] = {0};
    uint8_t vals[256] = {0};
    int32_t maxcode[17];   // largest code of each length, -1 where the length has none
    int32_t valoff[17];    // vals index of a code = code + valoff[length]
    uint16_t look[512];    // the next 9 bits -> (length << 8) | symbol, 0: the code is longer
    bool ok = false;       // a consistent code
    bool dc_ok = false;    // ... whose symbols are magnitude categories (<= 15)
};

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

struct Header {
    Desc d;
    int comp_id[3] = {0, 0, 0};
    int comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1};
    int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    int restart = 0;
    Huff dc[4], ac[4];
    uint16_t q[4][64];
    bool q_def[4] = {false, false, false, false};
    size_t scan = 0;  // offset of the first entropy-coded byte
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// One annex-K table into `t`, from its DHT segment above (marker, length, class / id, 16 counts, the symbols)
void assume_std(Huff& t, const uint8_t* seg, int count) {
    t.bits[0] = 0;
    memcpy(t.bits + 1, seg + 5, 16);
    memset(t.vals, 0, sizeof(t.vals));
    memcpy(t.vals, seg + 21, (size_t)count);
    t.defined = true;
    derive(t);
}

// Everything up to the first entropy-coded byte.  Returns a reason; on R_OK h.d holds the geometry and the tables of the scan.
// std_tables (AVCER_JPEG_STD_TABLES): a table 0 or 1 the scan references and no DHT segment of the file defined is the standard's
// annex-K table of that class and id -- what libjpeg-turbo (jdhuff.c, std_huff_tables) and ffmpeg's mjpeg2jpeg assume for Motion-JPEG
// frames.  A table the file defines is the file's; ids 2 and 3 have no standard table and stay R_TABLE.
int parse_header(const uint8_t* s, size_t len, Header& h, bool std_tables = false) {
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

// threads of the entropy pass: what the caller asks for, 16 at most and by default -- never the machine's core count.  The library
// reads no environment: avcer_amd/jpeg.py turns OMP_NUM_THREADS into the argument.
int pool_size(int threads) { return threads <= 0 || threads > 16 ? 16 : threads; }

// ------------------------------------------------------------------------------------------------ device
constexpr int CONST_BITS = 13, PASS1_BITS = 2;

// libjpeg's jidctint.c (jpeg_idct_islow), one 1-D pass: 13-bit constants, DESCALE(x, n) = (x + 2^(n-1)) >> n.  The all-zero-AC
// shortcuts of both passes (dc << PASS1_BITS; DESCALE(ws0, PASS1_BITS + 3)) ARE this arithmetic's results for such input -- the
// even part is then (dc << 13) alone and the rounding term divides out -- so they are not restated.
template <int SHIFT>
__device__ __forceinline__ void idct_1d(int (&v)[8]) {
    // Sums and products in uint32_t: modulo 2^32, the same bits as libjpeg's arithmetic wherever that stays inside 32 bits (every
    // image the range guard passes), and defined -- no signed overflow -- where a corrupt file's does not (its result is discarded).
    typedef uint32_t U;
    const auto mul = [](U a, int k) { return a * (U)k; };
    U z2 = (U)v[2], z3 = (U)v[6];
    U z1 = mul(z2 + z3, 4433);
    U tmp2 = z1 + mul(z3, -15137);
    U tmp3 = z1 + mul(z2, 6270);
    z2 = (U)v[0];
    z3 = (U)v[4];
    U tmp0 = (z2 + z3) << CONST_BITS;
    U tmp1 = (z2 - z3) << CONST_BITS;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (U)v[7];
    tmp1 = (U)v[5];
    tmp2 = (U)v[3];
    tmp3 = (U)v[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    U z4 = tmp1 + tmp3;
    const U z5 = mul(z3 + z4, 9633);
    tmp0 = mul(tmp0, 2446);
    tmp1 = mul(tmp1, 16819);
    tmp2 = mul(tmp2, 25172);
    tmp3 = mul(tmp3, 12299);
    z1 = mul(z1, -7373);
    z2 = mul(z2, -20995);
    z3 = mul(z3, -16069) + z5;
    z4 = mul(z4, -3196) + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    constexpr U R = (U)1 << (SHIFT - 1);
    const auto descale = [](U x) { return (int)(x + R) >> SHIFT; };  // arithmetic shift of the two's-complement value
    v[0] = descale(tmp10 + tmp3);
    v[7] = descale(tmp10 - tmp3);
    v[1] = descale(tmp11 + tmp2);
    v[6] = descale(tmp11 - tmp2);
    v[2] = descale(tmp12 + tmp1);
    v[5] = descale(tmp12 - tmp1);
    v[3] = descale(tmp13 + tmp0);
    v[4] = descale(tmp13 - tmp0);
}

// the image whose coefficient blocks hold block g: the last one that starts at or before it (offsets ascend, avcer_jpeg_entropy_batch)
__device__ __forceinline__ int image_of_block(const Desc* __restrict__ desc, int n, long g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[mid].coef_block <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

constexpr int IDCT_THREADS = 256;  // 4 waves, 8 blocks each
constexpr int WS_LD = 9;           // dwords per row of a block's 8 x 8 workspace in LDS

// Kernel A.  A wave takes 8 consecutive blocks; lane = 8 * block + j.  Lane j loads ROW j of its block's coefficients and of the
// quantisation table (16 bytes each: the wave reads 1 KiB of coefficients in one instruction), multiplies and leaves the
// products in LDS; then takes COLUMN j (pass 1), then ROW j (pass 2) and stores that row's 8 samples with one 8-byte store.
// LDS rows are 9 dwords and blocks 72, so within a 32-lane half both the column access (bank 8 b + j + 9 r) and the row access
// (bank 8 b + 9 j + k) touch 32 distinct banks: neither pass has a bank conflict.
//
// Range guard.  libjpeg's C code (wide integers, a range table that wraps at 10 bits) and its SIMD code (16-bit pair sums,
// pass-1 results saturated to int16, saturating packs at the end) compute the same picture only while the values stay small:
// dequantised coefficients and pass-1 results within +-IDCT_PAIR_MAX (any two add up inside int16), samples within [-512, 511]
// before the +128.  Every picture an encoder wrote is far inside (pass 1 reaches ~4096 for full-swing samples plus the
// quantisation error); a corrupt stream or table may not be, and then "PIL's decode" depends on how libjpeg was built.  Such an
// image is not guessed at: its flag is raised, kernel B leaves it zero, and the caller decodes it some other way.
constexpr int IDCT_PAIR_MAX = 16383;

// Kernel A behind the dequantisation, for every lane of the workgroup (it holds the two barriers): `w` is the lane's block in LDS
// with the dequantised row j written by this lane, `wild` what the range guard has seen so far.  Column pass, row pass, the guard,
// and row j of the block's samples to `dst` with one 8-byte store; `flag` is the image's.
__device__ __forceinline__ void idct_block_store(int* w, int j, bool live, bool wild, uint8_t* dst, int32_t* flag) {
    __syncthreads();
    int v[8];
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = w[r * WS_LD + j];
        idct_1d<CONST_BITS - PASS1_BITS>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            w[r * WS_LD + j] = v[r];
            wild = wild || abs(v[r]) > IDCT_PAIR_MAX;
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = w[j * WS_LD + k];
        idct_1d<CONST_BITS + PASS1_BITS + 3>(v);
        // range limit around +128 (the guard above keeps to where libjpeg's wrapping table and its saturating packs agree)
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) wild = wild || v[k] < -512 || v[k] > 511;
        if (wild) *flag = 1;  // every lane that sees it stores the same 1
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)min(max(v[k] + 128, 0), 255) << (8 * k);
            hi |= (uint32_t)min(max(v[k + 4] + 128, 0), 255) << (8 * k);
        }
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
    }
}

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

// The component planes in the context's JPEG workspace, sized by their own carving (one byte per coefficient)
int jpeg_plane_ws(avcer_ctx* ctx, int64_t n_blocks, uint8_t** planes) {
    return ws_carve(ctx, WS_JPEG, "jpeg", [&](Arena& a) { *planes = a.get<uint8_t>(64 * (size_t)n_blocks); });
}

// Kernel A into them
int jpeg_planes(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const Desc* desc, int n, int32_t* flags, uint8_t** planes,
                hipStream_t st) {
    uint8_t* p = nullptr;
    TRY(jpeg_plane_ws(ctx, n_blocks, &p));
    HIP_TRY(ctx, hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)n, st));
    const long per = IDCT_THREADS / 64 * 8;
    jpeg_idct_kernel<<<(unsigned)((n_blocks + per - 1) / per), IDCT_THREADS, 0, st>>>(coeffs, desc, n, (long)n_blocks, p, flags);
    HIP_TRY(ctx, hipGetLastError());
    *planes = p;
    return AVCER_OK;
}

int jpeg_args(avcer_ctx* ctx, const char* what, const void* coeffs, int64_t n_blocks, const void* desc, int n, const void* flags,
              const void* out) {
    if (!ctx) return AVCER_EINVAL;
    if (!coeffs || !desc || !out || !flags || n <= 0 || n_blocks <= 0 || n_blocks >= (1LL << 34) || ((uintptr_t)coeffs & 15) || ((uintptr_t)desc & 15))
        return set_err(ctx, AVCER_EINVAL, "%s: bad arguments (n %d, %lld blocks; coefficients and descriptors 16-byte aligned)", what, n,
                       (long long)n_blocks);
    return AVCER_OK;
}

}  // namespace

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

namespace {
int entropy_batch(avcer_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, int16_t* coeffs, int64_t cap_blocks,
                  avcer_jpeg_desc* desc, int threads, int hflags, int64_t* blocks_needed) {
    const bool std_tables = (hflags & AVCER_JPEG_STD_TABLES) != 0;
    // ctx may be NULL (host-only call, no device needed): errors then come back as the code alone
    if (n < 0 || (n && (!files || !lens || !desc)) || cap_blocks < 0 || (cap_blocks && !coeffs) || (hflags & ~AVCER_JPEG_STD_TABLES))
        return set_err(ctx, AVCER_EINVAL, "jpeg_entropy_batch: bad arguments");
    try {
        const int nt = std::min(pool_size(threads), n);
        // fn(i, h) for every file, files handed out one at a time to nt threads (this one included); h is the thread's one Header
        // (13 KB of Huffman look-up tables), so the tables in memory are nt sets and not n
        const auto each_file = [&](const auto& fn) {
            std::atomic<int> next(0);
            std::atomic<bool> failed(false);
            const auto work = [&]() {
                try {
                    std::unique_ptr<Header> h(new Header());
                    for (int i; (i = next.fetch_add(1)) < n;) fn(i, *h);
                } catch (...) {
                    failed = true;  // nothing may leave a thread; the files it did not take are taken by the others
                }
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; ++t) {
                try {
                    pool.emplace_back(work);
                } catch (...) {
                    break;  // no more threads to be had: the ones running and this one do the work
                }
            }
            work();
            for (auto& t : pool) t.join();
            if (failed) throw std::bad_alloc();
        };
        // headers first; then, in file order, every supported file gets the next free blocks of the storage, so offsets ascend
        // (kernel A finds a block's image by them); a file that does not fit is not handled and takes nothing
        each_file([&](int i, Header& h) {
            const int r = parse_header(files[i], lens[i] < 0 ? 0 : (size_t)lens[i], h, std_tables);  // no bytes: R_NO_SOI
            desc[i] = h.d;
            desc[i].reason = r;
        });
        int64_t used = 0, needed = 0;
        for (int i = 0; i < n; ++i) {
            Desc& d = desc[i];
            int r = d.reason;
            if (r == R_OK) {
                needed += d.n_blocks;
                if (d.n_blocks > cap_blocks - used) r = R_NO_SPACE;
            }
            d.coef_block = used;
            if (r == R_OK) used += d.n_blocks; else d.n_blocks = 0;
            d.reason = r;
            d.status = r == R_OK ? AVCER_JPEG_OK : AVCER_JPEG_NOT_HANDLED;
        }
        if (blocks_needed) *blocks_needed = needed;
        // the scans: independent.  The header is parsed again (some hundred bytes) rather than kept for every file of the batch
        each_file([&](int i, Header& h) {
            if (desc[i].status != AVCER_JPEG_OK) return;
            int r = parse_header(files[i], (size_t)lens[i], h, std_tables);
            if (r == R_OK) r = decode_scan(files[i], (size_t)lens[i], h, coeffs + 64 * desc[i].coef_block);
            if (r != R_OK) {
                desc[i].reason = r;
                desc[i].status = AVCER_JPEG_NOT_HANDLED;
            }
        });
    } catch (...) {
        return set_err(ctx, AVCER_ENOMEM, "jpeg_entropy_batch: out of host memory");
    }
    return AVCER_OK;
}
}  // namespace

extern "C" int avcer_jpeg_entropy_batch(avcer_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, int16_t* coeffs,
                                        int64_t cap_blocks, avcer_jpeg_desc* desc, int threads, int64_t* blocks_needed) {
    return entropy_batch(ctx, files, lens, n, coeffs, cap_blocks, desc, threads, 0, blocks_needed);
}

extern "C" int avcer_jpeg_entropy_batch_ex(avcer_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, int16_t* coeffs,
                                           int64_t cap_blocks, avcer_jpeg_desc* desc, int threads, int hflags, int64_t* blocks_needed) {
    return entropy_batch(ctx, files, lens, n, coeffs, cap_blocks, desc, threads, hflags, blocks_needed);
}

extern "C" int avcer_jpeg_tiles(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const avcer_jpeg_desc* desc, int n,
                                int32_t* flags, uint8_t* tiles, avcer_stream_t stream) {
    TRY(jpeg_args(ctx, "jpeg_tiles", coeffs, n_blocks, desc, n, flags, tiles));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint8_t* planes = nullptr;
    TRY(jpeg_planes(ctx, coeffs, n_blocks, desc, n, flags, &planes, st));
    const long total = (long)n * 224 * 56;
    jpeg_tiles_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(planes, desc, flags, n, tiles);
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}

extern "C" int avcer_jpeg_rgb(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const avcer_jpeg_desc* desc, int n,
                              int32_t* flags, uint8_t* canvas, int hmax, int wmax, avcer_stream_t stream) {
    TRY(jpeg_args(ctx, "jpeg_rgb", coeffs, n_blocks, desc, n, flags, canvas));
    if (hmax <= 0 || wmax <= 0 || (long)n * hmax * wmax >= (1L << 38))
        return set_err(ctx, AVCER_EINVAL, "jpeg_rgb: canvas %d x %d x %d", n, hmax, wmax);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint8_t* planes = nullptr;
    TRY(jpeg_planes(ctx, coeffs, n_blocks, desc, n, flags, &planes, st));
    const long total = (long)n * hmax * wmax;
    jpeg_canvas_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(planes, desc, flags, n, hmax, wmax, canvas);
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}

extern "C" int avcer_jpeg_frames(avcer_ctx* ctx, const int16_t* coeffs, int64_t n_blocks, const avcer_jpeg_desc* desc, int n,
                                 int32_t* flags, uint8_t* frames, int H, int W, int bgr, avcer_stream_t stream) {
    TRY(jpeg_args(ctx, "jpeg_frames", coeffs, n_blocks, desc, n, flags, frames));
    if (H <= 0 || W <= 0 || H > 65535 || W > 65535 || (long)n * H * W >= (1L << 36))
        return set_err(ctx, AVCER_EINVAL, "jpeg_frames: frames %d x %d x %d (1..65535 a side, fewer than 2^36 pixels)", n, H, W);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    uint8_t* planes = nullptr;
    TRY(jpeg_planes(ctx, coeffs, n_blocks, desc, n, flags, &planes, st));
    frames_size_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(desc, n, H, W, flags);
    HIP_TRY(ctx, hipGetLastError());
    const int per_row = (3 * W + 15) / 16 + 1;  // aligned 16-byte pieces a row of 3 W bytes can touch
    const long total = (long)n * H * per_row;
    jpeg_frames_kernel<<<(unsigned)((total + FRAME_THREADS - 1) / FRAME_THREADS), FRAME_THREADS, 0, st>>>(planes, desc, flags, n, H, W, per_row,
                                                                                                        bgr, frames);
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}

// ================================================================================================ encoding
// The mirror image of the above: the device computes the quantised coefficients of every image straight from the decoded frames
// (avcer_jpeg_forward: one launch per batch), the host writes the files (avcer_jpeg_write_batch: headers and Huffman coding, a
// small thread pool, files are independent) -- or the device does that as well (avcer_jpeg_pack: a wave per block, prefix sums
// for the bit and byte positions; whole files leave the device, and the host writer is its oracle).  All of it restates libjpeg(-turbo)'s compressor with the parameters PIL's
// Image.save(f, "JPEG", quality=q, subsampling=s) gives it -- jccolor.c, jcsample.c, jcprepct.c's edges, jfdctint.c ("islow"),
// jcdctmgr.c's quantisation, jccoefct.c's dummy blocks, jcmarker.c, jchuff.c with the standard tables -- and the contract is
// byte-identity with the file PIL writes (tests/test_jpeg_encode_host.py holds the numpy statement of the kernel,
// avcer_amd/jpeg.py forward_numpy, and the writer to PIL; tests/test_gpu_jpeg_encode.py holds the kernel to both).
//
// Dummy blocks (those that only pad a component to whole MCUs; with chroma at 1 x 1 only luma has any) get their final value in
// the KERNEL: zero AC and the DC of the block libjpeg codes before them in the MCU.  The writer codes what it is given.
namespace {

// ------------------------------------------------------------------------------------------------ host: tables and headers
// jcparam.c: the standard's two example tables, natural order
const uint8_t kStdLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                              80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72,
                              92, 95, 98, 112, 100, 103, 99};
const uint8_t kStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// (the four DHT segments of the standard's annex K, kDhtDc0 .. kDhtAc1, stand at the top of this file: the reader implies them too)
constexpr size_t HEADER_BYTES = 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 14;  // SOI, APP0, two DQT, SOF0, four DHT, SOS: 623

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

// what the writer relies on before it reads a coefficient: the geometry avcer_jpeg_plan derives from the size and the sampling
__host__ __device__ bool plan_consistent(const Desc& d) {
    if (d.width < 1 || d.width > 65535 || d.height < 1 || d.height > 65535 || d.ncomp != 3) return false;
    if (!((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2))) return false;
    const int mx = (d.width + 8 * d.hs - 1) / (8 * d.hs), my = (d.height + 8 * d.vs - 1) / (8 * d.vs);
    if (d.bw[0] != mx * d.hs || d.bh[0] != my * d.vs || d.bw[1] != mx || d.bw[2] != mx || d.bh[1] != my || d.bh[2] != my) return false;
    if (d.tq[0] != 0 || d.tq[1] != 1 || d.tq[2] != 1 || d.coef_block < 0) return false;
    for (int k = 0; k < 64; ++k)
        if (d.qt[0][k] < 1 || d.qt[0][k] > 255 || d.qt[1][k] < 1 || d.qt[1][k] > 255 || d.qt[2][k] != d.qt[1][k]) return false;
    return d.n_blocks == (int64_t)mx * my * (d.hs * d.vs + 2);
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

// fn(i) for every i < n, handed out one at a time to nt threads (this one included); nothing may leave a thread
template <class Fn>
void each_index(int n, int nt, const Fn& fn) {
    std::atomic<int> next(0);
    std::atomic<bool> failed(false);
    const auto work = [&]() {
        try {
            for (int i; (i = next.fetch_add(1)) < n;) fn(i);
        } catch (...) {
            failed = true;
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) {
        try {
            pool.emplace_back(work);
        } catch (...) {
            break;  // no more threads to be had: the ones running and this one do the work
        }
    }
    work();
    for (auto& t : pool) t.join();
    if (failed) throw std::bad_alloc();
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


// ------------------------------------------------------------------------------------------------ device: entropy coding
// avcer_jpeg_pack: write_file / encode_block / BitWriter above on the device, byte for byte.  A WAVE codes one 8 x 8 block, lane k
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
constexpr int PACK_THREADS = 256;                  // 4 waves
constexpr int PACK_WAVES = PACK_THREADS / 64;
constexpr int BLOCK_WORDS = 52;                    // an unstuffed block: ceil((20 + 63 * 26) / 8) = 208 bytes at the most
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

// The combine rules of the scans below, op(a, b) with `a` what stands in front of `b`: sums, maxima, and sums that start again at
// every element with its flag set -- a (value, flag) pair under the usual associative operator, values modulo 2^32
struct ScanSum {
    template <class T> __device__ T operator()(T a, T b) const { return a + b; }
};
struct ScanMax {
    template <class T> __device__ T operator()(T a, T b) const { return max(a, b); }
};
struct SegSum { uint32_t v, f; };
struct ScanSeg {
    __device__ SegSum operator()(SegSum a, SegSum b) const { return SegSum{b.f ? b.v : a.v + b.v, a.f | b.f}; }
};
template <class T> __device__ __forceinline__ T shfl_up(T x, int d) { return __shfl_up(x, d, 64); }
__device__ __forceinline__ SegSum shfl_up(SegSum x, int d) { return SegSum{__shfl_up(x.v, d, 64), __shfl_up(x.f, d, 64)}; }

// inclusive scan under `op` (sums unless stated) along the lanes of a wave
template <class T, class Op = ScanSum>
__device__ __forceinline__ T wave_scan(T v, int lane, Op op = Op()) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = shfl_up(v, d);
        if (lane >= d) v = op(o, v);
    }
    return v;
}

// the same along the PACK_THREADS threads of a workgroup (every thread calls it), *total = the last of them; `tot`: PACK_WAVES
// values of LDS, free again on return
template <class T, class Op = ScanSum>
__device__ __forceinline__ T block_scan(T v, T* tot, T* total, Op op = Op()) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_scan(v, lane, op);
    if (lane == 63) tot[wave] = v;
    __syncthreads();
    T all = tot[0], mine = v;
#pragma unroll
    for (int k = 1; k < PACK_WAVES; ++k) {
        if (k == wave) mine = op(all, v);
        all = op(all, tot[k]);
    }
    __syncthreads();
    *total = all;
    return mine;
}

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
            d.status = AVCER_JPEG_NOT_HANDLED;
            d.reason = R_ENC_SIZE;
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
        const int nt = std::max(1, std::min(pool_size(threads), n));
        each_index(n, nt, [&](int i) {
            if (desc[i].status != AVCER_JPEG_OK) return;
            const int r = write_file(coeffs, desc[i], files[i], &lens[i]);
            if (r != R_OK) {
                lens[i] = 0;
                desc[i].reason = r;
                desc[i].status = AVCER_JPEG_NOT_HANDLED;
            }
        });
        int64_t used = 0, needed = 0;
        for (int i = 0; i < n; ++i) {
            offsets[i] = used;
            if (desc[i].status != AVCER_JPEG_OK) continue;
            needed += (int64_t)lens[i];
            if ((int64_t)lens[i] > cap_bytes - used) {
                desc[i].reason = R_NO_SPACE;
                desc[i].status = AVCER_JPEG_NOT_HANDLED;
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
    if (!ctx) return AVCER_EINVAL;
    if (!src || !rects || !desc || !coeffs || n <= 0 || N <= 0 || H <= 0 || W <= 0 || n_blocks <= 0 || n_blocks >= (1LL << 34) ||
        ((uintptr_t)coeffs & 15) || ((uintptr_t)desc & 15) || ((uintptr_t)rects & 3))
        return set_err(ctx, AVCER_EINVAL, "jpeg_forward: bad arguments (n %d, frames %d x %d x %d, %lld blocks; coefficients and descriptors 16-byte aligned)",
                       n, N, H, W, (long long)n_blocks);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const long per = FWD_THREADS / 64 * 8;
    jpeg_forward_kernel<<<(unsigned)((n_blocks + per - 1) / per), FWD_THREADS, 0, (hipStream_t)stream>>>(src, N, H, W, rects, desc, n, bgr ? 1 : 0,
                                                                                                        coeffs, (long)n_blocks);
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}

namespace {

// avcer_jpeg_roundtrip_*: arguments, workspace, the flags and the fused kernel; *planes is what kernel B then reads
int jpeg_roundtrip_planes(avcer_ctx* ctx, const char* what, const uint8_t* src, int N, int H, int W, const int32_t* rects, const Desc* desc,
                          int n, int bgr, int16_t* coeffs, int64_t n_blocks, int32_t* flags, const void* out, uint8_t** planes,
                          hipStream_t st) {
    if (!ctx) return AVCER_EINVAL;
    if (!src || !rects || !desc || !flags || !out || n <= 0 || N <= 0 || H <= 0 || W <= 0 || n_blocks <= 0 || n_blocks >= (1LL << 34) ||
        ((uintptr_t)coeffs & 15) || ((uintptr_t)desc & 15) || ((uintptr_t)rects & 3) || ((uintptr_t)flags & 3))
        return set_err(ctx, AVCER_EINVAL, "%s: bad arguments (n %d, frames %d x %d x %d, %lld blocks; coefficients and descriptors 16-byte aligned)",
                       what, n, N, H, W, (long long)n_blocks);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TRY(jpeg_plane_ws(ctx, n_blocks, planes));
    roundtrip_check_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(desc, n, (long)n_blocks, flags);
    HIP_TRY(ctx, hipGetLastError());
    const long per = FWD_THREADS / 64 * 8;
    jpeg_roundtrip_kernel<<<(unsigned)((n_blocks + per - 1) / per), FWD_THREADS, 0, st>>>(src, N, H, W, rects, desc, n, bgr ? 1 : 0, coeffs,
                                                                                           (long)n_blocks, *planes, flags);
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}

}  // namespace

extern "C" int avcer_jpeg_roundtrip_tiles(avcer_ctx* ctx, const uint8_t* src, int N, int H, int W, const int32_t* rects,
                                          const avcer_jpeg_desc* desc, int n, int bgr, int16_t* coeffs, int64_t n_blocks, int32_t* flags,
                                          uint8_t* tiles, avcer_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    uint8_t* planes = nullptr;
    TRY(jpeg_roundtrip_planes(ctx, "jpeg_roundtrip_tiles", src, N, H, W, rects, desc, n, bgr, coeffs, n_blocks, flags, tiles, &planes, st));
    const long total = (long)n * 224 * 56;
    jpeg_tiles_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(planes, desc, flags, n, tiles);
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}

extern "C" int avcer_jpeg_roundtrip_rgb(avcer_ctx* ctx, const uint8_t* src, int N, int H, int W, const int32_t* rects,
                                        const avcer_jpeg_desc* desc, int n, int bgr, int16_t* coeffs, int64_t n_blocks, int32_t* flags,
                                        uint8_t* canvas, int hmax, int wmax, avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    if (hmax <= 0 || wmax <= 0 || n <= 0 || (long)n * hmax * wmax >= (1L << 38))
        return set_err(ctx, AVCER_EINVAL, "jpeg_roundtrip_rgb: canvas %d x %d x %d", n, hmax, wmax);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* planes = nullptr;
    TRY(jpeg_roundtrip_planes(ctx, "jpeg_roundtrip_rgb", src, N, H, W, rects, desc, n, bgr, coeffs, n_blocks, flags, canvas, &planes, st));
    const long total = (long)n * hmax * wmax;
    jpeg_canvas_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(planes, desc, flags, n, hmax, wmax, canvas);
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}

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
    pack_check_kernel<<<1, PACK_THREADS, 0, st>>>(desc, n, n_blocks, wb, status, range);
    HIP_TRY(ctx, hipGetLastError());
    pack_count_kernel<<<per_item, PACK_THREADS, 0, st>>>(coeffs, desc, n, wb, n_blocks, status, range, nbits);
    HIP_TRY(ctx, hipGetLastError());
    pack_scan_kernel<<<(unsigned)n, PACK_THREADS, 0, st>>>(wb, range, status, nbits, fbits, bits);
    HIP_TRY(ctx, hipGetLastError());
    pack_emit_kernel<<<per_item, PACK_THREADS, 0, st>>>(coeffs, desc, n, wb, n_blocks, status, nbits, bits);
    HIP_TRY(ctx, hipGetLastError());
    pack_stuff_kernel<<<(unsigned)n, PACK_THREADS, 0, st>>>(wb, status, fbits, bits, flen);
    HIP_TRY(ctx, hipGetLastError());
    pack_place_kernel<<<1, PACK_THREADS, 0, st>>>(flen, n, cap_bytes, offsets, status, bytes_needed);
    HIP_TRY(ctx, hipGetLastError());
    pack_write_kernel<<<(unsigned)n, PACK_THREADS, 0, st>>>(desc, wb, status, fbits, flen, bits, offsets, out);
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}

// ================================================================================================ entropy decoding on the device
// avcer_jpeg_unpack: decode_scan / decode_block / Bits above as self-synchronising subsequence decoding (Klein & Wiseman; Weissenberger
// & Schmidt, "Accelerating JPEG Decompression on GPUs"), shaped for thousands of small independent files: a WORKGROUP takes a file
// and nothing ever waits for another workgroup.  The host (avcer_jpeg_scan_batch) parses the headers and copies the entropy-coded
// bytes; it does not walk them.  Phases of a workgroup, all counted loops with workgroup barriers between them:
//   marker   every byte gets its class from its neighbours (jsync::byte_class); prefix sums of the data bytes and of the stops give
//            the UNSTUFFED stream (words, first byte on top) and the list of stops: where the bit supply ends and which marker code
//            stands there.  Segment j (restart interval j, or the whole scan) is the data between stop j - 1 and stop j; a marker
//            where none is due therefore ends its segment's bits, exactly as Bits::fill does.
//   units    a segment is cut into subsequences of sub_bits; THREADS consecutive subsequences of the file are decoded side by side,
//            one thread each.  The first subsequence of a segment enters with the true state (the segment's first bit, slot 0, k 0),
//            thread 0 of a later unit of the same segment with the converged exit of the unit before; every other thread enters
//            with its left neighbour's last exit ("fresh block at my first bit" while that is unknown or an error).  Rounds repeat
//            until no exit changed.  Then every exit is the decode of the true chain: thread 0's entry is true, so its exit is final
//            after round 1, thread i's after round i + 1 by induction, and "nothing changed" means every thread decoded from the
//            exit its neighbour holds.  At most THREADS + 2 rounds; a thread whose entry did not change does not decode again.
//            A decode that meets an undefined code or the end of the bits parks at its subsequence's end, not synchronised.
//   write    a prefix sum of the finished blocks gives each subsequence the ordinal of its first block in the segment; the threads
//            decode once more from their final entry states and write AC values and DC differences to the zeroed storage
//            (jsync::storage_block: decode_scan's interleave).  A subsequence behind an error of the true chain writes nothing.
//            The decode ends with the segment's last block; fewer than 8 bits may be left, and the stop's code must be the one due.
//   predict  per component, a segmented prefix sum along the scan (restarting at every segment) turns differences into DC values;
//            decode_block's range checks of the prediction follow.
// Every defect carries its place in scan order (jsync::defect); the smallest is the file's reason, as the host pass returns at the
// first one.  Coefficients of a file that is not OK are unspecified, as they are there.
namespace {
namespace js = jsync;
static_assert(js::R_SCAN == R_SCAN && js::R_TRUNCATED == R_TRUNCATED && js::R_CODE == R_CODE && js::R_INDEX == R_INDEX &&
              js::R_RESTART == R_RESTART && js::R_NO_EOI == R_NO_EOI && js::R_RANGE == R_RANGE && js::R_SIZE == R_SIZE &&
              js::R_TABLE == R_TABLE, "one set of reasons");
static_assert(js::THREADS == PACK_THREADS, "block_scan is written for this many threads");
static_assert(sizeof(avcer_jpeg_tab) == 288 && sizeof(avcer_jpeg_scan) == 48, "layout of the ABI structs");

// where file i keeps its stops and segments in the per-block scratch arrays: n_blocks + 2 entries of its own (a file has at most
// as many segments as MCUs, and the segment table one entry more)
__host__ __device__ inline int64_t seg_scratch(const Desc& d, int i) { return d.coef_block + 2 * (int64_t)i; }

__global__ void unpack_tabs_kernel(const avcer_jpeg_tab* __restrict__ tabs, int n_tabs, js::DTab* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_tabs) js::derive_tab(tabs[i], out[i]);
}

__global__ void __launch_bounds__(js::THREADS) unpack_kernel(const uint8_t* __restrict__ bytes, int64_t n_bytes,
                                                             const avcer_jpeg_scan* __restrict__ scan, const js::DTab* __restrict__ dtabs,
                                                             int n_tabs, Desc* desc, int16_t* __restrict__ coeffs, int64_t n_blocks,
                                                             int32_t* __restrict__ status, int sub, uint8_t* __restrict__ comp,
                                                             int32_t* __restrict__ stop_pos, int32_t* __restrict__ stop_code,
                                                             int32_t* __restrict__ seg_sub) {
    __shared__ js::DTab tabs[6];
    __shared__ js::State exits[js::THREADS];
    __shared__ int32_t pex[js::THREADS];
    __shared__ uint32_t tot[PACK_WAVES];
    __shared__ SegSum segtot[PACK_WAVES];
    __shared__ unsigned long long errkey;
    __shared__ js::Carry carry;
    const int i = blockIdx.x, t = threadIdx.x;
    Desc& d = desc[i];
    if (d.status != AVCER_JPEG_OK) {  // the whole workgroup
        if (t == 0) status[i] = d.status;
        return;
    }
    const avcer_jpeg_scan sc = scan[i];
    js::File f;
    int r = js::check_file(d, sc, n_bytes, n_tabs, n_blocks, f);
    if (r == R_OK)
        for (int c = 0; c < f.ncomp; ++c)
            if (!dtabs[sc.dc[c]].dc_ok || !dtabs[sc.ac[c]].ok) r = R_TABLE;
    if (r != R_OK) {  // the whole workgroup
        if (t == 0) {
            d.reason = r;
            d.status = status[i] = AVCER_JPEG_NOT_HANDLED;
        }
        return;
    }
    for (int c = 0; c < f.ncomp; ++c)
        for (int k = 0; k < 2; ++k) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(dtabs + (k ? sc.ac[c] : sc.dc[c]));
            uint32_t* dst = reinterpret_cast<uint32_t*>(tabs + 2 * c + k);
            for (int x = t; x < (int)(sizeof(js::DTab) / 4); x += js::THREADS) dst[x] = src[x];
        }
    const int64_t sb = seg_scratch(d, i);
    const int32_t nseg = f.nseg;
    js::View v = {&f, tabs, &d, coeffs + 64 * d.coef_block, reinterpret_cast<uint32_t*>(comp + sc.offset), stop_pos + sb, stop_code + sb,
                  seg_sub + sb, sub, 0, 0};
    for (int j = t; j < nseg; j += js::THREADS) v.stop_code[j] = -1;
    {
        uint4* z = reinterpret_cast<uint4*>(v.fc);
        for (int64_t x = t; x < 8 * d.n_blocks; x += js::THREADS) z[x] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (t == 0) {
        errkey = js::NO_DEFECT;
        carry = js::Carry{js::State{0, js::NOSYNC}, 0};
    }
    __syncthreads();

    // ---- marker: 16 bytes a thread and turn
    const uint8_t* fb = bytes + sc.offset;
    const int32_t nb = (int32_t)sc.nbytes;
    int32_t total_data = 0, all_stops = 0;
    for (int32_t c0 = 0; c0 < nb; c0 += 16 * js::THREADS) {
        const int32_t p0 = c0 + 16 * t;
        const int cnt = max(0, min(16, nb - p0));
        uint8_t b[16];
        if (cnt == 16) {
            const uint4 q = *reinterpret_cast<const uint4*>(fb + p0);
            const uint32_t vw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) b[k] = (uint8_t)(vw[k >> 2] >> (8 * (k & 3)));
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) b[k] = k < cnt ? fb[p0 + k] : (uint8_t)0;
        }
        int prev2 = cnt && p0 >= 2 ? fb[p0 - 2] : 0, prev = cnt && p0 >= 1 ? fb[p0 - 1] : 0;
        const bool hn = p0 + 16 < nb;
        const int nx = hn ? fb[p0 + 16] : 0;
        uint64_t cls = 0;
        uint32_t nd = 0, ns = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < cnt) {
                const int cl = js::byte_class(prev2, prev, b[k], k < 15 ? k + 1 < cnt : hn, k < 15 ? b[(k + 1) & 15] : nx);
                nd += cl == js::B_DATA;
                ns += cl == js::B_STOP;
                cls |= (uint64_t)cl << (3 * k);
                prev2 = prev;
                prev = b[k];
            }
        uint32_t total;
        const uint32_t incl = block_scan(nd | (ns << 16), tot, &total);  // at most 4096 data bytes and 2048 stops a turn
        int32_t dpos = total_data + (int32_t)((incl & 0xffff) - nd), spos = all_stops + (int32_t)((incl >> 16) - ns);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < cnt) js::place_byte(v, (int)(cls >> (3 * k)) & 7, b[k], dpos, spos);
        total_data += (int32_t)(total & 0xffff);
        all_stops += (int32_t)(total >> 16);
    }
    v.total_data = total_data;
    v.nstops = min(all_stops, nseg);
    __syncthreads();

    // ---- segments: the first subsequence of segment j among the file's
    int32_t total_sub = 0;
    for (int32_t j0 = 0; j0 < nseg; j0 += js::THREADS) {
        const int32_t j = j0 + t;
        const uint32_t ns = j < nseg ? (uint32_t)js::seg_subs(v, j) : 0u;
        uint32_t total;
        const uint32_t incl = block_scan(ns, tot, &total);
        if (j < nseg) v.seg_sub[j] = total_sub + (int32_t)(incl - ns);
        total_sub += (int32_t)total;
    }
    if (t == 0) v.seg_sub[nseg] = total_sub;
    __syncthreads();

    // ---- units
    for (int32_t b0 = 0; b0 < total_sub; b0 += js::THREADS) {
        const js::Sub x = js::locate(v, b0 + t, b0, t, total_sub, carry.state);
        js::Round rd = js::before_rounds(x);
        exits[t] = x.park();
        __syncthreads();
        for (int round = 0; round < js::THREADS + 2; ++round) {
            const int changed = js::round_step(v, x, js::entry(x, t, exits), rd);
            __syncthreads();  // every thread has read its neighbour's exit
            if (changed) exits[t] = rd.mine;
            if (!__syncthreads_or(changed)) break;
        }
        // ---- write
        const js::State in = js::entry(x, t, exits);
        int32_t top;
        const int32_t lastflag = block_scan(js::unsynced(x, t, in), reinterpret_cast<int32_t*>(tot), &top, ScanMax());
        const bool valid = js::valid(x, lastflag);
        uint32_t total;
        pex[t] = (int32_t)(block_scan((uint32_t)rd.cnt, tot, &total) - (uint32_t)rd.cnt);
        __syncthreads();
        const long long ord = js::entry_ordinal(x, t, pex, carry.ord);
        if (valid) {
            const unsigned long long key = js::write_step(v, x, in, ord);
            if (key != js::NO_DEFECT) atomicMin(&errkey, key);
        }
        __syncthreads();  // carry and exits are read
        if (t == js::THREADS - 1 && x.live) carry = js::hand_over(x, valid, rd, ord);
        __syncthreads();
    }

    // ---- predict
    for (int c = 0; c < f.ncomp; ++c) {
        const int64_t count = js::predict_count(f, c);
        SegSum sum = {0u, 0u};  // the running prediction in front of thread 0
        for (int64_t q0 = 0; q0 < count; q0 += js::THREADS) {
            const int64_t q = q0 + t;
            js::Item it = {};
            int16_t* blk = nullptr;
            SegSum mine = {0u, 0u}, all;
            if (q < count) {
                it = js::predict_item(f, c, q);
                blk = v.fc + 64 * js::storage_block(f, it.mcu, it.slot);
                mine = SegSum{(uint32_t)(int32_t)blk[0], it.restart};
            }
            mine = ScanSeg()(sum, block_scan(mine, segtot, &all, ScanSeg()));
            sum = ScanSeg()(sum, all);
            if (q < count) {
                // exact up to and including the first block out of range (sums are modulo 2^32); later ones lose to it
                const unsigned long long key = js::predict_check(v, c, it, (int32_t)mine.v);
                if (key != js::NO_DEFECT) atomicMin(&errkey, key);
                blk[0] = (int16_t)(int32_t)mine.v;
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        const unsigned long long key = errkey;
        if (key != js::NO_DEFECT) {
            d.reason = (int32_t)(key & 31);
            d.status = AVCER_JPEG_NOT_HANDLED;
        }
        status[i] = key != js::NO_DEFECT ? AVCER_JPEG_NOT_HANDLED : AVCER_JPEG_OK;
    }
}

// One file of avcer_jpeg_unpack_host: the driver of unpack_kernel once more, with the threads of a unit as a loop.  Every decision
// is the kernel's own (the per-thread functions of jpeg_sync_dev.h); here are only the running sums that stand in for its scans,
// the loop ends that stand in for its barriers, and std::min for its atomicMin.  Returns the reason.
int unpack_file_host(const uint8_t* bytes, int64_t n_bytes, const avcer_jpeg_scan& sc, const js::DTab* dtabs, int n_tabs, const Desc& d,
                     int16_t* coeffs, int64_t n_blocks, int sub) {
    js::File f;
    const int r = js::check_file(d, sc, n_bytes, n_tabs, n_blocks, f);
    if (r != R_OK) return r;
    js::DTab tabs[6];
    for (int c = 0; c < f.ncomp; ++c) {
        if (!dtabs[sc.dc[c]].dc_ok || !dtabs[sc.ac[c]].ok) return R_TABLE;
        tabs[2 * c] = dtabs[sc.dc[c]];
        tabs[2 * c + 1] = dtabs[sc.ac[c]];
    }
    const int32_t nseg = f.nseg, nb = (int32_t)sc.nbytes;
    std::vector<int32_t> stop_pos((size_t)nseg, 0), stop_code((size_t)nseg, -1), seg_sub((size_t)nseg + 1, 0);
    std::vector<uint32_t> words(((size_t)nb + 3) / 4 + 1, 0u);
    js::View v = {&f, tabs, &d, coeffs + 64 * d.coef_block, words.data(), stop_pos.data(), stop_code.data(), seg_sub.data(), sub, 0, 0};
    memset(v.fc, 0, sizeof(int16_t) * 64 * (size_t)d.n_blocks);
    unsigned long long errkey = js::NO_DEFECT;
    // ---- marker
    const uint8_t* fb = bytes + sc.offset;
    int32_t total_data = 0, all_stops = 0;
    for (int32_t p = 0; p < nb; ++p) {
        const int cl = js::byte_class(p >= 2 ? fb[p - 2] : 0, p >= 1 ? fb[p - 1] : 0, fb[p], p + 1 < nb, p + 1 < nb ? fb[p + 1] : 0);
        js::place_byte(v, cl, fb[p], total_data, all_stops);
    }
    v.total_data = total_data;
    v.nstops = std::min(all_stops, nseg);
    // ---- segments
    int32_t total_sub = 0;
    for (int32_t j = 0; j < nseg; ++j) {
        seg_sub[(size_t)j] = total_sub;
        total_sub += js::seg_subs(v, j);
    }
    seg_sub[(size_t)nseg] = total_sub;
    // ---- units
    constexpr int T = js::THREADS;
    std::vector<js::Sub> th((size_t)T);
    std::vector<js::Round> rs((size_t)T);
    std::vector<js::State> exits((size_t)T);
    std::vector<int32_t> pex((size_t)T);
    js::Carry carry = {js::State{0, js::NOSYNC}, 0};
    for (int32_t b0 = 0; b0 < total_sub; b0 += T) {
        for (int t = 0; t < T; ++t) {
            th[(size_t)t] = js::locate(v, b0 + t, b0, t, total_sub, carry.state);
            rs[(size_t)t] = js::before_rounds(th[(size_t)t]);
            exits[(size_t)t] = th[(size_t)t].park();
        }
        for (int round = 0; round < T + 2; ++round) {
            bool any = false;
            for (int t = 0; t < T; ++t) any |= js::round_step(v, th[(size_t)t], js::entry(th[(size_t)t], t, exits.data()), rs[(size_t)t]);
            for (int t = 0; t < T; ++t) exits[(size_t)t] = rs[(size_t)t].mine;  // behind the barrier: every entry has been read
            if (!any) break;
        }
        // ---- write
        int32_t pre = 0;
        for (int t = 0; t < T; ++t) {
            pex[(size_t)t] = pre;
            pre += rs[(size_t)t].cnt;
        }
        int32_t lastflag = -1;
        for (int t = 0; t < T; ++t) {
            const js::Sub& x = th[(size_t)t];
            const js::State in = js::entry(x, t, exits.data());
            lastflag = std::max(lastflag, js::unsynced(x, t, in));
            const bool valid = js::valid(x, lastflag);
            const long long ord = js::entry_ordinal(x, t, pex.data(), carry.ord);
            if (valid) errkey = std::min(errkey, js::write_step(v, x, in, ord));
            if (t == T - 1 && x.live) carry = js::hand_over(x, valid, rs[(size_t)t], ord);
        }
    }
    // ---- predict
    for (int c = 0; c < f.ncomp; ++c) {
        const int64_t count = js::predict_count(f, c);
        uint32_t sum = 0;
        for (int64_t q = 0; q < count; ++q) {
            const js::Item it = js::predict_item(f, c, q);
            int16_t* blk = v.fc + 64 * js::storage_block(f, it.mcu, it.slot);
            const uint32_t dv = (uint32_t)(int32_t)blk[0];
            sum = it.restart ? dv : sum + dv;
            errkey = std::min(errkey, js::predict_check(v, c, it, (int32_t)sum));
            blk[0] = (int16_t)(int32_t)sum;
        }
    }
    return errkey == js::NO_DEFECT ? R_OK : (int)(errkey & 31);
}

int unpack_args(avcer_ctx* ctx, const char* what, const void* bytes, int64_t n_bytes, const void* scan, const void* tabs, int n_tabs,
                const void* desc, int n, const void* coeffs, int64_t n_blocks, const void* status, int sub_bits, bool device) {
    const uintptr_t a16 = device ? 15 : 0;  // the kernel moves 16 bytes at a time
    if (!bytes || !scan || !tabs || !desc || !coeffs || !status || n <= 0 || n_tabs <= 0 || n_bytes <= 0 || n_blocks <= 0 ||
        n_blocks >= (1LL << 31) - 2 * (int64_t)n || ((uintptr_t)bytes & a16) || ((uintptr_t)coeffs & (a16 | 1)) ||
        ((uintptr_t)desc & (a16 | 7)) || ((uintptr_t)scan & 7) || ((uintptr_t)status & 3) ||
        (sub_bits != 0 && (sub_bits < 128 || sub_bits > js::MAX_SUB_BITS || sub_bits % 32 != 0)))
        return set_err(ctx, AVCER_EINVAL,
                       "%s: bad arguments (n %d, %d tables, %lld bytes, %lld blocks < 2^31; sub_bits %d: 0 or a multiple of 32 in [128, 2^20]; "
                       "bytes, coefficients and descriptors 16-byte aligned)",
                       what, n, n_tabs, (long long)n_bytes, (long long)n_blocks, sub_bits);
    return AVCER_OK;
}

}  // namespace

namespace {
int scan_batch(avcer_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, uint8_t* bytes, int64_t cap_bytes,
               avcer_jpeg_desc* desc, avcer_jpeg_scan* scan, avcer_jpeg_tab* tabs, int cap_tabs, int threads, int hflags, int32_t* n_tabs,
               int64_t* bytes_needed, int64_t* blocks_needed) {
    const bool std_tables = (hflags & AVCER_JPEG_STD_TABLES) != 0;
    // ctx may be NULL (host-only call, no device needed): errors then come back as the code alone
    if (n < 0 || (n && (!files || !lens || !desc || !scan)) || cap_bytes < 0 || (cap_bytes && !bytes) || cap_tabs < 0 || (cap_tabs && !tabs) ||
        !n_tabs || (hflags & ~AVCER_JPEG_STD_TABLES))
        return set_err(ctx, AVCER_EINVAL, "jpeg_scan_batch: bad arguments");
    try {
        struct Found {  // what the header of one file says beyond its descriptor
            avcer_jpeg_tab tab[6];  // [2 c] the DC and [2 c + 1] the AC table of component c, as their DHT segments state them
            size_t at = 0;          // the first entropy-coded byte
            int restart = 0;
        };
        std::vector<Found> found((size_t)n);
        const int nt = std::max(1, std::min(pool_size(threads), n));
        each_index(n, nt, [&](int i) {
            std::unique_ptr<Header> h(new Header());
            const int r = parse_header(files[i], lens[i] < 0 ? 0 : (size_t)lens[i], *h, std_tables);  // no bytes: R_NO_SOI
            desc[i] = h->d;
            desc[i].reason = r;
            if (r != R_OK) return;
            Found& fo = found[(size_t)i];
            memset(fo.tab, 0, sizeof(fo.tab));
            for (int c = 0; c < h->d.ncomp; ++c)
                for (int k = 0; k < 2; ++k) {
                    const Huff& t = k ? h->ac[h->ta[c]] : h->dc[h->td[c]];
                    memcpy(fo.tab[2 * c + k].bits, t.bits, sizeof(t.bits));
                    fo.tab[2 * c + k].bits[0] = 0;
                    memcpy(fo.tab[2 * c + k].vals, t.vals, sizeof(t.vals));
                }
            fo.at = h->scan;
            fo.restart = h->restart;
        });
        // in file order: blocks as in avcer_jpeg_entropy_batch, the next free 16-byte aligned bytes, tables by content
        std::map<std::string, int> seen;
        std::vector<const avcer_jpeg_tab*> list;
        int64_t used_blocks = 0, need_blocks = 0, used_bytes = 0, need_bytes = 0;
        for (int i = 0; i < n; ++i) {
            Desc& d = desc[i];
            int r = d.reason;
            memset(&scan[i], 0, sizeof(scan[i]));
            if (r == R_OK) {
                const Found& fo = found[(size_t)i];
                const int64_t nb = lens[i] - (int64_t)fo.at, room = (nb + 15) & ~(int64_t)15;
                need_blocks += d.n_blocks;
                need_bytes += room;
                bool fits = room <= cap_bytes - used_bytes;
                avcer_jpeg_scan s;
                memset(&s, 0, sizeof(s));
                for (int c = 0; c < d.ncomp; ++c)
                    for (int k = 0; k < 2; ++k) {
                        const avcer_jpeg_tab* t = &fo.tab[2 * c + k];
                        const auto at = seen.emplace(std::string(reinterpret_cast<const char*>(t), sizeof(*t)), (int)list.size());
                        if (at.second) list.push_back(t);
                        (k ? s.ac : s.dc)[c] = at.first->second;
                        fits = fits && at.first->second < cap_tabs;
                    }
                if (fits) {
                    s.offset = used_bytes;
                    s.nbytes = nb;
                    s.restart = fo.restart;
                    scan[i] = s;
                    used_bytes += room;
                } else {
                    r = R_NO_SPACE;
                }
            }
            d.coef_block = used_blocks;
            if (r == R_OK) used_blocks += d.n_blocks; else d.n_blocks = 0;
            d.reason = r;
            d.status = r == R_OK ? AVCER_JPEG_OK : AVCER_JPEG_NOT_HANDLED;
        }
        for (size_t k = 0; k < list.size() && (int)k < cap_tabs; ++k) tabs[k] = *list[k];
        *n_tabs = (int32_t)list.size();
        if (bytes_needed) *bytes_needed = need_bytes;
        if (blocks_needed) *blocks_needed = need_blocks;
        each_index(n, nt, [&](int i) {
            if (desc[i].status != AVCER_JPEG_OK) return;
            const avcer_jpeg_scan& s = scan[i];
            memcpy(bytes + s.offset, files[i] + found[(size_t)i].at, (size_t)s.nbytes);
            memset(bytes + s.offset + s.nbytes, 0, (size_t)(((s.nbytes + 15) & ~(int64_t)15) - s.nbytes));
        });
    } catch (...) {
        return set_err(ctx, AVCER_ENOMEM, "jpeg_scan_batch: out of host memory");
    }
    return AVCER_OK;
}
}  // namespace

extern "C" int avcer_jpeg_scan_batch(avcer_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, uint8_t* bytes, int64_t cap_bytes,
                                     avcer_jpeg_desc* desc, avcer_jpeg_scan* scan, avcer_jpeg_tab* tabs, int cap_tabs, int threads,
                                     int32_t* n_tabs, int64_t* bytes_needed, int64_t* blocks_needed) {
    return scan_batch(ctx, files, lens, n, bytes, cap_bytes, desc, scan, tabs, cap_tabs, threads, 0, n_tabs, bytes_needed, blocks_needed);
}

extern "C" int avcer_jpeg_scan_batch_ex(avcer_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, uint8_t* bytes,
                                        int64_t cap_bytes, avcer_jpeg_desc* desc, avcer_jpeg_scan* scan, avcer_jpeg_tab* tabs, int cap_tabs,
                                        int threads, int hflags, int32_t* n_tabs, int64_t* bytes_needed, int64_t* blocks_needed) {
    return scan_batch(ctx, files, lens, n, bytes, cap_bytes, desc, scan, tabs, cap_tabs, threads, hflags, n_tabs, bytes_needed, blocks_needed);
}

extern "C" int avcer_jpeg_unpack(avcer_ctx* ctx, const uint8_t* bytes, int64_t n_bytes, const avcer_jpeg_scan* scan, const avcer_jpeg_tab* tabs,
                                 int n_tabs, avcer_jpeg_desc* desc, int n, int16_t* coeffs, int64_t n_blocks, int32_t* status, int sub_bits,
                                 avcer_stream_t stream) {
    if (!ctx) return AVCER_EINVAL;
    TRY(unpack_args(ctx, "jpeg_unpack", bytes, n_bytes, scan, tabs, n_tabs, desc, n, coeffs, n_blocks, status, sub_bits, true));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    js::DTab* dtabs = nullptr;
    uint8_t* comp = nullptr;
    int32_t *stop_pos = nullptr, *stop_code = nullptr, *seg_sub = nullptr;
    const size_t per_block = (size_t)n_blocks + 2 * (size_t)n;
    TRY(ws_carve(ctx, WS_JPEG, "jpeg_unpack", [&](Arena& a) {
        dtabs = a.get<js::DTab>(sizeof(js::DTab) * (size_t)n_tabs);       // the derived tables
        comp = a.get<uint8_t>((size_t)n_bytes + 16);                      // the unstuffed bytes, file by file where `bytes` has them
        stop_pos = a.get<int32_t>(sizeof(int32_t) * per_block);           // per segment: the data bytes in front of its stop,
        stop_code = a.get<int32_t>(sizeof(int32_t) * per_block);          // ... the marker code there (-1: none),
        seg_sub = a.get<int32_t>(sizeof(int32_t) * per_block);            // ... its first subsequence among the file's
    }));
    unpack_tabs_kernel<<<(unsigned)((n_tabs + 63) / 64), 64, 0, st>>>(tabs, n_tabs, dtabs);
    HIP_TRY(ctx, hipGetLastError());
    unpack_kernel<<<(unsigned)n, js::THREADS, 0, st>>>(bytes, n_bytes, scan, dtabs, n_tabs, desc, coeffs, n_blocks, status,
                                                        sub_bits ? sub_bits : js::DEFAULT_SUB_BITS, comp, stop_pos, stop_code, seg_sub);
    HIP_TRY(ctx, hipGetLastError());
    return AVCER_OK;
}

extern "C" int avcer_jpeg_unpack_host(avcer_ctx* ctx, const uint8_t* bytes, int64_t n_bytes, const avcer_jpeg_scan* scan,
                                      const avcer_jpeg_tab* tabs, int n_tabs, avcer_jpeg_desc* desc, int n, int16_t* coeffs, int64_t n_blocks,
                                      int32_t* status, int sub_bits) {
    // ctx may be NULL.  Not a product path (include/avcer_hip.h): the device algorithm, phase by phase, for tests and sanitisers
    if (int rc = unpack_args(ctx, "jpeg_unpack_host", bytes, n_bytes, scan, tabs, n_tabs, desc, n, coeffs, n_blocks, status, sub_bits, false)) return rc;
    try {
        std::vector<js::DTab> dtabs((size_t)n_tabs);
        for (int k = 0; k < n_tabs; ++k) js::derive_tab(tabs[k], dtabs[(size_t)k]);
        each_index(n, std::min(pool_size(0), n), [&](int i) {
            if (desc[i].status == AVCER_JPEG_OK) {
                const int r = unpack_file_host(bytes, n_bytes, scan[i], dtabs.data(), n_tabs, desc[i], coeffs, n_blocks,
                                               sub_bits ? sub_bits : js::DEFAULT_SUB_BITS);
                if (r != R_OK) {
                    desc[i].reason = r;
                    desc[i].status = AVCER_JPEG_NOT_HANDLED;
                }
            }
            status[i] = desc[i].status;
        });
    } catch (...) {
        return set_err(ctx, AVCER_ENOMEM, "jpeg_unpack_host: out of host memory");
    }
    return AVCER_OK;
}
