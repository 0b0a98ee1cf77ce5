// What more than one of the four JPEG sources needs, stated once (jpeg_decode.hip: files -> pixels; jpeg_encode.hip: pixels ->
// files; jpeg_pack.hip: the Huffman coder on the device; jpeg_unpack.hip: the Huffman decoder on the device): the descriptor's
// reasons, the standard's tables, the header parser's types, the host thread pool and the storage placement, the device pieces
// the round-trip kernel shares with kernel A, the wave / block scans of pack and unpack, and the host launchers that cross files.
// Device functions are __device__ __forceinline__ here; every __global__ kernel lives in exactly one .hip.
#pragma once

#include "common.h"

#include <algorithm>
#include <atomic>
#include <memory>
#include <new>
#include <thread>

// a kernel launch and its check: LAUNCH(ctx, kernel<<<grid, block, 0, st>>>(...)) returns from the launcher when the launch failed
#define LAUNCH(ctx, ...)                    \
    do {                                    \
        __VA_ARGS__;                        \
        HIP_TRY(ctx, hipGetLastError());    \
    } while (0)

typedef avcer_jpeg_desc Desc;

// ------------------------------------------------------------------------------------------------ across files
// The header parser (jpeg_decode.hip); jpeg_unpack.hip's avcer_jpeg_scan_batch_ex reads the tables and the scan's place from it
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

int parse_header(const uint8_t* s, size_t len, Header& h, bool std_tables = false);

// jpeg_decode.hip, for the round trip of jpeg_encode.hip as well: the component planes in the context's JPEG workspace, and kernel B
// from them (tiles; the canvas, whose size canvas_args checks under the entry's name `what` before anything is launched)
int jpeg_plane_ws(avcer_ctx* ctx, int64_t n_blocks, uint8_t** planes);
int launch_jpeg_tiles(avcer_ctx* ctx, const uint8_t* planes, const Desc* desc, const int32_t* flags, int n, uint8_t* tiles, hipStream_t st);
int canvas_args(avcer_ctx* ctx, const char* what, int n, int hmax, int wmax);
int launch_jpeg_canvas(avcer_ctx* ctx, const uint8_t* planes, const Desc* desc, const int32_t* flags, int n, int hmax, int wmax,
                       uint8_t* canvas, hipStream_t st);

// What the device entries of jpeg_decode.hip and jpeg_encode.hip check of the coefficient storage and its descriptors (defined in
// jpeg_decode.hip): a context, n > 0 descriptors and fewer than 2^34 blocks, both 16-byte aligned; `coeffs` may be null only where
// `null_ok` (the round trip).  `own`: the entry's own conditions; `frames`: N, H, W of the entry's source frames, for the text.
int coeff_args(avcer_ctx* ctx, const char* what, const void* coeffs, bool null_ok, int64_t n_blocks, const void* desc, int n, bool own,
               const int* frames = nullptr);

namespace {

// ------------------------------------------------------------------------------------------------ host: reasons and tables
enum {  // Desc::reason: why a file is not handled (0 = it is)
    R_OK = 0, R_NO_SOI = 1, R_MARKER = 2, R_SOF_KIND = 3, R_PRECISION = 4, R_COMPONENTS = 5, R_SAMPLING = 6, R_COLOUR = 7, R_TABLE = 8,
    R_SCAN = 9, R_TRUNCATED = 10, R_CODE = 11, R_NO_SPACE = 12, R_INDEX = 13, R_RESTART = 14, R_NO_EOI = 15, R_RANGE = 16, R_SIZE = 17,
    R_ENC_SIZE = 18, R_ENC_DESC = 19  // encoding: an image of no or of more than 65535 pixels a side; a descriptor avcer_jpeg_plan did not write
};

constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// The four DHT segments as libjpeg writes them (the standard's tables K.3 - K.6), marker and length included: DC 0, AC 0, DC 1, AC 1.
// The ONE statement of these tables: the writers emit them (jpeg_encode.hip, jpeg_pack.hip), and the reader assumes them for a table
// a scan references and no DHT segment defined when AVCER_JPEG_STD_TABLES asks for it (MJPEG frames, parse_header)
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

constexpr size_t HEADER_BYTES = 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 14;  // SOI, APP0, two DQT, SOF0, four DHT, SOS: 623

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

// threads of the entropy pass: what the caller asks for, 16 at most and by default -- never the machine's core count.  The library
// reads no environment: avcer_amd/jpeg.py turns OMP_NUM_THREADS into the argument.
int pool_size(int threads) { return threads <= 0 || threads > 16 ? 16 : threads; }
int threads_for(int threads, int n) { return std::max(1, std::min(pool_size(threads), n)); }  // ... and no more than there are files

// fn(i, s) for every i < n, handed out one at a time to nt threads (this one included); s is the thread's one State, made inside it
// (a Header is 13 KB of Huffman look-up tables: nt sets in memory and not n).  Nothing may leave a thread; what one did not take
// the others take.
template <class State, class Fn>
void each_index(int n, int nt, const Fn& fn) {
    std::atomic<int> next(0);
    std::atomic<bool> failed(false);
    const auto work = [&]() {
        try {
            std::unique_ptr<State> s(new State());
            for (int i; (i = next.fetch_add(1)) < n;) fn(i, *s);
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

// fn(i) where a thread needs nothing of its own
struct NoState {};
template <class Fn>
void each_index(int n, int nt, const Fn& fn) {
    each_index<NoState>(n, nt, [&](int i, NoState&) { fn(i); });
}

// file `d` is not handled, and why
inline void not_handled(Desc& d, int reason) {
    d.reason = reason;
    d.status = AVCER_JPEG_NOT_HANDLED;
}

// The coefficient storage of a batch whose headers are parsed (Desc::reason says how that went).  In file order every handled file
// takes the next free blocks, so offsets ascend (kernel A finds a block's image by them); a file for which fits(i, d, used) -- is
// there room for it behind `used` blocks, and for whatever else the caller places with it -- does not hold becomes R_NO_SPACE and
// takes nothing.  Every file gets its coef_block and its final status; returns the blocks all handled files would take.
template <class Fits>
int64_t place_blocks(Desc* desc, int n, const Fits& fits) {
    int64_t used = 0, needed = 0;
    for (int i = 0; i < n; ++i) {
        Desc& d = desc[i];
        int r = d.reason;
        if (r == R_OK) {
            needed += d.n_blocks;
            if (!fits(i, d, used)) r = R_NO_SPACE;
        }
        d.coef_block = used;
        if (r == R_OK) used += d.n_blocks; else d.n_blocks = 0;
        d.reason = r;
        d.status = r == R_OK ? AVCER_JPEG_OK : AVCER_JPEG_NOT_HANDLED;
    }
    return needed;
}

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

constexpr int WS_LD = 9;  // dwords per row of a block's 8 x 8 workspace in LDS

// Range guard (kernel A and the round trip).  libjpeg's C code (wide integers, a range table that wraps at 10 bits) and its SIMD
// code (16-bit pair sums,
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

// ------------------------------------------------------------------------------------------------ device: scans (pack, unpack)
constexpr int PACK_THREADS = 256;  // 4 waves
constexpr int PACK_WAVES = PACK_THREADS / 64;

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

}  // namespace
