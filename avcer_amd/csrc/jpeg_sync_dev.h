// Self-synchronising Huffman decoding of a JPEG scan (avcer_jpeg_unpack, csrc/jpeg_unpack.hip): the pieces that the device kernel and its
// host statement avcer_jpeg_unpack_host share, which is every decision of the algorithm -- the byte classes of the marker pass and
// where a classified byte goes, the derived Huffman table, the bit reader over the unstuffed bytes, the cut of a segment into
// subsequences, where a subsequence lies and what it enters with, ONE subsequence's decode from an entry state, a round's step, the
// write step with its marker check, the hand-over between units, the DC prediction's items and range check, the block-ordinal ->
// storage mapping.  Everything is __host__ __device__, integer and free of barriers.  Written per side is only how the threads of a
// unit run and combine: jpeg_unpack.hip's kernel loads 16 bytes a thread, scans across the workgroup, waits at barriers and takes the
// smallest defect with atomicMin; the host statement loops over the "threads" with running sums and std::min.
//
// Semantics are those of Bits / decode_block / decode_scan in jpeg_decode.hip, restated on the UNSTUFFED bytes of one segment (a restart
// interval, or the whole scan): bits behind the segment's end read as zero and cannot be consumed (`bad`).
#pragma once

#include <cstdint>

#include "../../include/avcer_hip.h"

#define JS_HD __host__ __device__ inline

namespace jsync {

enum { R_SCAN = 9, R_TRUNCATED = 10, R_CODE = 11, R_INDEX = 13, R_RESTART = 14, R_NO_EOI = 15, R_RANGE = 16, R_SIZE = 17, R_TABLE = 8 };

constexpr int THREADS = 256;              // subsequences a workgroup decodes side by side: one unit at the most
constexpr int DEFAULT_SUB_BITS = 512;     // a 17 KB crop: one to two units
constexpr int MAX_SUB_BITS = 1 << 20;
constexpr int64_t MAX_SCAN_BYTES = 1 << 27;  // bit positions inside a file are 32 bits wide
constexpr int32_t NOSYNC = -1;            // State::sk of a subsequence whose decode met an error: its exit is no symbol boundary
constexpr int32_t NO_STOP = 0x7fffffff;   // the last subsequence of a segment decodes until the blocks are complete or the bits run out

constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ------------------------------------------------------------------------------------------------ marker pass
// Class of byte `cur` of the entropy-coded bytes, from its two predecessors and its successor (0 where there is none, has_next
// false).  What Bits::fill and Bits::marker do with it: a 0xFF is data when a zero follows (and no 0xFF precedes: that one opened a
// marker, and marker() skips every 0xFF behind it); any other 0xFF belongs to a marker, the first of a run STOPS the bit supply;
// the byte behind such a run is the marker's code, whatever it is (0x00 behind FF FF too); the zero behind a data 0xFF is dropped.
enum { B_DROP = 0, B_DATA = 1, B_STOP = 2, B_FILL = 3, B_CODE = 4 };
JS_HD int byte_class(int prev2, int prev, int cur, bool has_next, int next) {
    if (cur == 0xFF) {
        if (prev == 0xFF) return B_FILL;
        return has_next && next == 0 ? B_DATA : B_STOP;
    }
    if (prev != 0xFF) return B_DATA;
    return cur == 0 && prev2 != 0xFF ? B_DROP : B_CODE;
}

// ------------------------------------------------------------------------------------------------ tables
// One Huffman table as Bits::symbol reads it (jpeg_decode.hip derive(), libjpeg's jpeg_make_d_derived_tbl)
struct DTab {
    uint16_t look[512];   // the next 9 bits -> (length << 8) | symbol, 0: the code is longer
    int32_t maxcode[17];  // largest code of each length, -1 where the length has none
    int32_t valoff[17];   // vals index of a code = code + valoff[length]
    uint8_t vals[256];
    int32_t ok, dc_ok;    // a consistent code; ... whose symbols are magnitude categories
};
static_assert(sizeof(DTab) == 1424 && sizeof(DTab) % 4 == 0, "DTab is copied into LDS as dwords");

JS_HD void derive_tab(const avcer_jpeg_tab& in, DTab& t) {
    t.ok = t.dc_ok = 0;
    for (int i = 0; i < 512; ++i) t.look[i] = 0;
    for (int i = 0; i < 256; ++i) t.vals[i] = in.vals[i];
    int c = 0, p = 0;
    bool fine = true;
    for (int l = 1; l <= 16; ++l) {
        const int nb = in.bits[l];
        t.maxcode[l] = -1;
        t.valoff[l] = 0;
        if (fine && (p + nb > 256 || c + nb > (1 << l))) fine = false;  // more than 256 symbols; a length over-subscribed
        if (fine && nb) {
            t.valoff[l] = p - c;
            if (l <= 9)
                for (int i = 0; i < nb; ++i)
                    for (int k = 0; k < (1 << (9 - l)); ++k) t.look[((c + i) << (9 - l)) + k] = (uint16_t)((l << 8) | in.vals[p + i]);
            p += nb;
            c += nb;
            t.maxcode[l] = c - 1;
        }
        c <<= 1;
    }
    t.maxcode[0] = -1;
    t.valoff[0] = 0;
    if (!fine) return;
    t.ok = 1;
    t.dc_ok = 1;
    for (int i = 0; i < p; ++i)
        if (in.vals[i] > 15) t.dc_ok = 0;
}

// ------------------------------------------------------------------------------------------------ geometry
// What decode_scan derives from a descriptor: blocks per MCU, MCUs, where each component's blocks start
struct File {
    int32_t ncomp, hs, vs, bpm, mx, nmcu, rst;  // rst: MCUs per segment (the restart interval, or all of them)
    int32_t nseg;
    int32_t bw[3];
    int64_t base[3];
};

// The descriptor and scan record of one file, checked before anything is read through them: the geometry is the one parse_header
// derives from the size and the sampling (so every storage block the mapping below yields lies inside the file's n_blocks), the
// blocks lie inside the storage, the bytes inside `bytes`, the tables inside `tabs`.  Returns a reason.
JS_HD int check_file(const avcer_jpeg_desc& d, const avcer_jpeg_scan& s, int64_t n_bytes, int n_tabs, int64_t n_blocks, File& f) {
    if (d.width < 1 || d.width > 65535 || d.height < 1 || d.height > 65535 || (d.ncomp != 1 && d.ncomp != 3)) return R_SCAN;
    int64_t total;
    if (d.ncomp == 3) {
        if (!((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2))) return R_SCAN;
        const int mx = (d.width + 8 * d.hs - 1) / (8 * d.hs), my = (d.height + 8 * d.vs - 1) / (8 * d.vs);
        if (d.bw[0] != mx * d.hs || d.bh[0] != my * d.vs || d.bw[1] != mx || d.bw[2] != mx || d.bh[1] != my || d.bh[2] != my) return R_SCAN;
        f.hs = d.hs;
        f.vs = d.vs;
        f.mx = mx;
        f.nmcu = mx * my;
        f.bpm = d.hs * d.vs + 2;
        total = (int64_t)f.nmcu * f.bpm;
        f.base[0] = 0;
        f.base[1] = (int64_t)d.bw[0] * d.bh[0];
        f.base[2] = f.base[1] + (int64_t)mx * my;
        f.bw[0] = d.bw[0];
        f.bw[1] = f.bw[2] = mx;
    } else {
        if (d.bw[0] != (d.width + 7) / 8 || d.bh[0] != (d.height + 7) / 8) return R_SCAN;
        f.hs = f.vs = 1;
        f.mx = d.bw[0];
        f.nmcu = d.bw[0] * d.bh[0];
        f.bpm = 1;
        total = f.nmcu;
        f.base[0] = f.base[1] = f.base[2] = 0;
        f.bw[0] = f.bw[1] = f.bw[2] = d.bw[0];
    }
    f.ncomp = d.ncomp;
    if (d.n_blocks != total || d.coef_block < 0 || d.n_blocks > n_blocks || d.coef_block > n_blocks - d.n_blocks) return R_SCAN;
    if (s.offset < 0 || (s.offset & 15) || s.nbytes < 0 || s.nbytes > n_bytes || s.offset > n_bytes - s.nbytes) return R_SCAN;
    if (s.nbytes > MAX_SCAN_BYTES) return R_SIZE;
    if (d.n_blocks > 4 * s.nbytes) return R_TRUNCATED;  // parse_header's refusal: a block costs two bits at the least
    if (s.restart < 0 || s.restart > 65535) return R_SCAN;
    for (int c = 0; c < d.ncomp; ++c)
        if (s.dc[c] < 0 || s.dc[c] >= n_tabs || s.ac[c] < 0 || s.ac[c] >= n_tabs) return R_SCAN;
    f.rst = s.restart ? s.restart : f.nmcu;
    f.nseg = (f.nmcu + f.rst - 1) / f.rst;
    return 0;
}

JS_HD int comp_of_slot(const File& f, int slot) { return f.ncomp == 1 || slot < f.hs * f.vs ? 0 : slot - f.hs * f.vs + 1; }

// Block `slot` of MCU `mcu` (decode_scan's loops: hs * vs luma blocks row by row, Cb, Cr; a one-component scan is not interleaved)
// -> its place among the file's coefficient blocks
JS_HD int64_t storage_block(const File& f, int64_t mcu, int slot) {
    const int64_t y = mcu / f.mx, x = mcu % f.mx;
    const int nl = f.hs * f.vs;
    if (f.ncomp == 1) return mcu;
    if (slot < nl) return (y * f.vs + slot / f.hs) * f.bw[0] + x * f.hs + slot % f.hs;
    return f.base[slot - nl + 1] + mcu;
}

// ------------------------------------------------------------------------------------------------ bits
// The unstuffed bytes of a file are kept as 32-bit words with the first byte on top (byte q of the stream is stored at q ^ 3 on
// a little-endian machine), so a bit position is (word, shift).  Up to 32 bits at `pos`; bits at or behind `end` read as zero.
JS_HD uint32_t peek32(const uint32_t* w, int32_t pos, int32_t end) {
    if (pos >= end) return 0u;
    const int32_t i = pos >> 5, sh = pos & 31;
    uint32_t v = w[i] << sh;
    if (sh && ((i + 1) << 5) < end) v |= w[i + 1] >> (32 - sh);
    const int32_t avail = end - pos;
    if (avail < 32) v &= ~(0xffffffffu >> avail);
    return v;
}

JS_HD void skip(int32_t& pos, int32_t end, int len, bool& bad) {
    if (len > end - pos) {
        bad = true;
        pos = end;
    } else {
        pos += len;
    }
}

JS_HD int symbol(const uint32_t* w, int32_t& pos, int32_t end, bool& bad, const DTab* t) {
    const uint32_t v = peek32(w, pos, end);
    const int e = t->look[v >> 23];
    if (e) {
        skip(pos, end, e >> 8, bad);
        return e & 255;
    }
    const int w16 = (int)(v >> 16);
    for (int l = 10; l <= 16; ++l) {
        const int c = w16 >> (16 - l);
        if (c <= t->maxcode[l]) {
            skip(pos, end, l, bad);
            return t->vals[(c + t->valoff[l]) & 255];
        }
    }
    bad = true;  // a code the table does not define
    return 0;
}

JS_HD int receive_extend(const uint32_t* w, int32_t& pos, int32_t end, bool& bad, int s) {  // s in 1..15
    const int v = (int)(peek32(w, pos, end) >> (32 - s));
    skip(pos, end, s, bad);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// ------------------------------------------------------------------------------------------------ one subsequence
// Where a decode stands at a symbol boundary: the bit position in the file's unstuffed bytes, the block slot inside the MCU, the
// zigzag index k (0: the next symbol is a DC code).  sk = slot << 8 | k, or NOSYNC.
struct State {
    int32_t pos, sk;
};
JS_HD bool same(const State& a, const State& b) { return a.pos == b.pos && a.sk == b.sk; }

struct Result {
    State exit;        // the first symbol boundary at or behind `stop` (unless err, or the blocks were complete before)
    int32_t blocks;    // blocks finished
    int32_t err;       // 0, or the reason the decode ended
    int32_t err_stage; // 0: the DC code, 2: behind it (stage 1, the DC range check, is the prediction pass's)
    int64_t err_ord;   // WRITE: the ordinal of the block it ended in
    int32_t done_pos;  // WRITE: the bit position behind block limit - 1 when this subsequence finished it, else -1
};

// Decodes from `in` to the first symbol boundary at or behind `stop`.  tabs: the file's tables, [2 c] the DC and [2 c + 1] the AC
// table of component c.  WRITE (the last pass, entry states final): `ord` is the ordinal, inside the segment, of the block `in`
// stands in, `limit` the blocks of the segment, mcu0 its first MCU; non-zero AC values go to their natural place and the DC
// DIFFERENCE to [0] of the block's storage (zeroed before), the v * q range check of decode_block is made, and the decode ends
// behind block limit - 1.  Every turn of the loop consumes a bit or ends it.
template <bool WRITE>
JS_HD void run(const uint32_t* w, int32_t end, int32_t stop, State in, const DTab* tabs, const File& f, int64_t ord, int64_t limit,
               int64_t mcu0, int16_t* blocks, const avcer_jpeg_desc* d, Result& o) {
    int32_t pos = in.pos;
    int slot = in.sk >> 8, k = in.sk & 255;
    bool bad = false;
    o.blocks = 0;
    o.err = 0;
    o.err_stage = 0;
    o.err_ord = ord;
    o.done_pos = -1;
    o.exit = in;
    if (WRITE && ord >= limit) return;
    int c = comp_of_slot(f, slot);
    int16_t* blk = nullptr;
    if (WRITE) blk = blocks + 64 * storage_block(f, mcu0 + ord / f.bpm, (int)(ord % f.bpm));
    while (pos < stop) {
        if (k == 0) {
            const int s = symbol(w, pos, end, bad, tabs + 2 * c) & 15;
            if (bad) {
                o.err = R_CODE;
                break;
            }
            const int v = s ? receive_extend(w, pos, end, bad, s) : 0;
            if (WRITE) blk[0] = (int16_t)v;
            k = 1;
            continue;
        }
        const int rs = symbol(w, pos, end, bad, tabs + 2 * c + 1);
        o.err_stage = 2;
        if (bad) {
            o.err = R_CODE;
            break;
        }
        const int r = rs >> 4, z = rs & 15;
        bool done = false;
        if (z) {
            k += r;
            if (k > 63) {
                o.err = R_INDEX;
                break;
            }
            const int v = receive_extend(w, pos, end, bad, z);
            if (WRITE) {
                const int nat = kZigzag[k], p = v * (int)d->qt[c][nat];
                if (p < -32768 || p > 32767) {
                    o.err = R_RANGE;
                    break;
                }
                blk[nat] = (int16_t)v;
            }
            done = ++k >= 64;
        } else if (r == 15) {
            k += 16;
            if (k > 64) {
                o.err = R_INDEX;
                break;
            }
            done = k >= 64;
        } else {
            done = true;
        }
        if (done) {
            if (bad) {
                o.err = R_TRUNCATED;
                break;
            }
            ++o.blocks;
            k = 0;
            slot = slot + 1 == f.bpm ? 0 : slot + 1;
            c = comp_of_slot(f, slot);
            o.err_stage = 0;
            if (WRITE) {
                ++ord;
                o.err_ord = ord;
                if (ord >= limit) {
                    o.done_pos = pos;
                    break;
                }
                blk = blocks + 64 * storage_block(f, mcu0 + ord / f.bpm, (int)(ord % f.bpm));
            }
        }
    }
    o.exit.pos = pos;
    o.exit.sk = (slot << 8) | k;
}

// The order of a file's defects along its scan: block g's DC code (0), its DC range (1), the rest of it (2), the marker behind it
// (3); the reason rides in the low bits, the smallest key is the file's reason.
constexpr unsigned long long NO_DEFECT = ~0ULL;
JS_HD unsigned long long defect(int64_t g, int stage, int reason) { return ((unsigned long long)(4 * g + stage) << 5) | (unsigned)reason; }

// ------------------------------------------------------------------------------------------------ the phases, thread by thread
// One file as its phases see it.  The per-segment arrays are the file's own: f.nseg entries, seg_sub one more.
struct View {
    const File* f;
    const DTab* tabs;             // [2 c] the DC and [2 c + 1] the AC table of component c
    const avcer_jpeg_desc* d;
    int16_t* fc;                  // the file's coefficient blocks, zeroed
    uint32_t* w;                  // its unstuffed bytes (peek32)
    int32_t *stop_pos, *stop_code;  // per segment: the data bytes in front of its stop, the marker code there (-1: none)
    int32_t* seg_sub;             // ... its first subsequence among the file's; [f.nseg]: all of them
    int32_t sub;                  // bits of a subsequence
    int32_t nstops, total_data;   // behind the marker pass: the stops that end a segment, the data bytes
};

// marker pass: byte `b` of class `cl`, behind dpos data bytes and spos stops
JS_HD void place_byte(const View& v, int cl, uint8_t b, int32_t& dpos, int32_t& spos) {
    if (cl == B_DATA) {
        reinterpret_cast<uint8_t*>(v.w)[dpos ^ 3] = b;
        ++dpos;
    } else if (cl == B_STOP) {
        if (spos < v.f->nseg) v.stop_pos[spos] = dpos;
        ++spos;
    } else if (cl == B_CODE) {
        if (spos >= 1 && spos <= v.f->nseg) v.stop_code[spos - 1] = b;
    }
}

// segments: the data bytes [seg_lo, seg_hi) of segment j, and the subsequences it is cut into
JS_HD int32_t seg_lo(const View& v, int j) { return j == 0 ? 0 : (j - 1 < v.nstops ? v.stop_pos[j - 1] : v.total_data); }
JS_HD int32_t seg_hi(const View& v, int j) { return j < v.nstops ? v.stop_pos[j] : v.total_data; }
JS_HD int32_t seg_subs(const View& v, int j) {
    const int32_t n = (8 * (seg_hi(v, j) - seg_lo(v, j)) + v.sub - 1) / v.sub;
    return n > 1 ? n : 1;
}

// Subsequence s of the file as thread t of the unit that begins at subsequence b0 holds it
struct Sub {
    bool live;               // there is such a subsequence
    bool first, last;        // of its segment
    bool is_true;            // its entry is known: the segment's start, or the hand-over of the unit before
    int32_t j;               // its segment
    int32_t start, stop;     // its bits; the last of a segment has NO_STOP
    int32_t end;             // the segment's bits end here
    int32_t sf;              // the thread that holds the segment's first subsequence: negative when a unit before does
    State true_in;           // the known entry
    // "a block begins at my first bit"; where a failed decode rests, not synchronised.  Derived where they are used: as fields they
    // cost unpack_kernel the registers that keep five of its workgroups on a CU
    JS_HD State fresh() const { return State{start, 0}; }
    JS_HD State park() const { return State{last ? end : stop, NOSYNC}; }
};

JS_HD Sub locate(const View& v, int32_t s, int32_t b0, int t, int32_t total_sub, const State& carry_state) {
    Sub x = {};
    x.live = s < total_sub;
    if (x.live) {
        int32_t lo = 0, hi = v.f->nseg - 1;  // the last segment that begins at or before s
        while (lo < hi) {
            const int32_t mid = (lo + hi + 1) >> 1;
            if (v.seg_sub[mid] <= s) lo = mid; else hi = mid - 1;
        }
        x.j = lo;
        const int32_t m = s - v.seg_sub[lo];
        x.sf = v.seg_sub[lo] - b0;
        x.start = 8 * seg_lo(v, lo) + m * v.sub;
        x.end = 8 * seg_hi(v, lo);
        x.first = m == 0;
        x.last = s + 1 == v.seg_sub[lo + 1];
        x.stop = x.last ? NO_STOP : x.start + v.sub;
    }
    x.is_true = x.live && (x.first || t == 0);
    x.true_in = x.first ? x.fresh() : carry_state;
    return x;
}

// The state thread t enters with; exits: every thread's last exit
JS_HD State entry(const Sub& x, int t, const State* exits) { return x.is_true ? x.true_in : (t > 0 ? exits[t - 1] : x.fresh()); }

// What a thread keeps from round to round: its exit, the entry that gave it, the blocks that decode finished
struct Round {
    State mine, last_in;
    int32_t cnt;
};
JS_HD Round before_rounds(const Sub& x) { return Round{x.park(), State{-1, -2}, 0}; }

// One round of one thread: decodes again only if its entry `in` changed.  True when its exit changed.
JS_HD bool round_step(const View& v, const Sub& x, State in, Round& r) {
    if (in.sk == NOSYNC) in = x.fresh();
    if (!x.live || same(in, r.last_in)) return false;
    Result o;
    run<false>(v.w, x.end, x.stop, in, v.tabs, *v.f, 0, 0, 0, nullptr, v.d, o);
    const State e = o.err ? x.park() : o.exit;
    const bool changed = !same(e, r.mine);
    r.mine = e;
    r.cnt = o.blocks;
    r.last_in = in;
    return changed;
}

// write: a thread behind a not-synchronised final entry `in` in its segment is behind an error of the true chain.  The inclusive
// maximum of unsynced() along the threads is `lastflag`.
JS_HD int32_t unsynced(const Sub& x, int t, const State& in) { return x.live && in.sk == NOSYNC ? t : -1; }
JS_HD bool valid(const Sub& x, int32_t lastflag) { return x.live && lastflag < (x.sf > 0 ? x.sf : 0); }

// The ordinal, inside its segment, of the block thread t enters in.  pex: the blocks the threads in front of each thread finished;
// carry_ord: those of the units before, for the segment that thread 0 continues
JS_HD long long entry_ordinal(const Sub& x, int t, const int32_t* pex, long long carry_ord) {
    if (!x.live) return 0;
    return x.sf >= 0 ? (long long)(pex[t] - pex[x.sf]) : carry_ord + pex[t];
}

// The last decode of a valid thread, from its final entry: writes its blocks and returns its defect, or NO_DEFECT
JS_HD unsigned long long write_step(const View& v, const Sub& x, const State& in, long long ord) {
    const File& f = *v.f;
    const int64_t mcu0 = (int64_t)x.j * f.rst;
    const int64_t limit = ((mcu0 + f.rst < f.nmcu ? mcu0 + f.rst : (int64_t)f.nmcu) - mcu0) * f.bpm;
    Result o;
    run<true>(v.w, x.end, x.stop, in, v.tabs, f, ord, limit, mcu0, v.fc, v.d, o);
    if (o.err) return defect(mcu0 * f.bpm + o.err_ord, o.err_stage, o.err);  // err and done_pos exclude each other: one defect at the most
    if (o.done_pos >= 0) {  // behind the segment's last block: fewer than 8 bits are left, and the stop's code is the one due
        const bool final = x.j == f.nseg - 1;
        const int code = x.j < v.nstops ? v.stop_code[x.j] : -1;
        if (x.end - o.done_pos >= 8 || code != (final ? 0xD9 : 0xD0 + (x.j & 7)))
            return defect(mcu0 * f.bpm + limit - 1, 3, final ? R_NO_EOI : R_RESTART);
    }
    return NO_DEFECT;
}

// What the last thread of a unit, if live, hands to thread 0 of the next
struct Carry {
    State state;    // its converged exit, or its park
    long long ord;  // the ordinal of the block that exit stands in
};
JS_HD Carry hand_over(const Sub& x, bool valid, const Round& r, long long ord) {
    return Carry{valid && r.mine.sk != NOSYNC ? r.mine : x.park(), ord + r.cnt};
}

// predict: component c's blocks in scan order are items 0 .. predict_count - 1
struct Item {
    int64_t mcu;
    int slot;
    bool restart;  // the prediction starts again here
};
JS_HD int blocks_per_mcu(const File& f, int c) { return c == 0 && f.ncomp == 3 ? f.hs * f.vs : 1; }
JS_HD int64_t predict_count(const File& f, int c) { return (int64_t)f.nmcu * blocks_per_mcu(f, c); }
JS_HD Item predict_item(const File& f, int c, int64_t q) {
    const int per = blocks_per_mcu(f, c), at = (int)(q % per);
    const int64_t mcu = q / per;
    return Item{mcu, (c == 0 ? 0 : f.hs * f.vs + c - 1) + at, at == 0 && mcu % f.rst == 0};
}
// decode_block's range checks of the DC value `pred` of component c's block `it`: the defect, or NO_DEFECT
JS_HD unsigned long long predict_check(const View& v, int c, const Item& it, int32_t pred) {
    const int64_t pq = (int64_t)pred * (int64_t)v.d->qt[c][0];
    const bool fine = pred >= -32768 && pred <= 32767 && pq >= -32768 && pq <= 32767;
    return fine ? NO_DEFECT : defect(it.mcu * v.f->bpm + it.slot, 1, R_RANGE);
}

}  // namespace jsync
