// JPEG entropy decoding on the device.
// avcer_jpeg_unpack: decode_scan / decode_block / Bits of jpeg_decode.hip as self-synchronising subsequence decoding (Klein &
// Wiseman; Weissenberger
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
#include "jpeg.h"
#include "jpeg_sync_dev.h"

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

extern "C" int avcer_jpeg_scan_batch(avcer_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, uint8_t* bytes, int64_t cap_bytes,
                                     avcer_jpeg_desc* desc, avcer_jpeg_scan* scan, avcer_jpeg_tab* tabs, int cap_tabs, int threads,
                                     int32_t* n_tabs, int64_t* bytes_needed, int64_t* blocks_needed) {
    return avcer_jpeg_scan_batch_ex(ctx, files, lens, n, bytes, cap_bytes, desc, scan, tabs, cap_tabs, threads, 0, n_tabs, bytes_needed,
                                    blocks_needed);
}

extern "C" int avcer_jpeg_scan_batch_ex(avcer_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, uint8_t* bytes,
                                        int64_t cap_bytes, avcer_jpeg_desc* desc, avcer_jpeg_scan* scan, avcer_jpeg_tab* tabs, int cap_tabs,
                                        int threads, int hflags, int32_t* n_tabs, int64_t* bytes_needed, int64_t* blocks_needed) {
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
        const int nt = threads_for(threads, n);
        each_index<Header>(n, nt, [&](int i, Header& h) {
            const int r = parse_header(files[i], lens[i] < 0 ? 0 : (size_t)lens[i], h, std_tables);  // no bytes: R_NO_SOI
            desc[i] = h.d;
            desc[i].reason = r;
            if (r != R_OK) return;
            Found& fo = found[(size_t)i];
            memset(fo.tab, 0, sizeof(fo.tab));
            for (int c = 0; c < h.d.ncomp; ++c)
                for (int k = 0; k < 2; ++k) {
                    const Huff& t = k ? h.ac[h.ta[c]] : h.dc[h.td[c]];
                    memcpy(fo.tab[2 * c + k].bits, t.bits, sizeof(t.bits));
                    fo.tab[2 * c + k].bits[0] = 0;
                    memcpy(fo.tab[2 * c + k].vals, t.vals, sizeof(t.vals));
                }
            fo.at = h.scan;
            fo.restart = h.restart;
        });
        // in file order: blocks as in avcer_jpeg_entropy_batch (place_blocks; their storage is the caller's and has no bound here), and
        // with them the next free 16-byte aligned bytes and the tables by content.  A file's tables are entered before it is known to
        // fit: one that does not still claims their indices.
        std::map<std::string, int> seen;
        std::vector<const avcer_jpeg_tab*> list;
        int64_t used_bytes = 0, need_bytes = 0;
        if (n) memset(scan, 0, sizeof(*scan) * (size_t)n);
        const int64_t need_blocks = place_blocks(desc, n, [&](int i, const Desc& d, int64_t) {
            const Found& fo = found[(size_t)i];
            const int64_t nb = lens[i] - (int64_t)fo.at, room = (nb + 15) & ~(int64_t)15;
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
            }
            return fits;
        });
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
    LAUNCH(ctx, unpack_tabs_kernel<<<(unsigned)((n_tabs + 63) / 64), 64, 0, st>>>(tabs, n_tabs, dtabs));
    LAUNCH(ctx, unpack_kernel<<<(unsigned)n, js::THREADS, 0, st>>>(bytes, n_bytes, scan, dtabs, n_tabs, desc, coeffs, n_blocks, status,
                                                                    sub_bits ? sub_bits : js::DEFAULT_SUB_BITS, comp, stop_pos, stop_code,
                                                                    seg_sub));
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
        each_index(n, threads_for(0, n), [&](int i) {
            if (desc[i].status == AVCER_JPEG_OK) {
                const int r = unpack_file_host(bytes, n_bytes, scan[i], dtabs.data(), n_tabs, desc[i], coeffs, n_blocks,
                                               sub_bits ? sub_bits : js::DEFAULT_SUB_BITS);
                if (r != R_OK) not_handled(desc[i], r);
            }
            status[i] = desc[i].status;
        });
    } catch (...) {
        return set_err(ctx, AVCER_ENOMEM, "jpeg_unpack_host: out of host memory");
    }
    return AVCER_OK;
}
