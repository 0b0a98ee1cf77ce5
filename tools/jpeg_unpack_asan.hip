// Host sanitiser check of the device entropy decoder's host side: a stand-alone program around avcer_jpeg_scan_batch and
// avcer_jpeg_unpack_host (csrc/jpeg_unpack.hip: the phases of the kernel as loops over its threads), built with AddressSanitizer and UBSan on
// the HOST side only and run on a CPU machine:
//   python tools/jpeg_unpack_asan.py      (writes the input files, compiles this file, runs it)
// Input file: i32 n; i64 [n] lengths; the files back to back.  Every buffer given to the library is a heap block of EXACTLY the
// size stated to it, so one byte past a capacity is a report.  The oracle is avcer_jpeg_entropy_batch on the same files.  No device is
// touched: ctx is NULL and no kernel is launched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/avcer_hip.h"

// what csrc/api.hip gives the library; this program links jpeg_decode.hip and jpeg_unpack.hip alone
struct avcer_ctx;
int set_err(avcer_ctx*, int code, const char*, ...) { return code; }
int ws_reserve(avcer_ctx*, int, size_t, void**) { return -1; }

static bool get(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0;
    if (!get(f, &n, 4) || n <= 0) return 2;
    std::vector<int64_t> lens((size_t)n);
    if (!get(f, lens.data(), 8 * (size_t)n)) return 2;
    std::vector<uint8_t*> files((size_t)n);
    for (int i = 0; i < n; ++i) {
        files[i] = (uint8_t*)malloc((size_t)lens[i] ? (size_t)lens[i] : 1);  // exact: a read past a file's end is a report
        if (!get(f, files[i], (size_t)lens[i])) return 2;
    }
    fclose(f);

    // the oracle
    std::vector<avcer_jpeg_desc> want((size_t)n);
    int64_t blocks = 0;
    if (avcer_jpeg_entropy_batch(nullptr, files.data(), lens.data(), n, nullptr, 0, want.data(), 1, &blocks) != 0 || blocks <= 0) return 3;
    int16_t* ref = (int16_t*)malloc((size_t)blocks * 128);
    if (avcer_jpeg_entropy_batch(nullptr, files.data(), lens.data(), n, ref, blocks, want.data(), 3, &blocks) != 0) return 3;

    // sizes first (no room at all), then exact-size buffers
    std::vector<avcer_jpeg_desc> desc((size_t)n);
    avcer_jpeg_scan* scan = (avcer_jpeg_scan*)malloc(sizeof(avcer_jpeg_scan) * (size_t)n);
    int32_t n_tabs = 0;
    int64_t need_bytes = 0, need_blocks = 0;
    if (avcer_jpeg_scan_batch(nullptr, files.data(), lens.data(), n, nullptr, 0, desc.data(), scan, nullptr, 0, 2, &n_tabs, &need_bytes, &need_blocks) != 0)
        return 4;
    if (need_blocks != blocks || n_tabs <= 0 || need_bytes <= 0) return 4;
    const int tabs_all = n_tabs;
    const int64_t bytes_all = need_bytes;
    int checked = 0;
    for (int threads : {1, 3, 16})
        for (int sub_bits : {128, 0, 4096}) {
            uint8_t* data = (uint8_t*)malloc((size_t)bytes_all);
            avcer_jpeg_tab* tabs = (avcer_jpeg_tab*)malloc(sizeof(avcer_jpeg_tab) * (size_t)tabs_all);
            if (avcer_jpeg_scan_batch(nullptr, files.data(), lens.data(), n, data, bytes_all, desc.data(), scan, tabs, tabs_all, threads, &n_tabs,
                                      &need_bytes, &need_blocks) != 0)
                return 5;
            if (n_tabs != tabs_all || need_bytes != bytes_all) return 5;
            int16_t* coeffs = (int16_t*)malloc((size_t)blocks * 128);
            int32_t* status = (int32_t*)malloc(4 * (size_t)n);
            if (avcer_jpeg_unpack_host(nullptr, data, bytes_all, scan, tabs, tabs_all, desc.data(), n, coeffs, blocks, status, sub_bits) != 0) return 6;
            for (int i = 0; i < n; ++i) {
                if (desc[i].status != want[i].status || status[i] != want[i].status || desc[i].reason != want[i].reason) {
                    fprintf(stderr, "file %d: status %d reason %d, the host pass says %d / %d\n", i, desc[i].status, desc[i].reason, want[i].status,
                            want[i].reason);
                    return 7;
                }
                if (want[i].status == AVCER_JPEG_OK &&
                    (desc[i].coef_block != want[i].coef_block ||
                     memcmp(coeffs + 64 * desc[i].coef_block, ref + 64 * want[i].coef_block, 128 * (size_t)want[i].n_blocks) != 0))
                    return 8;
                ++checked;
            }
            free(status);
            free(coeffs);
            free(tabs);
            free(data);
        }
    // short capacities: bytes from nothing to one short, tables one short; what fits is decoded
    int short_runs = 0;
    for (int64_t cap : {(int64_t)0, (int64_t)15, (int64_t)16, bytes_all / 3, bytes_all / 2, bytes_all - 1})
        for (int cap_tabs : {tabs_all, tabs_all - 1}) {
            uint8_t* data = (uint8_t*)malloc(cap ? (size_t)cap : 1);
            avcer_jpeg_tab* tabs = (avcer_jpeg_tab*)malloc(sizeof(avcer_jpeg_tab) * (size_t)(cap_tabs ? cap_tabs : 1));
            if (avcer_jpeg_scan_batch(nullptr, files.data(), lens.data(), n, cap ? data : nullptr, cap, desc.data(), scan, cap_tabs ? tabs : nullptr, cap_tabs,
                                      3, &n_tabs, &need_bytes, &need_blocks) != 0)
                return 9;
            int refused = 0, kept = 0;
            int64_t used_blocks = 0, used_bytes = 0;
            for (int i = 0; i < n; ++i) {
                refused += desc[i].status != AVCER_JPEG_OK && desc[i].reason == 12;
                if (desc[i].status == AVCER_JPEG_OK) {
                    ++kept;
                    used_blocks = desc[i].coef_block + desc[i].n_blocks;
                    used_bytes = scan[i].offset + scan[i].nbytes;
                }
            }
            if (need_bytes != bytes_all || n_tabs != tabs_all || refused == 0 || used_bytes > cap) return 10;
            if (kept && cap_tabs) {
                int16_t* coeffs = (int16_t*)malloc((size_t)used_blocks * 128);
                int32_t* status = (int32_t*)malloc(4 * (size_t)n);
                if (avcer_jpeg_unpack_host(nullptr, data, used_bytes, scan, tabs, cap_tabs, desc.data(), n, coeffs, used_blocks, status, 128) != 0) return 11;
                free(status);
                free(coeffs);
            }
            free(tabs);
            free(data);
            ++short_runs;
        }
    free(scan);
    free(ref);
    for (auto p : files) free(p);
    printf("jpeg_unpack_asan: %d files, %lld bytes of scan, %d tables, %d comparisons, %d short buffers: clean\n", n, (long long)bytes_all, tabs_all,
           checked, short_runs);
    return 0;
}
