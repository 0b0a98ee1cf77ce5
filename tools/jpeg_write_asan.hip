// Host sanitiser check of the JPEG writer: a stand-alone program around the host code of csrc/jpeg_encode.hip (avcer_jpeg_plan,
// avcer_jpeg_write_batch), built with AddressSanitizer and UBSan on the HOST side only and run on a CPU machine:
//   python tools/jpeg_write_asan.py      (writes the input with jpeg.forward_numpy, compiles this file, runs it)
// Input file: i32 n, quality, subsampling; i32 [n,2] sizes (w, h); i64 count; i16 [count] coefficients; i64 bytes; u8 [bytes] the
// files PIL wrote, back to back.  The output buffers are heap blocks of EXACTLY the size given to the writer, so one byte past
// cap_bytes is a report.  No device is touched: ctx is NULL and no kernel is launched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/avcer_hip.h"

// what csrc/api.hip gives the library; this program links jpeg_encode.hip and, for the launchers it calls, jpeg_decode.hip alone
struct avcer_ctx;
int set_err(avcer_ctx*, int code, const char*, ...) { return code; }
int ws_reserve(avcer_ctx*, int, size_t, void**) { return -1; }

static bool get(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[3];
    int64_t count = 0, bytes = 0;
    if (!get(f, head, sizeof(head))) return 2;
    const int n = head[0];
    std::vector<int32_t> sizes(2 * (size_t)n);
    if (!get(f, sizes.data(), sizes.size() * 4) || !get(f, &count, 8)) return 2;
    int16_t* coeffs = (int16_t*)malloc((size_t)count * 2);  // exact: a read past the last block is a report too
    if (!get(f, coeffs, (size_t)count * 2) || !get(f, &bytes, 8)) return 2;
    std::vector<uint8_t> want((size_t)bytes);
    if (!get(f, want.data(), want.size())) return 2;
    fclose(f);

    std::vector<avcer_jpeg_desc> desc((size_t)n), plan;
    int64_t blocks = 0, need = 0;
    if (avcer_jpeg_plan(sizes.data(), n, head[2], head[1], desc.data(), &blocks) != 0 || blocks * 64 != count) return 3;
    plan = desc;
    std::vector<int64_t> offsets((size_t)n + 1);
    for (int threads : {1, 3, 16}) {
        desc = plan;
        uint8_t* out = (uint8_t*)malloc((size_t)bytes);
        if (avcer_jpeg_write_batch(nullptr, coeffs, desc.data(), n, out, bytes, offsets.data(), threads, &need) != 0) return 4;
        if (need != bytes || offsets[n] != bytes || memcmp(out, want.data(), (size_t)bytes) != 0) return 5;
        free(out);
    }
    // short buffers: every capacity class from nothing to one byte short
    for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)622, (int64_t)623, bytes / 3, bytes / 2, bytes - 1}) {
        desc = plan;
        uint8_t* out = (uint8_t*)malloc((size_t)cap ? (size_t)cap : 1);
        if (avcer_jpeg_write_batch(nullptr, coeffs, desc.data(), n, cap ? out : nullptr, cap, offsets.data(), 3, &need) != 0) return 6;
        int refused = 0;
        for (int i = 0; i < n; ++i) refused += desc[i].status != AVCER_JPEG_OK && desc[i].reason == 12;
        if (need != bytes || offsets[n] > cap || refused == 0) return 7;
        free(out);
    }
    free(coeffs);
    printf("jpeg_write_asan: %d files, %lld bytes, 3 thread counts, 7 short buffers: clean\n", n, (long long)bytes);
    return 0;
}
