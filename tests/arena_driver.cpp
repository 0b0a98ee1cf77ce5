// Host-only driver of avcer_amd/csrc/arena.h for tests/test_arena.py: one carving of mixed sizes, measured and then bound to a
// base address that is never dereferenced.  Prints what the test asserts on; decides nothing itself.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "arena.h"

int main() {
    const std::vector<size_t> sizes = {0, 1, 255, 256, 257, ((size_t)5 << 30) + 3, 1, 0, 4096};
    std::vector<void*> got(sizes.size());
    auto carve = [&](Arena& ar) {
        for (size_t i = 0; i < sizes.size(); ++i) got[i] = ar.get(sizes[i]);
    };
    const size_t measured = Arena().run(carve);
    bool measuring_null = true;
    for (void* p : got) measuring_null = measuring_null && p == nullptr;
    printf("measured %zu\nmeasuring_null %d\n", measured, (int)measuring_null);

    void* base = (void*)(uintptr_t)0x7f0000000000ull;
    Arena bound(base, measured);
    carve(bound);
    printf("base %" PRIuPTR "\nbound_end %zu\n", (uintptr_t)base, bound.off);
    for (size_t i = 0; i < sizes.size(); ++i) printf("region %" PRIuPTR " %zu\n", (uintptr_t)got[i], sizes[i]);
    printf("end_exact %zu\n", Arena(base, measured).run(carve));

    printf("end_short %zu\n", Arena(base, measured - 1).run(carve));
    printf("short_last %" PRIuPTR "\n", (uintptr_t)got.back());
    return 0;
}
