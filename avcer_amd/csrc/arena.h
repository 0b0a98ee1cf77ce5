// Bump allocation of 256-byte aligned regions out of one device allocation, written so that the size of the allocation follows
// from its layout: a carving (a function of Arena&) runs once on a MEASURING arena, which has no base, hands out null and only
// advances -- `bytes = Arena().run(carve)` --, and once on an arena BOUND to the allocation made from the measured size, where
// it must end exactly at that size: `Arena(p, bytes).run(carve) == bytes`.  Nothing of HIP in here: host C++ only.
#pragma once

#include <cstddef>
#include <cstdint>

struct Arena {
    char* base;  // null: measuring
    size_t cap, off = 0;
    explicit Arena(void* p = nullptr, size_t c = SIZE_MAX) : base((char*)p), cap(c) {}
    // the next region of `bytes` bytes; null when measuring or when the region ends behind `cap`
    template <class T = void>
    T* get(size_t bytes) {
        off = (off + 255) & ~(size_t)255;
        const size_t at = off;
        off += bytes;
        return base && off <= cap ? (T*)((uintptr_t)base + at) : nullptr;
    }
    // where `carve` ends on this arena
    template <class Carve>
    size_t run(const Carve& carve) {
        carve(*this);
        return off;
    }
};
