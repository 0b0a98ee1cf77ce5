// What the whole-head attention kernels (kernels.hip) and the streaming ones (attention_long.hip) share: the MFMA operand types of
// the two 16-bit arithmetic forms, the K image's LDS swizzle and the launchers' one-time LDS attribute.
#pragma once

#include "act_io.h"

typedef __attribute__((ext_vector_type(8))) __bf16 att_bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float att_f32x4_t;
// operand element by arithmetic: the split type (fp16) in the x3 form, bf16 in the plain form
template <int X3> struct AttOp {
    typedef spe_t elem_t;
    typedef spx8_t frag_t;
    static __device__ __forceinline__ att_f32x4_t mfma(const frag_t a, const frag_t b, const att_f32x4_t c) { return mfma_sp(a, b, c); }
};
template <> struct AttOp<0> {
    typedef __bf16 elem_t;
    typedef att_bf16x8_t frag_t;
    static __device__ __forceinline__ uint16_t bits(float f) { return f2bf(f); }
    static __device__ __forceinline__ att_f32x4_t mfma(const frag_t a, const frag_t b, const att_f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

__device__ __forceinline__ int att_swz(int row, int chunk) {
    return row * 128 + ((chunk ^ (int)((0x32765410u >> (((row >> 1) & 7) * 4)) & 7u)) << 4);
}

namespace {
// More than 64 KiB of dynamic LDS is an attribute of the kernel PER DEVICE: raised to the chip's 160 KiB before KERNEL's first
// launch on the context's device (one bit per device index)
template <auto KERNEL>
int big_lds_once(avcer_ctx* ctx) {
    static uint64_t done = 0;
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (!(done & bit)) {
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        done |= bit;
    }
    return AVCER_OK;
}
}  // namespace
