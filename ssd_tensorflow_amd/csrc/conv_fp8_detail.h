// What the e4m3 kernels of conv_fp8.hip and conv_mxfp8.hip share: operand types, the tile row constants, the clamped converts
// and the wait in front of a pipeline stage.
#pragma once
#include "conv_detail.h"

namespace ssd {

typedef int i32x8 __attribute__((ext_vector_type(8)));
#define LDS_PTR8(p) ((__attribute__((address_space(3))) void*)(p))

constexpr int KB8 = 64;                 // k per pipeline iteration = bytes per tile row
constexpr unsigned OOB8 = 0xFFFFFFF0u;  // offset no buffer covers: the DMA writes zeros (code 0 = +0)
constexpr int SCALE_ONE = 0x7F7F7F7F;   // E8M0 block scale 127 = 2^0 in every byte

// four floats -> four e4m3 codes in one dword, clamped in fp32 first (the convert's own overflow behaviour is not relied on)
__device__ __forceinline__ float clamp448(float v) { return fminf(fmaxf(v, -448.f), 448.f); }
__device__ __forceinline__ unsigned pack4_e4m3(float a, float b, float c, float d) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp448(a), clamp448(b), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp448(c), clamp448(d), w, true);
    return (unsigned)w;
}
__device__ __forceinline__ unsigned char to_e4m3(float v) {
    return (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(clamp448(v), 0.f, 0, false) & 0xFF);
}

// conv_bf16.hip wait_tiles_and_sync: all but the `ahead` most recent tiles of this lane's DMA have landed, then the barrier
template <int L, int MAXA>
__device__ __forceinline__ void wait_tiles_and_sync8(int ahead) {
    static_assert(MAXA * L <= 63, "vmcnt field");
    if constexpr (MAXA >= 4) {
        if (ahead >= 4) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * L) : "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            return;
        }
    }
    if constexpr (MAXA >= 3) {
        if (ahead == 3) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * L) : "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            return;
        }
    }
    if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * L) : "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

}  // namespace ssd
