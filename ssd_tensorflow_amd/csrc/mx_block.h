// The two MX code formats (e4m3: DESIGN.md 20, e2m3: DESIGN.md 24) as traits, and what is written once over them: the scale rule, the
// stand-alone quantiser and max-pooling.  A block is 32 consecutive channels under one E8M0 byte; on the device it
// belongs to 4 adjacent lanes ("quarters" q = 0 ... 3) that hold 8 values each.  The kernels and their host functions are `static`
// templates, instantiated by the file of each format (conv_mxfp8.hip, conv_mxfp6.hip), the pattern of conv_fp8_detail.h.
#pragma once
#include "bf16.h"
#include "ops.h"
#include <algorithm>

namespace ssd {

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

// A format F: the scale rule's two constants -- x = E - BIAS + (mantissa bits > ROUND_UP), the smallest power of two with absmax /
// 2^x <= the clamp (448 = 1.75 * 2^8, 7.5 = 1.875 * 2^2) -- the bytes of a block, a thread's 8 codes as a register type, and:
//   dec(c, e)        the value of code e of a thread's 8, by the format's definition (exact)
//   pack8(v, x)      a thread's 8 values at block exponent x -> its 8 codes
//   store8(y, blk, q, c) / load8(x, blk, q)   a thread's 8 codes of block blk of a tensor, quarter q
// (The clamp is each format's own: e4m3 clamps the signed value in front of the convert, e2m3 the magnitude inside enc.)
struct MxE4M3 {      // OCP e4m3fn, one byte per code
    static constexpr int BLOCK_BYTES = 32, BIAS = 8;
    static constexpr unsigned ROUND_UP = 0x600000u;
    typedef u32x2 Codes8;
    static __device__ __forceinline__ float clamp(float v) { return clamp448(v); }
    // (the NaN codes read as 480: outside the contract)
    static __device__ __forceinline__ float dec(Codes8 w, int i) {
        const unsigned c = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        const unsigned e = (c >> 3) & 15u, m = c & 7u;
        const float a = e ? __uint_as_float(((e + 120u) << 23) | (m << 20)) : (float)m * 0.001953125f;
        return (c & 0x80u) ? -a : a;
    }
    static __device__ __forceinline__ Codes8 pack8(const float (&v)[8], int x) {
        return u32x2{pack4_e4m3(ldexpf(v[0], -x), ldexpf(v[1], -x), ldexpf(v[2], -x), ldexpf(v[3], -x)),
                     pack4_e4m3(ldexpf(v[4], -x), ldexpf(v[5], -x), ldexpf(v[6], -x), ldexpf(v[7], -x))};
    }
    // (a block's 32 bytes are its channels' bytes: 8-byte group 4 blk + q of the tensor)
    static __device__ __forceinline__ void store8(unsigned char* y, size_t blk, int q, Codes8 mine) { *reinterpret_cast<u32x2*>(y + (blk * 4 + q) * 8) = mine; }
    static __device__ __forceinline__ Codes8 load8(const unsigned char* x, size_t blk, int q) { return *reinterpret_cast<const u32x2*>(x + (blk * 4 + q) * 8); }
};

struct MxE2M3 {      // OCP MX FP6 E2M3: code j of a block in bits 6 j ... 6 j + 5 of a little-endian 24-byte string
    static constexpr int BLOCK_BYTES = 24, BIAS = 2;
    static constexpr unsigned ROUND_UP = 0x700000u;
    typedef unsigned long long Codes8;      // 48 bits, value e in bits 6 e ... 6 e + 5
    static __device__ __forceinline__ float clamp_abs(float v) { return fminf(fabsf(v), 7.5f); }
    // one value -> its code in plain arithmetic: clamp to 7.5, round to nearest even on the grid (step 1/8 below 2, 1/4 below 4, 1/2
    // above; the subnormals share the first binade's step), the sign bit is the input's.  (tools/probes/mxfp6_probe.hip reports what
    // v_cvt_scalef32_2xpk16_fp6_f32 does; nothing here depends on it.)
    static __device__ __forceinline__ unsigned enc(float v) {
        const float a = clamp_abs(v);
        const unsigned c = a < 2.f ? (unsigned)rintf(a * 8.f) : a < 4.f ? 8u + (unsigned)rintf(a * 4.f) : 16u + (unsigned)rintf(a * 2.f);
        return c | ((__float_as_uint(v) >> 31) << 5);
    }
    static __device__ __forceinline__ float dec(Codes8 w, int i) {
        const unsigned c = (unsigned)(w >> (6 * i)) & 63u;
        const unsigned e = (c >> 3) & 3u, m = c & 7u;
        const float a = e ? __uint_as_float(((e + 126u) << 23) | (m << 20)) : (float)m * 0.125f;
        return (c & 32u) ? -a : a;
    }
    static __device__ __forceinline__ Codes8 pack8(const float (&v)[8], int x) {
        unsigned long long w = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) w |= (unsigned long long)enc(ldexpf(v[e], -x)) << (6 * e);
        return w;
    }
    // The block's four lanes q = 0 ... 3 (adjacent, all active) hold 48 bits each; the 24-byte string is written by lanes 0 ... 2 as three
    // 8-byte stores: lane q's store is bits 64 q ... 64 q + 63 = its own bits from 16 q on and the next lane's first 16 (q + 1) bits.
    static __device__ __forceinline__ void store8(unsigned char* y, size_t blk, int q, Codes8 mine) {
        const unsigned nlo = (unsigned)__shfl_down((int)(unsigned)mine, 1, 64), nhi = (unsigned)__shfl_down((int)(unsigned)(mine >> 32), 1, 64);
        const unsigned long long next = ((unsigned long long)nhi << 32) | nlo;
        if (q < 3) {
            const unsigned long long out = (mine >> (16 * q)) | (next << (48 - 16 * q));
            *reinterpret_cast<u32x2*>(y + blk * 24 + 8 * q) = u32x2{(unsigned)out, (unsigned)(out >> 32)};
        }
    }
    // (48 bits of the string, read as three 16-bit words)
    static __device__ __forceinline__ Codes8 load8(const unsigned char* x, size_t blk, int q) {
        const unsigned short* h = reinterpret_cast<const unsigned short*>(x + blk * 24 + 6 * q);
        return (unsigned long long)h[0] | ((unsigned long long)h[1] << 16) | ((unsigned long long)h[2] << 32);
    }
};

// the MX scale rule: fp32 absmax (>= 0) -> x in -127 ... 127.  Non-finite input gives 120 / 121 (e4m3): no byte 255, no fault
template <typename F>
__device__ __forceinline__ int mx_exponent(float amax) {
    const unsigned u = __float_as_uint(amax);
    const int x = (int)(u >> 23) - 127 - F::BIAS + ((u & 0x7FFFFFu) > F::ROUND_UP ? 1 : 0);
    return x < -127 ? -127 : x > 127 ? 127 : x;
}
// a thread's 8 values of a 32-channel block held by 4 adjacent lanes -> the block's exponent; every lane of the four gets it
template <typename F>
__device__ __forceinline__ int mx_block_exponent(const float (&v)[8]) {
    float am = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf(v[e]));
    am = fmaxf(am, __shfl_xor(am, 1, 64));
    am = fmaxf(am, __shfl_xor(am, 2, 64));
    return mx_exponent<F>(am);
}
// ... and the block quantised and written: quarter q's 8 values `v` of block `blk` of the tensor (codes y, scales ys)
template <typename F>
__device__ __forceinline__ void mx_quantize_store(const float (&v)[8], unsigned char* y, unsigned char* ys, size_t blk, int q) {
    const int x = mx_block_exponent<F>(v);
    F::store8(y, blk, q, F::pack8(v, x));
    if (q == 0) ys[blk] = (unsigned char)(x + 127);
}

// values 8 i ... 8 i + 7 of x as floats: one 16-byte (bf16) or two 16-byte (fp32) loads
template <typename T>
__device__ __forceinline__ void load8(const T* x, size_t i, float (&v)[8]) {
    if constexpr (sizeof(T) == 2) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(x + i * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[2 * e] = lo2f(w[e]);
            v[2 * e + 1] = hi2f(w[e]);
        }
    } else {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + i * 8), b = *reinterpret_cast<const f32x4*>(x + i * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = a[e];
            v[4 + e] = b[e];
        }
    }
}

// blocks of a grid-stride kernel: enough for `items`, at most 32 per CU
inline int grid8(size_t items, int per_block) {
    const size_t g = (items + per_block - 1) / per_block;
    return (int)std::min<size_t>(std::max<size_t>(g, 1), 256 * 32);
}

// =================================================================================
// stand-alone quantiser: bf16 or fp32 [rows][C] -> codes + scales.  8 values per thread, a block = 4 adjacent lanes.
// =================================================================================
template <typename F, typename T>
__global__ __launch_bounds__(256) void quantize_mx_kernel(const T* __restrict__ x, unsigned char* __restrict__ y, unsigned char* __restrict__ ys,
                                                          size_t n8) {
    const size_t stride = (size_t)gridDim.x * 256;      // (n8 and the stride are multiples of 4: a block's lanes loop together)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        float v[8];
        load8(x, i, v);
        mx_quantize_store<F>(v, y, ys, i >> 2, (int)(i & 3));
    }
}

// `who`: the entry point, for the messages and as the profile label
template <typename F>
static void quantize_mx(const char* who, const void* x, bool x_f32, size_t rows, int C, unsigned char* y, unsigned char* ys, hipStream_t s) {
    SSD_REQUIRE(x && y && ys, "%s: null argument", who);
    SSD_REQUIRE(C > 0 && C % 32 == 0, "%s: C must be a multiple of 32 (got %d)", who, C);
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(y) % 8 == 0, "%s: unaligned tensor", who);
    if (rows == 0) return;
    const size_t n8 = rows * (size_t)C / 8;
    ProfScope prof(who, 0.0, ((x_f32 ? 4.0 : 2.0) + F::BLOCK_BYTES / 32.0 + 1.0 / 32) * (double)n8 * 8, s);
    if (x_f32) hipLaunchKernelGGL((quantize_mx_kernel<F, float>), dim3(grid8(n8, 256)), dim3(256), 0, s, (const float*)x, y, ys, n8);
    else hipLaunchKernelGGL((quantize_mx_kernel<F, bf16_t>), dim3(grid8(n8, 256)), dim3(256), 0, s, (const bf16_t*)x, y, ys, n8);
    HIP_OK(hipGetLastError());
}

// =================================================================================
// max-pooling.  The cells of a window carry different scales, so the byte order of maxpool_fwd_fp8 says nothing: per output pixel and
// block the window's cells are dequantised (exact in fp32), the maximum is taken per channel -- cells outside the image never win (TF
// SAME) -- and the block is quantised again by the scale rule: one more rounding.  8 channels per thread, a block = 4 adjacent lanes.
// =================================================================================
template <typename F>
__global__ __launch_bounds__(256) void maxpool_fwd_mx_kernel(PoolDesc d, const unsigned char* __restrict__ x, const unsigned char* __restrict__ xs,
                                                             unsigned char* __restrict__ y, unsigned char* __restrict__ ys) {
    const int c8 = d.C / 8, cb = d.C / 32;
    const size_t total = (size_t)d.B * d.Ho * d.Wo * c8;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
        const int cq = (int)(idx % c8);
        size_t t = idx / c8;
        const int ow = (int)(t % d.Wo);
        t /= d.Wo;
        const int oh = (int)(t % d.Ho);
        const int b = (int)(t / d.Ho);
        float best[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) best[e] = -INFINITY;
        for (int kh = 0; kh < d.k; ++kh) {
            const int ih = oh * d.stride - d.pad_h + kh;
            if ((unsigned)ih >= (unsigned)d.Hi) continue;
            for (int kw = 0; kw < d.k; ++kw) {
                const int iw = ow * d.stride - d.pad_w + kw;
                if ((unsigned)iw >= (unsigned)d.Wi) continue;
                const size_t blk = (((size_t)b * d.Hi + ih) * d.Wi + iw) * cb + (cq >> 2);
                const typename F::Codes8 c = F::load8(x, blk, cq & 3);
                const int ex = (int)xs[blk] - 127;
#pragma unroll
                for (int e = 0; e < 8; ++e) best[e] = fmaxf(best[e], ldexpf(F::dec(c, e), ex));
            }
        }
        mx_quantize_store<F>(best, y, ys, idx >> 2, cq & 3);
    }
}

// what the quantised pools ask of a geometry
inline void require_pool_geometry(const char* who, const PoolDesc& d) {
    SSD_REQUIRE(d.k >= 1 && d.stride >= 1 && d.B > 0 && d.Ho > 0 && d.Wo > 0, "%s: bad geometry", who);
    // every window must hold at least one cell of the image
    SSD_REQUIRE((d.Ho - 1) * d.stride - d.pad_h < d.Hi && (d.Wo - 1) * d.stride - d.pad_w < d.Wi && d.pad_h < d.k && d.pad_w < d.k,
                "%s: a window lies outside the image", who);
}

template <typename F>
static void maxpool_fwd_mx(const char* who, const PoolDesc& d, const unsigned char* x, const unsigned char* xs, unsigned char* y, unsigned char* ys,
                           hipStream_t s) {
    SSD_REQUIRE(x && xs && y && ys, "%s: null argument", who);
    SSD_REQUIRE(d.C % 32 == 0 && d.C > 0, "%s: C must be a multiple of 32 (got %d)", who, d.C);
    require_pool_geometry(who, d);
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(x) % 8 == 0 && reinterpret_cast<uintptr_t>(y) % 8 == 0, "%s: unaligned tensor", who);
    const size_t total = (size_t)d.B * d.Ho * d.Wo * (d.C / 8);
    ProfScope prof(who, 0.0, (F::BLOCK_BYTES / 32.0 + 1.0 / 32) * d.C * d.B * ((double)d.Hi * d.Wi + (double)d.Ho * d.Wo), s);
    hipLaunchKernelGGL(maxpool_fwd_mx_kernel<F>, dim3(grid8(total, 256)), dim3(256), 0, s, d, x, xs, y, ys);
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
