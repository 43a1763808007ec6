// mxfp8 inference kernels for gfx950 (MI355X): the forward gather convolution on e4m3 operands with the pixel operand's E8M0 block
// scales fed to v_mfma_scale_f32_32x32x64_f8f6f4 -- the kernel and its host path are conv_fp8_detail.h's, instantiated here with MX =
// true -- and the other producers of the format: a stand-alone quantiser and max-pooling.  DESIGN.md 20; more than 9 taps (the fc
// graph's 7 x 7 fc6): DESIGN.md 21.
//
// Format: an activation tensor is codes uint8 [B][H][W][C] (OCP e4m3fn) + scales uint8 [B][H][W][C / 32] (E8M0, byte e = 2^(e - 127)),
// one scale per pixel and 32 consecutive channels.  (The hardware's scale byte of lane l does NOT cover that lane's own 32 consecutive
// k: tools/probes/mxfp8_probe.hip pins what it covers, and the kernel assigns channels to lanes accordingly.)  Scale rule on the bits
// of the block's fp32 absmax a (E = unbiased exponent, m = mantissa bits): x = clamp(E - 8 + (m > 0x600000), -127, 127), the smallest
// power of two with a / 2^x <= 448 = 1.75 * 2^8; byte x + 127 (an all-zero block: byte 0, what a padded tap's zero fill also holds);
// codes = RNE(clamp(ldexp(v, -x), -448, 448)).  Filters stay as in conv_fp8.hip: e4m3 [tap][Co][Ci], one fp32 scale per output
// channel, block scale 2^0.  Epilogue: y = relu?(acc * s_w[co] + bias[co]) in fp32.
#include "conv.h"
#include "conv_detail.h"
#include "conv_fp8_detail.h"
#include "bf16.h"
#include "ops.h"
#include <algorithm>

namespace ssd {

// a code's value, by the format's definition (exact; the NaN codes read as 480: outside the contract)
__device__ __forceinline__ float dec_e4m3(unsigned c) {
    const unsigned e = (c >> 3) & 15u, m = c & 7u;
    const float a = e ? __uint_as_float(((e + 120u) << 23) | (m << 20)) : (float)m * 0.001953125f;
    return (c & 0x80u) ? -a : a;
}

bool conv_bigk_fwd_mxfp8_supported(const ConvDesc& d, int out_mode, const char** why) {
    const char* w = conv_e4m3_refusal(true, true, d, out_mode);
    if (why) *why = w;
    return w == nullptr;
}

// Where an mxfp8 handle uses the kernel for more than 9 taps: SSD_MXFP8_BIGK (read per handle) = 1 takes every supported layer with at
// least 256 input channels (the fc graph's mod_conv6); 0 or unset leaves it on conv_bigk_fwd_bf16 with a quantise pass behind it
// (DESIGN.md 21).  Up to 9 taps an mxfp8 handle follows conv_fwd_fp8_supported and conv_fwd_fp8_worthwhile.
constexpr int MXFP8_BIGK_DEFAULT = 0;
bool conv_bigk_fwd_mxfp8_worthwhile(const ConvDesc& d) { return d.Ci >= 256 && env_int("SSD_MXFP8_BIGK", MXFP8_BIGK_DEFAULT) == 1; }

static void run_mxfp8(bool bigk, const ConvDesc& d, const unsigned char* x8, const unsigned char* xs, const unsigned char* w8, const float* s_w,
                      const float* bias, void* y, unsigned char* y8, unsigned char* ys, int out_mode, bool relu, hipStream_t s) {
    GatherArgs8 a{};
    a.src = x8; a.src_sc = xs; a.wgt = w8; a.bias = bias; a.s_w = s_w; a.dst = y; a.dst8 = y8; a.dst_sc = ys;
    conv_fwd_e4m3<true>(bigk, d, a, out_mode, relu, s);
}
void conv_fwd_mxfp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* xs, const unsigned char* w8, const float* s_w,
                    const float* bias, void* y, unsigned char* y8, unsigned char* ys, int out_mode, bool relu, hipStream_t s) {
    run_mxfp8(false, d, x8, xs, w8, s_w, bias, y, y8, ys, out_mode, relu, s);
}
void conv_bigk_fwd_mxfp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* xs, const unsigned char* w8, const float* s_w,
                         const float* bias, void* y, unsigned char* y8, unsigned char* ys, int out_mode, bool relu, hipStream_t s) {
    run_mxfp8(true, d, x8, xs, w8, s_w, bias, y, y8, ys, out_mode, relu, s);
}

// =================================================================================
// stand-alone quantiser: bf16 or fp32 [rows][C] -> codes + scales.  8 values per thread, a block = 4 adjacent lanes.
// =================================================================================
template <typename T>
__global__ __launch_bounds__(256) void quantize_mxfp8_kernel(const T* __restrict__ x, unsigned char* __restrict__ y, unsigned char* __restrict__ ys,
                                                             size_t n8) {
    const size_t stride = (size_t)gridDim.x * 256;      // (n8 and the stride are multiples of 4: a block's lanes loop together)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        float v[8];
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
        const int ex = mx_block_exponent(v);
        *reinterpret_cast<u32x2*>(y + i * 8) = mx_pack8(v, ex);
        if ((i & 3) == 0) ys[i >> 2] = (unsigned char)(ex + 127);
    }
}

void quantize_mxfp8(const void* x, bool x_f32, size_t rows, int C, unsigned char* y8, unsigned char* ys, hipStream_t s) {
    SSD_REQUIRE(x && y8 && ys, "quantize_mxfp8: null argument");
    SSD_REQUIRE(C > 0 && C % 32 == 0, "quantize_mxfp8: C must be a multiple of 32 (got %d)", C);
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(y8) % 8 == 0, "quantize_mxfp8: unaligned tensor");
    if (rows == 0) return;
    const size_t n8 = rows * (size_t)C / 8;
    ProfScope prof("quantize_mxfp8", 0.0, ((x_f32 ? 5.0 : 3.0) + 1.0 / 32) * (double)n8 * 8, s);
    if (x_f32) hipLaunchKernelGGL(quantize_mxfp8_kernel<float>, dim3(grid8(n8, 256)), dim3(256), 0, s, (const float*)x, y8, ys, n8);
    else hipLaunchKernelGGL(quantize_mxfp8_kernel<bf16_t>, dim3(grid8(n8, 256)), dim3(256), 0, s, (const bf16_t*)x, y8, ys, n8);
    HIP_OK(hipGetLastError());
}

// =================================================================================
// max-pooling.  The cells of a window carry different scales, so the byte order of maxpool_fwd_fp8 says nothing: per output pixel and
// block the window's cells are dequantised (exact in fp32), the maximum is taken per channel -- cells outside the image never win (TF
// SAME) -- and the block is quantised again by the scale rule: one more rounding.  8 channels per thread, a block = 4 adjacent lanes.
// =================================================================================
__global__ __launch_bounds__(256) void maxpool_fwd_mxfp8_kernel(PoolDesc d, const unsigned char* __restrict__ x, const unsigned char* __restrict__ xs,
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
                const size_t pix = ((size_t)b * d.Hi + ih) * d.Wi + iw;
                const u32x2 c = *reinterpret_cast<const u32x2*>(x + pix * d.C + (size_t)cq * 8);
                const int ex = (int)xs[pix * cb + (cq >> 2)] - 127;
#pragma unroll
                for (int e = 0; e < 8; ++e) best[e] = fmaxf(best[e], ldexpf(dec_e4m3((c[e >> 2] >> (8 * (e & 3))) & 0xFFu), ex));
            }
        }
        const int ex = mx_block_exponent(best);
        *reinterpret_cast<u32x2*>(y + idx * 8) = mx_pack8(best, ex);
        if ((cq & 3) == 0) ys[idx >> 2] = (unsigned char)(ex + 127);
    }
}

void maxpool_fwd_mxfp8(const PoolDesc& d, const unsigned char* x8, const unsigned char* xs, unsigned char* y8, unsigned char* ys, hipStream_t s) {
    SSD_REQUIRE(x8 && xs && y8 && ys, "maxpool_fwd_mxfp8: null argument");
    SSD_REQUIRE(d.C % 32 == 0 && d.C > 0, "maxpool_fwd_mxfp8: C must be a multiple of 32 (got %d)", d.C);
    SSD_REQUIRE(d.k >= 1 && d.stride >= 1 && d.B > 0 && d.Ho > 0 && d.Wo > 0, "maxpool_fwd_mxfp8: bad geometry");
    // every window must hold at least one cell of the image
    SSD_REQUIRE((d.Ho - 1) * d.stride - d.pad_h < d.Hi && (d.Wo - 1) * d.stride - d.pad_w < d.Wi && d.pad_h < d.k && d.pad_w < d.k,
                "maxpool_fwd_mxfp8: a window lies outside the image");
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(x8) % 8 == 0 && reinterpret_cast<uintptr_t>(y8) % 8 == 0, "maxpool_fwd_mxfp8: unaligned tensor");
    const size_t total = (size_t)d.B * d.Ho * d.Wo * (d.C / 8);
    ProfScope prof("maxpool_fwd_mxfp8", 0.0, (1.0 + 1.0 / 32) * d.C * d.B * ((double)d.Hi * d.Wi + (double)d.Ho * d.Wo), s);
    hipLaunchKernelGGL(maxpool_fwd_mxfp8_kernel, dim3(grid8(total, 256)), dim3(256), 0, s, d, x8, xs, y8, ys);
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
