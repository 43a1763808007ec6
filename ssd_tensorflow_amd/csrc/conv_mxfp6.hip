// mxfp6 inference kernels for gfx950 (MI355X): the forward gather convolution on e2m3 operands with E8M0 block scales on both operands
// of v_mfma_scale_f32_32x32x64_f8f6f4 (conv_mxfp6_detail.h), and the other producers of the format: a stand-alone quantiser, the filter
// quantiser and max-pooling.  DESIGN.md 24.
//
// Format: OCP MX FP6 E2M3 (1 sign, 2 exponent bits of bias 1, 3 mantissa bits; magnitudes 0, 0.125 ... 0.875, 1 ... 1.875, 2 ... 3.75,
// 4 ... 7.5; no Inf / NaN).  32 consecutive channels share one E8M0 byte e = 2^(e - 127).  Scale rule on the bits of the block's fp32
// absmax a (E = unbiased exponent, m = mantissa bits): x = clamp(E - 2 + (m > 0x700000), -127, 127), the smallest power of two with
// a / 2^x <= 7.5; byte x + 127 (an all-zero block: byte 0, what a padded tap's zero fill also holds; byte 255 is never written);
// codes = RNE(clamp(ldexp(v, -x), -7.5, 7.5)).  Code j of a block sits in bits 6 j ... 6 j + 5 of a little-endian 24-byte string.
// Activations: codes [B][H][W][C / 32][24] + scales [B][H][W][C / 32].  Filters: blocks along Ci, w6 [tap][Co][Ci / 32][24] + wscales
// [tap][Co][Ci / 32], no per-channel scale.  Epilogue: y = relu?(acc + bias[co]) in fp32.
#include "conv.h"
#include "conv_detail.h"
#include "conv_mxfp6_detail.h"
#include "bf16.h"
#include "ops.h"
#include <algorithm>

namespace ssd {

bool conv_fwd_mxfp6_supported(const ConvDesc& d, const char** why) {
    const char* w = conv_quant_refusal(FMT_MXFP6, false, d, -1);
    if (why) *why = w;
    return w == nullptr;
}

// Tiles (gather_tile, the e4m3 kernel's rule): 128 x 128 runs five stages of 13 KB, 64 x 64 six stages of 9 KB.
void conv_fwd_mxfp6(const ConvDesc& d, const unsigned char* x6, const unsigned char* xs, const unsigned char* w6, const unsigned char* ws,
                    const float* bias, void* y, unsigned char* y6, unsigned char* ys, int out_mode, bool relu, hipStream_t s) {
    require_conv_quant(FMT_MXFP6, false, d, out_mode);
    const bool wants_mx = out_mode == FP8_OUT_MX || out_mode == FP8_OUT_BF16_MX;
    SSD_REQUIRE(!wants_mx || (y6 != nullptr && ys != nullptr), "mxfp6 conv: an MX output needs its code and scale buffers");
    SSD_REQUIRE(out_mode == FP8_OUT_MX || y != nullptr, "mxfp6 conv: null output");
    SSD_REQUIRE(x6 && xs && w6 && ws, "mxfp6 conv: null operand");
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(xs) % 2 == 0 && reinterpret_cast<uintptr_t>(ws) % 2 == 0, "mxfp6 conv: a scale buffer must start at an even address");
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(x6) % 8 == 0 && reinterpret_cast<uintptr_t>(w6) % 8 == 0 && (!wants_mx || reinterpret_cast<uintptr_t>(y6) % 8 == 0),
                "mxfp6 conv: a code buffer must start at a multiple of 8 bytes");
    GatherArgs6 a{};
    a.src = x6; a.wgt = w6; a.bias = bias; a.dst = y; a.dst8 = y6; a.dst_sc = ys;
    a.src_sc = dword_base(xs, a.sc_delta);
    a.wgt_sc = dword_base(ws, a.wsc_delta);
    gather_geometry(a, d, out_mode, relu);
    const double fl = conv_flops(d);
    const double code_b = 0.75 + 1.0 / 32;      // bytes per element: codes + scales
    const double out_b = out_mode == FP8_OUT_F32 ? 4.0 : out_mode == FP8_OUT_BF16 ? 2.0 : (out_mode == FP8_OUT_BF16_MX ? 2.0 : 0.0) + code_b;
    const double by = ((double)d.B * d.Hi * d.Wi * d.Ci + (double)d.KH * d.KW * d.Ci * d.Co) * code_b + (double)d.B * d.Ho * d.Wo * d.Co * out_b;
    if (gather_tile(a) == 0) launch_fwd_mxfp6<2, 2, 2, 2, 5>(a, "conv_fwd_mxfp6_128x128", fl, by, s);
    else launch_fwd_mxfp6<2, 2, 1, 1, 6>(a, "conv_fwd_mxfp6_64x64x6", fl, by, s);
}

// the stand-alone quantiser and max-pooling: mx_block.h's, on this format
void quantize_mxfp6(const void* x, bool x_f32, size_t rows, int C, unsigned char* y6, unsigned char* ys, hipStream_t s) {
    quantize_mx<MxE2M3>("quantize_mxfp6", x, x_f32, rows, C, y6, ys, s);
}
void maxpool_fwd_mxfp6(const PoolDesc& d, const unsigned char* x6, const unsigned char* xs, unsigned char* y6, unsigned char* ys, hipStream_t s) {
    maxpool_fwd_mx<MxE2M3>("maxpool_fwd_mxfp6", d, x6, xs, y6, ys, s);
}

// =================================================================================
// filter quantisation: fp32 [tap][Ci][Co] -> codes [tap][Co][Ci / 32][24] + scales [tap][Co][Ci / 32], all layers in one launch.  One
// thread per block of 32 input channels, output channel fastest: the 32 loads of a wave are rows of consecutive floats.
// =================================================================================
__global__ __launch_bounds__(256) void quantize_filters_mxfp6_kernel(QuantTable t, const float* __restrict__ w, unsigned char* __restrict__ w6,
                                                                    unsigned char* __restrict__ ws) {
    int s = 0;
    while (s + 1 < t.n && (int)blockIdx.x >= t.seg[s + 1].blk0) ++s;
    const QuantTable::Seg g = t.seg[s];
    const int cbn = g.ci / 32;
    const long long idx = (long long)((int)blockIdx.x - g.blk0) * 256 + threadIdx.x;
    if (idx >= (long long)g.taps * cbn * g.co) return;
    const int co = (int)(idx % g.co);
    const int t2 = (int)(idx / g.co);
    const int cb = t2 % cbn, tap = t2 / cbn;
    const float* src = w + g.off + ((size_t)tap * g.ci + (size_t)cb * 32) * g.co + co;
    float v[32];
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        v[j] = src[(size_t)j * g.co];
        am = fmaxf(am, fabsf(v[j]));
    }
    const int x = mx_exponent<MxE2M3>(am);
    const size_t blk = ((size_t)tap * g.co + co) * cbn + cb;
    unsigned long long q[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        q[h] = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) q[h] |= (unsigned long long)MxE2M3::enc(ldexpf(v[8 * h + e], -x)) << (6 * e);
    }
    const unsigned long long o0 = q[0] | (q[1] << 48), o1 = (q[1] >> 16) | (q[2] << 32), o2 = (q[2] >> 32) | (q[3] << 16);
    unsigned char* d = w6 + g.off8 + blk * 24;
    *reinterpret_cast<u32x2*>(d) = u32x2{(unsigned)o0, (unsigned)(o0 >> 32)};
    *reinterpret_cast<u32x2*>(d + 8) = u32x2{(unsigned)o1, (unsigned)(o1 >> 32)};
    *reinterpret_cast<u32x2*>(d + 16) = u32x2{(unsigned)o2, (unsigned)(o2 >> 32)};
    ws[g.offs + blk] = (unsigned char)(x + 127);
}

void quantize_filters_mxfp6(const FilterQuantPlan& plan, const float* w, unsigned char* w6, unsigned char* ws, hipStream_t s) {
    if (plan.n == 0) return;
    SSD_REQUIRE(w && w6 && ws, "quantize_filters_mxfp6: null argument");
    for (int i = 0; i < plan.n; ++i) {
        const FilterQuantPlan::Layer& L = plan.L[i];
        SSD_REQUIRE(L.taps >= 1 && L.co >= 1 && L.ci >= 32 && L.ci % 32 == 0, "quantize_filters_mxfp6: Ci must be a multiple of 32 (got %d)", L.ci);
        SSD_REQUIRE(reinterpret_cast<uintptr_t>(w6 + L.off8) % 8 == 0, "quantize_filters_mxfp6: a code image must start at a multiple of 8 bytes");
    }
    QuantTable t{};
    double elems;
    const int blk = fill_quant_table(
        t, plan, elems, [](const FilterQuantPlan::Layer&) { return true; },
        [](const FilterQuantPlan::Layer& L) { return cdiv((long long)L.taps * (L.ci / 32) * L.co, 256); });
    ProfScope prof("quantize_filters_mxfp6", 0.0, (4.75 + 1.0 / 32) * elems, s);
    hipLaunchKernelGGL(quantize_filters_mxfp6_kernel, dim3(blk), dim3(256), 0, s, t, w, w6, ws);
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
