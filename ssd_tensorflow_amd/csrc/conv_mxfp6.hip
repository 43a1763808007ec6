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

// Why conv_fwd_mxfp6 refuses a layer, or nullptr (a string literal).  out_mode < 0: the shape alone.
static const char* conv_mxfp6_refusal(const ConvDesc& d, int out_mode) {
    const long long taps = (long long)d.KH * d.KW;
    const bool wants_mx = out_mode == FP8_OUT_MX || out_mode == FP8_OUT_BF16_MX;
    if (d.KH < 1 || d.KW < 1 || taps > 9) return "mxfp6 conv: at most 9 taps (a layer with more stays on its bf16 kernel: there is no mxfp6 kernel for it)";
    if (d.Ci < 64 || d.Ci % 64 != 0) return "mxfp6 conv: Ci must be a multiple of 64";
    if (d.Co < 8 || d.Co % 8 != 0) return "mxfp6 conv: Co must be a multiple of 8";
    if (d.stride < 1 || d.dil < 1) return "mxfp6 conv: stride and dilation must be positive";
    if (d.B < 1 || d.Ho < 1 || d.Wo < 1 || d.Hi < 1 || d.Wi < 1) return "mxfp6 conv: empty tensor";
    if ((long long)d.B * d.Hi * d.Wi * d.Ci >= (1LL << 31) - 16 || (long long)d.B * d.Ho * d.Wo * d.Co >= (1LL << 31) - 16)
        return "mxfp6 conv: a tensor of this layer exceeds the 32-bit offsets: lower the batch";
    if (taps * d.Co * d.Ci >= (1LL << 31) - 16) return "mxfp6 conv: the filter image exceeds the 32-bit offsets";
    if (out_mode >= 0 && !(out_mode == FP8_OUT_BF16 || out_mode == FP8_OUT_F32 || wants_mx)) return "mxfp6 conv: unknown output mode";
    if (out_mode >= 0 && wants_mx && d.Co % 32 != 0) return "mxfp6 conv: an MX output needs Co to be a multiple of 32";
    return nullptr;
}

bool conv_fwd_mxfp6_supported(const ConvDesc& d, const char** why) {
    const char* w = conv_mxfp6_refusal(d, -1);
    if (why) *why = w;
    return w == nullptr;
}

// Tiles: 0 = 128 x 128, five stages of 13 KB (the fp32 epilogue tile's 66 KB sets the allocation: two workgroups per CU); 1 = 64 x 64,
// six stages of 9 KB, where the 128 x 128 tiling would leave CUs empty -- the e4m3 kernel's rule.  SSD_TILE_FP8 forces one (tests, tuning).
void conv_fwd_mxfp6(const ConvDesc& d, const unsigned char* x6, const unsigned char* xs, const unsigned char* w6, const unsigned char* ws,
                    const float* bias, void* y, unsigned char* y6, unsigned char* ys, int out_mode, bool relu, hipStream_t s) {
    const char* why = conv_mxfp6_refusal(d, out_mode);
    SSD_REQUIRE(why == nullptr, "%s (got %dx%d taps, Ci %d, Co %d, output mode %d)", why, d.KH, d.KW, d.Ci, d.Co, out_mode);
    const bool wants_mx = out_mode == FP8_OUT_MX || out_mode == FP8_OUT_BF16_MX;
    SSD_REQUIRE(!wants_mx || (y6 != nullptr && ys != nullptr), "mxfp6 conv: an MX output needs its code and scale buffers");
    SSD_REQUIRE(out_mode == FP8_OUT_MX || y != nullptr, "mxfp6 conv: null output");
    SSD_REQUIRE(x6 && xs && w6 && ws, "mxfp6 conv: null operand");
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(xs) % 2 == 0 && reinterpret_cast<uintptr_t>(ws) % 2 == 0, "mxfp6 conv: a scale buffer must start at an even address");
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(x6) % 8 == 0 && reinterpret_cast<uintptr_t>(w6) % 8 == 0 && (!wants_mx || reinterpret_cast<uintptr_t>(y6) % 8 == 0),
                "mxfp6 conv: a code buffer must start at a multiple of 8 bytes");
    GatherArgs6 a{};
    a.src = x6; a.wgt = w6; a.bias = bias; a.dst = y; a.dst8 = y6; a.dst_sc = ys;
    a.sc_delta = (int)(reinterpret_cast<uintptr_t>(xs) & 3);      // (a sample's scales inside a batch may start between two dwords)
    a.src_sc = xs - a.sc_delta;
    a.wsc_delta = (int)(reinterpret_cast<uintptr_t>(ws) & 3);
    a.wgt_sc = ws - a.wsc_delta;
    a.M = d.B * d.Ho * d.Wo; a.DH = d.Ho; a.DW = d.Wo; a.DN = d.Co;
    a.SH = d.Hi; a.SW = d.Wi; a.SC = d.Ci;
    a.KH = d.KH; a.KW = d.KW; a.dil = d.dil; a.pad_h = d.pad_h; a.pad_w = d.pad_w;
    a.mul = d.stride; a.relu = relu; a.mode = out_mode;
    const double fl = conv_flops(d);
    const double code_b = 0.75 + 1.0 / 32;      // bytes per element: codes + scales
    const double out_b = out_mode == FP8_OUT_F32 ? 4.0 : out_mode == FP8_OUT_BF16 ? 2.0 : (out_mode == FP8_OUT_BF16_MX ? 2.0 : 0.0) + code_b;
    const double by = ((double)d.B * d.Hi * d.Wi * d.Ci + (double)d.KH * d.KW * d.Ci * d.Co) * code_b + (double)d.B * d.Ho * d.Wo * d.Co * out_b;
    int cfg = env_int("SSD_TILE_FP8", -1);
    if (cfg != 0 && cfg != 1) cfg = (long long)cdiv(a.M, 128) * cdiv(a.DN, 128) <= 256 ? 1 : 0;
    if (cfg == 0) launch_fwd_mxfp6<2, 2, 2, 2, 5>(a, "conv_fwd_mxfp6_128x128", fl, by, s);
    else launch_fwd_mxfp6<2, 2, 1, 1, 6>(a, "conv_fwd_mxfp6_64x64x6", fl, by, s);
}

// =================================================================================
// stand-alone quantiser: bf16 or fp32 [rows][C] -> codes + scales.  8 values per thread, a block = 4 adjacent lanes.
// =================================================================================
template <typename T>
__global__ __launch_bounds__(256) void quantize_mxfp6_kernel(const T* __restrict__ x, unsigned char* __restrict__ y, unsigned char* __restrict__ ys,
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
        const int ex = mx6_block_exponent(v);
        mx6_store_block(y + (i >> 2) * 24, mx6_pack8(v, ex), (int)(i & 3));
        if ((i & 3) == 0) ys[i >> 2] = (unsigned char)(ex + 127);
    }
}

void quantize_mxfp6(const void* x, bool x_f32, size_t rows, int C, unsigned char* y6, unsigned char* ys, hipStream_t s) {
    SSD_REQUIRE(x && y6 && ys, "quantize_mxfp6: null argument");
    SSD_REQUIRE(C > 0 && C % 32 == 0, "quantize_mxfp6: C must be a multiple of 32 (got %d)", C);
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(y6) % 8 == 0, "quantize_mxfp6: unaligned tensor");
    if (rows == 0) return;
    const size_t n8 = rows * (size_t)C / 8;
    ProfScope prof("quantize_mxfp6", 0.0, ((x_f32 ? 4.75 : 2.75) + 1.0 / 32) * (double)n8 * 8, s);
    if (x_f32) hipLaunchKernelGGL(quantize_mxfp6_kernel<float>, dim3(grid8(n8, 256)), dim3(256), 0, s, (const float*)x, y6, ys, n8);
    else hipLaunchKernelGGL(quantize_mxfp6_kernel<bf16_t>, dim3(grid8(n8, 256)), dim3(256), 0, s, (const bf16_t*)x, y6, ys, n8);
    HIP_OK(hipGetLastError());
}

// =================================================================================
// filter quantisation: fp32 [tap][Ci][Co] -> codes [tap][Co][Ci / 32][24] + scales [tap][Co][Ci / 32], all layers in one launch.  One
// thread per block of 32 input channels, output channel fastest: the 32 loads of a wave are rows of consecutive floats.
// =================================================================================
struct QuantTable6 {
    int n;
    struct Seg {
        unsigned long long off, off6, offs;      // fp32 filter (elements), code image (bytes), scales (bytes)
        int taps, ci, co;
        int blk0;                                // first workgroup of this layer
    } seg[FilterQuantPlan::MAX_LAYERS];
};

__global__ __launch_bounds__(256) void quantize_filters_mxfp6_kernel(QuantTable6 t, const float* __restrict__ w, unsigned char* __restrict__ w6,
                                                                    unsigned char* __restrict__ ws) {
    int s = 0;
    while (s + 1 < t.n && (int)blockIdx.x >= t.seg[s + 1].blk0) ++s;
    const QuantTable6::Seg g = t.seg[s];
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
    const int x = mx6_exponent(am);
    const size_t blk = ((size_t)tap * g.co + co) * cbn + cb;
    unsigned long long q[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        q[h] = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) q[h] |= (unsigned long long)enc_e2m3(ldexpf(v[8 * h + e], -x)) << (6 * e);
    }
    const unsigned long long o0 = q[0] | (q[1] << 48), o1 = (q[1] >> 16) | (q[2] << 32), o2 = (q[2] >> 32) | (q[3] << 16);
    unsigned char* d = w6 + g.off6 + blk * 24;
    *reinterpret_cast<u32x2*>(d) = u32x2{(unsigned)o0, (unsigned)(o0 >> 32)};
    *reinterpret_cast<u32x2*>(d + 8) = u32x2{(unsigned)o1, (unsigned)(o1 >> 32)};
    *reinterpret_cast<u32x2*>(d + 16) = u32x2{(unsigned)o2, (unsigned)(o2 >> 32)};
    ws[g.offs + blk] = (unsigned char)(x + 127);
}

void quantize_filters_mxfp6(const FilterQuantPlan& plan, const float* w, unsigned char* w6, unsigned char* ws, hipStream_t s) {
    if (plan.n == 0) return;
    SSD_REQUIRE(w && w6 && ws, "quantize_filters_mxfp6: null argument");
    QuantTable6 t{};
    t.n = plan.n;
    int blk = 0;
    double elems = 0;
    for (int i = 0; i < plan.n; ++i) {
        const FilterQuantPlan::Layer& L = plan.L[i];
        SSD_REQUIRE(L.taps >= 1 && L.co >= 1 && L.ci >= 32 && L.ci % 32 == 0, "quantize_filters_mxfp6: Ci must be a multiple of 32 (got %d)", L.ci);
        SSD_REQUIRE(reinterpret_cast<uintptr_t>(w6 + L.off8) % 8 == 0, "quantize_filters_mxfp6: a code image must start at a multiple of 8 bytes");
        QuantTable6::Seg& g = t.seg[i];
        g.off = L.off; g.off6 = L.off8; g.offs = L.offs;
        g.taps = L.taps; g.ci = L.ci; g.co = L.co;
        g.blk0 = blk;
        blk += cdiv((long long)L.taps * (L.ci / 32) * L.co, 256);
        elems += (double)L.taps * L.ci * L.co;
    }
    ProfScope prof("quantize_filters_mxfp6", 0.0, (4.75 + 1.0 / 32) * elems, s);
    hipLaunchKernelGGL(quantize_filters_mxfp6_kernel, dim3(blk), dim3(256), 0, s, t, w, w6, ws);
    HIP_OK(hipGetLastError());
}

// =================================================================================
// max-pooling: per output pixel and block the window's cells are dequantised (exact in fp32), the maximum is taken per channel --
// cells outside the image never win (TF SAME) -- and the block is quantised again by the scale rule: one more rounding.  8 channels
// per thread (48 bits of a block's string, read as three 16-bit words), a block = 4 adjacent lanes.
// =================================================================================
__global__ __launch_bounds__(256) void maxpool_fwd_mxfp6_kernel(PoolDesc d, const unsigned char* __restrict__ x, const unsigned char* __restrict__ xs,
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
                const unsigned short* h = reinterpret_cast<const unsigned short*>(x + blk * 24 + 6 * (cq & 3));
                const unsigned long long c = (unsigned long long)h[0] | ((unsigned long long)h[1] << 16) | ((unsigned long long)h[2] << 32);
                const int ex = (int)xs[blk] - 127;
#pragma unroll
                for (int e = 0; e < 8; ++e) best[e] = fmaxf(best[e], ldexpf(dec_e2m3((unsigned)(c >> (6 * e)) & 63u), ex));
            }
        }
        const int ex = mx6_block_exponent(best);
        mx6_store_block(y + (idx >> 2) * 24, mx6_pack8(best, ex), cq & 3);
        if ((cq & 3) == 0) ys[idx >> 2] = (unsigned char)(ex + 127);
    }
}

void maxpool_fwd_mxfp6(const PoolDesc& d, const unsigned char* x6, const unsigned char* xs, unsigned char* y6, unsigned char* ys, hipStream_t s) {
    SSD_REQUIRE(x6 && xs && y6 && ys, "maxpool_fwd_mxfp6: null argument");
    SSD_REQUIRE(d.C % 32 == 0 && d.C > 0, "maxpool_fwd_mxfp6: C must be a multiple of 32 (got %d)", d.C);
    SSD_REQUIRE(d.k >= 1 && d.stride >= 1 && d.B > 0 && d.Ho > 0 && d.Wo > 0, "maxpool_fwd_mxfp6: bad geometry");
    // every window must hold at least one cell of the image
    SSD_REQUIRE((d.Ho - 1) * d.stride - d.pad_h < d.Hi && (d.Wo - 1) * d.stride - d.pad_w < d.Wi && d.pad_h < d.k && d.pad_w < d.k,
                "maxpool_fwd_mxfp6: a window lies outside the image");
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(x6) % 8 == 0 && reinterpret_cast<uintptr_t>(y6) % 8 == 0, "maxpool_fwd_mxfp6: unaligned tensor");
    const size_t total = (size_t)d.B * d.Ho * d.Wo * (d.C / 8);
    ProfScope prof("maxpool_fwd_mxfp6", 0.0, (0.75 + 1.0 / 32) * d.C * d.B * ((double)d.Hi * d.Wi + (double)d.Ho * d.Wo), s);
    hipLaunchKernelGGL(maxpool_fwd_mxfp6_kernel, dim3(grid8(total, 256)), dim3(256), 0, s, d, x6, xs, y6, ys);
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
