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

bool conv_bigk_fwd_mxfp8_supported(const ConvDesc& d, int out_mode, const char** why) {
    const char* w = conv_quant_refusal(FMT_MXFP8, true, d, out_mode);
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

// the stand-alone quantiser and max-pooling: mx_block.h's, on this format
void quantize_mxfp8(const void* x, bool x_f32, size_t rows, int C, unsigned char* y8, unsigned char* ys, hipStream_t s) {
    quantize_mx<MxE4M3>("quantize_mxfp8", x, x_f32, rows, C, y8, ys, s);
}
void maxpool_fwd_mxfp8(const PoolDesc& d, const unsigned char* x8, const unsigned char* xs, unsigned char* y8, unsigned char* ys, hipStream_t s) {
    maxpool_fwd_mx<MxE4M3>("maxpool_fwd_mxfp8", d, x8, xs, y8, ys, s);
}

}  // namespace ssd
