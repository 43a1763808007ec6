// The storage layout of a quantised tensor, in one place: how many code and scale bytes n elements take in each format (n = a sample's
// H * W * C, or a filter's taps * Co * Ci; MX blocks are 32 consecutive channels, so n is a multiple of 32 there).
#pragma once
#include <cmath>
#include <cstddef>

namespace ssd {

// none: no quantised form (fp32 and bf16 handles); fp8: e4m3 codes with one fp32 scale per tensor (conv_fp8.hip); mxfp8: e4m3 codes
// with one E8M0 scale byte per 32 channels (conv_mxfp8.hip); mxfp6: e2m3 codes, 24 bytes per 32 channels, and the same scale bytes
// (conv_mxfp6.hip)
enum class Quant { none, fp8, mxfp8, mxfp6 };

constexpr bool quant_block_scales(Quant q) { return q == Quant::mxfp8 || q == Quant::mxfp6; }
constexpr bool quant_tensor_scale(Quant q) { return q == Quant::fp8; }
constexpr size_t quant_code_bytes(Quant q, size_t n) { return q == Quant::none ? 0 : q == Quant::mxfp6 ? n / 32 * 24 : n; }
constexpr size_t quant_scale_bytes(Quant q, size_t n) { return quant_block_scales(q) ? n / 32 : 0; }

// one sample of a quantised tensor and what follows it: null members where the tensor has no such form
struct QView {
    unsigned char* codes;
    unsigned char* scales;      // E8M0 block scales (MX kinds)
    float scale;                // the tensor's scale (fp8)
};

// The values of `count` quantised elements on the host: an fp8 tensor's codes times its scale, an MX tensor's codes (mxfp6: 24 bytes per
// block, code j in bits 6 j ... 6 j + 5) times their blocks' 2^x; exact in fp32.
inline void dequantize_host(Quant q, const unsigned char* codes, const unsigned char* scales, float scale, size_t count, float* out) {
    for (size_t i = 0; i < count; ++i) {
        if (q == Quant::mxfp6) {
            const unsigned char* blk = codes + i / 32 * 24;
            const int bit = 6 * (int)(i % 32);
            const int c = ((blk[bit >> 3] | (bit + 6 > ((bit >> 3) + 1) * 8 ? blk[(bit >> 3) + 1] << 8 : 0)) >> (bit & 7)) & 63;
            const int e = (c >> 3) & 3, m = c & 7;
            const float v = e == 0 ? m / 8.f : ldexpf(1.f + m / 8.f, e - 1);
            out[i] = ldexpf(c & 32 ? -v : v, (int)scales[i / 32] - 127);
        } else {
            const int c = codes[i], e = (c >> 3) & 15, m = c & 7;
            const float v = (e == 15 && m == 7) ? NAN : e == 0 ? ldexpf((float)m, -9) : ldexpf(1.f + m / 8.f, e - 7);
            out[i] = scales ? ldexpf(c & 0x80 ? -v : v, (int)scales[i / 32] - 127) : (c & 0x80 ? -v : v) * scale;
        }
    }
}

}  // namespace ssd
