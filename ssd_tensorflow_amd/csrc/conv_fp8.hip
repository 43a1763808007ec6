// fp8 (OCP e4m3fn) inference kernels for gfx950 (MI355X): the forward gather convolution on e4m3 operands at one fp32 scale per
// activation tensor -- the kernel and its host path are conv_fp8_detail.h's, instantiated here with MX = false -- plus what surrounds
// it: filter quantisation (per output channel), activation quantisation (per tensor), the absmax reduction calibration needs and
// max-pooling on e4m3 bytes.  DESIGN.md 18; more than 9 taps (the fc graph's 7 x 7 fc6): DESIGN.md 19.
//
// Numeric contract: code = RNE(clamp(v / s, -448, 448)); products of two e4m3 numbers are exact in fp32, the MFMA adds in
// fp32; epilogue in fp32: y = relu?(acc * (s_in * s_w[co]) + bias[co]), then bf16 / fp32 / e4m3 at the consumer's scale.
#include "conv.h"
#include "conv_detail.h"
#include "conv_fp8_detail.h"
#include "bf16.h"
#include "ops.h"
#include <algorithm>

namespace ssd {

static bool supported_fp8(bool bigk, const ConvDesc& d, const char** why) {
    const char* w = conv_quant_refusal(FMT_FP8, bigk, d, -1);
    if (why) *why = w;
    return w == nullptr;
}
bool conv_fwd_fp8_supported(const ConvDesc& d, const char** why) { return supported_fp8(false, d, why); }
bool conv_bigk_fwd_fp8_supported(const ConvDesc& d, const char** why) { return supported_fp8(true, d, why); }

// Where an fp8 handle uses the kernel for up to 9 taps.  Interleaved rounds against the bf16 handle at batch 128 (tools/infer_rate.py,
// profiles/fp8_infer_rate_all_layers.txt, profiles/fp8_infer_rate.txt): every layer with at least 256 input channels
// ran 1.09 ... 1.46 x faster than its bf16 kernel in every round; the layers with 64 or 128 did not (conv1_2 0.42 x, conv2_1
// 0.91 x, conv2_2 not separated and it loses its fused pool, conv3_1 1.10 x in one run and not separated in the next) -- there a tap
// is one or two 64-byte chunks, and the bf16 handle runs the 64-channel and kernel-row gathers of conv_bf16.hip with the pool in the
// epilogue, forms this per-tap kernel does not have.
// They stay on bf16.  SSD_FP8_ALL=1 (read per handle) takes every supported layer: the A/B that produced the table.
bool conv_fwd_fp8_worthwhile(const ConvDesc& d) { return d.Ci >= 256 || env_int("SSD_FP8_ALL", 0) == 1; }

// ... and for more than 9 taps: SSD_FP8_BIGK (read per handle) = 1 takes every supported layer with at least 256 input
// channels (the fc graph's mod_conv6), 0 leaves it on conv_bigk_fwd_bf16 with a quantise pass behind it.  Unset = 1: in interleaved
// rounds at batch 128 (tools/infer_rate.py --a-trous false, profiles/fp8_fc_infer_rate.txt) the mod_conv6 row separated
// from the bf16 kernel's in fp8's favour, and the whole handle from the handle under SSD_FP8_BIGK=0.
constexpr int FP8_BIGK_DEFAULT = 1;
bool conv_bigk_fwd_fp8_worthwhile(const ConvDesc& d) { return d.Ci >= 256 && env_int("SSD_FP8_BIGK", FP8_BIGK_DEFAULT) == 1; }

static void run_fp8(bool bigk, const ConvDesc& d, const unsigned char* x8, const unsigned char* w8, float s_in, const float* s_w, const float* bias,
                    void* y, unsigned char* y8, int out_mode, float s_out, bool relu, hipStream_t s) {
    GatherArgs8 a{};
    a.src = x8; a.wgt = w8; a.bias = bias; a.s_w = s_w; a.dst = y; a.dst8 = y8; a.s_in = s_in; a.s_out = s_out;
    conv_fwd_e4m3<false>(bigk, d, a, out_mode, relu, s);
}
void conv_fwd_fp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* w8, float s_in, const float* s_w, const float* bias,
                  void* y, unsigned char* y8, int out_mode, float s_out, bool relu, hipStream_t s) {
    run_fp8(false, d, x8, w8, s_in, s_w, bias, y, y8, out_mode, s_out, relu, s);
}
void conv_bigk_fwd_fp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* w8, float s_in, const float* s_w, const float* bias,
                       void* y, unsigned char* y8, int out_mode, float s_out, bool relu, hipStream_t s) {
    run_fp8(true, d, x8, w8, s_in, s_w, bias, y, y8, out_mode, s_out, relu, s);
}

// =================================================================================
// filter quantisation: fp32 [tap][Ci][Co] -> e4m3 [tap][Co][Ci] + one fp32 scale per output channel, all layers in one launch
// (the table: conv_fp8_detail.h; one workgroup per 32 output channels)
// =================================================================================
__global__ __launch_bounds__(1024) void quantize_filters_fp8_kernel(QuantTable t, const float* __restrict__ w, unsigned char* __restrict__ w8,
                                                                   float* __restrict__ s_w) {
    __shared__ float red[32][33];
    __shared__ float scale[32];
    __shared__ float tile[32][33];
    int s = 0;
    while (s + 1 < t.n && (int)blockIdx.x >= t.seg[s + 1].blk0) ++s;
    const QuantTable::Seg g = t.seg[s];
    const int co0 = ((int)blockIdx.x - g.blk0) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int co = co0 + tx;
    const float* wl = w + g.off;
    // pass 1: absmax of this block's 32 output channels over every tap and input channel
    float am = 0.f;
    if (co < g.co)
        for (int r = ty; r < g.taps * g.ci; r += 32) am = fmaxf(am, fabsf(wl[(size_t)r * g.co + co]));
    red[ty][tx] = am;
    __syncthreads();
    if (ty == 0) {
#pragma unroll
        for (int q = 1; q < 32; ++q) am = fmaxf(am, red[q][tx]);
        const float sv = am > 0.f ? am / 448.0f : 1.0f;
        scale[tx] = sv;
        if (co < g.co) s_w[g.offs + co] = sv;
    }
    __syncthreads();
    // pass 2: 32 (ci) x 32 (co) tiles through LDS (one element per thread), written as rows of 32 consecutive ci bytes
    const int cit_n = (g.ci + 31) / 32;
    for (int it = 0; it < g.taps * cit_n; ++it) {
        const int tap = it / cit_n, cit = it - tap * cit_n;
        {
            const int ci = cit * 32 + ty;
            tile[ty][tx] = (ci < g.ci && co < g.co) ? wl[((size_t)tap * g.ci + ci) * g.co + co] : 0.f;
        }
        __syncthreads();
        {
            const int r = ty;                         // output channel inside the tile
            const int ci = cit * 32 + tx;
            if (co0 + r < g.co && ci < g.ci) w8[g.off8 + ((size_t)tap * g.co + co0 + r) * g.ci + ci] = to_e4m3(tile[tx][r] / scale[r]);
        }
        __syncthreads();
    }
}

// A layer with more than 9 taps (the fc graph's fc6: 25 088 rows of 4096) would keep its 128 workgroups of the kernel above walking
// every row twice while the rest of the chip idles, on every pass of an fp8 handle.  Its rows are split instead:
// absmax per output channel by row slices (the maximum of |w|'s bit patterns lands in s_w), the codes by 64 (ci) x 64 (co) tiles of
// one tap each, then s_w becomes the scale.  The same fp32 operations per element as above: identical scales and codes.
__global__ __launch_bounds__(256) void filter_absmax_rows_kernel(const float* __restrict__ wl, unsigned* __restrict__ amax, int rows, int co, int rows_per) {
    __shared__ unsigned red[4][64][4];
    const int cq = threadIdx.x & 63, rl = threadIdx.x >> 6;      // 64 channel quads x 4 row lanes
    const int c = ((int)blockIdx.x * 64 + cq) * 4;
    const int r0 = (int)blockIdx.y * rows_per, r1 = min(r0 + rows_per, rows);
    float am[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < co)      // co is a multiple of 4 (host check): a quad is inside or outside as a whole
        for (int r = r0 + rl; r < r1; r += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(wl + (size_t)r * co + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) am[e] = fmaxf(am[e], fabsf(v[e]));
        }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[rl][cq][e] = __float_as_uint(am[e]);      // non-negative floats order like their bit patterns
    __syncthreads();
    if (rl == 0 && c < co)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned m = red[0][cq][e];
            for (int q = 1; q < 4; ++q) m = red[q][cq][e] > m ? red[q][cq][e] : m;
            if (m) atomicMax(amax + c + e, m);
        }
}

__global__ __launch_bounds__(256) void quantize_filter_tiles_fp8_kernel(const float* __restrict__ wl, unsigned char* __restrict__ w8l,
                                                                        const float* __restrict__ amax, int ci, int co) {
    __shared__ float tile[64][65];
    __shared__ float scale[64];
    const int tid = threadIdx.x;
    const int cot_n = (co + 63) / 64, cit_n = ci / 64;      // ci is a multiple of 64 (host check)
    const int cot = (int)blockIdx.x % cot_n, t = (int)blockIdx.x / cot_n;
    const int cit = t % cit_n, tap = t / cit_n;
    const int co0 = cot * 64, ci0 = cit * 64;
    if (tid < 64) {
        const float am = co0 + tid < co ? amax[co0 + tid] : 0.f;
        scale[tid] = am > 0.f ? am / 448.0f : 1.0f;
    }
    {
        const int r = tid >> 4, c4 = (tid & 15) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cl = r + 16 * j;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (co0 + c4 < co) v = *reinterpret_cast<const f32x4*>(wl + ((size_t)tap * ci + ci0 + cl) * co + co0 + c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[cl][c4 + e] = v[e];
        }
    }
    __syncthreads();
    const int col = tid >> 2, q = tid & 3;      // one output channel's 16 consecutive ci: a 16-byte store
    if (co0 + col >= co) return;
    const float sv = scale[col];
    unsigned w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        w[e] = pack4_e4m3(tile[q * 16 + 4 * e][col] / sv, tile[q * 16 + 4 * e + 1][col] / sv, tile[q * 16 + 4 * e + 2][col] / sv,
                          tile[q * 16 + 4 * e + 3][col] / sv);
    *reinterpret_cast<u32x4*>(w8l + ((size_t)tap * co + co0 + col) * ci + ci0 + q * 16) = u32x4{w[0], w[1], w[2], w[3]};
}

__global__ __launch_bounds__(256) void filter_scales_from_absmax_kernel(float* __restrict__ s_w, int co) {
    const int c = (int)blockIdx.x * 256 + threadIdx.x;
    if (c < co) {
        const float am = s_w[c];
        s_w[c] = am > 0.f ? am / 448.0f : 1.0f;
    }
}

static bool quantize_rows_split(const FilterQuantPlan::Layer& L, const float* w, const unsigned char* w8) {
    return L.taps > 9 && L.ci % 64 == 0 && L.co % 4 == 0 && reinterpret_cast<uintptr_t>(w + L.off) % 16 == 0 &&
           reinterpret_cast<uintptr_t>(w8 + L.off8) % 16 == 0;
}

void FilterQuantPlan::add(size_t off, size_t off8, size_t offs, int taps, int ci, int co) {
    SSD_REQUIRE(n < MAX_LAYERS, "too many conv layers for the filter quantisation table");
    L[n].off = off; L[n].off8 = off8; L[n].offs = offs; L[n].taps = taps; L[n].ci = ci; L[n].co = co;
    ++n;
}

void quantize_filters_fp8(const FilterQuantPlan& plan, const float* w, unsigned char* w8, float* s_w, hipStream_t s) {
    QuantTable t{};
    double elems;      // (layers whose rows are split below are not in the table)
    const int blk = fill_quant_table(
        t, plan, elems, [&](const FilterQuantPlan::Layer& L) { return !quantize_rows_split(L, w, w8); },
        [](const FilterQuantPlan::Layer& L) { return cdiv(L.co, 32); });
    if (plan.n == 0) return;
    ProfScope prof("quantize_filters_fp8", 0.0, 9.0 * elems, s);
    if (blk > 0) hipLaunchKernelGGL(quantize_filters_fp8_kernel, dim3(blk), dim3(1024), 0, s, t, w, w8, s_w);
    for (int i = 0; i < plan.n; ++i) {
        const FilterQuantPlan::Layer& L = plan.L[i];
        if (!quantize_rows_split(L, w, w8)) continue;
        const int rows = L.taps * L.ci;
        const int slices = std::min(cdiv(rows, 64), 64);      // at least 64 rows a slice, at most 64 atomic maxima per channel
        HIP_OK(hipMemsetAsync(s_w + L.offs, 0, (size_t)L.co * sizeof(float), s));
        hipLaunchKernelGGL(filter_absmax_rows_kernel, dim3(cdiv(L.co, 256), slices), dim3(256), 0, s, w + L.off,
                           reinterpret_cast<unsigned*>(s_w + L.offs), rows, L.co, cdiv(rows, slices));
        hipLaunchKernelGGL(quantize_filter_tiles_fp8_kernel, dim3(L.taps * (L.ci / 64) * cdiv(L.co, 64)), dim3(256), 0, s, w + L.off,
                           w8 + L.off8, s_w + L.offs, L.ci, L.co);
        hipLaunchKernelGGL(filter_scales_from_absmax_kernel, dim3(cdiv(L.co, 256)), dim3(256), 0, s, s_w + L.offs, L.co);
    }
    HIP_OK(hipGetLastError());
}

// =================================================================================
// activation quantisation (bf16 or fp32 -> e4m3 at one scale) and the absmax reduction of calibration
// =================================================================================
__device__ __forceinline__ float ld1(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float ld1(const bf16_t* p, size_t i) { return bf2f(p[i].v); }

template <typename T>
__global__ __launch_bounds__(256) void quantize_fp8_kernel(const T* __restrict__ x, unsigned char* __restrict__ y, size_t n, float scale) {
    const size_t stride = (size_t)gridDim.x * 256 * 4;
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 4 <= n) {
            *reinterpret_cast<unsigned*>(y + i) =
                pack4_e4m3(ld1(x, i) / scale, ld1(x, i + 1) / scale, ld1(x, i + 2) / scale, ld1(x, i + 3) / scale);
        } else {
            for (size_t j = i; j < n; ++j) y[j] = to_e4m3(ld1(x, j) / scale);
        }
    }
}

// 8 values per thread: one 16-byte (bf16) or two 16-byte (fp32) loads, one 8-byte store; n a multiple of 8, pointers aligned
template <typename T>
__global__ __launch_bounds__(256) void quantize_fp8_x8_kernel(const T* __restrict__ x, unsigned char* __restrict__ y, size_t n8, float scale) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        float v[8];
        load8(x, i, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] / scale;
        *reinterpret_cast<u32x2*>(y + i * 8) = u32x2{pack4_e4m3(v[0], v[1], v[2], v[3]), pack4_e4m3(v[4], v[5], v[6], v[7])};
    }
}

void quantize_fp8(const void* x, bool x_f32, size_t n, float scale, unsigned char* y8, hipStream_t s) {
    SSD_REQUIRE(x && y8 && scale > 0.f, "quantize_fp8: null argument or non-positive scale");
    if (n == 0) return;
    ProfScope prof("quantize_fp8", 0.0, (x_f32 ? 5.0 : 3.0) * (double)n, s);
    const bool wide = n % 8 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(y8) % 8 == 0;
    if (wide && x_f32) hipLaunchKernelGGL(quantize_fp8_x8_kernel<float>, dim3(grid8(n / 8, 256)), dim3(256), 0, s, (const float*)x, y8, n / 8, scale);
    else if (wide) hipLaunchKernelGGL(quantize_fp8_x8_kernel<bf16_t>, dim3(grid8(n / 8, 256)), dim3(256), 0, s, (const bf16_t*)x, y8, n / 8, scale);
    else if (x_f32) hipLaunchKernelGGL(quantize_fp8_kernel<float>, dim3(grid8(n, 1024)), dim3(256), 0, s, (const float*)x, y8, n, scale);
    else hipLaunchKernelGGL(quantize_fp8_kernel<bf16_t>, dim3(grid8(n, 1024)), dim3(256), 0, s, (const bf16_t*)x, y8, n, scale);
    HIP_OK(hipGetLastError());
}

// |x| of finite values orders like its bit pattern: the maximum is taken on unsigned words, NaN / Inf are skipped
__global__ __launch_bounds__(256) void absmax_bf16_kernel(const bf16_t* __restrict__ x, size_t n, unsigned* __restrict__ out) {
    __shared__ unsigned red[4];
    unsigned m = 0;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const unsigned a = ((unsigned)x[i].v & 0x7FFFu) << 16;
        if (a < 0x7F800000u) m = a > m ? a : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)m, o, 64);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) m = red[q] > m ? red[q] : m;
        atomicMax(out, m);
    }
}

void absmax_bf16(const bf16_t* x, size_t n, float* out, bool accumulate, hipStream_t s) {
    SSD_REQUIRE(x && out, "absmax_bf16: null argument");
    if (!accumulate) HIP_OK(hipMemsetAsync(out, 0, sizeof(float), s));
    if (n == 0) return;
    ProfScope prof("absmax_bf16", 0.0, 2.0 * (double)n, s);
    hipLaunchKernelGGL(absmax_bf16_kernel, dim3(grid8(n, 256 * 16)), dim3(256), 0, s, x, n, reinterpret_cast<unsigned*>(out));
    HIP_OK(hipGetLastError());
}

// =================================================================================
// max-pooling on e4m3 bytes.  A code's order key: positive codes 0x00..0x7F -> 0x80..0xFF, negative codes 0x80..0xFF
// (-0 .. the most negative) -> 0x7F..0x00; the maximum of the keys is the maximum of the values, any sign.  Cells outside
// the image never win (TF SAME).  16 channels per thread.
// =================================================================================
__device__ __forceinline__ unsigned key4(unsigned c) { return c ^ (0x80808080u | (((c & 0x80808080u) >> 7) * 0x7Fu)); }
__device__ __forceinline__ unsigned unkey4(unsigned k) { return k ^ (0x80808080u | (((~k & 0x80808080u) >> 7) * 0x7Fu)); }
__device__ __forceinline__ unsigned max4_u8(unsigned a, unsigned b) {
    unsigned r = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned x = (a >> (8 * e)) & 0xFFu, y = (b >> (8 * e)) & 0xFFu;
        r |= (x > y ? x : y) << (8 * e);
    }
    return r;
}

__global__ __launch_bounds__(256) void maxpool_fwd_fp8_kernel(PoolDesc d, const unsigned char* __restrict__ x, unsigned char* __restrict__ y) {
    const int c16 = d.C / 16;
    const size_t total = (size_t)d.B * d.Ho * d.Wo * c16;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
        const int cq = (int)(idx % c16);
        size_t t = idx / c16;
        const int ow = (int)(t % d.Wo);
        t /= d.Wo;
        const int oh = (int)(t % d.Ho);
        const int b = (int)(t / d.Ho);
        u32x4 best = u32x4{0u, 0u, 0u, 0u};      // key 0 = the most negative code: every in-image cell is at least that
        for (int kh = 0; kh < d.k; ++kh) {
            const int ih = oh * d.stride - d.pad_h + kh;
            if ((unsigned)ih >= (unsigned)d.Hi) continue;
            for (int kw = 0; kw < d.k; ++kw) {
                const int iw = ow * d.stride - d.pad_w + kw;
                if ((unsigned)iw >= (unsigned)d.Wi) continue;
                const u32x4 v = *reinterpret_cast<const u32x4*>(x + (((size_t)b * d.Hi + ih) * d.Wi + iw) * d.C + (size_t)cq * 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) best[e] = max4_u8(best[e], key4(v[e]));
            }
        }
        *reinterpret_cast<u32x4*>(y + idx * 16) = u32x4{unkey4(best[0]), unkey4(best[1]), unkey4(best[2]), unkey4(best[3])};
    }
}

void maxpool_fwd_fp8(const PoolDesc& d, const unsigned char* x8, unsigned char* y8, hipStream_t s) {
    SSD_REQUIRE(x8 && y8, "maxpool_fwd_fp8: null argument");
    SSD_REQUIRE(d.C % 16 == 0 && d.C > 0, "maxpool_fwd_fp8: C must be a multiple of 16 (got %d)", d.C);
    require_pool_geometry("maxpool_fwd_fp8", d);
    const size_t total = (size_t)d.B * d.Ho * d.Wo * (d.C / 16);
    ProfScope prof("maxpool_fwd_fp8", 0.0, (double)d.C * d.B * ((double)d.Hi * d.Wi + (double)d.Ho * d.Wo), s);
    hipLaunchKernelGGL(maxpool_fwd_fp8_kernel, dim3(grid8(total, 256)), dim3(256), 0, s, d, x8, y8);
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
