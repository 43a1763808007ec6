// Convolutions with more than 9 taps on gfx950 (MI355X): the fc graph's fc6, a 7x7 / stride 1 / SAME convolution 512 -> 4096
// (ssdvgg.py __build_vgg_mods).  The gather kernels of conv_igemm.hip / conv_bf16.hip carry 9-entry tap tables in their kernel
// arguments; these kernels compute a tap's offsets from (KH, KW, pad) instead, so every existing launch keeps its arguments.
//
// One implicit-GEMM kernel, C[m][n] = sum_k A[m][k] * B[k][n], for all three passes, fp32 (v_mfma_f32_32x32x2_f32) or bf16
// (v_mfma_f32_32x32x16_bf16, fp32 accumulation):
//   forward         m = pixel,           n = Co, k = (tap, Ci)  A = x shifted by the tap, B = the filter
//   data gradient   m = pixel,           n = Ci, k = (tap, Co)  A = dy shifted by the mirrored tap, B = the filter [tap][Ci][Co]
//   weight gradient m = (tap, Ci),       n = Co, k = pixel      A = x shifted by the tap, B = dy
// A k iteration covers 128 bytes of k (32 fp32 / 64 bf16): forward and data gradient walk channel chunks outer, taps inner, so
// the 49 taps re-read the same pixels from L1 / L2.  Both LDS tiles are [rows][128 + 16 bytes] with k contiguous, read as one
// ds_read_b128 per MFMA operand (fp32: 4 k of the lane half, the k index permuted as in conv_igemm.hip; bf16: 8 k).  An operand
// whose global rows are k-contiguous (activations by channel, the filter mirrors) is staged as 16-byte chunks; one whose global
// rows run along m / n (the fp32 forward filter [tap][Ci][Co], both operands of the weight gradient) is loaded as 4 k-rows of one
// 16-byte chunk per thread and transposed in registers (4 b128 / 8 b64 LDS writes).  Global -> registers one k iteration ahead of
// the MFMAs, two LDS buffers, one barrier per iteration; the SAME padding is a per-row out-of-range buffer offset (zeros).
//
// Every output element is owned by one workgroup and summed in one fixed order: bit-identical results run to run.  No workspace:
// the weight gradient's 6,272 tiles (fc6 at vgg300) fill the chip without a pixel split, the data gradient fills it with
// 64-wide n tiles (pick_bn), the bias gradient is a second launch over dy.
#include "conv.h"
#include "conv_detail.h"
#include "bf16.h"
#include <algorithm>

namespace ssd {

__device__ __forceinline__ int cdiv_dev(int a, int b) { return (a + b - 1) / b; }

enum { BIGK_FWD = 0, BIGK_DGRAD = 1, BIGK_WGRAD = 2 };

struct BigKArgs {
    const void* src;     // forward / weight gradient: x [P][Ci];  data gradient: dy [P][Co]
    const void* wgt;     // forward: fp32 filter [tap][Ci][Co] or bf16 mirror [tap][Co][Ci];  data gradient: [tap][Ci][Co];  weight gradient: dy [P][Co]
    const float* bias;   // forward
    const void* mask;    // data gradient: relu mask (dx's shape and type) or nullptr
    void* dst;           // forward: y (T, or fp32 when out_f32);  data gradient: dx (T);  weight gradient: dw (fp32)
    const float* w;      // weight gradient: the filter of the decay term (or nullptr)
    float wd;
    int H, W, KH, KW, ph, pw;
    int SC, DN;          // channels of the gathered source (weight gradient: Ci) / of the output (weight gradient: Co)
    int P;               // pixels B * H * W
    int MT, NT, CT;      // tiles along m and n; weight gradient: channel tiles per tap (MT = taps * CT)
    int relu, accum, out_f32;
    unsigned src_bytes, wgt_bytes;
};

template <int PASS, typename T, int TN>
__global__ __launch_bounds__(256) void conv_bigk_kernel(BigKArgs p) {
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int VEC = 16 / sizeof(T);           // elements per 16-byte chunk
    constexpr int BK = 8 * VEC;                   // k per iteration: 128 bytes
    constexpr int ROWB = 144;                     // LDS row: 128 bytes of k + 16 bytes pad
    constexpr int BM = 128, BN = 64 * TN;
    constexpr int STAGE = (BM + BN) * ROWB;
    constexpr bool A_MN = PASS == BIGK_WGRAD;
    constexpr bool B_MN = PASS == BIGK_WGRAD || (PASS == BIGK_FWD && F32);
    static_assert(!B_MN || BN == 128, "m/n-contiguous operands are staged for 128 rows");
    constexpr int QK = BK / 4;                    // m/n-contiguous staging: k quads per iteration ...
    constexpr unsigned OOB = 0xFFFFFFF0u;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = wg % p.MT, nt = wg / p.MT;     // m fastest: the workgroups in flight share the n operand's slab
    const int n0 = nt * BN;
    const int taps = p.KH * p.KW;
    // weight gradient: the tile's tap and first input channel
    const int wtap = PASS == BIGK_WGRAD ? mt / p.CT : 0;
    const int m0 = PASS == BIGK_WGRAD ? (mt - wtap * p.CT) * BM : mt * BM;
    const int wkh = wtap / p.KW, wkw = wtap - wkh * p.KW;

    const __amdgpu_buffer_rsrc_t src_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.src), 0, p.src_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wgt_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.wgt), 0, p.wgt_bytes, 0x00020000);

    // ---- staging coordinates ------------------------------------------------------
    // k-contiguous rows: row = (tid >> 3) + 32 i, chunk q = tid & 7
    const int q = tid & 7;
    // m/n-contiguous rows: k rows 4 kq .. 4 kq + 3, chunk mc (VEC consecutive m / n)
    const int kq = tid % QK, mn0 = (tid / QK) * VEC;
    // forward / data gradient: the A rows' pixels
    constexpr int NA = BM / 32;
    int a_h[NA], a_w[NA];
    unsigned a_base[NA];
    if constexpr (!A_MN) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int m = m0 + (tid >> 3) + 32 * i;
            const int mm = m < p.P ? m : 0;
            const int ow = mm % p.W, t = mm / p.W;
            const int oh = t % p.H;
            a_h[i] = m < p.P ? oh : -(1 << 20);
            a_w[i] = ow;
            a_base[i] = (unsigned)mm * p.SC + q * VEC;
        }
    }
    u32x4 areg[4], breg[4];

    auto load_tiles = [&](int kiter) {
        if constexpr (PASS != BIGK_WGRAD) {
            const int cc = kiter / taps, tap = kiter - cc * taps;
            const int kh = tap / p.KW, kw = tap - kh * p.KW;
            const int dh = PASS == BIGK_FWD ? kh - p.ph : p.ph - kh;
            const int dw = PASS == BIGK_FWD ? kw - p.pw : p.pw - kw;
            const int c0 = cc * BK;
            const int toff = (dh * p.W + dw) * p.SC + c0;
            const bool cok = c0 + q * VEC < p.SC;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int sh = a_h[i] + dh, sw = a_w[i] + dw;
                const bool ok = cok && (unsigned)sh < (unsigned)p.H && (unsigned)sw < (unsigned)p.W;
                const unsigned off = ok ? (unsigned)((int)a_base[i] + toff) * (unsigned)sizeof(T) : OOB;
                areg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(src_rsrc, off, 0, 0));
            }
            if constexpr (B_MN) {      // fp32 forward: filter [tap][SC][DN], k rows c0 + 4 kq + i, columns n0 + mn0 ..
                const int n = n0 + mn0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = c0 + 4 * kq + i;
                    const bool ok = c < p.SC && n < p.DN;
                    const unsigned off = ok ? (unsigned)((tap * p.SC + c) * p.DN + n) * (unsigned)sizeof(T) : OOB;
                    breg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wgt_rsrc, off, 0, 0));
                }
            } else {                   // [tap][DN][SC]: the bf16 forward mirror [tap][Co][Ci], the data gradient's [tap][Ci][Co]
                const int c = c0 + q * VEC;
#pragma unroll
                for (int i = 0; i < BN / 32; ++i) {
                    const int n = n0 + (tid >> 3) + 32 * i;
                    const bool ok = cok && n < p.DN;
                    const unsigned off = ok ? (unsigned)((tap * p.DN + n) * p.SC + c) * (unsigned)sizeof(T) : OOB;
                    breg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wgt_rsrc, off, 0, 0));
                }
            }
        } else {
            // k rows = pixels k0 + 4 kq + i; A = x at the pixel shifted by the tile's tap, channels m0 + mn0 ..; B = dy, channels n0 + mn0 ..
            const int pix0 = kiter * BK + 4 * kq;
            const int ci = m0 + mn0, n = n0 + mn0;
            const bool cok = ci < p.SC, nok = n < p.DN;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int pix = pix0 + i;
                const bool pok = pix < p.P;
                const int ow = pix % p.W, t = pix / p.W;
                const int oh = t % p.H, b = t / p.H;
                const int sh = oh + wkh - p.ph, sw = ow + wkw - p.pw;
                const bool ok = pok && cok && (unsigned)sh < (unsigned)p.H && (unsigned)sw < (unsigned)p.W;
                const unsigned aoff = ok ? (unsigned)(((b * p.H + sh) * p.W + sw) * p.SC + ci) * (unsigned)sizeof(T) : OOB;
                areg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(src_rsrc, aoff, 0, 0));
                const unsigned boff = (pok && nok) ? (unsigned)(pix * p.DN + n) * (unsigned)sizeof(T) : OOB;
                breg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wgt_rsrc, boff, 0, 0));
            }
        }
    };

    // 4 k-rows of one 16-byte m/n chunk -> rows mn0 .. mn0 + VEC - 1 of the tile, k columns 4 kq .. 4 kq + 3
    auto store_mn = [&](char* L, const u32x4* v) {
        if constexpr (F32) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<u32x4*>(L + (mn0 + j) * ROWB + kq * 16) = u32x4{v[0][j], v[1][j], v[2][j], v[3][j]};
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int w = j >> 1, sh = (j & 1) * 16;
                const unsigned e0 = (v[0][w] >> sh) & 0xFFFFu, e1 = (v[1][w] >> sh) & 0xFFFFu;
                const unsigned e2 = (v[2][w] >> sh) & 0xFFFFu, e3 = (v[3][w] >> sh) & 0xFFFFu;
                *reinterpret_cast<u32x2*>(L + (mn0 + j) * ROWB + kq * 8) = u32x2{e0 | (e1 << 16), e2 | (e3 << 16)};
            }
        }
    };
    auto store_tiles = [&](int buf) {
        char* As = smem + buf * STAGE;
        char* Bs = As + BM * ROWB;
        if constexpr (A_MN) store_mn(As, areg);
        else {
#pragma unroll
            for (int i = 0; i < NA; ++i) *reinterpret_cast<u32x4*>(As + ((tid >> 3) + 32 * i) * ROWB + q * 16) = areg[i];
        }
        if constexpr (B_MN) store_mn(Bs, breg);
        else {
#pragma unroll
            for (int i = 0; i < BN / 32; ++i) *reinterpret_cast<u32x4*>(Bs + ((tid >> 3) + 32 * i) * ROWB + q * 16) = breg[i];
        }
    };

    // ---- accumulators: 4 waves as 2 x 2, a wave owns 64 x (32 TN) ------------------------
    f32x16 acc[2][TN];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;

    auto compute = [&](int buf) {
        const char* As = smem + buf * STAGE;
        const char* Bs = As + BM * ROWB;
        if constexpr (F32) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int kb = (g * 8 + lh * 4) * 4;
                f32x4 a[2], b[TN];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) a[mi] = *reinterpret_cast<const f32x4*>(As + (wm * 64 + mi * 32 + li) * ROWB + kb);
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) b[ni] = *reinterpret_cast<const f32x4*>(Bs + (wn * 32 * TN + ni * 32 + li) * ROWB + kb);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < TN; ++ni)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi][t], b[ni][t], acc[mi][ni], 0, 0, 0);
            }
        } else {
            typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int kb = (st * 16 + lh * 8) * 2;
                bf16x8 a[2], b[TN];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) a[mi] = *reinterpret_cast<const bf16x8*>(As + (wm * 64 + mi * 32 + li) * ROWB + kb);
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) b[ni] = *reinterpret_cast<const bf16x8*>(Bs + (wn * 32 * TN + ni * 32 + li) * ROWB + kb);
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
            }
        }
    };

    // ---- main loop ---------------------------------------------------------------------
    const int nk = PASS == BIGK_WGRAD ? cdiv_dev(p.P, BK) : cdiv_dev(p.SC, BK) * taps;
    load_tiles(0);
    store_tiles(0);
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
        const bool more = k + 1 < nk;
        if (more) load_tiles(k + 1);
        compute(k & 1);
        if (more) store_tiles((k + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) ----------------
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
            const int n = n0 + wn * 32 * TN + ni * 32 + li;
            if (n >= p.DN) continue;
            const int mb = m0 + wm * 64 + mi * 32 + 4 * lh;
            if constexpr (PASS == BIGK_FWD) {
                const float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mb + (r & 3) + 8 * (r >> 2);
                    if (m >= p.P) continue;
                    float v = acc[mi][ni][r] + bv;
                    if (p.relu) v = v > 0.f ? v : 0.f;
                    const size_t o = (size_t)m * p.DN + n;
                    if (F32 || p.out_f32) static_cast<float*>(p.dst)[o] = v;
                    else static_cast<unsigned short*>(p.dst)[o] = f2bf(v);
                }
            } else if constexpr (PASS == BIGK_DGRAD) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mb + (r & 3) + 8 * (r >> 2);
                    if (m >= p.P) continue;
                    const size_t o = (size_t)m * p.DN + n;
                    float v = acc[mi][ni][r];
                    if constexpr (F32) {
                        if (p.accum) v += static_cast<const float*>(p.dst)[o];
                        if (p.mask) v = static_cast<const float*>(p.mask)[o] > 0.f ? v : 0.f;
                        static_cast<float*>(p.dst)[o] = v;
                    } else {
                        if (p.accum) v += bf2f(static_cast<const unsigned short*>(p.dst)[o]);
                        if (p.mask) v = bf2f(static_cast<const unsigned short*>(p.mask)[o]) > 0.f ? v : 0.f;
                        static_cast<unsigned short*>(p.dst)[o] = f2bf(v);
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ci = mb + (r & 3) + 8 * (r >> 2);
                    if (ci >= p.SC) continue;
                    const size_t o = ((size_t)wtap * p.SC + ci) * p.DN + n;
                    float v = acc[mi][ni][r];
                    if (p.w && p.wd != 0.f) v += p.wd * p.w[o];
                    static_cast<float*>(p.dst)[o] = v;
                }
            }
        }
    }
}

// dbias = column sums of dy [P][C] in a fixed order: 16 row groups per 4 channels, combined in group order through LDS
template <typename T>
__global__ __launch_bounds__(256) void conv_bigk_bias_grad_kernel(const T* __restrict__ dy, int P, int C, float* __restrict__ db) {
    __shared__ f32x4 part[256];
    const int cq = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int c = (blockIdx.x * 16 + cq) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (c < C) {
        const T* col = dy + c;
        for (int m = g; m < P; m += 16) s += ld4t(col + (size_t)m * C);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (g == 0 && c < C) {
        f32x4 t = part[cq];
        for (int j = 1; j < 16; ++j) t += part[j * 16 + cq];
        *reinterpret_cast<f32x4*>(db + c) = t;
    }
}

// =================================================================================
// host side
// =================================================================================
bool conv_bigk(const ConvDesc& d) { return d.KH * d.KW > 9; }

static void check_bigk(const ConvDesc& d, int esize) {
    const int vec = 16 / esize;
    SSD_REQUIRE(d.stride == 1 && d.dil == 1 && d.Ho == d.Hi && d.Wo == d.Wi && d.pad_h >= 0 && d.pad_w >= 0 && d.pad_h < d.KH &&
                    d.pad_w < d.KW,
                "conv with %dx%d taps: stride 1 / dilation 1 / SAME only", d.KH, d.KW);
    SSD_REQUIRE(d.Ci % vec == 0 && d.Co % vec == 0, "conv with %dx%d taps: Ci and Co must be multiples of %d (got %d, %d)", d.KH, d.KW,
                vec, d.Ci, d.Co);
    // buffer descriptors and offsets are 32-bit byte quantities (0xFFFFFFF0 is the out-of-range sentinel)
    const long long lim = (1LL << 32) - 64;
    SSD_REQUIRE((long long)d.B * d.Hi * d.Wi * std::max(d.Ci, d.Co) * esize < lim && (long long)d.KH * d.KW * d.Ci * d.Co * esize < lim,
                "conv with %dx%d taps: a tensor of this layer exceeds 4 GiB (32-bit byte offsets): lower the batch", d.KH, d.KW);
}

static BigKArgs bigk_args(const ConvDesc& d, int esize) {
    BigKArgs a{};
    a.H = d.Ho; a.W = d.Wo; a.KH = d.KH; a.KW = d.KW; a.ph = d.pad_h; a.pw = d.pad_w;
    a.P = d.B * d.Ho * d.Wo;
    (void)esize;
    return a;
}

// n tile of the forward / data gradient: 128 unless the 64-wide tile fills the chip's rounds better (the data gradient of fc6 at
// vgg300 b32: 91 x 4 = 364 tiles of 128 are 1.4 rounds on 256 CUs, 728 tiles of 64 are 2.8); 64-wide tiles re-use their A tile
// over half the columns (efficiency 0.85, the bf16 kernels' measured ratio)
static int pick_bn(int P, int N, bool allow64) {
    if (!allow64) return 128;
    const long long t128 = (long long)cdiv(P, 128) * cdiv(N, 128), t64 = (long long)cdiv(P, 128) * cdiv(N, 64);
    const double c128 = (double)cdiv(t128, 256) * 128, c64 = (double)cdiv(t64, 256) * 64 / 0.85;
    return c64 < c128 * 0.999 ? 64 : 128;
}

template <int PASS, typename T, int TN>
static void launch_bigk(BigKArgs& a, const char* label, double flops, double bytes, hipStream_t s, bool stop_event) {
    constexpr size_t lds = 2 * (size_t)(128 + 64 * TN) * 144;
    static_assert(lds <= 160 * 1024, "LDS");
    auto kern = conv_bigk_kernel<PASS, T, TN>;
    static bool once = (set_lds(kern, lds), true);
    (void)once;
    ProfScope prof(label, flops, bytes, s);
    const dim3 grid(a.MT * a.NT);
    if (stop_event) SSD_LAUNCH_STOP(kern, grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
    HIP_OK(hipGetLastError());
}

// the work the kernels execute, padding taps included (conv_flops counts what the layer needs: every tap of every pixel -- the
// same number; the useful part excludes the products with SAME padding): 2 * pixels * Ci * Co * (taps that land inside the image)
double conv_bigk_useful_flops(const ConvDesc& d) {
    auto inside = [](int n, int k, int pad) {
        long long s = 0;
        for (int o = 0; o < n; ++o)
            for (int t = 0; t < k; ++t) s += (unsigned)(o + t - pad) < (unsigned)n;
        return s;
    };
    return 2.0 * d.B * (double)inside(d.Ho, d.KH, d.pad_h) * (double)inside(d.Wo, d.KW, d.pad_w) * d.Ci * d.Co;
}

template <typename T>
static void bigk_fwd(const ConvDesc& d, const T* x, const T* w, const float* bias, void* y, bool y_f32, bool relu, hipStream_t s) {
    constexpr bool F32 = sizeof(T) == 4;
    check_bigk(d, sizeof(T));
    BigKArgs a = bigk_args(d, sizeof(T));
    a.src = x; a.wgt = w; a.bias = bias; a.dst = y; a.relu = relu; a.out_f32 = y_f32;
    a.SC = d.Ci; a.DN = d.Co;
    a.src_bytes = (unsigned)((size_t)a.P * d.Ci * sizeof(T));
    a.wgt_bytes = (unsigned)((size_t)d.KH * d.KW * d.Ci * d.Co * sizeof(T));
    a.MT = cdiv(a.P, 128);
    const double fl = conv_flops(d), by = sizeof(T) * conv_elems(d);
    // the fp32 filter is staged through the register transpose, which is built for 128-wide tiles
    if constexpr (!F32) {
        if (pick_bn(a.P, d.Co, true) == 64) {
            a.NT = cdiv(d.Co, 64);
            launch_bigk<BIGK_FWD, T, 1>(a, "conv_bigk_fwd_bf16_128x64", fl, by, s, true);
            return;
        }
    }
    a.NT = cdiv(d.Co, 128);
    launch_bigk<BIGK_FWD, T, 2>(a, F32 ? "conv_bigk_fwd_128x128" : "conv_bigk_fwd_bf16_128x128", fl, by, s, true);
}

template <typename T>
static void bigk_dgrad(const ConvDesc& d, const T* dy, const T* w, T* dx, const T* mask, bool accumulate, hipStream_t s) {
    constexpr bool F32 = sizeof(T) == 4;
    check_bigk(d, sizeof(T));
    BigKArgs a = bigk_args(d, sizeof(T));
    a.src = dy; a.wgt = w; a.dst = dx; a.mask = mask; a.accum = accumulate;
    a.SC = d.Co; a.DN = d.Ci;
    a.src_bytes = (unsigned)((size_t)a.P * d.Co * sizeof(T));
    a.wgt_bytes = (unsigned)((size_t)d.KH * d.KW * d.Ci * d.Co * sizeof(T));
    a.MT = cdiv(a.P, 128);
    const double fl = conv_flops(d), by = sizeof(T) * conv_elems(d);
    if (pick_bn(a.P, d.Ci, true) == 64) {
        a.NT = cdiv(d.Ci, 64);
        launch_bigk<BIGK_DGRAD, T, 1>(a, F32 ? "conv_bigk_dgrad_128x64" : "conv_bigk_dgrad_bf16_128x64", fl, by, s, true);
    } else {
        a.NT = cdiv(d.Ci, 128);
        launch_bigk<BIGK_DGRAD, T, 2>(a, F32 ? "conv_bigk_dgrad_128x128" : "conv_bigk_dgrad_bf16_128x128", fl, by, s, true);
    }
}

template <typename T>
static void bigk_wgrad(const ConvDesc& d, const T* x, const T* dy, float* dw, float* dbias, const float* w, float weight_decay,
                       hipStream_t s) {
    constexpr bool F32 = sizeof(T) == 4;
    check_bigk(d, sizeof(T));
    BigKArgs a = bigk_args(d, sizeof(T));
    a.src = x; a.wgt = dy; a.dst = dw; a.w = w; a.wd = weight_decay;
    a.SC = d.Ci; a.DN = d.Co;
    a.src_bytes = (unsigned)((size_t)a.P * d.Ci * sizeof(T));
    a.wgt_bytes = (unsigned)((size_t)a.P * d.Co * sizeof(T));
    a.CT = cdiv(d.Ci, 128);
    a.MT = d.KH * d.KW * a.CT;
    a.NT = cdiv(d.Co, 128);
    const double fl = conv_flops(d), by = sizeof(T) * conv_elems(d);
    launch_bigk<BIGK_WGRAD, T, 2>(a, F32 ? "conv_bigk_wgrad_128x128" : "conv_bigk_wgrad_bf16_128x128", fl, by, s, false);
    if (dbias) {
        ProfScope prof(F32 ? "conv_bigk_bias_grad" : "conv_bigk_bias_grad_bf16", 0.0, (double)a.P * d.Co * sizeof(T), s);
        hipLaunchKernelGGL(conv_bigk_bias_grad_kernel<T>, dim3(cdiv(d.Co, 64)), dim3(256), 0, s, dy, a.P, d.Co, dbias);
        HIP_OK(hipGetLastError());
    }
}

void conv_bigk_fwd(const ConvDesc& d, const float* x, const float* w, const float* bias, float* y, bool relu, hipStream_t s) {
    bigk_fwd<float>(d, x, w, bias, y, true, relu, s);
}
void conv_bigk_dgrad(const ConvDesc& d, const float* dy, const float* w, float* dx, const float* mask, bool accumulate, hipStream_t s) {
    bigk_dgrad<float>(d, dy, w, dx, mask, accumulate, s);
}
void conv_bigk_wgrad(const ConvDesc& d, const float* x, const float* dy, float* dw, float* dbias, const float* w, float weight_decay,
                     hipStream_t s) {
    bigk_wgrad<float>(d, x, dy, dw, dbias, w, weight_decay, s);
}
void conv_bigk_fwd_bf16(const ConvDesc& d, const bf16_t* x, const bf16_t* w_oi, const float* bias, void* y, bool y_f32, bool relu,
                        hipStream_t s) {
    bigk_fwd<bf16_t>(d, x, w_oi, bias, y, y_f32, relu, s);
}
void conv_bigk_dgrad_bf16(const ConvDesc& d, const bf16_t* dy, const bf16_t* w_io, bf16_t* dx, const bf16_t* mask, bool accumulate,
                          hipStream_t s) {
    bigk_dgrad<bf16_t>(d, dy, w_io, dx, mask, accumulate, s);
}
void conv_bigk_wgrad_bf16(const ConvDesc& d, const bf16_t* x, const bf16_t* dy, float* dw, float* dbias, const float* w,
                          float weight_decay, hipStream_t s) {
    bigk_wgrad<bf16_t>(d, x, dy, dw, dbias, w, weight_decay, s);
}

}  // namespace ssd
