// mxfp8 inference kernels for gfx950 (MI355X): conv_fp8.hip's forward gather convolution with the pixel operand's E8M0 block scales
// fed to v_mfma_scale_f32_32x32x64_f8f6f4, and the producers of the format: the epilogue, a stand-alone quantiser and max-pooling.
// DESIGN.md 20; the form for more than 9 taps (the fc graph's 7 x 7 fc6): DESIGN.md 21.
//
// Format: an activation tensor is codes uint8 [B][H][W][C] (OCP e4m3fn) + scales uint8 [B][H][W][C / 32] (E8M0, byte e = 2^(e - 127)),
// one scale per pixel and 32 consecutive channels.  (The hardware's scale byte of lane l does NOT cover that lane's own 32 values in
// the operand layout of conv_fp8.hip: tools/probes/mxfp8_probe.hip pins what it covers, and the kernel assigns channels to lanes
// accordingly -- see the fragment loads.)  Scale rule on the bits of the block's fp32
// absmax a (E = unbiased exponent, m = mantissa bits): x = clamp(E - 8 + (m > 0x600000), -127, 127), the smallest power of two with
// a / 2^x <= 448 = 1.75 * 2^8; byte x + 127 (an all-zero block: byte 0, what a padded tap's zero fill also holds); codes =
// RNE(clamp(ldexp(v, -x), -448, 448)).  Filters stay as in conv_fp8.hip: e4m3 [tap][Co][Ci], one fp32 scale per output channel, block
// scale 2^0.  Epilogue: y = relu?(acc * s_w[co] + bias[co]) in fp32.
#include "conv.h"
#include "conv_detail.h"
#include "conv_fp8_detail.h"
#include "bf16.h"
#include "ops.h"
#include <algorithm>

namespace ssd {

// the scale rule: fp32 absmax (>= 0) -> x in -127 ... 127.  Non-finite input gives 120 / 121: no byte 255, no fault
__device__ __forceinline__ int mx_exponent(float amax) {
    const unsigned u = __float_as_uint(amax);
    const int x = (int)(u >> 23) - 127 - 8 + ((u & 0x7FFFFFu) > 0x600000u ? 1 : 0);
    return x < -127 ? -127 : x > 127 ? 127 : x;
}
// a code's value, by the format's definition (exact; the NaN codes read as 480: outside the contract)
__device__ __forceinline__ float dec_e4m3(unsigned c) {
    const unsigned e = (c >> 3) & 15u, m = c & 7u;
    const float a = e ? __uint_as_float(((e + 120u) << 23) | (m << 20)) : (float)m * 0.001953125f;
    return (c & 0x80u) ? -a : a;
}
// a thread's 8 values of a 32-channel block held by 4 adjacent lanes -> the block's exponent; every lane of the four gets it
__device__ __forceinline__ int mx_block_exponent(const float (&v)[8]) {
    float am = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf(v[e]));
    am = fmaxf(am, __shfl_xor(am, 1, 64));
    am = fmaxf(am, __shfl_xor(am, 2, 64));
    return mx_exponent(am);
}
__device__ __forceinline__ u32x2 mx_pack8(const float (&v)[8], int x) {
    return u32x2{pack4_e4m3(ldexpf(v[0], -x), ldexpf(v[1], -x), ldexpf(v[2], -x), ldexpf(v[3], -x)),
                 pack4_e4m3(ldexpf(v[4], -x), ldexpf(v[5], -x), ldexpf(v[6], -x), ldexpf(v[7], -x))};
}

struct GatherArgsMX {
    const unsigned char* src;      // e4m3 [B][SH][SW][SC]
    const unsigned char* src_sc;   // E8M0 [B][SH][SW][SC / 32], from the dword boundary sc_delta bytes in front of it
    const unsigned char* wgt;      // e4m3 [tap][DN][SC]
    const float* bias;             // [DN] or nullptr
    const float* s_w;              // [DN] filter scales
    void* dst;                     // bf16 or fp32 [M][DN] (modes 0, 1, 3)
    unsigned char* dst8;           // e4m3 [M][DN] (modes 2, 3)
    unsigned char* dst_sc;         // E8M0 [M][DN / 32] (modes 2, 3)
    int M, DH, DW, DN;
    int SH, SW, SC;
    int ntaps, mul, relu, mode, NT, sc_delta;
    int tap_dh[9], tap_dw[9];
};

// conv_fwd_fp8_kernel with one more staged item per stage: a dword per thread, of which the first BM hold the pixel rows' scale bytes.
// The two bytes a tile row needs for chunk cc sit at byte pixel * (SC / 32) + 2 cc of the scale buffer, an even address: thread r < BM
// fetches the aligned dword around row r's with one 4-byte LDS-DMA (zeros for a padded tap or a row past M, like the codes); threads
// BM ... fetch zeros from the out-of-range offset, so that every wave issues the same number of DMA instructions per stage -- the wait
// in front of a stage counts them in vmcnt.  The lane that multiplies row r shifts the dword to its byte: (address & 3) + (lane >> 5).
template <int WM, int WN, int TM, int TN, int NS>
__global__ __launch_bounds__(64 * WM * WN) void conv_fwd_mxfp8_kernel(GatherArgsMX pp) {
    const GatherArgsMX& p = pp;
    constexpr int NTHR = 64 * WM * WN;
    constexpr int RPP_S = NTHR / 4;                   // tile rows one staging pass covers (4 lanes per 64-byte row)
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int A_N = BM / RPP_S, B_N = BN / RPP_S; // DMA instructions per thread and tile
    constexpr int CODES = (BM + BN) * KB8;
    constexpr int STAGE = CODES + NTHR * 4;           // + the scale dwords
    constexpr int LDC = BN + 4;
    static_assert(BM % RPP_S == 0 && BN % RPP_S == 0 && RPP_S % 16 == 0 && BM <= NTHR, "tile vs staging pass");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = wg / p.NT, nt = wg - mt * p.NT;
    const int m0 = mt * BM, n0 = nt * BN;
    const int SB = p.SC >> 5;                         // scale bytes per pixel (even: SC is a multiple of 64)

    // output row -> its pixel at tap (0, 0), in pixels of the source
    auto pixel_of = [&](int m, int& rh, int& rw) {
        const int ow = m % p.DW;
        const int t2 = m / p.DW;
        const int oh = t2 % p.DH;
        const int b = t2 / p.DH;
        rh = oh * p.mul;
        rw = ow * p.mul;
        return b * p.SH * p.SW + rh * p.SW + rw;
    };
    auto tap_mask = [&](int rh, int rw) {
        unsigned mk = 0;
        for (int t = 0; t < p.ntaps; ++t) {
            const int sh = rh + p.tap_dh[t], sw = rw + p.tap_dw[t];
            if ((unsigned)sh < (unsigned)p.SH && (unsigned)sw < (unsigned)p.SW) mk |= 1u << t;
        }
        return mk;
    };

    // ---- staging: thread -> rows (tid >> 2) + RPP_S i, LDS slot tid & 3, global chunk slot ^ ((row >> 2) & 3)
    const int a_ck = ((tid & 3) ^ ((tid >> 4) & 3)) * 16;
    unsigned a_off[A_N], a_msk[A_N];
#pragma unroll
    for (int i = 0; i < A_N; ++i) {
        const int m = m0 + (tid >> 2) + RPP_S * i;
        int rh, rw;
        const int pix = pixel_of(m < p.M ? m : 0, rh, rw);
        a_off[i] = (unsigned)(pix * p.SC + a_ck);
        a_msk[i] = m < p.M ? tap_mask(rh, rw) : 0u;
    }
    unsigned b_off[B_N], b_ok[B_N];
#pragma unroll
    for (int i = 0; i < B_N; ++i) {
        const int n = n0 + (tid >> 2) + RPP_S * i;
        b_ok[i] = 0u - (unsigned)(n < p.DN);
        b_off[i] = (unsigned)((n < p.DN ? n : 0) * p.SC + a_ck);
    }
    // ... and the scale dword of tile row tid
    unsigned s_off = 0, s_msk = 0;
    if (tid < BM && m0 + tid < p.M) {
        int rh, rw;
        s_off = (unsigned)(pixel_of(m0 + tid, rh, rw) * SB + p.sc_delta);
        s_msk = tap_mask(rh, rw);
    }
    const size_t src_pixels = (size_t)(p.M / (p.DH * p.DW)) * p.SH * p.SW;
    const __amdgpu_buffer_rsrc_t src_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.src), 0, (unsigned)(src_pixels * p.SC), 0x00020000);
    // (rounded up to whole dwords: the last pixel's dword may end two bytes behind the tensor, inside its allocation -- conv.h)
    const __amdgpu_buffer_rsrc_t sc_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.src_sc), 0, (unsigned)((src_pixels * SB + p.sc_delta + 3) & ~(size_t)3), 0x00020000);
    const __amdgpu_buffer_rsrc_t wgt_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.wgt), 0, (unsigned)((size_t)p.ntaps * p.DN * p.SC), 0x00020000);

    const int nk = (p.SC / KB8) * p.ntaps;      // SC is a multiple of 64 (host check): no channel-chunk mask

    auto issue = [&](int kiter, int stage) {
        const int cc = kiter / p.ntaps;
        const int tap = kiter - cc * p.ntaps;
        unsigned char* As = smem + stage * STAGE + wave * 1024;        // wave-uniform: 16 rows x 64 B per DMA
        unsigned char* Bs = As + BM * KB8;
        const int tpix = p.tap_dh[tap] * p.SW + p.tap_dw[tap];
        const unsigned toff = (unsigned)(tpix * p.SC + cc * KB8);
#pragma unroll
        for (int i = 0; i < A_N; ++i) {
            const unsigned m = 0u - ((a_msk[i] >> tap) & 1u);
            const unsigned off = ((a_off[i] + toff) & m) | (OOB8 & ~m);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rsrc, LDS_PTR8(As + i * (RPP_S * KB8)), 16, off, 0, 0, 0);
        }
        const unsigned woff = (unsigned)(tap * p.DN * p.SC + cc * KB8);
#pragma unroll
        for (int i = 0; i < B_N; ++i) {
            const unsigned m = b_ok[i];
            const unsigned off = ((b_off[i] + woff) & m) | (OOB8 & ~m);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wgt_rsrc, LDS_PTR8(Bs + i * (RPP_S * KB8)), 16, off, 0, 0, 0);
        }
        {
            const unsigned m = 0u - ((s_msk >> tap) & 1u);
            const unsigned off = ((s_off + (unsigned)(tpix * SB + 2 * cc)) & ~3u & m) | (OOB8 & ~m);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(sc_rsrc, LDS_PTR8(smem + stage * STAGE + CODES + wave * 256), 4, off, 0, 0, 0);
        }
    };

    // ---- accumulators: D rows = output channels (filter operand first), D cols = pixels, as in conv_bf16.hip
    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int wm = wave / WN, wn = wave - wm * WN;
    const int li = lane & 31, lh = lane >> 5;
    // fragment = chunks lh and lh + 2 of row li (not conv_fp8.hip's 2 lh and 2 lh + 1): the scale byte of lane li + 32 h multiplies
    // registers 4 h ... 4 h + 3 of BOTH lanes li and li + 32 (mxfp8_probe), so with this assignment -- the same for the filter operand,
    // a dot product does not care -- those 32 values are the 32 consecutive channels 32 h ... 32 h + 31 of the chunk pair, one block.
    // Slots lh ^ f and lh ^ f ^ 2, f = (row >> 2) & 3 = (li >> 2) & 3; a ds_read_b128 lane group (16 rows of one lh) still covers the
    // 16 units of its bank line.
    const int q0 = (lh ^ ((li >> 2) & 3)) * 16;
    const int a_row = (wm * 32 * TM + li) * KB8 + q0;
    const int b_row = BM * KB8 + (wn * 32 * TN + li) * KB8 + q0;
    // byte of this lane's scale inside its row's dword = (scale address & 3) + lh; the row's share of the address, mod 4:
    unsigned s_rb[TM];
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
        const int m = m0 + wm * 32 * TM + mi * 32 + li;
        int rh, rw;
        s_rb[mi] = (unsigned)(pixel_of(m < p.M ? m : 0, rh, rw) * SB + p.sc_delta);
    }

    auto load_frag = [&](const unsigned char* S, int addr) -> i32x8 {
        const i32x4 lo = *reinterpret_cast<const i32x4*>(S + addr);
        const i32x4 hi = *reinterpret_cast<const i32x4*>(S + (addr ^ 32));
        return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    int c_cc = 0, c_tap = 0;      // the tile being multiplied, wave-uniform
    auto compute = [&](int stage) {
        const unsigned char* S = smem + stage * STAGE;
        const unsigned* Sc = reinterpret_cast<const unsigned*>(S + CODES);
        const unsigned s_tb = (unsigned)((p.tap_dh[c_tap] * p.SW + p.tap_dw[c_tap]) * SB + 2 * c_cc);
        i32x8 a[TM], b[TN];
        int sa[TM];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            a[mi] = load_frag(S, a_row + mi * 32 * KB8);
            sa[mi] = (int)(Sc[wm * 32 * TM + mi * 32 + li] >> (8 * (((s_rb[mi] + s_tb) & 3u) + lh)));
        }
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) b[ni] = load_frag(S, b_row + ni * 32 * KB8);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b[ni], a[mi], acc[mi][ni], 0, 0, 0, SCALE_ONE, 0, sa[mi]);
        if (++c_tap == p.ntaps) {
            c_tap = 0;
            ++c_cc;
        }
    };

    // ---- main loop: NS stages; tiles k+1 .. k+NS-1 stream in while tile k is multiplied
#pragma unroll
    for (int t = 0; t < NS - 1; ++t)
        if (t < nk) issue(t, t);
    int st_c = 0, st_i = NS - 1;
    for (int k = 0; k < nk; ++k) {
        const int later = nk - 1 - k;
        wait_tiles_and_sync8<A_N + B_N + 1, (NS - 2 > 4 ? 4 : NS - 2)>(later < NS - 2 ? later : NS - 2);      // tile k visible; stage st_i is free
        if (k + NS - 1 < nk) issue(k + NS - 1, st_i);
        compute(st_c);
        st_c = st_c + 1 == NS ? 0 : st_c + 1;
        st_i = st_i + 1 == NS ? 0 : st_i + 1;
    }
    __syncthreads();

    // ---- epilogue through an fp32 LDS tile [BM][BN + 4]: filter scale, bias, relu, one rounding per output format
    float* Cs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ml = wm * 32 * TM + mi * 32 + li;
                const int nl = wn * 32 * TN + ni * 32 + 8 * g + 4 * lh;
                const f32x16& c = acc[mi][ni];
                *reinterpret_cast<f32x4*>(Cs + ml * LDC + nl) = f32x4{c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]};
            }
    __syncthreads();
    constexpr int TPR = BN / 8;               // threads per row, 8 channels each: a 32-channel block is 4 adjacent lanes
    constexpr int RPP = NTHR / TPR;           // rows per pass
    static_assert(TPR % 4 == 0, "a block's four lanes share a row");
    const int cg = tid % TPR, r0 = tid / TPR;
    const int n = n0 + cg * 8;
    if (n >= p.DN) return;                    // (an MX output has DN % 32 == 0: the four lanes of a block leave or stay together)
    float sc[8], bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sc[e] = p.s_w[n + e];
        bv[e] = p.bias ? p.bias[n + e] : 0.f;
    }
#pragma unroll
    for (int ps = 0; ps < BM / RPP; ++ps) {
        const int ml = r0 + ps * RPP;
        const int m = m0 + ml;
        if (m >= p.M) continue;               // (the same m for the four lanes of a block)
        const size_t o = (size_t)m * p.DN + n;
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(Cs + ml * LDC + cg * 8);
        const f32x4 c1 = *reinterpret_cast<const f32x4*>(Cs + ml * LDC + cg * 8 + 4);
        float v[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[e] = v[e] * sc[e] + bv[e];
            if (p.relu) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        if (p.mode == FP8_OUT_F32) {
            float* d = reinterpret_cast<float*>(p.dst) + o;
            *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(d + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else if (p.mode != FP8_OUT_MX) {
            *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(p.dst) + o) =
                u32x4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
        }
        if (p.mode == FP8_OUT_MX || p.mode == FP8_OUT_BF16_MX) {
            const int x = mx_block_exponent(v);
            *reinterpret_cast<u32x2*>(p.dst8 + o) = mx_pack8(v, x);
            if ((cg & 3) == 0) p.dst_sc[(size_t)m * (p.DN >> 5) + (n >> 5)] = (unsigned char)(x + 127);
        }
    }
}

template <int WM, int WN, int TM, int TN, int NS>
static void launch_fwd_mx(GatherArgsMX& a, const char* label, double flops, double bytes, hipStream_t s) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr size_t stages = NS * ((size_t)(BM + BN) * KB8 + 64 * WM * WN * 4), ctile = (size_t)BM * (BN + 4) * 4;
    constexpr size_t lds = stages > ctile ? stages : ctile;
    static_assert(lds <= 80 * 1024, "LDS: two workgroups per CU");
    auto kern = conv_fwd_mxfp8_kernel<WM, WN, TM, TN, NS>;
    static bool once = (set_lds(kern, lds), true);
    (void)once;
    a.NT = cdiv(a.DN, BN);
    ProfScope prof(label, flops, bytes, s);
    SSD_LAUNCH_STOP(kern, dim3(cdiv(a.M, BM) * a.NT), dim3(64 * WM * WN), lds, s, a);
    HIP_OK(hipGetLastError());
}

// Tiles as in conv_fwd_fp8: 0 = 128 x 128 with four stages, 1 = 64 x 64 with six; SSD_TILE_FP8 forces one.
void conv_fwd_mxfp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* xs, const unsigned char* w8, const float* s_w,
                    const float* bias, void* y, unsigned char* y8, unsigned char* ys, int out_mode, bool relu, hipStream_t s) {
    const char* why = nullptr;
    if (!conv_fwd_fp8_supported(d, &why))      // the same eligibility; the reason text without its "fp8 conv: "
        SSD_REQUIRE(false, "mxfp8 conv: %s (got %dx%d taps, Ci %d, Co %d)", why + 10, d.KH, d.KW, d.Ci, d.Co);
    SSD_REQUIRE(out_mode == FP8_OUT_BF16 || out_mode == FP8_OUT_F32 || out_mode == FP8_OUT_MX || out_mode == FP8_OUT_BF16_MX,
                "mxfp8 conv: unknown output mode %d", out_mode);
    const bool wants8 = out_mode == FP8_OUT_MX || out_mode == FP8_OUT_BF16_MX;
    SSD_REQUIRE(!wants8 || d.Co % 32 == 0, "mxfp8 conv: an MX output needs Co to be a multiple of 32 (got %d)", d.Co);
    SSD_REQUIRE(!wants8 || (y8 != nullptr && ys != nullptr), "mxfp8 conv: an MX output needs its code and scale buffers");
    SSD_REQUIRE(out_mode == FP8_OUT_MX || y != nullptr, "mxfp8 conv: null output");
    SSD_REQUIRE(x8 && xs && w8 && s_w, "mxfp8 conv: null operand");
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(xs) % 2 == 0, "mxfp8 conv: the scale buffer must start at an even address");
    GatherArgsMX a{};
    a.sc_delta = (int)(reinterpret_cast<uintptr_t>(xs) & 3);      // (a sample's scales inside a batch may start between two dwords)
    a.src = x8; a.src_sc = xs - a.sc_delta; a.wgt = w8; a.bias = bias; a.s_w = s_w; a.dst = y; a.dst8 = y8; a.dst_sc = ys;
    a.M = d.B * d.Ho * d.Wo; a.DH = d.Ho; a.DW = d.Wo; a.DN = d.Co;
    a.SH = d.Hi; a.SW = d.Wi; a.SC = d.Ci;
    a.ntaps = d.KH * d.KW; a.mul = d.stride; a.relu = relu; a.mode = out_mode;
    for (int kh = 0; kh < d.KH; ++kh)
        for (int kw = 0; kw < d.KW; ++kw) {
            a.tap_dh[kh * d.KW + kw] = kh * d.dil - d.pad_h;
            a.tap_dw[kh * d.KW + kw] = kw * d.dil - d.pad_w;
        }
    const double fl = conv_flops(d);
    const double out_b = out_mode == FP8_OUT_F32 ? 4.0 : out_mode == FP8_OUT_BF16 ? 2.0 : (out_mode == FP8_OUT_MX ? 1.0 : 3.0) + 1.0 / 32;
    const double by = (double)d.B * d.Hi * d.Wi * d.Ci * (1.0 + 1.0 / 32) + (double)d.KH * d.KW * d.Ci * d.Co + (double)d.B * d.Ho * d.Wo * d.Co * out_b;
    int cfg = env_int("SSD_TILE_FP8", -1);
    if (cfg != 0 && cfg != 1) cfg = (long long)cdiv(a.M, 128) * cdiv(a.DN, 128) <= 256 ? 1 : 0;
    if (cfg == 0) launch_fwd_mx<2, 2, 2, 2, 4>(a, "conv_fwd_mxfp8_128x128", fl, by, s);
    else launch_fwd_mx<2, 2, 1, 1, 6>(a, "conv_fwd_mxfp8_64x64x6", fl, by, s);
}

// =================================================================================
// More than 9 taps (the fc graph's 7 x 7 fc6): conv_bigk_fwd_fp8_kernel's tap walk -- the tap's offset computed from the
// wave-uniform counters (i_cc, i_kh, i_kw) when its tile is issued, the separable validity mask (bit kh: kernel row kh lands on an image
// row, bit 16 + kw: kernel column kw lands on an image column), pixel tiles fastest in the workgroup order -- joined with
// conv_fwd_mxfp8_kernel's scale dword per thread and stage, fragment order and MX epilogue.  The scale row takes the code rows' mask
// and `sel`: the dword of a padded tap is zeros (byte 0 x code 0 = +0).  The multiply side runs NS - 1 tiles behind the issue side and
// keeps counters (c_cc, c_kh, c_kw) of its own for the tap's share of the scale address mod 4.  The existing kernels are left as they
// are: their instantiations' code does not change.
// =================================================================================
struct GatherArgsMXK {
    const unsigned char* src;      // e4m3 [B][SH][SW][SC]
    const unsigned char* src_sc;   // E8M0 [B][SH][SW][SC / 32], from the dword boundary sc_delta bytes in front of it
    const unsigned char* wgt;      // e4m3 [tap][DN][SC]
    const float* bias;             // [DN] or nullptr
    const float* s_w;              // [DN] filter scales
    void* dst;                     // bf16 or fp32 [M][DN] (modes 0, 1, 5)
    unsigned char* dst8;           // e4m3 [M][DN] (modes 4, 5)
    unsigned char* dst_sc;         // E8M0 [M][DN / 32] (modes 4, 5)
    int M, DH, DW, DN;
    int SH, SW, SC;
    int KH, KW, dil, pad_h, pad_w;
    int mul, relu, mode, MT, sc_delta;
};

template <int WM, int WN, int TM, int TN, int NS>
__global__ __launch_bounds__(64 * WM * WN) void conv_bigk_fwd_mxfp8_kernel(GatherArgsMXK pp) {
    const GatherArgsMXK& p = pp;
    constexpr int NTHR = 64 * WM * WN;
    constexpr int RPP_S = NTHR / 4;                   // tile rows one staging pass covers (4 lanes per 64-byte row)
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int A_N = BM / RPP_S, B_N = BN / RPP_S; // DMA instructions per thread and tile
    constexpr int CODES = (BM + BN) * KB8;
    constexpr int STAGE = CODES + NTHR * 4;           // + the scale dwords
    constexpr int LDC = BN + 4;
    static_assert(BM % RPP_S == 0 && BN % RPP_S == 0 && RPP_S % 16 == 0 && BM <= NTHR, "tile vs staging pass");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    // pixel tiles fastest: the workgroups resident on an XCD stream the same filter rows through its L2 (conv_fp8.hip launch_fwd8k)
    const int nt = wg / p.MT, mt = wg - nt * p.MT;
    const int m0 = mt * BM, n0 = nt * BN;
    const int SB = p.SC >> 5;                         // scale bytes per pixel (even: SC is a multiple of 64)

    // output row -> its pixel at tap (0, 0), in pixels of the source
    auto pixel_of = [&](int m, int& rh, int& rw) {
        const int ow = m % p.DW;
        const int t2 = m / p.DW;
        const int oh = t2 % p.DH;
        const int b = t2 / p.DH;
        rh = oh * p.mul;
        rw = ow * p.mul;
        return b * p.SH * p.SW + rh * p.SW + rw;
    };
    auto row_col_mask = [&](int rh, int rw) {
        unsigned mk = 0;
        for (int kh = 0; kh < p.KH; ++kh)
            if ((unsigned)(rh + kh * p.dil - p.pad_h) < (unsigned)p.SH) mk |= 1u << kh;
        for (int kw = 0; kw < p.KW; ++kw)
            if ((unsigned)(rw + kw * p.dil - p.pad_w) < (unsigned)p.SW) mk |= 0x10000u << kw;
        return mk;
    };

    // ---- staging: thread -> rows (tid >> 2) + RPP_S i, LDS slot tid & 3, global chunk slot ^ ((row >> 2) & 3)
    const int a_ck = ((tid & 3) ^ ((tid >> 4) & 3)) * 16;
    unsigned a_off[A_N], a_msk[A_N];
#pragma unroll
    for (int i = 0; i < A_N; ++i) {
        const int m = m0 + (tid >> 2) + RPP_S * i;
        int rh, rw;
        const int pix = pixel_of(m < p.M ? m : 0, rh, rw);
        a_off[i] = (unsigned)(pix * p.SC + a_ck);
        a_msk[i] = m < p.M ? row_col_mask(rh, rw) : 0u;
    }
    unsigned b_off[B_N], b_ok[B_N];
#pragma unroll
    for (int i = 0; i < B_N; ++i) {
        const int n = n0 + (tid >> 2) + RPP_S * i;
        b_ok[i] = 0u - (unsigned)(n < p.DN);
        b_off[i] = (unsigned)((n < p.DN ? n : 0) * p.SC + a_ck);
    }
    // ... and the scale dword of tile row tid (threads BM ... and rows past M: mask 0, the out-of-range offset)
    unsigned s_off = 0, s_msk = 0;
    if (tid < BM && m0 + tid < p.M) {
        int rh, rw;
        s_off = (unsigned)(pixel_of(m0 + tid, rh, rw) * SB + p.sc_delta);
        s_msk = row_col_mask(rh, rw);
    }
    const size_t src_pixels = (size_t)(p.M / (p.DH * p.DW)) * p.SH * p.SW;
    const __amdgpu_buffer_rsrc_t src_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.src), 0, (unsigned)(src_pixels * p.SC), 0x00020000);
    // (rounded up to whole dwords: the last pixel's dword may end two bytes behind the tensor, inside its allocation -- conv.h)
    const __amdgpu_buffer_rsrc_t sc_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.src_sc), 0, (unsigned)((src_pixels * SB + p.sc_delta + 3) & ~(size_t)3), 0x00020000);
    const __amdgpu_buffer_rsrc_t wgt_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.wgt), 0,
                                                                              (unsigned)((size_t)p.KH * p.KW * p.DN * p.SC), 0x00020000);

    const int nk = (p.SC / KB8) * p.KH * p.KW;      // SC is a multiple of 64 (host check): no channel-chunk mask

    // tiles are issued in k order, taps inside a channel chunk: (i_cc, i_kh, i_kw) is the next one, wave-uniform
    int i_cc = 0, i_kh = 0, i_kw = 0;
    auto issue_next = [&](int stage) {
        unsigned char* As = smem + stage * STAGE + wave * 1024;        // wave-uniform: 16 rows x 64 B per DMA
        unsigned char* Bs = As + BM * KB8;
        const int tpix = (i_kh * p.dil - p.pad_h) * p.SW + (i_kw * p.dil - p.pad_w);
        const unsigned toff = (unsigned)(tpix * p.SC + i_cc * KB8);
        const unsigned sel = (1u << i_kh) | (0x10000u << i_kw);
#pragma unroll
        for (int i = 0; i < A_N; ++i) {
            const unsigned m = 0u - (unsigned)((a_msk[i] & sel) == sel);
            const unsigned off = ((a_off[i] + toff) & m) | (OOB8 & ~m);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rsrc, LDS_PTR8(As + i * (RPP_S * KB8)), 16, off, 0, 0, 0);
        }
        const unsigned woff = (unsigned)((i_kh * p.KW + i_kw) * p.DN * p.SC + i_cc * KB8);
#pragma unroll
        for (int i = 0; i < B_N; ++i) {
            const unsigned m = b_ok[i];
            const unsigned off = ((b_off[i] + woff) & m) | (OOB8 & ~m);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wgt_rsrc, LDS_PTR8(Bs + i * (RPP_S * KB8)), 16, off, 0, 0, 0);
        }
        {
            const unsigned m = 0u - (unsigned)((s_msk & sel) == sel);
            const unsigned off = ((s_off + (unsigned)(tpix * SB + 2 * i_cc)) & ~3u & m) | (OOB8 & ~m);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(sc_rsrc, LDS_PTR8(smem + stage * STAGE + CODES + wave * 256), 4, off, 0, 0, 0);
        }
        if (++i_kw == p.KW) {
            i_kw = 0;
            if (++i_kh == p.KH) {
                i_kh = 0;
                ++i_cc;
            }
        }
    };

    // ---- accumulators: D rows = output channels (filter operand first), D cols = pixels, as in conv_fwd_mxfp8_kernel
    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int wm = wave / WN, wn = wave - wm * WN;
    const int li = lane & 31, lh = lane >> 5;
    // fragment = chunks lh and lh + 2 of row li, for both operands (conv_fwd_mxfp8_kernel: what the hardware's scale byte covers)
    const int q0 = (lh ^ ((li >> 2) & 3)) * 16;
    const int a_row = (wm * 32 * TM + li) * KB8 + q0;
    const int b_row = BM * KB8 + (wn * 32 * TN + li) * KB8 + q0;
    // byte of this lane's scale inside its row's dword = (scale address & 3) + lh; the row's share of the address, mod 4:
    unsigned s_rb[TM];
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
        const int m = m0 + wm * 32 * TM + mi * 32 + li;
        int rh, rw;
        s_rb[mi] = (unsigned)(pixel_of(m < p.M ? m : 0, rh, rw) * SB + p.sc_delta);
    }

    auto load_frag = [&](const unsigned char* S, int addr) -> i32x8 {
        const i32x4 lo = *reinterpret_cast<const i32x4*>(S + addr);
        const i32x4 hi = *reinterpret_cast<const i32x4*>(S + (addr ^ 32));
        return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    // the tile being multiplied, NS - 1 behind the issue side, wave-uniform; its share of the scale address is negative for leading
    // taps: the sum is taken mod 4 in unsigned arithmetic (2^32 is a multiple of 4)
    int c_cc = 0, c_kh = 0, c_kw = 0;
    auto compute = [&](int stage) {
        const unsigned char* S = smem + stage * STAGE;
        const unsigned* Sc = reinterpret_cast<const unsigned*>(S + CODES);
        const unsigned s_tb = (unsigned)(((c_kh * p.dil - p.pad_h) * p.SW + (c_kw * p.dil - p.pad_w)) * SB + 2 * c_cc);
        i32x8 a[TM], b[TN];
        int sa[TM];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            a[mi] = load_frag(S, a_row + mi * 32 * KB8);
            sa[mi] = (int)(Sc[wm * 32 * TM + mi * 32 + li] >> (8 * (((s_rb[mi] + s_tb) & 3u) + lh)));
        }
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) b[ni] = load_frag(S, b_row + ni * 32 * KB8);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b[ni], a[mi], acc[mi][ni], 0, 0, 0, SCALE_ONE, 0, sa[mi]);
        if (++c_kw == p.KW) {
            c_kw = 0;
            if (++c_kh == p.KH) {
                c_kh = 0;
                ++c_cc;
            }
        }
    };

    // ---- main loop: NS stages; tiles k+1 .. k+NS-1 stream in while tile k is multiplied
#pragma unroll
    for (int t = 0; t < NS - 1; ++t)
        if (t < nk) issue_next(t);
    int st_c = 0, st_i = NS - 1;
    for (int k = 0; k < nk; ++k) {
        const int later = nk - 1 - k;
        wait_tiles_and_sync8<A_N + B_N + 1, (NS - 2 > 4 ? 4 : NS - 2)>(later < NS - 2 ? later : NS - 2);      // tile k visible; stage st_i is free
        if (k + NS - 1 < nk) issue_next(st_i);
        compute(st_c);
        st_c = st_c + 1 == NS ? 0 : st_c + 1;
        st_i = st_i + 1 == NS ? 0 : st_i + 1;
    }
    __syncthreads();

    // ---- epilogue through an fp32 LDS tile [BM][BN + 4], as in conv_fwd_mxfp8_kernel: filter scale, bias, relu, one rounding per format
    float* Cs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ml = wm * 32 * TM + mi * 32 + li;
                const int nl = wn * 32 * TN + ni * 32 + 8 * g + 4 * lh;
                const f32x16& c = acc[mi][ni];
                *reinterpret_cast<f32x4*>(Cs + ml * LDC + nl) = f32x4{c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]};
            }
    __syncthreads();
    constexpr int TPR = BN / 8;               // threads per row, 8 channels each: a 32-channel block is 4 adjacent lanes
    constexpr int RPP = NTHR / TPR;           // rows per pass
    static_assert(TPR % 4 == 0, "a block's four lanes share a row");
    const int cg = tid % TPR, r0 = tid / TPR;
    const int n = n0 + cg * 8;
    if (n >= p.DN) return;                    // (an MX output has DN % 32 == 0: the four lanes of a block leave or stay together)
    float sc[8], bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sc[e] = p.s_w[n + e];
        bv[e] = p.bias ? p.bias[n + e] : 0.f;
    }
#pragma unroll
    for (int ps = 0; ps < BM / RPP; ++ps) {
        const int ml = r0 + ps * RPP;
        const int m = m0 + ml;
        if (m >= p.M) continue;               // (the same m for the four lanes of a block)
        const size_t o = (size_t)m * p.DN + n;
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(Cs + ml * LDC + cg * 8);
        const f32x4 c1 = *reinterpret_cast<const f32x4*>(Cs + ml * LDC + cg * 8 + 4);
        float v[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[e] = v[e] * sc[e] + bv[e];
            if (p.relu) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        if (p.mode == FP8_OUT_F32) {
            float* d = reinterpret_cast<float*>(p.dst) + o;
            *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(d + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else if (p.mode != FP8_OUT_MX) {
            *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(p.dst) + o) =
                u32x4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
        }
        if (p.mode == FP8_OUT_MX || p.mode == FP8_OUT_BF16_MX) {
            const int x = mx_block_exponent(v);
            *reinterpret_cast<u32x2*>(p.dst8 + o) = mx_pack8(v, x);
            if ((cg & 3) == 0) p.dst_sc[(size_t)m * (p.DN >> 5) + (n >> 5)] = (unsigned char)(x + 127);
        }
    }
}

template <int WM, int WN, int TM, int TN, int NS>
static void launch_fwd_mxk(GatherArgsMXK& a, const char* label, double flops, double bytes, hipStream_t s) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr size_t stages = NS * ((size_t)(BM + BN) * KB8 + 64 * WM * WN * 4), ctile = (size_t)BM * (BN + 4) * 4;
    constexpr size_t lds = stages > ctile ? stages : ctile;
    static_assert(lds <= 80 * 1024, "LDS: two workgroups per CU");
    auto kern = conv_bigk_fwd_mxfp8_kernel<WM, WN, TM, TN, NS>;
    static bool once = (set_lds(kern, lds), true);
    (void)once;
    a.MT = cdiv(a.M, BM);      // pixel tiles fastest (the kernel)
    ProfScope prof(label, flops, bytes, s);
    SSD_LAUNCH_STOP(kern, dim3(a.MT * cdiv(a.DN, BN)), dim3(64 * WM * WN), lds, s, a);
    HIP_OK(hipGetLastError());
}

static bool wants_mx(int out_mode) { return out_mode == FP8_OUT_MX || out_mode == FP8_OUT_BF16_MX; }

// conv_bigk_fwd_fp8_supported's shapes; an MX output needs whole 32-channel blocks, and the scale tensors stay below the offset guard too
bool conv_bigk_fwd_mxfp8_supported(const ConvDesc& d, int out_mode, const char** why) {
    const char* w = nullptr;
    const long long taps = (long long)d.KH * d.KW;
    if (d.KH < 1 || d.KW < 1 || d.KH > 11 || d.KW > 11 || taps < 10) w = "mxfp8 conv (more than 9 taps): KH and KW in 1 ... 11 with 10 ... 121 taps";
    else if (d.Ci < 64 || d.Ci % 64 != 0) w = "mxfp8 conv (more than 9 taps): Ci must be a multiple of 64";
    else if (d.Co < 8 || d.Co % 8 != 0) w = "mxfp8 conv (more than 9 taps): Co must be a multiple of 8";
    else if (d.stride < 1 || d.dil < 1) w = "mxfp8 conv (more than 9 taps): stride and dilation must be positive";
    else if (d.B < 1 || d.Ho < 1 || d.Wo < 1 || d.Hi < 1 || d.Wi < 1) w = "mxfp8 conv (more than 9 taps): empty tensor";
    else if ((long long)d.B * d.Hi * d.Wi * d.Ci >= (1LL << 31) - 16 || (long long)d.B * d.Ho * d.Wo * d.Co >= (1LL << 31) - 16)
        w = "mxfp8 conv (more than 9 taps): a tensor of this layer exceeds the 32-bit offsets: lower the batch";
    else if (taps * d.Co * d.Ci >= (1LL << 31) - 16) w = "mxfp8 conv (more than 9 taps): the filter image exceeds the 32-bit offsets";
    else if ((long long)d.B * d.Hi * d.Wi * (d.Ci / 32) + 8 >= (1LL << 31) - 16 || (long long)d.B * d.Ho * d.Wo * (d.Co / 32) >= (1LL << 31) - 16)
        w = "mxfp8 conv (more than 9 taps): a scale tensor of this layer exceeds the 32-bit offsets: lower the batch";
    else if (out_mode != FP8_OUT_BF16 && out_mode != FP8_OUT_F32 && !wants_mx(out_mode)) w = "mxfp8 conv (more than 9 taps): unknown output mode";
    else if (wants_mx(out_mode) && d.Co % 32 != 0) w = "mxfp8 conv (more than 9 taps): an MX output needs Co to be a multiple of 32";
    if (why) *why = w;
    return w == nullptr;
}

// Where an mxfp8 handle uses this kernel: SSD_MXFP8_BIGK (read per handle) = 1 takes every supported layer with at least 256 input
// channels (the fc graph's mod_conv6); 0 or unset leaves it on conv_bigk_fwd_bf16 with a quantise pass behind it.
constexpr int MXFP8_BIGK_DEFAULT = 0;
bool conv_bigk_fwd_mxfp8_worthwhile(const ConvDesc& d) { return d.Ci >= 256 && env_int("SSD_MXFP8_BIGK", MXFP8_BIGK_DEFAULT) == 1; }

// Tiles as in conv_bigk_fwd_fp8: 0 = 128 x 128 with four stages, 1 = 64 x 64 with six; SSD_TILE_FP8 forces one.
void conv_bigk_fwd_mxfp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* xs, const unsigned char* w8, const float* s_w,
                         const float* bias, void* y, unsigned char* y8, unsigned char* ys, int out_mode, bool relu, hipStream_t s) {
    SSD_REQUIRE(d.KH * d.KW > 9, "mxfp8 conv: %dx%d taps: 9 taps or fewer run on conv_fwd_mxfp8 (ssd_op_conv2d_fwd_mxfp8)", d.KH, d.KW);
    const char* why = nullptr;
    SSD_REQUIRE(conv_bigk_fwd_mxfp8_supported(d, out_mode, &why), "%s (got %dx%d taps, Ci %d, Co %d, output mode %d)", why, d.KH, d.KW, d.Ci,
                d.Co, out_mode);
    SSD_REQUIRE(!wants_mx(out_mode) || (y8 != nullptr && ys != nullptr), "mxfp8 conv: an MX output needs its code and scale buffers");
    SSD_REQUIRE(out_mode == FP8_OUT_MX || y != nullptr, "mxfp8 conv: null output");
    SSD_REQUIRE(x8 && xs && w8 && s_w, "mxfp8 conv: null operand");
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(xs) % 2 == 0, "mxfp8 conv: the scale buffer must start at an even address");
    GatherArgsMXK a{};
    a.sc_delta = (int)(reinterpret_cast<uintptr_t>(xs) & 3);      // (a sample's scales inside a batch may start between two dwords)
    a.src = x8; a.src_sc = xs - a.sc_delta; a.wgt = w8; a.bias = bias; a.s_w = s_w; a.dst = y; a.dst8 = y8; a.dst_sc = ys;
    a.M = d.B * d.Ho * d.Wo; a.DH = d.Ho; a.DW = d.Wo; a.DN = d.Co;
    a.SH = d.Hi; a.SW = d.Wi; a.SC = d.Ci;
    a.KH = d.KH; a.KW = d.KW; a.dil = d.dil; a.pad_h = d.pad_h; a.pad_w = d.pad_w;
    a.mul = d.stride; a.relu = relu; a.mode = out_mode;
    const double fl = conv_flops(d);
    const double out_b = out_mode == FP8_OUT_F32 ? 4.0 : out_mode == FP8_OUT_BF16 ? 2.0 : (out_mode == FP8_OUT_MX ? 1.0 : 3.0) + 1.0 / 32;
    const double by = (double)d.B * d.Hi * d.Wi * d.Ci * (1.0 + 1.0 / 32) + (double)d.KH * d.KW * d.Ci * d.Co + (double)d.B * d.Ho * d.Wo * d.Co * out_b;
    int cfg = env_int("SSD_TILE_FP8", -1);
    if (cfg != 0 && cfg != 1) cfg = (long long)cdiv(a.M, 128) * cdiv(a.DN, 128) <= 256 ? 1 : 0;
    if (cfg == 0) launch_fwd_mxk<2, 2, 2, 2, 4>(a, "conv_bigk_fwd_mxfp8_128x128", fl, by, s);
    else launch_fwd_mxk<2, 2, 1, 1, 6>(a, "conv_bigk_fwd_mxfp8_64x64x6", fl, by, s);
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

static int grid_mx(size_t items, int per_block) {
    const size_t g = (items + per_block - 1) / per_block;
    return (int)std::min<size_t>(std::max<size_t>(g, 1), 256 * 32);
}

void quantize_mxfp8(const void* x, bool x_f32, size_t rows, int C, unsigned char* y8, unsigned char* ys, hipStream_t s) {
    SSD_REQUIRE(x && y8 && ys, "quantize_mxfp8: null argument");
    SSD_REQUIRE(C > 0 && C % 32 == 0, "quantize_mxfp8: C must be a multiple of 32 (got %d)", C);
    SSD_REQUIRE(reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(y8) % 8 == 0, "quantize_mxfp8: unaligned tensor");
    if (rows == 0) return;
    const size_t n8 = rows * (size_t)C / 8;
    ProfScope prof("quantize_mxfp8", 0.0, ((x_f32 ? 5.0 : 3.0) + 1.0 / 32) * (double)n8 * 8, s);
    if (x_f32) hipLaunchKernelGGL(quantize_mxfp8_kernel<float>, dim3(grid_mx(n8, 256)), dim3(256), 0, s, (const float*)x, y8, ys, n8);
    else hipLaunchKernelGGL(quantize_mxfp8_kernel<bf16_t>, dim3(grid_mx(n8, 256)), dim3(256), 0, s, (const bf16_t*)x, y8, ys, n8);
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
    hipLaunchKernelGGL(maxpool_fwd_mxfp8_kernel, dim3(grid_mx(total, 256)), dim3(256), 0, s, d, x8, xs, y8, ys);
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
