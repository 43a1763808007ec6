// fp8 (OCP e4m3fn) inference kernels for gfx950 (MI355X): the forward gather convolution of conv_bf16.hip restated for
// e4m3 operands on the block-scaled matrix instruction v_mfma_scale_f32_32x32x64_f8f6f4 (format selector 0 = e4m3 for both
// operands, every block scale 2^0), plus what surrounds it: filter quantisation (per output channel), activation
// quantisation (per tensor), the absmax reduction calibration needs and max-pooling on e4m3 bytes.  DESIGN.md 18.
//
// Numeric contract: code = RNE(clamp(v / s, -448, 448)); products of two e4m3 numbers are exact in fp32, the MFMA adds in
// fp32; epilogue in fp32: y = relu?(acc * (s_in * s_w[co]) + bias[co]), then bf16 / fp32 / e4m3 at the consumer's scale.
//
// Operand layout (tools/probes/fp8_probe.hip pins it on the hardware): lane l holds row l & 31 of its operand and the 32
// consecutive k = 32 (l >> 5) + j, one byte each, in 8 registers -- two 16-byte LDS reads.  A tile row is 64 k = 64 bytes,
// filled by LDS-DMA (lane-linear, 16 bytes per lane, zero fill of padding by an out-of-range offset, like the bf16 tiles).
// Swizzle for 64-byte rows: LDS slot p of row r holds the global 16-byte chunk p ^ ((r >> 2) & 3).  A ds_read_b128 lane
// group is 16 rows of one k half ({0-3, 12-15, 20-27} or {4-11, 16-19, 28-31}, MI355X LDS banking); row r's slot sits at
// 16-byte unit 4 (r & 3) + slot of the 256-byte bank line, and the four rows of a group that share r & 3 have four
// different (r >> 2) & 3, so the group covers all 16 units: conflict-free.
#include "conv.h"
#include "conv_detail.h"
#include "conv_fp8_detail.h"
#include "bf16.h"
#include "ops.h"
#include <algorithm>

namespace ssd {

struct GatherArgs8 {
    const unsigned char* src;      // e4m3 [B][SH][SW][SC]
    const unsigned char* wgt;      // e4m3 [tap][DN][SC]
    const float* bias;             // [DN] or nullptr
    const float* s_w;              // [DN] filter scales
    void* dst;                     // bf16 or fp32 [M][DN] (modes 0, 1, 3)
    unsigned char* dst8;           // e4m3 [M][DN] (modes 2, 3)
    float s_in, s_out;
    int M, DH, DW, DN;
    int SH, SW, SC;
    int ntaps, mul, relu, mode, NT;
    int tap_dh[9], tap_dw[9];
};

// One pipeline iteration = one tap of one 64-channel chunk: BM pixel rows and BN filter rows of 64 bytes each.  At half the
// bytes per k of the bf16 tiles the ring is twice as deep for the same LDS (NS stages; the fp32 epilogue tile sets the size).
template <int WM, int WN, int TM, int TN, int NS>
__global__ __launch_bounds__(64 * WM * WN) void conv_fwd_fp8_kernel(GatherArgs8 pp) {
    const GatherArgs8& p = pp;
    constexpr int NTHR = 64 * WM * WN;
    constexpr int RPP_S = NTHR / 4;                   // tile rows one staging pass covers (4 lanes per 64-byte row)
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int A_N = BM / RPP_S, B_N = BN / RPP_S; // DMA instructions per thread and tile
    constexpr int STAGE = (BM + BN) * KB8;
    constexpr int LDC = BN + 4;
    static_assert(BM % RPP_S == 0 && BN % RPP_S == 0 && RPP_S % 16 == 0, "tile vs staging pass");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = wg / p.NT, nt = wg - mt * p.NT;
    const int m0 = mt * BM, n0 = nt * BN;

    // ---- staging: thread -> rows (tid >> 2) + RPP_S i, LDS slot tid & 3, global chunk slot ^ ((row >> 2) & 3)
    const int a_ck = ((tid & 3) ^ ((tid >> 4) & 3)) * 16;
    unsigned a_off[A_N], a_msk[A_N];
#pragma unroll
    for (int i = 0; i < A_N; ++i) {
        const int m = m0 + (tid >> 2) + RPP_S * i;
        const int mm = m < p.M ? m : 0;
        const int ow = mm % p.DW;
        const int t2 = mm / p.DW;
        const int oh = t2 % p.DH;
        const int b = t2 / p.DH;
        const int rh = oh * p.mul, rw = ow * p.mul;
        a_off[i] = (unsigned)((b * p.SH * p.SW + rh * p.SW + rw) * p.SC + a_ck);
        unsigned mk = 0;
        if (m < p.M)
            for (int t = 0; t < p.ntaps; ++t) {
                const int sh = rh + p.tap_dh[t], sw = rw + p.tap_dw[t];
                if ((unsigned)sh < (unsigned)p.SH && (unsigned)sw < (unsigned)p.SW) mk |= 1u << t;
            }
        a_msk[i] = mk;
    }
    unsigned b_off[B_N], b_ok[B_N];
#pragma unroll
    for (int i = 0; i < B_N; ++i) {
        const int n = n0 + (tid >> 2) + RPP_S * i;
        b_ok[i] = 0u - (unsigned)(n < p.DN);
        b_off[i] = (unsigned)((n < p.DN ? n : 0) * p.SC + a_ck);
    }
    const __amdgpu_buffer_rsrc_t src_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(p.src), 0, (unsigned)((size_t)(p.M / (p.DH * p.DW)) * p.SH * p.SW * p.SC), 0x00020000);
    const __amdgpu_buffer_rsrc_t wgt_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.wgt), 0, (unsigned)((size_t)p.ntaps * p.DN * p.SC), 0x00020000);

    const int nk = (p.SC / KB8) * p.ntaps;      // SC is a multiple of 64 (host check): no channel-chunk mask

    auto issue = [&](int kiter, int stage) {
        const int cc = kiter / p.ntaps;
        const int tap = kiter - cc * p.ntaps;
        unsigned char* As = smem + stage * STAGE + wave * 1024;        // wave-uniform: 16 rows x 64 B per DMA
        unsigned char* Bs = As + BM * KB8;
        const unsigned toff = (unsigned)((p.tap_dh[tap] * p.SW + p.tap_dw[tap]) * p.SC + cc * KB8);
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
    // fragment = chunks 2 lh and 2 lh + 1 of row li: slots (2 lh) ^ f and (2 lh) ^ f ^ 1, f = (row >> 2) & 3 = (li >> 2) & 3
    const int q0 = ((2 * lh) ^ ((li >> 2) & 3)) * 16;
    const int a_row = (wm * 32 * TM + li) * KB8 + q0;
    const int b_row = BM * KB8 + (wn * 32 * TN + li) * KB8 + q0;

    auto load_frag = [&](const unsigned char* S, int addr) -> i32x8 {
        const i32x4 lo = *reinterpret_cast<const i32x4*>(S + addr);
        const i32x4 hi = *reinterpret_cast<const i32x4*>(S + (addr ^ 16));
        return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    auto compute = [&](int stage) {
        const unsigned char* S = smem + stage * STAGE;
        i32x8 a[TM], b[TN];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) a[mi] = load_frag(S, a_row + mi * 32 * KB8);
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) b[ni] = load_frag(S, b_row + ni * 32 * KB8);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b[ni], a[mi], acc[mi][ni], 0, 0, 0, SCALE_ONE, 0, SCALE_ONE);
    };

    // ---- main loop: NS stages; tiles k+1 .. k+NS-1 stream in while tile k is multiplied
#pragma unroll
    for (int t = 0; t < NS - 1; ++t)
        if (t < nk) issue(t, t);
    int st_c = 0, st_i = NS - 1;
    for (int k = 0; k < nk; ++k) {
        const int later = nk - 1 - k;
        wait_tiles_and_sync8<A_N + B_N, (NS - 2 > 4 ? 4 : NS - 2)>(later < NS - 2 ? later : NS - 2);      // tile k visible; stage st_i is free
        if (k + NS - 1 < nk) issue(k + NS - 1, st_i);
        compute(st_c);
        st_c = st_c + 1 == NS ? 0 : st_c + 1;
        st_i = st_i + 1 == NS ? 0 : st_i + 1;
    }
    __syncthreads();

    // ---- epilogue through an fp32 LDS tile [BM][BN + 4]: dequantise, bias, relu, one rounding per output format
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
    constexpr int TPR = BN / 8;               // threads per row, 8 channels each
    constexpr int RPP = NTHR / TPR;           // rows per pass
    const int cg = tid % TPR, r0 = tid / TPR;
    const int n = n0 + cg * 8;
    if (n >= p.DN) return;
    float sc[8], bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sc[e] = p.s_in * p.s_w[n + e];
        bv[e] = p.bias ? p.bias[n + e] : 0.f;
    }
#pragma unroll
    for (int ps = 0; ps < BM / RPP; ++ps) {
        const int ml = r0 + ps * RPP;
        const int m = m0 + ml;
        if (m >= p.M) continue;
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
        } else if (p.mode != FP8_OUT_E4M3) {
            *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(p.dst) + o) =
                u32x4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
        }
        if (p.mode == FP8_OUT_E4M3 || p.mode == FP8_OUT_BF16_E4M3) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = v[e] / p.s_out;
            *reinterpret_cast<u32x2*>(p.dst8 + o) = u32x2{pack4_e4m3(v[0], v[1], v[2], v[3]), pack4_e4m3(v[4], v[5], v[6], v[7])};
        }
    }
}

template <int WM, int WN, int TM, int TN, int NS>
static void launch_fwd8(GatherArgs8& a, const char* label, double flops, double bytes, hipStream_t s) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr size_t stages = NS * (size_t)(BM + BN) * KB8, ctile = (size_t)BM * (BN + 4) * 4;
    constexpr size_t lds = stages > ctile ? stages : ctile;
    static_assert(lds <= 160 * 1024, "LDS");
    auto kern = conv_fwd_fp8_kernel<WM, WN, TM, TN, NS>;
    static bool once = (set_lds(kern, lds), true);
    (void)once;
    a.NT = cdiv(a.DN, BN);
    ProfScope prof(label, flops, bytes, s);
    SSD_LAUNCH_STOP(kern, dim3(cdiv(a.M, BM) * a.NT), dim3(64 * WM * WN), lds, s, a);
    HIP_OK(hipGetLastError());
}

bool conv_fwd_fp8_supported(const ConvDesc& d, const char** why) {
    const char* w = nullptr;
    if (d.KH * d.KW > 9 || d.KH * d.KW < 1) w = "fp8 conv: at most 9 taps";
    else if (d.Ci % 64 != 0) w = "fp8 conv: Ci must be a multiple of 64";
    else if (d.Co % 8 != 0) w = "fp8 conv: Co must be a multiple of 8";
    else if (d.stride < 1 || d.dil < 1) w = "fp8 conv: stride and dilation must be positive";
    else if ((long long)d.B * d.Hi * d.Wi * d.Ci >= (1LL << 31) - 16 || (long long)d.B * d.Ho * d.Wo * d.Co >= (1LL << 31) - 16)
        w = "fp8 conv: a tensor of this layer exceeds the 32-bit offsets: lower the batch";
    if (why) *why = w;
    return w == nullptr;
}

// Where an fp8 handle uses this kernel.  Interleaved rounds against the bf16 handle at batch 128 (tools/infer_rate.py,
// profiles/fp8_infer_rate_all_layers.txt, profiles/fp8_infer_rate.txt): every layer with at least 256 input channels
// ran 1.09 ... 1.46 x faster than its bf16 kernel in every round; the layers with 64 or 128 did not (conv1_2 0.42 x, conv2_1
// 0.91 x, conv2_2 not separated and it loses its fused pool, conv3_1 1.10 x in one run and not separated in the next) -- there a tap
// is one or two 64-byte chunks, and the bf16 handle runs the 64-channel and kernel-row gathers of conv_bf16.hip with the pool in the
// epilogue, forms this per-tap kernel does not have.
// They stay on bf16.  SSD_FP8_ALL=1 (read per handle) takes every supported layer: the A/B that produced the table.
bool conv_fwd_fp8_worthwhile(const ConvDesc& d) { return d.Ci >= 256 || env_int("SSD_FP8_ALL", 0) == 1; }

// Tiles: 0 = 128 x 128, four stages of 16 KB (the fp32 epilogue tile's 66 KB sets the allocation: two workgroups per CU);
// 1 = 64 x 64, six stages, where the 128 x 128 tiling would leave CUs empty.  SSD_TILE_FP8 forces one (tests, tuning).
void conv_fwd_fp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* w8, float s_in, const float* s_w, const float* bias,
                  void* y, unsigned char* y8, int out_mode, float s_out, bool relu, hipStream_t s) {
    const char* why = nullptr;
    SSD_REQUIRE(conv_fwd_fp8_supported(d, &why), "%s (got %dx%d taps, Ci %d, Co %d)", why, d.KH, d.KW, d.Ci, d.Co);
    SSD_REQUIRE(out_mode >= FP8_OUT_BF16 && out_mode <= FP8_OUT_BF16_E4M3, "fp8 conv: unknown output mode %d", out_mode);
    const bool wants8 = out_mode == FP8_OUT_E4M3 || out_mode == FP8_OUT_BF16_E4M3;
    SSD_REQUIRE(!wants8 || (y8 != nullptr && s_out > 0.f), "fp8 conv: an e4m3 output needs its buffer and a positive scale");
    SSD_REQUIRE(out_mode == FP8_OUT_E4M3 || y != nullptr, "fp8 conv: null output");
    SSD_REQUIRE(x8 && w8 && s_w && s_in > 0.f, "fp8 conv: null operand or non-positive input scale");
    GatherArgs8 a{};
    a.src = x8; a.wgt = w8; a.bias = bias; a.s_w = s_w; a.dst = y; a.dst8 = y8; a.s_in = s_in; a.s_out = wants8 ? s_out : 1.f;
    a.M = d.B * d.Ho * d.Wo; a.DH = d.Ho; a.DW = d.Wo; a.DN = d.Co;
    a.SH = d.Hi; a.SW = d.Wi; a.SC = d.Ci;
    a.ntaps = d.KH * d.KW; a.mul = d.stride; a.relu = relu; a.mode = out_mode;
    for (int kh = 0; kh < d.KH; ++kh)
        for (int kw = 0; kw < d.KW; ++kw) {
            a.tap_dh[kh * d.KW + kw] = kh * d.dil - d.pad_h;
            a.tap_dw[kh * d.KW + kw] = kw * d.dil - d.pad_w;
        }
    const double fl = conv_flops(d);
    const double by = (double)d.B * d.Hi * d.Wi * d.Ci + (double)d.KH * d.KW * d.Ci * d.Co +
                      (double)d.B * d.Ho * d.Wo * d.Co * (out_mode == FP8_OUT_F32 ? 4 : out_mode == FP8_OUT_BF16 ? 2 : out_mode == FP8_OUT_E4M3 ? 1 : 3);
    int cfg = env_int("SSD_TILE_FP8", -1);
    if (cfg != 0 && cfg != 1) cfg = (long long)cdiv(a.M, 128) * cdiv(a.DN, 128) <= 256 ? 1 : 0;
    if (cfg == 0) launch_fwd8<2, 2, 2, 2, 4>(a, "conv_fwd_fp8_128x128", fl, by, s);
    else launch_fwd8<2, 2, 1, 1, 6>(a, "conv_fwd_fp8_64x64x6", fl, by, s);
}

// =================================================================================
// More than 9 taps (the fc graph's 7 x 7 fc6): conv_fwd_fp8_kernel's per-tap gather, ring and epilogue with the
// two things that stop at 9 taps restated.  The tap's offset is computed from (kh, kw, dil, pad) when its tile is issued
// (wave-uniform counters, no table in the kernel arguments).  A row's validity is kept separably: bit kh of the low half-word
// = kernel row kh lands on an image row for this pixel, bit 16 + kw = kernel column kw lands on an image column; a tap is
// inside the image exactly when both hold, so one register per staged row serves any KH, KW <= 16 (a 64-bit mask per row
// would take two and stop at 64 taps).  The existing kernel is left as it is: its instantiations' code does not change.
// =================================================================================
struct GatherArgs8K {
    const unsigned char* src;      // e4m3 [B][SH][SW][SC]
    const unsigned char* wgt;      // e4m3 [tap][DN][SC]
    const float* bias;             // [DN] or nullptr
    const float* s_w;              // [DN] filter scales
    void* dst;                     // bf16 or fp32 [M][DN] (modes 0, 1, 3)
    unsigned char* dst8;           // e4m3 [M][DN] (modes 2, 3)
    float s_in, s_out;
    int M, DH, DW, DN;
    int SH, SW, SC;
    int KH, KW, dil, pad_h, pad_w;
    int mul, relu, mode, MT;
};

template <int WM, int WN, int TM, int TN, int NS>
__global__ __launch_bounds__(64 * WM * WN) void conv_bigk_fwd_fp8_kernel(GatherArgs8K pp) {
    const GatherArgs8K& p = pp;
    constexpr int NTHR = 64 * WM * WN;
    constexpr int RPP_S = NTHR / 4;                   // tile rows one staging pass covers (4 lanes per 64-byte row)
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int A_N = BM / RPP_S, B_N = BN / RPP_S; // DMA instructions per thread and tile
    constexpr int STAGE = (BM + BN) * KB8;
    constexpr int LDC = BN + 4;
    static_assert(BM % RPP_S == 0 && BN % RPP_S == 0 && RPP_S % 16 == 0, "tile vs staging pass");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    // Pixel tiles fastest: consecutive workgroups (one XCD's share, conv_detail.h xcd_remap) walk the pixel tiles of ONE filter column,
    // so the workgroups resident on an XCD stream the same filter rows through its L2 (launch_fwd8k: why not conv_fwd_fp8's order)
    const int nt = wg / p.MT, mt = wg - nt * p.MT;
    const int m0 = mt * BM, n0 = nt * BN;

    // ---- staging: thread -> rows (tid >> 2) + RPP_S i, LDS slot tid & 3, global chunk slot ^ ((row >> 2) & 3)
    const int a_ck = ((tid & 3) ^ ((tid >> 4) & 3)) * 16;
    unsigned a_off[A_N], a_msk[A_N];
#pragma unroll
    for (int i = 0; i < A_N; ++i) {
        const int m = m0 + (tid >> 2) + RPP_S * i;
        const int mm = m < p.M ? m : 0;
        const int ow = mm % p.DW;
        const int t2 = mm / p.DW;
        const int oh = t2 % p.DH;
        const int b = t2 / p.DH;
        const int rh = oh * p.mul, rw = ow * p.mul;
        a_off[i] = (unsigned)((b * p.SH * p.SW + rh * p.SW + rw) * p.SC + a_ck);
        unsigned mk = 0;
        if (m < p.M) {
            for (int kh = 0; kh < p.KH; ++kh)
                if ((unsigned)(rh + kh * p.dil - p.pad_h) < (unsigned)p.SH) mk |= 1u << kh;
            for (int kw = 0; kw < p.KW; ++kw)
                if ((unsigned)(rw + kw * p.dil - p.pad_w) < (unsigned)p.SW) mk |= 0x10000u << kw;
        }
        a_msk[i] = mk;
    }
    unsigned b_off[B_N], b_ok[B_N];
#pragma unroll
    for (int i = 0; i < B_N; ++i) {
        const int n = n0 + (tid >> 2) + RPP_S * i;
        b_ok[i] = 0u - (unsigned)(n < p.DN);
        b_off[i] = (unsigned)((n < p.DN ? n : 0) * p.SC + a_ck);
    }
    const __amdgpu_buffer_rsrc_t src_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(p.src), 0, (unsigned)((size_t)(p.M / (p.DH * p.DW)) * p.SH * p.SW * p.SC), 0x00020000);
    const __amdgpu_buffer_rsrc_t wgt_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.wgt), 0,
                                                                              (unsigned)((size_t)p.KH * p.KW * p.DN * p.SC), 0x00020000);

    const int nk = (p.SC / KB8) * p.KH * p.KW;      // SC is a multiple of 64 (host check): no channel-chunk mask

    // tiles are issued in k order, taps inside a channel chunk: (i_cc, i_kh, i_kw) is the next one, wave-uniform
    int i_cc = 0, i_kh = 0, i_kw = 0;
    auto issue_next = [&](int stage) {
        unsigned char* As = smem + stage * STAGE + wave * 1024;        // wave-uniform: 16 rows x 64 B per DMA
        unsigned char* Bs = As + BM * KB8;
        const unsigned toff = (unsigned)(((i_kh * p.dil - p.pad_h) * p.SW + (i_kw * p.dil - p.pad_w)) * p.SC + i_cc * KB8);
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
        if (++i_kw == p.KW) {
            i_kw = 0;
            if (++i_kh == p.KH) {
                i_kh = 0;
                ++i_cc;
            }
        }
    };

    // ---- accumulators: D rows = output channels (filter operand first), D cols = pixels, as in conv_fwd_fp8_kernel
    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int wm = wave / WN, wn = wave - wm * WN;
    const int li = lane & 31, lh = lane >> 5;
    const int q0 = ((2 * lh) ^ ((li >> 2) & 3)) * 16;
    const int a_row = (wm * 32 * TM + li) * KB8 + q0;
    const int b_row = BM * KB8 + (wn * 32 * TN + li) * KB8 + q0;

    auto load_frag = [&](const unsigned char* S, int addr) -> i32x8 {
        const i32x4 lo = *reinterpret_cast<const i32x4*>(S + addr);
        const i32x4 hi = *reinterpret_cast<const i32x4*>(S + (addr ^ 16));
        return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    auto compute = [&](int stage) {
        const unsigned char* S = smem + stage * STAGE;
        i32x8 a[TM], b[TN];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) a[mi] = load_frag(S, a_row + mi * 32 * KB8);
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) b[ni] = load_frag(S, b_row + ni * 32 * KB8);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b[ni], a[mi], acc[mi][ni], 0, 0, 0, SCALE_ONE, 0, SCALE_ONE);
    };

    // ---- main loop: NS stages; tiles k+1 .. k+NS-1 stream in while tile k is multiplied
#pragma unroll
    for (int t = 0; t < NS - 1; ++t)
        if (t < nk) issue_next(t);
    int st_c = 0, st_i = NS - 1;
    for (int k = 0; k < nk; ++k) {
        const int later = nk - 1 - k;
        wait_tiles_and_sync8<A_N + B_N, (NS - 2 > 4 ? 4 : NS - 2)>(later < NS - 2 ? later : NS - 2);      // tile k visible; stage st_i is free
        if (k + NS - 1 < nk) issue_next(st_i);
        compute(st_c);
        st_c = st_c + 1 == NS ? 0 : st_c + 1;
        st_i = st_i + 1 == NS ? 0 : st_i + 1;
    }
    __syncthreads();

    // ---- epilogue through an fp32 LDS tile [BM][BN + 4], as in conv_fwd_fp8_kernel
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
    constexpr int TPR = BN / 8;               // threads per row, 8 channels each
    constexpr int RPP = NTHR / TPR;           // rows per pass
    const int cg = tid % TPR, r0 = tid / TPR;
    const int n = n0 + cg * 8;
    if (n >= p.DN) return;
    float sc[8], bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sc[e] = p.s_in * p.s_w[n + e];
        bv[e] = p.bias ? p.bias[n + e] : 0.f;
    }
#pragma unroll
    for (int ps = 0; ps < BM / RPP; ++ps) {
        const int ml = r0 + ps * RPP;
        const int m = m0 + ml;
        if (m >= p.M) continue;
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
        } else if (p.mode != FP8_OUT_E4M3) {
            *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(p.dst) + o) =
                u32x4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
        }
        if (p.mode == FP8_OUT_E4M3 || p.mode == FP8_OUT_BF16_E4M3) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = v[e] / p.s_out;
            *reinterpret_cast<u32x2*>(p.dst8 + o) = u32x2{pack4_e4m3(v[0], v[1], v[2], v[3]), pack4_e4m3(v[4], v[5], v[6], v[7])};
        }
    }
}

template <int WM, int WN, int TM, int TN, int NS>
static void launch_fwd8k(GatherArgs8K& a, const char* label, double flops, double bytes, hipStream_t s) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr size_t stages = NS * (size_t)(BM + BN) * KB8, ctile = (size_t)BM * (BN + 4) * 4;
    constexpr size_t lds = stages > ctile ? stages : ctile;
    static_assert(lds <= 66 * 1024, "LDS: two workgroups per CU");
    auto kern = conv_bigk_fwd_fp8_kernel<WM, WN, TM, TN, NS>;
    static bool once = (set_lds(kern, lds), true);
    (void)once;
    // Workgroup order.  Consecutive workgroups share an XCD's L2 (xcd_remap).  With filter columns fastest (conv_fwd_fp8's order) the
    // workgroups resident on an XCD cover every column, and each row of pixel tiles streams the whole filter image: MT x its bytes
    // in all.  With pixel tiles fastest they share one column, and each column streams the input: NT x its bytes.  A column of a
    // filter with more than 9 taps (taps x BN x Ci bytes) is always larger than a pixel tile's input (about BM x Ci), so this kernel
    // takes pixel tiles fastest.  fc6 at batch 128 (102 MB of filter, 24 MB of input, MT 361, NT 32): 4.92 against 9.70 ms.
    a.MT = cdiv(a.M, BM);
    ProfScope prof(label, flops, bytes, s);
    SSD_LAUNCH_STOP(kern, dim3(a.MT * cdiv(a.DN, BN)), dim3(64 * WM * WN), lds, s, a);
    HIP_OK(hipGetLastError());
}

bool conv_bigk_fwd_fp8_supported(const ConvDesc& d, const char** why) {
    const char* w = nullptr;
    const long long taps = (long long)d.KH * d.KW;
    if (d.KH < 1 || d.KW < 1 || d.KH > 11 || d.KW > 11 || taps < 10) w = "fp8 conv (more than 9 taps): KH and KW in 1 ... 11 with 10 ... 121 taps";
    else if (d.Ci < 64 || d.Ci % 64 != 0) w = "fp8 conv (more than 9 taps): Ci must be a multiple of 64";
    else if (d.Co < 8 || d.Co % 8 != 0) w = "fp8 conv (more than 9 taps): Co must be a multiple of 8";
    else if (d.stride < 1 || d.dil < 1) w = "fp8 conv (more than 9 taps): stride and dilation must be positive";
    else if (d.B < 1 || d.Ho < 1 || d.Wo < 1 || d.Hi < 1 || d.Wi < 1) w = "fp8 conv (more than 9 taps): empty tensor";
    else if ((long long)d.B * d.Hi * d.Wi * d.Ci >= (1LL << 31) - 16 || (long long)d.B * d.Ho * d.Wo * d.Co >= (1LL << 31) - 16)
        w = "fp8 conv (more than 9 taps): a tensor of this layer exceeds the 32-bit offsets: lower the batch";
    else if (taps * d.Co * d.Ci >= (1LL << 31) - 16) w = "fp8 conv (more than 9 taps): the filter image exceeds the 32-bit offsets";
    if (why) *why = w;
    return w == nullptr;
}

// Where an fp8 handle uses this kernel: SSD_FP8_BIGK (read per handle) = 1 takes every supported layer with at least 256 input
// channels (the fc graph's mod_conv6), 0 leaves it on conv_bigk_fwd_bf16 with a quantise pass behind it.  Unset = 1: in interleaved
// rounds at batch 128 (tools/infer_rate.py --a-trous false, profiles/fp8_fc_infer_rate.txt) the mod_conv6 row separated
// from the bf16 kernel's in fp8's favour, and the whole handle from the handle under SSD_FP8_BIGK=0.
constexpr int FP8_BIGK_DEFAULT = 1;
bool conv_bigk_fwd_fp8_worthwhile(const ConvDesc& d) { return d.Ci >= 256 && env_int("SSD_FP8_BIGK", FP8_BIGK_DEFAULT) == 1; }

// Tiles as in conv_fwd_fp8: 0 = 128 x 128 with four stages, 1 = 64 x 64 with six; SSD_TILE_FP8 forces one.
void conv_bigk_fwd_fp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* w8, float s_in, const float* s_w, const float* bias,
                       void* y, unsigned char* y8, int out_mode, float s_out, bool relu, hipStream_t s) {
    SSD_REQUIRE(d.KH * d.KW > 9, "fp8 conv: %dx%d taps: 9 taps or fewer run on conv_fwd_fp8 (ssd_op_conv2d_fwd_fp8)", d.KH, d.KW);
    const char* why = nullptr;
    SSD_REQUIRE(conv_bigk_fwd_fp8_supported(d, &why), "%s (got %dx%d taps, Ci %d, Co %d)", why, d.KH, d.KW, d.Ci, d.Co);
    SSD_REQUIRE(out_mode >= FP8_OUT_BF16 && out_mode <= FP8_OUT_BF16_E4M3, "fp8 conv: unknown output mode %d", out_mode);
    const bool wants8 = out_mode == FP8_OUT_E4M3 || out_mode == FP8_OUT_BF16_E4M3;
    SSD_REQUIRE(!wants8 || (y8 != nullptr && s_out > 0.f), "fp8 conv: an e4m3 output needs its buffer and a positive scale");
    SSD_REQUIRE(out_mode == FP8_OUT_E4M3 || y != nullptr, "fp8 conv: null output");
    SSD_REQUIRE(x8 && w8 && s_w && s_in > 0.f, "fp8 conv: null operand or non-positive input scale");
    GatherArgs8K a{};
    a.src = x8; a.wgt = w8; a.bias = bias; a.s_w = s_w; a.dst = y; a.dst8 = y8; a.s_in = s_in; a.s_out = wants8 ? s_out : 1.f;
    a.M = d.B * d.Ho * d.Wo; a.DH = d.Ho; a.DW = d.Wo; a.DN = d.Co;
    a.SH = d.Hi; a.SW = d.Wi; a.SC = d.Ci;
    a.KH = d.KH; a.KW = d.KW; a.dil = d.dil; a.pad_h = d.pad_h; a.pad_w = d.pad_w;
    a.mul = d.stride; a.relu = relu; a.mode = out_mode;
    const double fl = conv_flops(d);
    const double by = (double)d.B * d.Hi * d.Wi * d.Ci + (double)d.KH * d.KW * d.Ci * d.Co +
                      (double)d.B * d.Ho * d.Wo * d.Co * (out_mode == FP8_OUT_F32 ? 4 : out_mode == FP8_OUT_BF16 ? 2 : out_mode == FP8_OUT_E4M3 ? 1 : 3);
    int cfg = env_int("SSD_TILE_FP8", -1);
    if (cfg != 0 && cfg != 1) cfg = (long long)cdiv(a.M, 128) * cdiv(a.DN, 128) <= 256 ? 1 : 0;
    if (cfg == 0) launch_fwd8k<2, 2, 2, 2, 4>(a, "conv_bigk_fwd_fp8_128x128", fl, by, s);
    else launch_fwd8k<2, 2, 1, 1, 6>(a, "conv_bigk_fwd_fp8_64x64x6", fl, by, s);
}

// =================================================================================
// filter quantisation: fp32 [tap][Ci][Co] -> e4m3 [tap][Co][Ci] + one fp32 scale per output channel, all layers in one launch
// =================================================================================
struct QuantTable {
    int n;
    struct Seg {
        unsigned long long off, off8, offs;      // element offsets: fp32 filter, e4m3 image, scales
        int taps, ci, co;
        int blk0;                                // first block of this layer (one block per 32 output channels)
    } seg[FilterQuantPlan::MAX_LAYERS];
};

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
    t.n = 0;      // (layers whose rows are split below are not in the table)
    int blk = 0;
    double elems = 0;
    for (int i = 0; i < plan.n; ++i) {
        elems += (double)plan.L[i].taps * plan.L[i].ci * plan.L[i].co;
        if (quantize_rows_split(plan.L[i], w, w8)) continue;      // below
        QuantTable::Seg& g = t.seg[t.n++];
        g.off = plan.L[i].off; g.off8 = plan.L[i].off8; g.offs = plan.L[i].offs;
        g.taps = plan.L[i].taps; g.ci = plan.L[i].ci; g.co = plan.L[i].co;
        g.blk0 = blk;
        blk += cdiv(plan.L[i].co, 32);
    }
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
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] / scale;
        *reinterpret_cast<u32x2*>(y + i * 8) = u32x2{pack4_e4m3(v[0], v[1], v[2], v[3]), pack4_e4m3(v[4], v[5], v[6], v[7])};
    }
}

static int grid8(size_t items, int per_block) {
    const size_t g = (items + per_block - 1) / per_block;
    return (int)std::min<size_t>(std::max<size_t>(g, 1), 256 * 32);
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
    SSD_REQUIRE(d.k >= 1 && d.stride >= 1 && d.B > 0 && d.Ho > 0 && d.Wo > 0, "maxpool_fwd_fp8: bad geometry");
    // every window must hold at least one cell of the image
    SSD_REQUIRE((d.Ho - 1) * d.stride - d.pad_h < d.Hi && (d.Wo - 1) * d.stride - d.pad_w < d.Wi && d.pad_h < d.k && d.pad_w < d.k,
                "maxpool_fwd_fp8: a window lies outside the image");
    const size_t total = (size_t)d.B * d.Ho * d.Wo * (d.C / 16);
    ProfScope prof("maxpool_fwd_fp8", 0.0, (double)d.C * d.B * ((double)d.Hi * d.Wi + (double)d.Ho * d.Wo), s);
    hipLaunchKernelGGL(maxpool_fwd_fp8_kernel, dim3(grid8(total, 256)), dim3(256), 0, s, d, x8, y8);
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
