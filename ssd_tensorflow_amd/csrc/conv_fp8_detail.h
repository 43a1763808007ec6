// The forward gather convolution on e4m3 operands for gfx950 (MI355X), once: the kernel, its launcher, the shape check and the host path
// behind the four entry points of conv.h.  conv_fp8.hip instantiates it with MX = false (one fp32 scale per activation tensor, DESIGN.md
// 18, 19), conv_mxfp8.hip with MX = true (one E8M0 scale byte per pixel and 32 channels); DESIGN.md 23 on the merge.
// The host functions are `static` templates on purpose: each object file gets the instantiations of its own format and nothing of the
// others', and no further file includes this header for them.
// Also what the e2m3 kernel of conv_mxfp6_detail.h shares with it: the shape check, the host prologue, the launcher and
// the filter table.  The frame of the kernel body around the staging and the fragments (gather_pixel_of ... gather_epilogue) is this
// kernel's alone: conv_mxfp6_detail.h says why the e2m3 kernel keeps its own.  The clamped converts and the MX scale rule are
// mx_block.h's.
#pragma once
#include "conv_detail.h"
#include "mx_block.h"

namespace ssd {

typedef int i32x8 __attribute__((ext_vector_type(8)));
#define LDS_PTR8(p) ((__attribute__((address_space(3))) void*)(p))

constexpr int KB8 = 64;                 // k per pipeline iteration = bytes per tile row
constexpr unsigned OOB8 = 0xFFFFFFF0u;  // offset no buffer covers: the DMA writes zeros (code 0 = +0)
constexpr int SCALE_ONE = 0x7F7F7F7F;   // E8M0 block scale 127 = 2^0 in every byte

// =================================================================================
// The kernel: the forward gather convolution of conv_bf16.hip restated for e4m3 operands on the block-scaled matrix instruction
// v_mfma_scale_f32_32x32x64_f8f6f4 (format selector 0 = e4m3 for both operands).  Products of two e4m3 numbers are exact in fp32, the
// MFMA adds in fp32, the epilogue runs in fp32 with one rounding per output format.
//
// Operand layout (tools/probes/fp8_probe.hip pins it on the hardware): lane l holds row l & 31 of its operand and 32 of the 64 k, one
// byte each, in 8 registers -- two 16-byte LDS reads.  A tile row is 64 k = 64 bytes = four 16-byte chunks, filled by LDS-DMA
// (lane-linear, 16 bytes per lane, zero fill of padding by an out-of-range offset, like the bf16 tiles).  Swizzle for 64-byte rows: LDS
// slot p of row r holds the global chunk p ^ f, f = (r >> 2) & 3.  A ds_read_b128 lane group is 16 rows of one k half ({0-3, 12-15,
// 20-27} or {4-11, 16-19, 28-31}, MI355X LDS banking); row r's slot sits at 16-byte unit 4 (r & 3) + slot of the 256-byte bank line, and
// the four rows of a group that share r & 3 have four different f, so the group covers all 16 units: conflict-free, for either of the
// two chunk assignments below.
//
// Which chunks a lane takes (lh = l >> 5), and the instruction's scale operand:
//   MX = false: chunks 2 lh and 2 lh + 1 (slots (2 lh) ^ f and (2 lh) ^ f ^ 1), the lane's 32 consecutive k; every block scale 2^0.
//   MX = true:  chunks lh and lh + 2 (slots lh ^ f and lh ^ f ^ 2), for both operands -- a dot product does not care as long as they
//               agree.  The hardware's scale byte of lane li + 32 h multiplies registers 4 h ... 4 h + 3 of BOTH lanes li and li + 32
//               (tools/probes/mxfp8_probe.hip), so with this assignment those 32 values are the 32 consecutive channels 32 h ... 32 h + 31
//               of the chunk, one MX block.  The filter operand's scale stays 2^0.
// The two orders are kept apart on purpose: the order in which the instruction sums its 64 k is not ours to assume, and each format's
// results stay what they were.
//
// One pipeline iteration = one tap of one 64-channel chunk: BM pixel rows and BN filter rows of 64 bytes each, in k order -- channel
// chunk outer, taps inner, kernel row major.  At half the bytes per k of the bf16 tiles the ring is twice as deep for the same LDS (NS
// stages; the fp32 epilogue tile sets the size at 128 x 128).  How the taps are walked is a compile-time policy, TapWalk8 below the
// arguments.  The counter walk: wave-uniform counters (cc, kh, kw), the tap's offset computed from (kh, kw, dil, pad) when its tile is
// issued, any KH, KW <= 16; a row's validity kept separably in one register: bit kh = kernel row kh lands on an image row for this
// pixel, bit 16 + kw = kernel column kw lands on an image column; a tap is inside the image exactly when both hold.  The table walk (up
// to 9 taps): the taps' offsets in the arguments and one mask bit per tap.
//
// MX = true stages one more item per stage: a dword per thread, of which the first BM hold the pixel rows' scale bytes.  The two bytes
// a tile row needs for chunk cc sit at byte pixel * (SC / 32) + 2 cc of the scale buffer, an even address: thread r < BM fetches the
// aligned dword around row r's with one 4-byte LDS-DMA, under the code rows' mask (zeros for a padded tap or a row past M: byte 0 x
// code 0 = +0); threads BM ... fetch zeros from the out-of-range offset, so that every wave issues the same number of DMA
// instructions per stage -- the wait in front of a stage counts them in vmcnt.  The lane that multiplies row r shifts the dword to its
// byte, (scale address & 3) + lh.  The multiply side runs NS - 1 tiles behind the issue side and keeps tap counters of its own for the
// tap's share of that address; the share is negative for leading taps and the sum is taken mod 4 in unsigned arithmetic.
// =================================================================================
struct GatherArgs8 {
    const unsigned char* src;      // e4m3 [B][SH][SW][SC]
    const unsigned char* src_sc;   // MX: E8M0 [B][SH][SW][SC / 32], from the dword boundary sc_delta bytes in front of it
    const unsigned char* wgt;      // e4m3 [tap][DN][SC]
    const float* bias;             // [DN] or nullptr
    const float* s_w;              // [DN] filter scales
    void* dst;                     // bf16 or fp32 [M][DN] (FP8_OUT_BF16, _F32, _BF16_E4M3, _BF16_MX: modes 0, 1, 3, 5)
    unsigned char* dst8;           // e4m3 [M][DN] (FP8_OUT_E4M3, _BF16_E4M3: modes 2, 3; MX: FP8_OUT_MX, _BF16_MX: modes 4, 5)
    unsigned char* dst_sc;         // MX: E8M0 [M][DN / 32] (modes 4, 5)
    float s_in, s_out;             // MX = false: the tensors' scales
    int M, DH, DW, DN;
    int SH, SW, SC;
    int KH, KW, dil, pad_h, pad_w;
    int mul, relu, mode, sc_delta;
    int m_fast, fast_n;            // workgroup order (launch_fwd_e4m3): pixel tiles fastest?, tiles along the fastest direction
    int ntaps, tap_dh[9], tap_dw[9];      // TapWalk8<true> only (up to 9 taps): KH * KW and every tap's offset in source pixels
};

// The tap walk: a compile-time policy of the one kernel body.  Both walk the tiles in the same k order (channel chunk outer, taps inner,
// kernel row major).  A walk is wave-uniform; mask() is what a staged row keeps, inside() turns it into all ones or zero for the
// current tap.
//   TapWalk8<false>: counters (cc, kh, kw), the tap's offset computed from (kh, kw, dil, pad), the separable mask (above the kernel).
//     Any KH, KW <= 16.
//   TapWalk8<true>: the tap table of the arguments, one mask bit per tap, (cc, tap) from the tile's number; up to 9 taps.  Kept for
//     the MX = false layers with up to 9 taps, where the counter walk lost on one layer.
template <bool TABLE>
struct TapWalk8;
template <>
struct TapWalk8<false> {
    int cc = 0, kh = 0, kw = 0;
    static __device__ __forceinline__ unsigned mask(const GatherArgs8& p, int rh, int rw) {
        unsigned mk = 0;
        for (int kh = 0; kh < p.KH; ++kh)
            if ((unsigned)(rh + kh * p.dil - p.pad_h) < (unsigned)p.SH) mk |= 1u << kh;
        for (int kw = 0; kw < p.KW; ++kw)
            if ((unsigned)(rw + kw * p.dil - p.pad_w) < (unsigned)p.SW) mk |= 0x10000u << kw;
        return mk;
    }
    // the tap against tap (0, 0) of an unpadded window, in pixels of the source; its index in the filter image
    __device__ __forceinline__ int pixel_offset(const GatherArgs8& p) const { return (kh * p.dil - p.pad_h) * p.SW + (kw * p.dil - p.pad_w); }
    __device__ __forceinline__ int filter_tap(const GatherArgs8& p) const { return kh * p.KW + kw; }
    __device__ __forceinline__ unsigned inside(unsigned mask) const {
        const unsigned sel = (1u << kh) | (0x10000u << kw);
        return 0u - (unsigned)((mask & sel) == sel);
    }
    __device__ __forceinline__ void advance(const GatherArgs8& p) {
        if (++kw == p.KW) {
            kw = 0;
            if (++kh == p.KH) {
                kh = 0;
                ++cc;
            }
        }
    }
};
template <>
struct TapWalk8<true> {
    int k = 0, cc = 0, tap = 0;
    static __device__ __forceinline__ unsigned mask(const GatherArgs8& p, int rh, int rw) {
        unsigned mk = 0;
        for (int t = 0; t < p.ntaps; ++t)
            if ((unsigned)(rh + p.tap_dh[t]) < (unsigned)p.SH && (unsigned)(rw + p.tap_dw[t]) < (unsigned)p.SW) mk |= 1u << t;
        return mk;
    }
    __device__ __forceinline__ int pixel_offset(const GatherArgs8& p) const { return p.tap_dh[tap] * p.SW + p.tap_dw[tap]; }
    __device__ __forceinline__ int filter_tap(const GatherArgs8&) const { return tap; }
    __device__ __forceinline__ unsigned inside(unsigned mask) const { return 0u - ((mask >> tap) & 1u); }
    __device__ __forceinline__ void advance(const GatherArgs8& p) {
        ++k;
        cc = k / p.ntaps;
        tap = k - cc * p.ntaps;
    }
};

// ---- The frame of conv_fwd_e4m3_kernel's body, one function per step, so that the kernel itself reads as what differs with MX and
// the tap walk: the staging, the fragment reads, the scale-byte shifts.
// output row -> its pixel at tap (0, 0), in pixels of the source
__device__ __forceinline__ int gather_pixel_of(const GatherArgs8& p, int m, int& rh, int& rw) {
    const int ow = m % p.DW;
    const int t2 = m / p.DW;
    const int oh = t2 % p.DH;
    const int b = t2 / p.DH;
    rh = oh * p.mul;
    rw = ow * p.mul;
    return b * p.SH * p.SW + rh * p.SW + rw;
}
// accumulators: D rows = output channels (filter operand first), D cols = pixels, as in conv_bf16.hip
template <int TM, int TN>
__device__ __forceinline__ void gather_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}
// the main loop: NS stages; tiles k+1 .. k+NS-1 stream in while tile k is multiplied.  L_N: DMA instructions per thread and stage
template <int NS, int L_N, typename Issue, typename Compute>
__device__ __forceinline__ void gather_ring(int nk, const Issue& issue_next, const Compute& compute) {
#pragma unroll
    for (int t = 0; t < NS - 1; ++t)
        if (t < nk) issue_next(t);
    int st_c = 0, st_i = NS - 1;
    for (int k = 0; k < nk; ++k) {
        const int later = nk - 1 - k;
        wait_tiles_and_sync<L_N, (NS - 2 > 4 ? 4 : NS - 2)>(later < NS - 2 ? later : NS - 2);      // tile k visible; stage st_i is free
        if (k + NS - 1 < nk) issue_next(st_i);
        compute(st_c);
        st_c = st_c + 1 == NS ? 0 : st_c + 1;
        st_i = st_i + 1 == NS ? 0 : st_i + 1;
    }
    __syncthreads();
}
// the accumulators into the fp32 LDS tile Cs [32 TM WM][LDC] of the epilogue, LDC = BN + 4
template <int TM, int TN, int LDC>
__device__ __forceinline__ void gather_acc_to_tile(float* Cs, const f32x16 (&acc)[TM][TN], int wm, int wn, int li, int lh) {
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
}
// The epilogue's row walk over that tile: y = relu?(acc * scale[co] + bias[co]) in fp32, scale = s_in * s_w (MX: s_w alone, the pixel
// scales went through the instruction), then one rounding per output format.  The arguments come by value: through a reference the
// output stores may alias them as far as the compiler knows, which costs the 64 x 64 instantiations two VGPRs.
template <bool MX, int NTHR, int BM, int BN>
__device__ __forceinline__ void gather_epilogue(const GatherArgs8 p, const float* Cs, int m0, int n0, int tid) {
    constexpr int LDC = BN + 4;
    constexpr int OUT8 = MX ? FP8_OUT_MX : FP8_OUT_E4M3, OUT16_8 = MX ? FP8_OUT_BF16_MX : FP8_OUT_BF16_E4M3;
    constexpr int TPR = BN / 8;               // threads per row, 8 channels each: a 32-channel MX block is 4 adjacent lanes
    constexpr int RPP = NTHR / TPR;           // rows per pass
    static_assert(TPR % 4 == 0, "a block's four lanes share a row");
    const int cg = tid % TPR, r0 = tid / TPR;
    const int n = n0 + cg * 8;
    if (n >= p.DN) return;                    // (an MX output has DN % 32 == 0: the four lanes of a block leave or stay together)
    float sc[8], bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if constexpr (MX) sc[e] = p.s_w[n + e];
        else sc[e] = p.s_in * p.s_w[n + e];
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
        } else if (p.mode != OUT8) {
            *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(p.dst) + o) =
                u32x4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
        }
        if (p.mode == OUT8 || p.mode == OUT16_8) {
            if constexpr (MX) {      // (a block's 32 bytes are its channels' bytes: the thread's 8 codes go to o)
                const int x = mx_block_exponent<MxE4M3>(v);
                *reinterpret_cast<u32x2*>(p.dst8 + o) = MxE4M3::pack8(v, x);
                if ((cg & 3) == 0) p.dst_sc[(size_t)m * (p.DN >> 5) + (n >> 5)] = (unsigned char)(x + 127);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = v[e] / p.s_out;
                *reinterpret_cast<u32x2*>(p.dst8 + o) = u32x2{pack4_e4m3(v[0], v[1], v[2], v[3]), pack4_e4m3(v[4], v[5], v[6], v[7])};
            }
        }
    }
}

template <bool MX, bool TABLE, int WM, int WN, int TM, int TN, int NS>
__global__ __launch_bounds__(64 * WM * WN) void conv_fwd_e4m3_kernel(GatherArgs8 pp) {
    const GatherArgs8& p = pp;
    constexpr int NTHR = 64 * WM * WN;
    constexpr int RPP_S = NTHR / 4;                   // tile rows one staging pass covers (4 lanes per 64-byte row)
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int A_N = BM / RPP_S, B_N = BN / RPP_S; // DMA instructions per thread and tile
    constexpr int L_N = A_N + B_N + (MX ? 1 : 0);     // ... and per stage: what the wait in front of a stage counts
    constexpr int CODES = (BM + BN) * KB8;
    constexpr int STAGE = CODES + (MX ? NTHR * 4 : 0);      // + the scale dwords
    static_assert(BM % RPP_S == 0 && BN % RPP_S == 0 && RPP_S % 16 == 0 && (!MX || BM <= NTHR), "tile vs staging pass");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int slow = wg / p.fast_n, fast = wg - slow * p.fast_n;      // (wave-uniform; the order: launch_fwd_e4m3)
    const int mt = p.m_fast ? fast : slow, nt = p.m_fast ? slow : fast;
    const int m0 = mt * BM, n0 = nt * BN;
    const int SB = p.SC >> 5;                         // MX: scale bytes per pixel (even: SC is a multiple of 64)

    using Walk = TapWalk8<TABLE>;

    // ---- staging: thread -> rows (tid >> 2) + RPP_S i, LDS slot tid & 3, global chunk slot ^ ((row >> 2) & 3)
    const int a_ck = ((tid & 3) ^ ((tid >> 4) & 3)) * 16;
    unsigned a_off[A_N], a_msk[A_N];
#pragma unroll
    for (int i = 0; i < A_N; ++i) {
        const int m = m0 + (tid >> 2) + RPP_S * i;
        int rh, rw;
        const int pix = gather_pixel_of(p, m < p.M ? m : 0, rh, rw);
        a_off[i] = (unsigned)(pix * p.SC + a_ck);
        a_msk[i] = m < p.M ? Walk::mask(p, rh, rw) : 0u;
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
    if constexpr (MX)
        if (tid < BM && m0 + tid < p.M) {
            int rh, rw;
            s_off = (unsigned)(gather_pixel_of(p, m0 + tid, rh, rw) * SB + p.sc_delta);
            s_msk = Walk::mask(p, rh, rw);
        }
    const size_t src_pixels = (size_t)(p.M / (p.DH * p.DW)) * p.SH * p.SW;
    const __amdgpu_buffer_rsrc_t src_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.src), 0, (unsigned)(src_pixels * p.SC), 0x00020000);
    const __amdgpu_buffer_rsrc_t wgt_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.wgt), 0,
                                                                              (unsigned)((size_t)p.KH * p.KW * p.DN * p.SC), 0x00020000);
    // (rounded up to whole dwords: the last pixel's dword may end two bytes behind the tensor, inside its allocation -- conv.h)
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t sc_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(p.src_sc), 0, MX ? (unsigned)((src_pixels * SB + p.sc_delta + 3) & ~(size_t)3) : 0u, 0x00020000);

    const int nk = (p.SC / KB8) * p.KH * p.KW;      // SC is a multiple of 64 (host check): no channel-chunk mask

    // tiles are issued in k order: `iw` is at the next one
    Walk iw;
    auto issue_next = [&](int stage) {
        unsigned char* As = smem + stage * STAGE + wave * 1024;        // wave-uniform: 16 rows x 64 B per DMA
        unsigned char* Bs = As + BM * KB8;
        const int tpix = iw.pixel_offset(p);
        const unsigned toff = (unsigned)(tpix * p.SC + iw.cc * KB8);
#pragma unroll
        for (int i = 0; i < A_N; ++i) {
            const unsigned m = iw.inside(a_msk[i]);
            const unsigned off = ((a_off[i] + toff) & m) | (OOB8 & ~m);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rsrc, LDS_PTR8(As + i * (RPP_S * KB8)), 16, off, 0, 0, 0);
        }
        const unsigned woff = (unsigned)(iw.filter_tap(p) * p.DN * p.SC + iw.cc * KB8);
#pragma unroll
        for (int i = 0; i < B_N; ++i) {
            const unsigned m = b_ok[i];
            const unsigned off = ((b_off[i] + woff) & m) | (OOB8 & ~m);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wgt_rsrc, LDS_PTR8(Bs + i * (RPP_S * KB8)), 16, off, 0, 0, 0);
        }
        if constexpr (MX) {
            const unsigned m = iw.inside(s_msk);
            const unsigned off = ((s_off + (unsigned)(tpix * SB + 2 * iw.cc)) & ~3u & m) | (OOB8 & ~m);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(sc_rsrc, LDS_PTR8(smem + stage * STAGE + CODES + wave * 256), 4, off, 0, 0, 0);
        }
        iw.advance(p);
    };

    f32x16 acc[TM][TN];
    gather_zero(acc);
    const int wm = wave / WN, wn = wave - wm * WN;
    const int li = lane & 31, lh = lane >> 5;
    // fragment = two chunks of row li, a fixed distance apart (the chunk assignment: above the kernel)
    constexpr int PAIR = MX ? 32 : 16;
    const int q0 = ((MX ? lh : 2 * lh) ^ ((li >> 2) & 3)) * 16;
    const int a_row = (wm * 32 * TM + li) * KB8 + q0;
    const int b_row = BM * KB8 + (wn * 32 * TN + li) * KB8 + q0;
    // MX: byte of this lane's scale inside its row's dword = (scale address & 3) + lh; the row's share of the address, mod 4:
    [[maybe_unused]] unsigned s_rb[TM];
    if constexpr (MX) {
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            const int m = m0 + wm * 32 * TM + mi * 32 + li;
            int rh, rw;
            s_rb[mi] = (unsigned)(gather_pixel_of(p, m < p.M ? m : 0, rh, rw) * SB + p.sc_delta);
        }
    }

    auto load_frag = [&](const unsigned char* S, int addr) -> i32x8 {
        const i32x4 lo = *reinterpret_cast<const i32x4*>(S + addr);
        const i32x4 hi = *reinterpret_cast<const i32x4*>(S + (addr ^ PAIR));
        return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    [[maybe_unused]] Walk cw;      // MX: at the tile being multiplied
    auto compute = [&](int stage) {
        const unsigned char* S = smem + stage * STAGE;
        [[maybe_unused]] const unsigned* Sc = reinterpret_cast<const unsigned*>(S + CODES);
        [[maybe_unused]] const unsigned s_tb = MX ? (unsigned)(cw.pixel_offset(p) * SB + 2 * cw.cc) : 0u;
        i32x8 a[TM], b[TN];
        int sa[TM];      // the pixel operand's scale bytes
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            a[mi] = load_frag(S, a_row + mi * 32 * KB8);
            if constexpr (MX) sa[mi] = (int)(Sc[wm * 32 * TM + mi * 32 + li] >> (8 * (((s_rb[mi] + s_tb) & 3u) + lh)));
            else sa[mi] = SCALE_ONE;
        }
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) b[ni] = load_frag(S, b_row + ni * 32 * KB8);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b[ni], a[mi], acc[mi][ni], 0, 0, 0, SCALE_ONE, 0, sa[mi]);
        if constexpr (MX) cw.advance(p);
    };

    gather_ring<NS, L_N>(nk, issue_next, compute);

    // ---- epilogue through an fp32 LDS tile [BM][BN + 4]
    float* Cs = reinterpret_cast<float*>(smem);
    gather_acc_to_tile<TM, TN, BN + 4>(Cs, acc, wm, wn, li, lh);
    gather_epilogue<MX, NTHR, BM, BN>(p, Cs, m0, n0, tid);
}

// =================================================================================
// The host path.  An entry point of conv.h is a format and a tap range: 1 ... 9 taps, or 10 ... 121 (`bigk`: the fc graph's 7 x 7 fc6,
// e4m3 only).
// =================================================================================
// One launcher for the gather kernels: KERN with NTHR threads per BM x BN tile and STAGES bytes of LDS for its ring.
template <auto KERN, int NTHR, int BM, int BN, size_t STAGES, typename Args>
static void launch_gather(Args& a, bool m_fast, const char* label, double flops, double bytes, hipStream_t s) {
    constexpr size_t ctile = (size_t)BM * (BN + 4) * 4, lds = STAGES > ctile ? STAGES : ctile;
    static_assert(lds <= 80 * 1024, "LDS: two workgroups per CU");
    static bool once = (set_lds(KERN, lds), true);
    (void)once;
    // Workgroup order.  Consecutive workgroups share an XCD's L2 (xcd_remap).  With filter columns fastest the workgroups resident on an
    // XCD cover every column, and each row of pixel tiles streams the whole filter image: MT x its bytes in all.  With pixel tiles fastest
    // they share one column, and each column streams the input: NT x its bytes.  A column of a filter with more than 9 taps (taps x BN x
    // Ci bytes) is always larger than a pixel tile's input (about BM x Ci), so those layers take pixel tiles fastest; up to 9 taps keep
    // filter columns fastest.  fc6 at batch 128 (102 MB of filter, 24 MB of input, MT 361, NT 32): 4.92 against 9.70 ms.
    const int MT = cdiv(a.M, BM), NT = cdiv(a.DN, BN);
    a.m_fast = m_fast;
    a.fast_n = m_fast ? MT : NT;
    ProfScope prof(label, flops, bytes, s);
    SSD_LAUNCH_STOP(KERN, dim3(MT * NT), dim3(NTHR), lds, s, a);
    HIP_OK(hipGetLastError());
}
template <bool MX, bool TABLE, int WM, int WN, int TM, int TN, int NS>
static void launch_fwd_e4m3(GatherArgs8& a, bool bigk, const char* label, double flops, double bytes, hipStream_t s) {
    constexpr int NTHR = 64 * WM * WN, BM = 32 * TM * WM, BN = 32 * TN * WN;
    launch_gather<conv_fwd_e4m3_kernel<MX, TABLE, WM, WN, TM, TN, NS>, NTHR, BM, BN, NS * ((size_t)(BM + BN) * KB8 + (MX ? NTHR * 4 : 0))>(
        a, bigk, label, flops, bytes, s);
}

// Why an entry point refuses a layer, or nullptr: a string literal "<fmt> conv[ (more than 9 taps)]: reason" (fmt = "fp8" / "mxfp8" /
// "mxfp6").  out_mode < 0: the shape alone.  An MX output needs whole 32-channel blocks, and the scale tensors of mxfp8 stay below the
// offset guard too.  mxfp6 has no kernel for more than 9 taps, so no `bigk` and one text of its own for every tap count it cannot run.
enum QuantFmt { FMT_FP8, FMT_MXFP8, FMT_MXFP6 };
#define QUANT_WHY(text)                                                                                           \
    (fmt == FMT_MXFP6 ? "mxfp6 conv: " text                                                                       \
     : fmt == FMT_MXFP8 ? (bigk ? "mxfp8 conv (more than 9 taps): " text : "mxfp8 conv: " text)                   \
                        : (bigk ? "fp8 conv (more than 9 taps): " text : "fp8 conv: " text))
inline const char* conv_quant_refusal(QuantFmt fmt, bool bigk, const ConvDesc& d, int out_mode) {
    const long long taps = (long long)d.KH * d.KW;
    const bool mx = fmt != FMT_FP8;
    const bool wants_mx = out_mode == FP8_OUT_MX || out_mode == FP8_OUT_BF16_MX;
    const bool mode_ok = out_mode == FP8_OUT_BF16 || out_mode == FP8_OUT_F32 ||
                         (mx ? wants_mx : out_mode == FP8_OUT_E4M3 || out_mode == FP8_OUT_BF16_E4M3);
    if (fmt == FMT_MXFP6) {
        if (d.KH < 1 || d.KW < 1 || taps > 9) return QUANT_WHY("at most 9 taps (a layer with more stays on its bf16 kernel: there is no mxfp6 kernel for it)");
    } else {
        if (d.KH < 1 || d.KW < 1 || d.KH > 11 || d.KW > 11) return QUANT_WHY("KH and KW must be in 1 ... 11");
        if (bigk && taps <= 9)      // (a wrong tap count names the entry point that runs it)
            return mx ? QUANT_WHY("9 taps or fewer run on conv_fwd_mxfp8 (ssd_op_conv2d_fwd_mxfp8)") : QUANT_WHY("9 taps or fewer run on conv_fwd_fp8 (ssd_op_conv2d_fwd_fp8)");
        if (!bigk && taps > 9)
            return mx ? QUANT_WHY("more than 9 taps run on conv_bigk_fwd_mxfp8 (ssd_op_conv2d_fwd_mxfp8_bigk)")
                      : QUANT_WHY("more than 9 taps run on conv_bigk_fwd_fp8 (ssd_op_conv2d_fwd_fp8_bigk)");
    }
    if (d.Ci < 64 || d.Ci % 64 != 0) return QUANT_WHY("Ci must be a multiple of 64");
    if (d.Co < 8 || d.Co % 8 != 0) return QUANT_WHY("Co must be a multiple of 8");
    if (d.stride < 1 || d.dil < 1) return QUANT_WHY("stride and dilation must be positive");
    if (d.B < 1 || d.Ho < 1 || d.Wo < 1 || d.Hi < 1 || d.Wi < 1) return QUANT_WHY("empty tensor");
    if ((long long)d.B * d.Hi * d.Wi * d.Ci >= (1LL << 31) - 16 || (long long)d.B * d.Ho * d.Wo * d.Co >= (1LL << 31) - 16)
        return QUANT_WHY("a tensor of this layer exceeds the 32-bit offsets: lower the batch");
    if (taps * d.Co * d.Ci >= (1LL << 31) - 16) return QUANT_WHY("the filter image exceeds the 32-bit offsets");
    if (fmt == FMT_MXFP8 && ((long long)d.B * d.Hi * d.Wi * (d.Ci / 32) + 8 >= (1LL << 31) - 16 || (long long)d.B * d.Ho * d.Wo * (d.Co / 32) >= (1LL << 31) - 16))
        return QUANT_WHY("a scale tensor of this layer exceeds the 32-bit offsets: lower the batch");
    if (out_mode >= 0 && !mode_ok) return QUANT_WHY("unknown output mode");
    if (out_mode >= 0 && wants_mx && d.Co % 32 != 0) return QUANT_WHY("an MX output needs Co to be a multiple of 32");
    return nullptr;
}
#undef QUANT_WHY

// ---- the host prologue of every gather entry point: the refusal as an error, the geometry, the scale pointers, the tile
inline void require_conv_quant(QuantFmt fmt, bool bigk, const ConvDesc& d, int out_mode) {
    const char* why = conv_quant_refusal(fmt, bigk, d, out_mode);
    SSD_REQUIRE(why == nullptr, "%s (got %dx%d taps, Ci %d, Co %d, output mode %d)", why, d.KH, d.KW, d.Ci, d.Co, out_mode);
}
inline void gather_geometry(GatherArgs8& a, const ConvDesc& d, int out_mode, bool relu) {
    a.M = d.B * d.Ho * d.Wo; a.DH = d.Ho; a.DW = d.Wo; a.DN = d.Co;
    a.SH = d.Hi; a.SW = d.Wi; a.SC = d.Ci;
    a.KH = d.KH; a.KW = d.KW; a.dil = d.dil; a.pad_h = d.pad_h; a.pad_w = d.pad_w;
    a.mul = d.stride; a.relu = relu; a.mode = out_mode;
}
// a scale tensor is fetched in aligned dwords, and a sample's scales inside a batch may start between two: the dword boundary in
// front of `sc`, and in `delta` how far in front
inline const unsigned char* dword_base(const unsigned char* sc, int& delta) {
    delta = (int)(reinterpret_cast<uintptr_t>(sc) & 3);
    return sc - delta;
}
// Tiles: 0 = 128 x 128 (the fp32 epilogue tile's 66 KB sets the allocation: two workgroups per CU); 1 = 64 x 64, six stages, where the
// 128 x 128 tiling would leave CUs empty.  SSD_TILE_FP8 forces one (tests, tuning).
inline int gather_tile(const GatherArgs8& a) {
    const int cfg = env_int("SSD_TILE_FP8", -1);
    return cfg == 0 || cfg == 1 ? cfg : (long long)cdiv(a.M, 128) * cdiv(a.DN, 128) <= 256 ? 1 : 0;
}

// What an entry point passes on: the operands in `a` (src, src_sc, wgt, bias, s_w, dst, dst8, dst_sc, s_in, s_out), the rest is filled
// here.  128 x 128 runs four stages of 16 KB.
template <bool MX>
static void conv_fwd_e4m3(bool bigk, const ConvDesc& d, GatherArgs8 a, int out_mode, bool relu, hipStream_t s) {
    require_conv_quant(MX ? FMT_MXFP8 : FMT_FP8, bigk, d, out_mode);
    const bool wants8 = out_mode == (MX ? FP8_OUT_MX : FP8_OUT_E4M3) || out_mode == (MX ? FP8_OUT_BF16_MX : FP8_OUT_BF16_E4M3);
    if constexpr (MX) {
        SSD_REQUIRE(!wants8 || (a.dst8 != nullptr && a.dst_sc != nullptr), "mxfp8 conv: an MX output needs its code and scale buffers");
        SSD_REQUIRE(out_mode == FP8_OUT_MX || a.dst != nullptr, "mxfp8 conv: null output");
        SSD_REQUIRE(a.src && a.src_sc && a.wgt && a.s_w, "mxfp8 conv: null operand");
        SSD_REQUIRE(reinterpret_cast<uintptr_t>(a.src_sc) % 2 == 0, "mxfp8 conv: the scale buffer must start at an even address");
        a.src_sc = dword_base(a.src_sc, a.sc_delta);
    } else {
        SSD_REQUIRE(!wants8 || (a.dst8 != nullptr && a.s_out > 0.f), "fp8 conv: an e4m3 output needs its buffer and a positive scale");
        SSD_REQUIRE(out_mode == FP8_OUT_E4M3 || a.dst != nullptr, "fp8 conv: null output");
        SSD_REQUIRE(a.src && a.wgt && a.s_w && a.s_in > 0.f, "fp8 conv: null operand or non-positive input scale");
        if (!wants8) a.s_out = 1.f;
    }
    gather_geometry(a, d, out_mode, relu);
    if (!bigk) {
        a.ntaps = d.KH * d.KW;
        for (int kh = 0; kh < d.KH; ++kh)
            for (int kw = 0; kw < d.KW; ++kw) {
                a.tap_dh[kh * d.KW + kw] = kh * d.dil - d.pad_h;
                a.tap_dw[kh * d.KW + kw] = kw * d.dil - d.pad_w;
            }
    }
    const double fl = conv_flops(d);
    const double sc_b = MX ? 1.0 / 32 : 0.0;      // scale bytes per code byte
    const double out_b = out_mode == FP8_OUT_F32 ? 4.0 : out_mode == FP8_OUT_BF16 ? 2.0 : (out_mode == FP8_OUT_BF16_E4M3 || out_mode == FP8_OUT_BF16_MX ? 3.0 : 1.0) + sc_b;
    const double by = (double)d.B * d.Hi * d.Wi * d.Ci * (1.0 + sc_b) + (double)d.KH * d.KW * d.Ci * d.Co + (double)d.B * d.Ho * d.Wo * d.Co * out_b;
    static const char* const LABEL[2][2][2] = {{{"conv_fwd_fp8_128x128", "conv_fwd_fp8_64x64x6"}, {"conv_bigk_fwd_fp8_128x128", "conv_bigk_fwd_fp8_64x64x6"}},
                                               {{"conv_fwd_mxfp8_128x128", "conv_fwd_mxfp8_64x64x6"}, {"conv_bigk_fwd_mxfp8_128x128", "conv_bigk_fwd_mxfp8_64x64x6"}}};
    const int cfg = gather_tile(a);
    // the tap walk (TapWalk8): the table for MX = false up to 9 taps, the counters everywhere else
    if constexpr (!MX)
        if (!bigk) {
            if (cfg == 0) launch_fwd_e4m3<MX, true, 2, 2, 2, 2, 4>(a, bigk, LABEL[MX][bigk][0], fl, by, s);
            else launch_fwd_e4m3<MX, true, 2, 2, 1, 1, 6>(a, bigk, LABEL[MX][bigk][1], fl, by, s);
            return;
        }
    if (cfg == 0) launch_fwd_e4m3<MX, false, 2, 2, 2, 2, 4>(a, bigk, LABEL[MX][bigk][0], fl, by, s);
    else launch_fwd_e4m3<MX, false, 2, 2, 1, 1, 6>(a, bigk, LABEL[MX][bigk][1], fl, by, s);
}

// =================================================================================
// The table of a filter-quantisation launch that covers several layers (quantize_filters_fp8_kernel, quantize_filters_mxfp6_kernel): a
// workgroup finds its layer by its number.
// =================================================================================
struct QuantTable {
    int n;
    struct Seg {
        unsigned long long off, off8, offs;      // fp32 filter (elements), code image (bytes), scales (elements of their type)
        int taps, ci, co;
        int blk0;                                // first workgroup of this layer
    } seg[FilterQuantPlan::MAX_LAYERS];
};
// the plan's layers that belong(L), at blocks(L) workgroups each; returns the grid.  elems: the elements of all layers of the plan
template <typename Belongs, typename Blocks>
static int fill_quant_table(QuantTable& t, const FilterQuantPlan& plan, double& elems, const Belongs& belongs, const Blocks& blocks) {
    int blk = 0;
    t.n = 0;
    elems = 0;
    for (int i = 0; i < plan.n; ++i) {
        const FilterQuantPlan::Layer& L = plan.L[i];
        elems += (double)L.taps * L.ci * L.co;
        if (!belongs(L)) continue;
        QuantTable::Seg& g = t.seg[t.n++];
        g.off = L.off; g.off8 = L.off8; g.offs = L.offs;
        g.taps = L.taps; g.ci = L.ci; g.co = L.co;
        g.blk0 = blk;
        blk += blocks(L);
    }
    return blk;
}

}  // namespace ssd
