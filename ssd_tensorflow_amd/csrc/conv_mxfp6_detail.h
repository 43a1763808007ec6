// The forward gather convolution on e2m3 (OCP MX FP6) operands for gfx950 (MI355X): the staging of 48-byte rows, the fragments and the
// scales on both operands.  DESIGN.md 24.  Included by conv_mxfp6.hip alone; the tap walks, the stage wait, the launcher and the
// operand types are conv_fp8_detail.h's, the format (scale rule, encoder, 24-byte block store) is mx_block.h's MxE2M3.  The kernel's
// body is written out here and does not use the gather_* frame of conv_fp8_detail.h: with the frame its 64 x 64 instantiation measured
// 0.2 ... 0.4 us slower per launch at batch 1, with this text its instructions are the earlier kernel's one for one.
#pragma once
#include "conv_fp8_detail.h"

namespace ssd {

constexpr int KB6 = 48;      // bytes per tile row: 64 channels = two 24-byte blocks = three 16-byte LDS-DMA units

// =================================================================================
// The kernel: conv_fp8_detail.h's gather convolution restated for e2m3 operands with E8M0 block scales on BOTH operands
// (v_mfma_scale_f32_32x32x64_f8f6f4, format selector 2 on both, 6 registers each).  Products of two e2m3 numbers and powers of two are
// exact in fp32, the MFMA adds in fp32, the epilogue is y = relu?(acc + bias[co]) in fp32 with one rounding per output format.
//
// Operand layout (tools/probes/mxfp6_probe.hip measures it): lane l holds row l & 31 of its operand and 32 of the 64 k as 32 six-bit
// fields, field f in bits 6 f ... 6 f + 5 of the 192 bits, register 0 first.  The lane's scale byte multiplies exactly the lane's own
// 32 fields, on either operand, and the two operands pair field f of lane half h with field f of lane half h.  So a lane's registers are
// one MX block as it lies in HBM: lane (r, h) reads block h of row r's 64-channel chunk, 24 consecutive bytes, with no permutation,
// and takes that block's scale byte.  (Which 32 of the instruction's 64 k a lane half feeds, in the e4m3 layout's names, does not
// matter to a dot product whose two operands agree.)
//
// A tile row is 64 channels = 48 bytes = three 16-byte units.  LDS-DMA writes lane-linear (16 bytes per lane, 1 KB per wave and
// instruction), so the BM pixel rows and the BN filter rows of a stage are ONE array of 3 (BM + BN) units in row order, unit u = 3 row +
// chunk at byte 16 u, staged by thread u mod NTHR in pass u / NTHR.  3 BM is a multiple of 64, so a wave's instruction lies in the
// pixel rows or in the filter rows as a whole and its buffer descriptor is wave-uniform.  The last pass may reach past the array (64 x
// 64: 384 units in two passes of 256): those lanes fetch zeros into the stage's padding, so that every wave issues the same number of
// DMA instructions per stage -- the wait in front of a stage counts them in vmcnt.  Padded taps, rows past M and filter rows past Co
// fetch zeros from an out-of-range offset: code 0 = +0 under scale byte 0.
//
// Scales: one more dword per thread and stage.  Threads 0 ... BM - 1 fetch the aligned dword around the two scale bytes of their pixel
// row's chunk (byte pixel * (SC / 32) + 2 cc of the scale tensor, an even address), threads BM ... BM + BN - 1 the one around their
// filter row's (byte (tap * Co + co) * (SC / 32) + 2 cc), the rest zeros.  The lane that multiplies a row shifts the dword to its byte,
// (scale address & 3) + h; the multiply side keeps a tap walk of its own for the tile's share of that address, as in the e4m3 kernel.
//
// A fragment is one ds_read_b128 and one ds_read_b64: lane half 0 takes the row's unit 0 and the first half of unit 1, lane half 1 the
// second half of unit 1 and unit 2, put in order by six selects.  Rows are 12 banks apart, so rows r and r + 16 start on the same bank.
// A ds_read_b128 lane group holds 16 rows that differ mod 16 (MI355X LDS banking): their units lie on the 16 different 4-bank slots,
// conflict-free.  The 32 lanes of a ds_read_b64 group hold rows r and r + 16: 2-way, and with 48-byte rows no placement of rows or
// units avoids it (an 8-byte piece at a fixed offset of a row has 16 possible bank positions for 32 lanes).  8 LDS cycles per fragment
// against 12 for three ds_read_b64 (the first form of this kernel) and 6 without any conflict.
// =================================================================================
struct GatherArgs6 : GatherArgs8 {      // src / wgt: packed codes; src_sc: the pixel scales; s_w, s_in, s_out, tap tables: unused
    const unsigned char* wgt_sc;        // E8M0 [tap][DN][SC / 32], from the dword boundary wsc_delta bytes in front of it
    int wsc_delta;
};

template <int WM, int WN, int TM, int TN, int NS>
__global__ __launch_bounds__(64 * WM * WN) void conv_fwd_mxfp6_kernel(GatherArgs6 pp) {
    const GatherArgs6& p = pp;
    constexpr int NTHR = 64 * WM * WN;
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int UNITS = 3 * (BM + BN);                     // 16-byte units per stage
    constexpr int NP = (UNITS + NTHR - 1) / NTHR;            // DMA passes per stage
    constexpr int CODES = NP * NTHR * 16;                    // (with the padding the last pass fills with zeros)
    constexpr int STAGE = CODES + NTHR * 4;                  // + the scale dwords
    constexpr int L_N = NP + 1;                              // DMA instructions per thread and stage
    constexpr int LDC = BN + 4;
    static_assert((3 * BM) % 64 == 0 && BM % 64 == 0 && BM + BN <= NTHR, "a wave's DMA instruction lies in one operand");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int slow = wg / p.fast_n, fast = wg - slow * p.fast_n;
    const int mt = p.m_fast ? fast : slow, nt = p.m_fast ? slow : fast;
    const int m0 = mt * BM, n0 = nt * BN;
    const int SB = p.SC >> 5;                                // scale bytes per row (even: SC is a multiple of 64)
    const int RB = SB * 24;                                  // code bytes per row

    auto pixel_of = [&](int m, int& rh, int& rw) {
        const int ow = m % p.DW;
        const int t2 = m / p.DW;
        const int oh = t2 % p.DH;
        const int b = t2 / p.DH;
        rh = oh * p.mul;
        rw = ow * p.mul;
        return b * p.SH * p.SW + rh * p.SW + rw;
    };
    using Walk = TapWalk8<false>;

    // ---- staging: pass i, thread tid -> unit u = i NTHR + tid = 3 row + chunk.  A filter row's mask is all ones (inside every tap) or 0.
    unsigned st_off[NP], st_msk[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int u = i * NTHR + tid;
        const int row = u / 3, ck = u - 3 * row;
        st_off[i] = 0u;
        st_msk[i] = 0u;
        if (u < 3 * BM) {
            const int m = m0 + row;
            int rh, rw;
            const int pix = pixel_of(m < p.M ? m : 0, rh, rw);
            st_off[i] = (unsigned)(pix * RB + ck * 16);
            if (m < p.M) st_msk[i] = Walk::mask(p, rh, rw);
        } else if (u < UNITS) {
            const int n = n0 + row - BM;
            if (n < p.DN) {
                st_off[i] = (unsigned)(n * RB + ck * 16);
                st_msk[i] = ~0u;
            }
        }
    }
    unsigned s_off = 0, s_msk = 0;
    if (tid < BM) {
        if (m0 + tid < p.M) {
            int rh, rw;
            s_off = (unsigned)(pixel_of(m0 + tid, rh, rw) * SB + p.sc_delta);
            s_msk = Walk::mask(p, rh, rw);
        }
    } else if (tid < BM + BN && n0 + tid - BM < p.DN) {
        s_off = (unsigned)((n0 + tid - BM) * SB + p.wsc_delta);
        s_msk = ~0u;
    }
    const size_t src_pixels = (size_t)(p.M / (p.DH * p.DW)) * p.SH * p.SW;
    const size_t wgt_rows = (size_t)p.KH * p.KW * p.DN;
    const __amdgpu_buffer_rsrc_t src_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.src), 0, (unsigned)(src_pixels * RB), 0x00020000);
    const __amdgpu_buffer_rsrc_t wgt_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.wgt), 0, (unsigned)(wgt_rows * RB), 0x00020000);
    // (rounded up to whole dwords: the last row's dword may end two bytes behind the tensor, inside its allocation -- conv.h)
    const __amdgpu_buffer_rsrc_t sc_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(p.src_sc), 0, (unsigned)((src_pixels * SB + p.sc_delta + 3) & ~(size_t)3), 0x00020000);
    const __amdgpu_buffer_rsrc_t wsc_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(p.wgt_sc), 0, (unsigned)((wgt_rows * SB + p.wsc_delta + 3) & ~(size_t)3), 0x00020000);

    const int nk = (p.SC / 64) * p.KH * p.KW;

    Walk iw;      // tiles are issued in k order: `iw` is at the next one
    auto issue_next = [&](int stage) {
        unsigned char* S = smem + stage * STAGE + wave * 1024;        // wave-uniform: 64 units per DMA
        const int tpix = iw.pixel_offset(p), ftap = iw.filter_tap(p);
        const unsigned toff = (unsigned)(tpix * RB + iw.cc * KB6), woff = (unsigned)(ftap * p.DN * RB + iw.cc * KB6);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const bool pixels = i * NTHR + 64 * wave < 3 * BM;        // wave-uniform
            const unsigned m = iw.inside(st_msk[i]);
            const unsigned off = ((st_off[i] + (pixels ? toff : woff)) & m) | (OOB8 & ~m);
            if (pixels) __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rsrc, LDS_PTR8(S + i * (NTHR * 16)), 16, off, 0, 0, 0);
            else __builtin_amdgcn_raw_ptr_buffer_load_lds(wgt_rsrc, LDS_PTR8(S + i * (NTHR * 16)), 16, off, 0, 0, 0);
        }
        {
            const bool pixels = 64 * wave < BM;                       // wave-uniform
            const unsigned m = iw.inside(s_msk);
            const unsigned share = (unsigned)((pixels ? tpix : ftap * p.DN) * SB + 2 * iw.cc);
            const unsigned off = ((s_off + share) & ~3u & m) | (OOB8 & ~m);
            unsigned char* Sc = smem + stage * STAGE + CODES + wave * 256;
            if (pixels) __builtin_amdgcn_raw_ptr_buffer_load_lds(sc_rsrc, LDS_PTR8(Sc), 4, off, 0, 0, 0);
            else __builtin_amdgcn_raw_ptr_buffer_load_lds(wsc_rsrc, LDS_PTR8(Sc), 4, off, 0, 0, 0);
        }
        iw.advance(p);
    };

    // ---- accumulators: D rows = output channels (filter operand first), D cols = pixels, as in the e4m3 kernel
    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int wm = wave / WN, wn = wave - wm * WN;
    const int li = lane & 31, lh = lane >> 5;
    const int a_row = (wm * 32 * TM + li) * KB6;
    const int b_row = (BM + wn * 32 * TN + li) * KB6;
    // byte of this lane's scale inside its row's dword = (scale address & 3) + lh; the row's share of the address:
    unsigned s_ra[TM], s_rb[TN];
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
        const int m = m0 + wm * 32 * TM + mi * 32 + li;
        int rh, rw;
        s_ra[mi] = (unsigned)(pixel_of(m < p.M ? m : 0, rh, rw) * SB + p.sc_delta);
    }
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) s_rb[ni] = (unsigned)((n0 + wn * 32 * TN + ni * 32 + li) * SB + p.wsc_delta);

    // block lh of the row at `addr`: the row's outer 16-byte unit (unit 0 or 2) and the half of the middle unit next to it
    // (the middle halves' addresses are kept in registers the compiler cannot relate to each other: two ds_read_b64 off one base
    // would be merged into a ds_read2_b64, which banks mod 32)
    int a_mid[TM], b_mid[TN];
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
        a_mid[mi] = a_row + mi * 32 * KB6 + 16 + 8 * lh;
        asm volatile("" : "+v"(a_mid[mi]));
    }
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
        b_mid[ni] = b_row + ni * 32 * KB6 + 16 + 8 * lh;
        asm volatile("" : "+v"(b_mid[ni]));
    }
    auto load_frag = [&](const unsigned char* S, int addr, int mid) -> i32x8 {
        const u32x4 q = *reinterpret_cast<const u32x4*>(S + addr + 32 * lh);
        const u32x2 d = *reinterpret_cast<const u32x2*>(S + mid);
        return lh ? i32x8{(int)d[0], (int)d[1], (int)q[0], (int)q[1], (int)q[2], (int)q[3], 0, 0}
                  : i32x8{(int)q[0], (int)q[1], (int)q[2], (int)q[3], (int)d[0], (int)d[1], 0, 0};
    };
    Walk cw;      // at the tile being multiplied
    auto compute = [&](int stage) {
        const unsigned char* S = smem + stage * STAGE;
        const unsigned* Sc = reinterpret_cast<const unsigned*>(S + CODES);
        const unsigned s_ta = (unsigned)(cw.pixel_offset(p) * SB + 2 * cw.cc), s_tb = (unsigned)(cw.filter_tap(p) * p.DN * SB + 2 * cw.cc);
        i32x8 a[TM], b[TN];
        int sa[TM], sb[TN];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            a[mi] = load_frag(S, a_row + mi * 32 * KB6, a_mid[mi]);
            sa[mi] = (int)(Sc[wm * 32 * TM + mi * 32 + li] >> (8 * (((s_ra[mi] + s_ta) & 3u) + lh)));
        }
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
            b[ni] = load_frag(S, b_row + ni * 32 * KB6, b_mid[ni]);
            sb[ni] = (int)(Sc[BM + wn * 32 * TN + ni * 32 + li] >> (8 * (((s_rb[ni] + s_tb) & 3u) + lh)));
        }
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b[ni], a[mi], acc[mi][ni], 2, 2, 0, sb[ni], 0, sa[mi]);
        cw.advance(p);
    };

    // ---- main loop: NS stages; tiles k+1 .. k+NS-1 stream in while tile k is multiplied
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

    // ---- epilogue through an fp32 LDS tile [BM][BN + 4]: y = relu?(acc + bias[co]), then one rounding per output format
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
    constexpr int TPR = BN / 8;               // threads per row, 8 channels each: a 32-channel MX block is 4 adjacent lanes
    constexpr int RPP = NTHR / TPR;           // rows per pass
    static_assert(TPR % 4 == 0, "a block's four lanes share a row");
    const int cg = tid % TPR, r0 = tid / TPR;
    const int n = n0 + cg * 8;
    if (n >= p.DN) return;                    // (an MX output has DN % 32 == 0: the four lanes of a block leave or stay together)
    float bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = p.bias ? p.bias[n + e] : 0.f;
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
            v[e] = v[e] + bv[e];
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
            const int x = mx_block_exponent<MxE2M3>(v);
            const size_t blk = (size_t)m * (p.DN >> 5) + (n >> 5);
            MxE2M3::store8(p.dst8, blk, cg & 3, MxE2M3::pack8(v, x));
            if ((cg & 3) == 0) p.dst_sc[blk] = (unsigned char)(x + 127);
        }
    }
}

// filter columns fastest, as the e4m3 kernel does up to 9 taps (launch_gather)
template <int WM, int WN, int TM, int TN, int NS>
static void launch_fwd_mxfp6(GatherArgs6& a, const char* label, double flops, double bytes, hipStream_t s) {
    constexpr int NTHR = 64 * WM * WN, BM = 32 * TM * WM, BN = 32 * TN * WN;
    launch_gather<conv_fwd_mxfp6_kernel<WM, WN, TM, TN, NS>, NTHR, BM, BN, NS * ((size_t)((3 * (BM + BN) + NTHR - 1) / NTHR) * NTHR * 16 + NTHR * 4)>(
        a, false, label, flops, bytes, s);
}

}  // namespace ssd
