// Ground-truth probe for the E8M0 block-scale operands of v_mfma_scale_f32_32x32x64_f8f6f4 on gfx950 (run on the GPU box).
// fp8_probe.hip pinned the e4m3 operand layout with every scale byte 127 (lane l holds row l & 31 and k = 32 (l >> 5) + j in its 8
// registers); this one pins what the mxfp8 path adds:
//   1. which lane's scale byte applies to which (row, k), for each of the two operands.  Lane l's byte is 96 + l, the other operand
//      is a selector matrix that picks one k per output line, so D = 2^(lane - 31) names the lane whose scale multiplied element
//      (row, k).  Found: the byte of lane r + 32 h multiplies registers 4 h ... 4 h + 3 of BOTH lanes r and r + 32, that is
//      k = 16 h ... 16 h + 15 and 32 + 16 h ... 47 + 16 h of row r -- NOT the lane's own 32 values.  A kernel that wants one scale per 32
//      consecutive channels therefore loads channels 16 (l >> 5) ... + 15 into registers 0 ... 3 and 32 + 16 (l >> 5) ... + 15 into
//      registers 4 ... 7 (conv_mxfp8.hip).
//   2. op_sel 0 ... 3 selects byte 0 ... 3 of the scale register (bytes 127, 128, 129, 130 -> result x 1, 2, 4, 8).
//   3. results are exact for scale exponents 120 ... 134 on small integers, both operands scaled at once, the two blocks of a row
//      at different scales.
//   4. code 0 under scale byte 0 (what a padded tap's zero fill puts in both buffers) contributes +0.
// hipcc --offload-arch=gfx950 -O2 mxfp8_probe.hip -o mxfp8_probe && ./mxfp8_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

static float dec(unsigned char c) {
    const int s = c >> 7, e = (c >> 3) & 15, m = c & 7;
    float v;
    if (e == 15 && m == 7) v = NAN;
    else if (e == 0) v = ldexpf((float)m, -9);
    else v = ldexpf(1.f + m / 8.f, e - 7);
    return s ? -v : v;
}
static unsigned char enc_exact(float v) {
    for (int c = 0; c < 256; ++c)
        if ((c & 0x7F) != 0x7F && dec((unsigned char)c) == v && !(v == 0.f && c == 0x80)) return (unsigned char)c;
    printf("value %g is no e4m3 number\n", v);
    exit(1);
}

// A [32][64] row-major (i, k), B [64][32] row-major (k, j), sa / sb: one scale register per lane; D [32][32]
template <int SEL_A, int SEL_B>
__global__ void mfma_probe(const unsigned char* A, const unsigned char* B, const unsigned* sa, const unsigned* sb, float* D) {
    const int l = threadIdx.x, li = l & 31, lh = l >> 5;
    i32x8 a, b;
    for (int r = 0; r < 8; ++r) {
        unsigned wa = 0, wb = 0;
        for (int e = 0; e < 4; ++e) {
            const int k = 32 * lh + 4 * r + e;
            wa |= (unsigned)A[li * 64 + k] << (8 * e);
            wb |= (unsigned)B[k * 32 + li] << (8 * e);
        }
        a[r] = (int)wa;
        b[r] = (int)wb;
    }
    f32x16 c;
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, SEL_A, (int)sa[l], SEL_B, (int)sb[l]);
    for (int r = 0; r < 16; ++r) D[((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + li] = c[r];
}

struct Dev {
    unsigned char *A, *B;
    unsigned *sa, *sb;
    float* D;
};
template <int SEL_A, int SEL_B>
static void run(const Dev& d, const std::vector<unsigned char>& A, const std::vector<unsigned char>& B, const std::vector<unsigned>& sa,
                const std::vector<unsigned>& sb, std::vector<float>& D) {
    CK(hipMemcpy(d.A, A.data(), 2048, hipMemcpyHostToDevice));
    CK(hipMemcpy(d.B, B.data(), 2048, hipMemcpyHostToDevice));
    CK(hipMemcpy(d.sa, sa.data(), 256, hipMemcpyHostToDevice));
    CK(hipMemcpy(d.sb, sb.data(), 256, hipMemcpyHostToDevice));
    mfma_probe<SEL_A, SEL_B><<<1, 64>>>(d.A, d.B, d.sa, d.sb, d.D);
    CK(hipDeviceSynchronize());
    D.resize(1024);
    CK(hipMemcpy(D.data(), d.D, 4096, hipMemcpyDeviceToHost));
}

int main() {
    Dev d;
    CK(hipMalloc(&d.A, 2048)); CK(hipMalloc(&d.B, 2048)); CK(hipMalloc(&d.sa, 256)); CK(hipMalloc(&d.sb, 256)); CK(hipMalloc(&d.D, 4096));
    std::vector<unsigned char> A(2048), B(2048);
    std::vector<unsigned> sa(64), sb(64), one(64, 0x7F7F7F7Fu);
    std::vector<float> D;
    int fails = 0;

    // ---- 1. lane -> (row, k): lane l's byte is 96 + l, the other operand is a selector matrix that picks one k per output line, so
    //         D = 2^(lane - 31) names the lane whose scale multiplied element (row, k)
    for (int operand = 0; operand < 2; ++operand) {
        std::vector<unsigned> sc(64);
        for (int l = 0; l < 64; ++l) sc[l] = 0x7F7F7F00u | (unsigned)(96 + l);
        int lane_of[32][64];
        for (int kh = 0; kh < 2; ++kh) {
            for (int i = 0; i < 32; ++i)
                for (int k = 0; k < 64; ++k) {
                    const unsigned char u = enc_exact(1.f), sel = enc_exact(k == i + 32 * kh ? 1.f : 0.f);
                    A[i * 64 + k] = operand == 0 ? u : sel;
                    B[k * 32 + i] = operand == 0 ? sel : u;
                }
            if (operand == 0) run<0, 0>(d, A, B, sc, one, D);
            else run<0, 0>(d, A, B, one, sc, D);
            for (int r = 0; r < 32; ++r)
                for (int q = 0; q < 32; ++q) {      // r: line of the probed operand, q: the selected k - 32 kh
                    const float x = operand == 0 ? D[r * 32 + q] : D[q * 32 + r];
                    int e;
                    const float mant = frexpf(x, &e);
                    lane_of[r][q + 32 * kh] = (mant == 0.5f) ? e - 1 + 31 : -1;
                }
        }
        int own = 0;
        for (int r = 0; r < 32; ++r)
            for (int k = 0; k < 64; ++k) own += lane_of[r][k] == r + 32 * ((k >> 4) & 1);
        printf("scale operand %s: %d of 2048 (row, k) carry the scale byte of lane row + 32 ((k >> 4) & 1): registers 4 h ... 4 h + 3 of lanes r and r + 32 (%s)\n",
               operand == 0 ? "A (first)" : "B (second)", own, own == 2048 ? "MAP AS FOUND" : "DIFFERENT MAP");
        if (own != 2048)
            for (int r : {0, 1, 17, 31}) {
                printf("  row %2d: lane per k:", r);
                for (int k = 0; k < 64; ++k) printf(" %d", lane_of[r][k]);
                printf("\n");
            }
        fails += own != 2048;
    }

    // ---- 2. op_sel picks the byte
    for (int i = 0; i < 2048; ++i) A[i] = B[i] = enc_exact(1.f);
    {
        std::vector<unsigned> bytes(64, 0x8281807Fu);     // byte 0..3 = 127, 128, 129, 130
        float got[2][4];
        run<0, 0>(d, A, B, bytes, one, D); got[0][0] = D[0];
        run<1, 0>(d, A, B, bytes, one, D); got[0][1] = D[0];
        run<2, 0>(d, A, B, bytes, one, D); got[0][2] = D[0];
        run<3, 0>(d, A, B, bytes, one, D); got[0][3] = D[0];
        run<0, 0>(d, A, B, one, bytes, D); got[1][0] = D[0];
        run<0, 1>(d, A, B, one, bytes, D); got[1][1] = D[0];
        run<0, 2>(d, A, B, one, bytes, D); got[1][2] = D[0];
        run<0, 3>(d, A, B, one, bytes, D); got[1][3] = D[0];
        for (int o = 0; o < 2; ++o) {
            bool ok = true;
            for (int s = 0; s < 4; ++s) ok = ok && got[o][s] == 64.f * (float)(1 << s);
            printf("op_sel operand %s, scale register 0x8281807F, op_sel 0 1 2 3 -> D[0][0] = %g %g %g %g (expected 64 128 256 512: %s)\n",
                   o == 0 ? "A" : "B", got[o][0], got[o][1], got[o][2], got[o][3], ok ? "BYTE = OP_SEL" : "MISMATCH");
            fails += !ok;
        }
    }

    // ---- 3. exact for exponents 120 ... 134, both operands scaled, small integers (fp8_probe's matrices)
    for (int i = 0; i < 32; ++i)
        for (int k = 0; k < 64; ++k) A[i * 64 + k] = enc_exact((float)((i * 7 + k * 3 + (k >> 5) + (i * k) % 5) % 8 - 3));
    for (int k = 0; k < 64; ++k)
        for (int j = 0; j < 32; ++j) B[k * 32 + j] = enc_exact((float)((k * 5 + j * 11 + (k * j) % 3 + (k >> 4)) % 5 - 2));
    {
        int ea[64], eb[64], lo = 255, hi = 0;
        for (int l = 0; l < 64; ++l) {
            ea[l] = 120 + (l & 31) % 13 + 2 * (l >> 5);            // 120 ... 134; a row's two blocks differ by up to 3 in the product
            eb[l] = 120 + ((l & 31) * 5) % 13 + (l >> 5);
            sa[l] = 0x7F7F7F00u | (unsigned)ea[l];
            sb[l] = 0x7F7F7F00u | (unsigned)eb[l];
            lo = std::min(lo, std::min(ea[l], eb[l]));
            hi = std::max(hi, std::max(ea[l], eb[l]));
        }
        run<0, 0>(d, A, B, sa, sb, D);
        int bad = 0, inexact = 0;
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                double s = 0;
                for (int k = 0; k < 64; ++k)
                    s += ldexp((double)dec(A[i * 64 + k]) * dec(B[k * 32 + j]), ea[i + 32 * ((k >> 4) & 1)] - 127 + eb[j + 32 * ((k >> 4) & 1)] - 127);
                inexact += (double)(float)s != s;
                bad += D[i * 32 + j] != (float)s;
            }
        printf("scale bytes %d ... %d on both operands, integers -3..4 x -2..2: %d of 1024 differ, %d references not fp32 numbers (%s)\n", lo, hi, bad,
               inexact, bad || inexact ? "MISMATCH" : "EXACT");
        fails += bad != 0 || inexact != 0;
    }

    // ---- 4. code 0 under scale byte 0: rows 0..15 of A all zero in both blocks, rows 16..31 zero in the block of lane r + 32 only;
    //         B at full range (+-448) under scale bytes up to 134
    {
        for (int i = 0; i < 32; ++i)
            for (int k = 0; k < 64; ++k) {
                const bool zero = i < 16 || ((k >> 4) & 1) == 1;
                A[i * 64 + k] = zero ? 0 : enc_exact((float)((i + k) % 5 - 2));
            }
        for (int k = 0; k < 64; ++k)
            for (int j = 0; j < 32; ++j) B[k * 32 + j] = (k + j) % 3 == 0 ? enc_exact(-448.f) : enc_exact(448.f);
        for (int l = 0; l < 64; ++l) {
            const bool zero = (l & 31) < 16 || (l >> 5) == 1;
            sa[l] = zero ? 0u : 0x7F7F7F7Fu;
            sb[l] = 0x7F7F7F00u | (unsigned)(127 + (l % 8));
        }
        run<0, 0>(d, A, B, sa, sb, D);
        int bad = 0, notpos0 = 0;
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                double s = 0;
                for (int k = 0; k < 64; ++k) s += ldexp((double)dec(A[i * 64 + k]) * dec(B[k * 32 + j]), (j % 8));
                if (i < 16) s = 0;
                if (D[i * 32 + j] != (float)s && bad++ < 6) printf("  D[%d][%d] = %.9g, expected %.9g\n", i, j, D[i * 32 + j], s);
                unsigned bits;
                memcpy(&bits, &D[i * 32 + j], 4);
                if (i < 16) notpos0 += bits != 0u;
            }
        printf("code 0 under scale byte 0 against +-448 under bytes 127 ... 134: %d of 1024 differ, %d of 512 all-zero rows' results are not +0 (%s)\n",
               bad, notpos0, bad || notpos0 ? "MISMATCH" : "ZERO BLOCKS ADD +0");
        fails += bad != 0 || notpos0 != 0;
    }
    printf("mxfp8_probe: %s\n", fails ? "FAILED" : "all four properties hold as described");
    return fails != 0;
}
