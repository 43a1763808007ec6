// Ground-truth probe for 6-bit (e2m3) operands of v_mfma_scale_f32_32x32x64_f8f6f4 on gfx950 (format selector 2 on cbsz / blgp; the
// operand is the first 6 registers of the builtin's 8) and for v_cvt_scalef32_2xpk16_fp6_f32 (run on the GPU box).  Nothing of the e4m3
// answers (fp8_probe.hip, mxfp8_probe.hip) is assumed: the maps are measured, printed, and compared with what conv_mxfp6.hip relies on.
//   1. operand layout: one 6-bit field of one lane is set to 1.0 (field f = bits 6 f ... 6 f + 5 of the lane's 192 bits, register 0
//      first, little-endian), the other operand is e4m3 in fp8_probe's layout (lane l: line l & 31, k = 32 (l >> 5) + j) and holds
//      2^(k & 7) or 2^(k >> 3): the one non-zero line of D names the field's row (column) and the two values name its k.  Both
//      operands, all 64 lanes x 32 fields.  Found: line = lane & 31; in fp8_probe's names of k, fields 0 ... 15 of lane half h are
//      k = 16 h ... 16 h + 15 and fields 16 ... 31 are k = 32 + 16 h ... 47 + 16 h, the same map on both operands.
//   2. scale coverage, both operands e2m3 (the kernel's case): lane l's scale byte is 96 + l, the probed operand is all 1.0, the other
//      one a selector of one k per line under scale 2^0, so D = 2^(lane - 31) names the lane whose byte multiplied (line, k).  Found:
//      a lane's byte multiplies exactly the 32 fields in that lane's own registers, on either operand.  So a lane's 6 registers are
//      one MX block as it lies in memory (24 bytes, code j in bits 6 j ... 6 j + 5): no permutation on the way to the fragment.
//   3. exact integer products: asymmetric A (-7 ... 7) and B (-3 ... 3), both operands under scale bytes 120 ... 134.
//   4. code 0 under scale byte 0 adds +0 (what a padded tap's zero fill holds).
//   5. the convert: field order of the 32 results, what the scale argument means, ties, subnormals, saturation, against a plain
//      integer encoder of OCP e2m3 (round to nearest even, clamp to 7.5).  Reported only: the kernels encode in integer arithmetic.
// hipcc --offload-arch=gfx950 -O2 mxfp6_probe.hip -o mxfp6_probe && ./mxfp6_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x6 __attribute__((ext_vector_type(6)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

// ---- e2m3 on the host
static float dec6(unsigned c) {
    const int e = (c >> 3) & 3, m = c & 7;
    const float a = e ? ldexpf(1.f + m / 8.f, e - 1) : m / 8.f;
    return (c & 32) ? -a : a;
}
static unsigned enc6(float v) {      // RNE, clamp to +-7.5
    float a = fminf(fabsf(v), 7.5f);
    unsigned c;
    if (a < 2.f) c = (unsigned)rintf(a * 8.f);
    else if (a < 4.f) c = 8u + (unsigned)rintf(a * 4.f);
    else c = 16u + (unsigned)rintf(a * 2.f);
    return c | (std::signbit(v) ? 32u : 0u);
}
static unsigned enc6_exact(float v) {
    const unsigned c = v == 0.f ? 0u : enc6(v);
    if (dec6(c) != v) { printf("value %g is no e2m3 number\n", v); exit(1); }
    return c;
}

// ---- 1. layout: block (lane, field) of the grid; operand 0 = first (A), 1 = second (B).  out [2][blocks][64][16]
__global__ void layout_probe(int operand, float* out) {
    const int l = threadIdx.x, li = l & 31, lh = l >> 5;
    const int pl = blockIdx.x >> 5, pf = blockIdx.x & 31;
    i32x8 six = {0, 0, 0, 0, 0, 0, 0, 0};
    if (l == pl) {
        const int bit = 6 * pf;      // code 8 = 1.0; a field may straddle two registers
        const unsigned long long v = 8ull << (bit & 31);
        six[bit >> 5] = (int)(unsigned)v;
        if ((bit >> 5) + 1 < 6) six[(bit >> 5) + 1] = (int)(unsigned)(v >> 32);
    }
    for (int pass = 0; pass < 2; ++pass) {
        i32x8 e;      // e4m3, fp8_probe's layout: lane l holds line li, k = 32 lh + 4 r + byte; the value depends on k alone
        for (int r = 0; r < 8; ++r) {
            unsigned w = 0;
            for (int b = 0; b < 4; ++b) {
                const int k = 32 * lh + 4 * r + b;
                w |= (unsigned)(((pass ? (k >> 3) : (k & 7)) + 7) << 3) << (8 * b);
            }
            e[r] = (int)w;
        }
        f32x16 c;
        for (int r = 0; r < 16; ++r) c[r] = 0.f;
        if (operand == 0) c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(six, e, c, 2, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
        else c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(e, six, c, 0, 2, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
        float* o = out + ((size_t)(pass * gridDim.x + blockIdx.x) * 64 + l) * 16;
        for (int r = 0; r < 16; ++r) o[r] = c[r];
    }
}

// ---- 2 ... 4: both operands e2m3, 6 dwords per lane given as they are; D [32][32] (i = line of A, j = line of B)
__global__ void mfma6(const unsigned* A, const unsigned* B, const unsigned* sa, const unsigned* sb, float* D) {
    const int l = threadIdx.x, li = l & 31, lh = l >> 5;
    i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < 6; ++r) {
        a[r] = (int)A[l * 6 + r];
        b[r] = (int)B[l * 6 + r];
    }
    f32x16 c;
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 2, 2, 0, (int)sa[l], 0, (int)sb[l]);
    for (int r = 0; r < 16; ++r) D[((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + li] = c[r];
}

// ---- 5. the convert: lane l converts x[32 l ... 32 l + 15] and x[32 l + 16 ... 32 l + 31] under scale sc[l]
__global__ void cvt6(const float* x, const float* sc, unsigned* y) {
    const int l = threadIdx.x;
    f32x16 a, b;
    for (int r = 0; r < 16; ++r) {
        a[r] = x[32 * l + r];
        b[r] = x[32 * l + 16 + r];
    }
    const u32x6 w = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, sc[l]);
    for (int r = 0; r < 6; ++r) y[6 * l + r] = w[r];
}

static unsigned field(const unsigned* w, int f) {
    const int bit = 6 * f;
    unsigned long long v = w[bit >> 5];
    if ((bit >> 5) + 1 < 6) v |= (unsigned long long)w[(bit >> 5) + 1] << 32;
    return (unsigned)(v >> (bit & 31)) & 63u;
}
static void set_field(unsigned* w, int f, unsigned c) {
    const int bit = 6 * f;
    const unsigned long long v = (unsigned long long)(c & 63u) << (bit & 31);
    w[bit >> 5] |= (unsigned)v;
    if ((bit >> 5) + 1 < 6) w[(bit >> 5) + 1] |= (unsigned)(v >> 32);
}

struct Map { int line[64][32], k[64][32]; };      // (lane, field) -> the operand's line (row of A / column of B) and k

int main() {
    int fails = 0;
    // ---- 1
    Map map[2];
    {
        const int blocks = 64 * 32;
        float* d;
        CK(hipMalloc(&d, (size_t)2 * blocks * 64 * 16 * 4));
        std::vector<float> h((size_t)2 * blocks * 64 * 16);
        for (int operand = 0; operand < 2; ++operand) {
            layout_probe<<<blocks, 64>>>(operand, d);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost));
            int as_expected = 0, broken = 0;
            for (int b = 0; b < blocks; ++b) {
                // D element (lane l, register r) is D[(r & 3) + 8 (r >> 2) + 4 lh][li]: row = line of A, column = line of B
                int line = -1, klo = -1, khi = -1, lines = 0;
                bool uniform = true;
                for (int ln = 0; ln < 32; ++ln) {      // a line of the probed operand: non-zero, and the same value along the other one
                    float v0[2] = {0.f, 0.f};
                    bool any = false;
                    for (int pass = 0; pass < 2; ++pass)
                        for (int o = 0; o < 32; ++o) {
                            const int i = operand == 0 ? ln : o, j = operand == 0 ? o : ln;
                            const int r = (i & 3) + 4 * (i >> 3), lh = (i >> 2) & 1;
                            const float v = h[((size_t)(pass * blocks + b) * 64 + (j + 32 * lh)) * 16 + r];
                            if (o == 0) v0[pass] = v;
                            uniform = uniform && v == v0[pass];
                            any = any || v != 0.f;
                        }
                    if (any) {
                        ++lines;
                        line = ln;
                        int e;
                        klo = frexpf(v0[0], &e) == 0.5f ? e - 1 : -1;
                        khi = frexpf(v0[1], &e) == 0.5f ? e - 1 : -1;
                    }
                }
                const int l = b >> 5, f = b & 31;
                const bool ok = lines == 1 && uniform && klo >= 0 && klo < 8 && khi >= 0 && khi < 8;
                map[operand].line[l][f] = ok ? line : -1;
                map[operand].k[l][f] = ok ? 8 * khi + klo : -1;
                broken += !ok;
                as_expected += ok && line == (l & 31) && 8 * khi + klo == (f < 16 ? 16 * (l >> 5) + f : 32 + 16 * (l >> 5) + f - 16);
            }
            printf("layout operand %s: %d of 2048 (lane, field) feed line lane & 31, k = 16 (lane >> 5) + field for fields 0 ... 15 and 32 + 16 (lane >> 5) + field - 16 for fields "
                   "16 ... 31, in fp8_probe's names of k; %d unreadable (%s)\n",
                   operand == 0 ? "A (first)" : "B (second)", as_expected, broken, as_expected == 2048 ? "MAP AS RELIED ON" : "DIFFERENT MAP");
            if (as_expected != 2048)
                for (int l : {0, 1, 33}) {
                    printf("  lane %2d: (line, k) per field:", l);
                    for (int f = 0; f < 32; ++f) printf(" (%d,%d)", map[operand].line[l][f], map[operand].k[l][f]);
                    printf("\n");
                }
            fails += as_expected != 2048;
        }
        CK(hipFree(d));
    }
    // logical matrices -> lane registers by the measured map
    auto pack = [&](int operand, const std::vector<float>& Mx /* [line][k] */, std::vector<unsigned>& regs) {
        regs.assign(64 * 6, 0u);
        for (int l = 0; l < 64; ++l)
            for (int f = 0; f < 32; ++f) {
                const int ln = map[operand].line[l][f], k = map[operand].k[l][f];
                if (ln >= 0) set_field(&regs[l * 6], f, enc6_exact(Mx[ln * 64 + k]));
            }
    };
    unsigned *dA, *dB, *dsa, *dsb;
    float* dD;
    CK(hipMalloc(&dA, 64 * 24)); CK(hipMalloc(&dB, 64 * 24)); CK(hipMalloc(&dsa, 256)); CK(hipMalloc(&dsb, 256)); CK(hipMalloc(&dD, 4096));
    std::vector<float> D(1024);
    auto run = [&](const std::vector<float>& A, const std::vector<float>& B, const std::vector<unsigned>& sa, const std::vector<unsigned>& sb) {
        std::vector<unsigned> ra, rb;
        pack(0, A, ra);
        pack(1, B, rb);
        CK(hipMemcpy(dA, ra.data(), 64 * 24, hipMemcpyHostToDevice));
        CK(hipMemcpy(dB, rb.data(), 64 * 24, hipMemcpyHostToDevice));
        CK(hipMemcpy(dsa, sa.data(), 256, hipMemcpyHostToDevice));
        CK(hipMemcpy(dsb, sb.data(), 256, hipMemcpyHostToDevice));
        mfma6<<<1, 64>>>(dA, dB, dsa, dsb, dD);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost));
    };
    std::vector<float> A(2048), B(2048);      // A [i][k], B [j][k]
    std::vector<unsigned> one(64, 0x7F7F7F7Fu), sa(64), sb(64);

    // ---- 2. scale coverage
    int cover[2][32][64];
    for (int operand = 0; operand < 2; ++operand) {
        std::vector<unsigned> sc(64);
        for (int l = 0; l < 64; ++l) sc[l] = 0x7F7F7F00u | (unsigned)(96 + l);
        for (int kh = 0; kh < 2; ++kh) {
            for (int i = 0; i < 32; ++i)
                for (int k = 0; k < 64; ++k) {
                    const float sel = k == i + 32 * kh ? 1.f : 0.f;
                    A[i * 64 + k] = operand == 0 ? 1.f : sel;
                    B[i * 64 + k] = operand == 0 ? sel : 1.f;
                }
            if (operand == 0) run(A, B, sc, one);
            else run(A, B, one, sc);
            for (int r = 0; r < 32; ++r)
                for (int q = 0; q < 32; ++q) {
                    const float x = operand == 0 ? D[r * 32 + q] : D[q * 32 + r];
                    int e;
                    cover[operand][r][q + 32 * kh] = frexpf(x, &e) == 0.5f ? e - 1 + 31 : -1;
                }
        }
        int holder[32][64];
        for (int r = 0; r < 32; ++r)
            for (int k = 0; k < 64; ++k) holder[r][k] = -2;
        for (int l = 0; l < 64; ++l)
            for (int f = 0; f < 32; ++f)
                if (map[operand].line[l][f] >= 0) holder[map[operand].line[l][f]][map[operand].k[l][f]] = l;
        int own = 0;
        for (int r = 0; r < 32; ++r)
            for (int k = 0; k < 64; ++k) own += cover[operand][r][k] == holder[r][k];
        printf("scale operand %s: %d of 2048 (line, k) carry the scale byte of the lane whose registers hold them (%s)\n",
               operand == 0 ? "A (first)" : "B (second)", own, own == 2048 ? "A LANE'S BYTE COVERS ITS OWN 32 FIELDS" : "DIFFERENT MAP");
        if (own != 2048)
            for (int r : {0, 17}) {
                printf("  line %2d: lane per k:", r);
                for (int k = 0; k < 64; ++k) printf(" %d", cover[operand][r][k]);
                printf("\n");
            }
        fails += own != 2048;
    }

    // ---- 3. exact integers, asymmetric, both operands scaled by the measured coverage
    for (int i = 0; i < 32; ++i)
        for (int k = 0; k < 64; ++k) A[i * 64 + k] = (float)((i * 7 + k * 3 + (k >> 5) + (i * k) % 5) % 15 - 7);
    for (int j = 0; j < 32; ++j)
        for (int k = 0; k < 64; ++k) B[j * 64 + k] = (float)((k * 5 + j * 11 + (k * j) % 3 + (k >> 4)) % 7 - 3);
    {
        int ea[64], eb[64];
        for (int l = 0; l < 64; ++l) {
            ea[l] = 120 + (l & 31) % 13 + 2 * (l >> 5);
            eb[l] = 120 + ((l & 31) * 5) % 13 + (l >> 5);
            sa[l] = 0x7F7F7F00u | (unsigned)ea[l];
            sb[l] = 0x7F7F7F00u | (unsigned)eb[l];
        }
        run(A, B, sa, sb);
        int bad = 0, inexact = 0;
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                double s = 0;
                for (int k = 0; k < 64; ++k) {
                    const int la = cover[0][i][k], lb = cover[1][j][k];
                    if (la < 0 || lb < 0) continue;
                    s += ldexp((double)A[i * 64 + k] * B[j * 64 + k], ea[la] - 127 + eb[lb] - 127);
                }
                inexact += (double)(float)s != s;
                if (D[i * 32 + j] != (float)s && bad++ < 4) printf("  D[%d][%d] = %.9g, expected %.9g\n", i, j, D[i * 32 + j], s);
            }
        printf("scale bytes 120 ... 134 on both operands, integers -7..7 x -3..3: %d of 1024 differ, %d references not fp32 numbers (%s)\n", bad, inexact,
               bad || inexact ? "MISMATCH" : "EXACT");
        fails += bad != 0 || inexact != 0;
    }

    // ---- 4. code 0 under scale byte 0: rows 0..15 of A zero in both lanes, rows 16..31 zero in the fields of lane r + 32; B +-7.5 under bytes up to 134
    {
        for (int i = 0; i < 32; ++i)
            for (int k = 0; k < 64; ++k) A[i * 64 + k] = (i < 16 || cover[0][i][k] >= 32) ? 0.f : (float)((i + k) % 5 - 2);
        for (int j = 0; j < 32; ++j)
            for (int k = 0; k < 64; ++k) B[j * 64 + k] = (k + j) % 3 == 0 ? -7.5f : 7.5f;
        for (int l = 0; l < 64; ++l) {
            sa[l] = 0x7F7F7F7Fu;
            sb[l] = 0x7F7F7F00u | (unsigned)(127 + (l % 8));
        }
        for (int i = 0; i < 32; ++i)
            for (int k = 0; k < 64; ++k)
                if ((i < 16 || cover[0][i][k] >= 32) && cover[0][i][k] >= 0) sa[cover[0][i][k]] = 0u;
        run(A, B, sa, sb);
        int bad = 0, notpos0 = 0;
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                double s = 0;
                for (int k = 0; k < 64; ++k)
                    if (cover[1][j][k] >= 0) s += ldexp((double)A[i * 64 + k] * B[j * 64 + k], cover[1][j][k] % 8);
                if (D[i * 32 + j] != (float)s && bad++ < 4) printf("  D[%d][%d] = %.9g, expected %.9g\n", i, j, D[i * 32 + j], s);
                unsigned bits;
                memcpy(&bits, &D[i * 32 + j], 4);
                if (i < 16) notpos0 += bits != 0u;
            }
        printf("code 0 under scale byte 0 against +-7.5 under bytes 127 ... 134: %d of 1024 differ, %d of 512 all-zero rows' results are not +0 (%s)\n", bad,
               notpos0, bad || notpos0 ? "MISMATCH" : "ZERO BLOCKS ADD +0");
        fails += bad != 0 || notpos0 != 0;
    }

    // ---- 5. the convert (reported, not relied on: conv_mxfp6.hip encodes in integer arithmetic).  Rounding is read from field 0 of a
    //         lane whose 32 inputs are all the same value, so that no assumption about the field order enters
    {
        float *dx, *dsc;
        unsigned* dy;
        CK(hipMalloc(&dx, 2048 * 4)); CK(hipMalloc(&dsc, 256)); CK(hipMalloc(&dy, 64 * 24));
        std::vector<float> x(2048), sc(64);
        std::vector<unsigned> y(64 * 6);
        auto cvt = [&]() {
            CK(hipMemcpy(dx, x.data(), 2048 * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(dsc, sc.data(), 256, hipMemcpyHostToDevice));
            cvt6<<<1, 64>>>(dx, dsc, dy);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(y.data(), dy, 64 * 24, hipMemcpyDeviceToHost));
        };
        // field order: input number v of the lane's 32 is the e2m3 value with code v
        for (int l = 0; l < 64; ++l) {
            sc[l] = 1.f;
            for (int v = 0; v < 32; ++v) x[32 * l + v] = dec6((unsigned)v);
        }
        cvt();
        int interleaved = 0;
        for (int f = 0; f < 32; ++f) interleaved += field(&y[0], f) == (unsigned)((f & 1) * 16 + (f >> 1));
        printf("convert field order: %d of 32 fields hold first[f / 2] (even f) / second[f / 2] (odd f); field f of lane 0 holds input number:", interleaved);
        for (int f = 0; f < 32; ++f) printf(" %u", field(&y[0], f));
        printf("\n  raw dwords of lane 0: %08x %08x %08x %08x %08x %08x\n", y[0], y[1], y[2], y[3], y[4], y[5]);
        // scale argument: value 3 under scales 2^-2 ... 2^3, and under 3.0 (only the exponent?)
        printf("convert scale argument, input 3.0:");
        for (int s = -2; s <= 3; ++s) {
            for (int l = 0; l < 64; ++l) sc[l] = ldexpf(1.f, s);
            for (int i = 0; i < 2048; ++i) x[i] = 3.f;
            cvt();
            printf("  scale 2^%d -> %g", s, dec6(field(&y[0], 0)));
        }
        for (int l = 0; l < 64; ++l) sc[l] = 3.f;
        cvt();
        printf("  scale 3.0 -> %g (1.5: the scale's exponent alone divides)\n", dec6(field(&y[0], 0)));
        // rounding and saturation at scale 1: every multiple of 1/64 up to 10, both signs, and large / tiny values
        std::vector<float> vals;
        for (int q = 0; q <= 640; ++q) { vals.push_back(q / 64.f); vals.push_back(-q / 64.f); }
        for (float v : {100.f, 1e30f, 7.500001f, 7.75f, 8.f, 0.06250001f, 0.0624999f, 1e-30f}) { vals.push_back(v); vals.push_back(-v); }
        int differ = 0, shown = 0, uneven = 0;
        for (size_t base = 0; base < vals.size(); base += 64) {
            for (int l = 0; l < 64; ++l) {
                sc[l] = 1.f;
                for (int v = 0; v < 32; ++v) x[32 * l + v] = base + l < vals.size() ? vals[base + l] : 0.f;
            }
            cvt();
            for (int l = 0; l < 64 && base + l < vals.size(); ++l) {
                const float in = vals[base + l];
                const unsigned got = field(&y[6 * l], 0), want = enc6(in);
                for (int f = 1; f < 32; ++f) uneven += field(&y[6 * l], f) != got;
                if (got != want && !((got & 31) == 0 && (want & 31) == 0)) {
                    ++differ;
                    if (shown++ < 8) printf("  convert(%.9g) = code %u (%g), integer encoder: code %u (%g)\n", in, got, dec6(got), want, dec6(want));
                }
            }
        }
        printf("convert at scale 1 against RNE with clamp to 7.5 over %zu values (every 1/64 up to 10, ties, subnormals, 100, 1e30, 1e-30), field 0: %d differ (%s); "
               "%d other fields of those lanes differ from their field 0 (32 equal inputs)\n",
               vals.size(), differ, differ ? "NOT THE CONTRACT'S ENCODER" : "SAME AS THE INTEGER ENCODER", uneven);
        const float ties[8] = {0.0625f, 0.1875f, 1.0625f, 1.1875f, 7.25f, 7.75f, 100.f, -100.f};
        for (int l = 0; l < 64; ++l)
            for (int v = 0; v < 32; ++v) x[32 * l + v] = ties[l & 7];
        cvt();
        printf("convert at scale 1:");
        for (int t = 0; t < 8; ++t) printf(" %g -> %g;", ties[t], dec6(field(&y[6 * t], 0)));
        printf("\n");
    }
    printf("mxfp6_probe: %s\n", fails ? "FAILED" : "layout, scale coverage, exactness and zero blocks hold as conv_mxfp6.hip relies on them");
    return fails != 0;
}
