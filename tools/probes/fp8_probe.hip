// Ground-truth probe for the two gfx950 features the fp8 path relies on (run on the GPU box):
//   1. v_mfma_scale_f32_32x32x64_f8f6f4 with 8-VGPR e4m3 operands (format selector 0, scale exponent 127 = 1.0):
//      the A/B lane-to-k map.  Expected: lane l holds row / column l & 31 and the 32 consecutive k = 32 (l >> 5) + j,
//      byte j of its 8 registers in memory order; C/D as every 32x32 form.  Checked with exact small integers and an
//      asymmetric B, so a permuted k or a swapped row / column cannot cancel.
//   2. v_cvt_pk_fp8_f32 (OCP e4m3fn): what it returns above 448, at ties and in the subnormal range, both halves of the
//      destination word.
// hipcc --offload-arch=gfx950 -O2 fp8_probe.hip -o fp8_probe && ./fp8_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

// e4m3fn on the host: decode by the format's definition, encode of the small integers the probe uses by search
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

__global__ void mfma_probe(const unsigned char* A, const unsigned char* B, float* D) {
    // A [32][64] row-major (i, k), B [64][32] row-major (k, j); D [32][32]
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
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
    for (int r = 0; r < 16; ++r) D[((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + li] = c[r];
}

__global__ void cvt_probe(const float* v, unsigned* lo, unsigned* hi, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // low half: (v, 0) into bits 0..15 of a word of ones; high half: (0, v) into bits 16..31
    lo[i] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(v[i], 0.f, -1, false);
    hi[i] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(0.f, v[i], -1, true);
}

int main() {
    // ---- 1. operand layout: A in {-3 .. 4}, B in {-2 .. 2} + a term that differs in k and in j
    std::vector<unsigned char> A(32 * 64), B(64 * 32);
    std::vector<float> D(1024), R(1024);
    for (int i = 0; i < 32; ++i)
        for (int k = 0; k < 64; ++k) A[i * 64 + k] = enc_exact((float)((i * 7 + k * 3 + (k >> 5) + (i * k) % 5) % 8 - 3));
    for (int k = 0; k < 64; ++k)
        for (int j = 0; j < 32; ++j) B[k * 32 + j] = enc_exact((float)((k * 5 + j * 11 + (k * j) % 3 + (k >> 4)) % 5 - 2));
    for (int i = 0; i < 32; ++i)
        for (int j = 0; j < 32; ++j) {
            double s = 0;
            for (int k = 0; k < 64; ++k) s += (double)dec(A[i * 64 + k]) * dec(B[k * 32 + j]);
            R[i * 32 + j] = (float)s;
        }
    unsigned char *dA, *dB;
    float* dD;
    CK(hipMalloc(&dA, 2048)); CK(hipMalloc(&dB, 2048)); CK(hipMalloc(&dD, 4096));
    CK(hipMemcpy(dA, A.data(), 2048, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, B.data(), 2048, hipMemcpyHostToDevice));
    mfma_probe<<<1, 64>>>(dA, dB, dD);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost));
    int bad = 0;
    for (int i = 0; i < 1024; ++i) bad += D[i] != R[i];
    printf("MFMA scale 32x32x64 e4m3 (fmt 0, scale 127): lane l = row/col l&31, k = 32*(l>>5)+j, C/D 32x32 map: %d of 1024 differ (%s)\n",
           bad, bad ? "LAYOUT MISMATCH" : "LAYOUT OK, exact");
    if (bad) printf("  D[0][0..3] = %g %g %g %g, expected %g %g %g %g\n", D[0], D[1], D[2], D[3], R[0], R[1], R[2], R[3]);

    // ---- 2. the convert
    const float vals[] = {0.f, -0.f, 1.f, 1.0625f, 1.125f, 1.1875f, -1.0625f, -1.1875f, 440.f, 448.f, 463.99f, 464.f, 465.f, 480.f, 1e6f,
                          -464.f, -480.f, -1e6f, INFINITY, -INFINITY, NAN,
                          0.001953125f /* 2^-9, the smallest subnormal */, 0.0009765625f /* 2^-10: tie to 0 */, 0.00146484375f /* 1.5 * 2^-10 */,
                          0.0029296875f /* 1.5 * 2^-9: tie to 2 * 2^-9 */, 0.0048828125f /* 2.5 * 2^-9: tie to 2 */, 0.013671875f /* 7 * 2^-9 */,
                          0.0146484375f /* 7.5 * 2^-9: tie to 2^-6 */, 0.015625f /* 2^-6, the smallest normal */};
    const int n = sizeof vals / sizeof vals[0];
    float* dV;
    unsigned *dLo, *dHi;
    CK(hipMalloc(&dV, n * 4)); CK(hipMalloc(&dLo, n * 4)); CK(hipMalloc(&dHi, n * 4));
    CK(hipMemcpy(dV, vals, n * 4, hipMemcpyHostToDevice));
    cvt_probe<<<1, 64>>>(dV, dLo, dHi, n);
    CK(hipDeviceSynchronize());
    std::vector<unsigned> lo(n), hi(n);
    CK(hipMemcpy(lo.data(), dLo, n * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(hi.data(), dHi, n * 4, hipMemcpyDeviceToHost));
    printf("v_cvt_pk_fp8_f32: value -> code (decoded) | word with (v, 0) in the low half of ~0, word with (0, v) in the high half\n");
    for (int i = 0; i < n; ++i) {
        const unsigned char c = lo[i] & 0xFF;
        printf("  %-14.9g -> 0x%02X (%g) | %08X %08X%s\n", vals[i], c, dec(c), lo[i], hi[i], ((hi[i] >> 24) & 0xFF) == c ? "" : "  HALVES DIFFER");
    }
    return bad != 0;
}
