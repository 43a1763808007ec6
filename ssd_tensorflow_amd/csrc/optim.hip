// AdamW update of the parameter arena for gfx950 (contract in include/ssdvgg_hip.h "update rule"), and the weight EMA
// behind every update with the kernel that swaps it in (same header, "weight EMA"; tests/ema_ref.py).
// Every fp32 operation below is one rounding, in the order written: this file is compiled with -ffp-contract=off (Makefile,
// EXTRA_optim) and must stay out of ops.hip, which is compiled with contraction on.  Division and square root are the
// compiler's correctly rounded sequences, so a numpy float32 restatement of the loop has the same bits (tests/adamw_ref.py).
#include "ops.h"
#include "bf16.h"
#include <algorithm>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace ssd {

static __device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
static __device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// what the host derives in double from the float32 hyper-parameters and the update's count, each rounded to float once
struct AdamScalars {
    float b1, omb1;     // beta1, (float)(1 - beta1)
    float b2, omb2;     // beta2, (float)(1 - beta2)
    float rs2;          // (float)(1 / sqrt(1 - beta2^t))
    float eps;
    float ld;           // (float)(lr * decay)
    float ss;           // (float)(lr / (1 - beta1^t))
};

// HBM-bound: 28 bytes per parameter (w, m, v, g in; w, m, v out).  momentum_kernel's shape: 16 bytes per lane and trip, so a lane
// has its four 16-byte loads in flight before the first use; the arithmetic (a division and a square root per element) hides
// behind them at 8 waves per SIMD (profiles/adamw_kernel_resources.txt).  CLIPPED: the scale comes from the norm pass's finish
// kernel, and a gradient that was not finite leaves w, m and v alone.
template <bool CLIPPED>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                    const float* __restrict__ g, size_t n4, size_t n_decay, AdamScalars a,
                                                    float gscale, const ClipState* __restrict__ st) {
    if (CLIPPED) {
        if (st->skip) return;
        gscale = st->gscale;
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 g4 = ld4(g + i * 4);
        f32x4 m4 = ld4(m + i * 4);
        f32x4 v4 = ld4(v + i * 4);
        f32x4 w4 = ld4(w + i * 4);
        // elements of this group in front of n_decay: 4 in the filters, 0 in the biases, 1..3 in the one group that straddles
        const size_t e0 = i * 4;
        const int nd = e0 + 4 <= n_decay ? 4 : e0 >= n_decay ? 0 : (int)(n_decay - e0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gs = gscale * g4[k];
            const float mn = (a.b1 * m4[k]) + (a.omb1 * gs);
            const float vn = (a.b2 * v4[k]) + (a.omb2 * (gs * gs));
            const float den = (sqrtf(vn) * a.rs2) + a.eps;
            const float u = mn / den;
            const float wk = w4[k];
            const float x = k < nd ? wk - (a.ld * wk) : wk;
            w4[k] = x - (a.ss * u);
            m4[k] = mn;
            v4[k] = vn;
        }
        st4(m + i * 4, m4);
        st4(v + i * 4, v4);
        st4(w + i * 4, w4);
    }
}

static inline int adamw_grid(size_t n4) {
    size_t g = (n4 + ADAMW_BLOCK - 1) / ADAMW_BLOCK;
    if (g > (size_t)ADAMW_GRID_CAP) g = ADAMW_GRID_CAP;
    return g < 1 ? 1 : (int)g;
}

void adamw_check(float b1, float b2, float eps, float decay) {
    SSD_REQUIRE(b1 >= 0.f && b1 < 1.f, "update rule: beta1 %g is outside [0, 1)", (double)b1);
    SSD_REQUIRE(b2 >= 0.f && b2 < 1.f, "update rule: beta2 %g is outside [0, 1)", (double)b2);
    SSD_REQUIRE(eps > 0.f && std::isfinite(eps), "update rule: eps %g is not a finite number > 0", (double)eps);
    SSD_REQUIRE(decay >= 0.f && std::isfinite(decay), "update rule: decay %g is not a finite number >= 0", (double)decay);
}

void adamw_update(float* w, float* m, float* v, const float* g, size_t n, size_t n_decay, float lr, float b1, float b2, float eps,
                  float decay, long long t, float gscale, float max_norm, void* ws, float* report, hipStream_t s) {
    adamw_check(b1, b2, eps, decay);
    SSD_REQUIRE(t >= 1, "update rule: the count of AdamW updates must be >= 1, got %lld", t);
    SSD_REQUIRE(n % 4 == 0, "update rule: arena size must be a multiple of 4");
    SSD_REQUIRE(n_decay <= n, "update rule: n_decay %zu exceeds the arena's %zu floats", n_decay, n);
    AdamScalars a;
    a.b1 = b1;
    a.b2 = b2;
    a.omb1 = (float)(1.0 - (double)b1);
    a.omb2 = (float)(1.0 - (double)b2);
    a.rs2 = (float)(1.0 / std::sqrt(1.0 - std::pow((double)b2, (double)t)));
    a.eps = eps;
    a.ld = (float)((double)lr * (double)decay);
    a.ss = (float)((double)lr / (1.0 - std::pow((double)b1, (double)t)));
    const dim3 grid(adamw_grid(n / 4)), block(ADAMW_BLOCK);
    if (max_norm == 0.f) {
        ProfScope prof("adamw_update", 0.0, 28.0 * n, s);
        hipLaunchKernelGGL(adamw_kernel<false>, grid, block, 0, s, w, m, v, g, n / 4, n_decay, a, gscale, (const ClipState*)nullptr);
        HIP_OK(hipGetLastError());
        return;
    }
    grad_norm_pass(g, n, gscale, max_norm, ws, report, s);
    ProfScope prof("adamw_update_clipped", 0.0, 28.0 * n, s);
    hipLaunchKernelGGL(adamw_kernel<true>, grid, block, 0, s, w, m, v, g, n / 4, n_decay, a, gscale, (const ClipState*)ws);
    HIP_OK(hipGetLastError());
}

// ---- weight EMA (contract in include/ssdvgg_hip.h "weight EMA"): e -= omd * (e - w), two roundings of their own and
// the subtraction's, in that order.  HBM-bound: 12 bytes per parameter (e, w in; e out); adamw_kernel's shape, 16 bytes per lane and
// trip with both loads in flight before the first use.  Padding floats of the arena are averaged like any other.
__global__ __launch_bounds__(ADAMW_BLOCK) void ema_kernel(float* __restrict__ e, const float* __restrict__ w, size_t n4, float omd) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        f32x4 e4 = ld4(e + i * 4);
        const f32x4 w4 = ld4(w + i * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float diff = e4[k] - w4[k];
            e4[k] = e4[k] - (omd * diff);
        }
        st4(e + i * 4, e4);
    }
}

// The contents of two arenas exchanged: 16 bytes per parameter (a, b in; a, b out).  Every group of four is read and written by one
// lane alone, so a and b need no order between lanes.  The two must not overlap (__restrict__): ema_buffers_check refuses that.
__global__ __launch_bounds__(ADAMW_BLOCK) void swap_kernel(float* __restrict__ a, float* __restrict__ b, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 a4 = ld4(a + i * 4);
        const f32x4 b4 = ld4(b + i * 4);
        st4(a + i * 4, b4);
        st4(b + i * 4, a4);
    }
}

void ema_check(float decay) {
    // (a NaN fails both comparisons; 0.99999999 is 1.0 by the time it is a float)
    SSD_REQUIRE(decay > 0.f && decay < 1.f, "weight EMA: decay %g is outside (0, 1)", (double)decay);
}

// what both kernels assume of their two buffers: n a multiple of 4, 16-byte aligned (they move f32x4), no overlap (__restrict__)
static void ema_buffers_check(const float* a, const float* b, size_t n) {
    SSD_REQUIRE(n % 4 == 0, "weight EMA: arena size must be a multiple of 4");
    SSD_REQUIRE(((uintptr_t)a | (uintptr_t)b) % 16 == 0, "weight EMA: the buffers must be 16-byte aligned");
    const uintptr_t lo = std::min((uintptr_t)a, (uintptr_t)b), hi = std::max((uintptr_t)a, (uintptr_t)b);
    SSD_REQUIRE(n == 0 || hi - lo >= n * sizeof(float), "weight EMA: the two buffers overlap");
}

void ema_update(float* e, const float* w, size_t n, float decay, long long t, hipStream_t s) {
    ema_check(decay);
    SSD_REQUIRE(t >= 0, "weight EMA: the count of EMA updates must be >= 0, got %lld", t);
    ema_buffers_check(e, w, n);
    // TensorFlow's num_updates form: the average follows quickly at first
    const double d = std::min((double)decay, (1.0 + (double)t) / (10.0 + (double)t));
    const float omd = (float)(1.0 - d);
    ProfScope prof("ema_update", 0.0, 12.0 * n, s);
    hipLaunchKernelGGL(ema_kernel, dim3(adamw_grid(n / 4)), dim3(ADAMW_BLOCK), 0, s, e, w, n / 4, omd);
    HIP_OK(hipGetLastError());
}

void ema_swap(float* a, float* b, size_t n, hipStream_t s) {
    ema_buffers_check(a, b, n);
    ProfScope prof("ema_swap", 0.0, 16.0 * n, s);
    hipLaunchKernelGGL(swap_kernel, dim3(adamw_grid(n / 4)), dim3(ADAMW_BLOCK), 0, s, a, b, n / 4);
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
