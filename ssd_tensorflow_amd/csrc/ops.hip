// HBM-bound layers of the SSD-VGG step for gfx950: pooling, L2 normalisation, the
// multibox head assembly / softmax / hard-negative-mined loss, momentum update.
// All reductions use a fixed order (no float atomics): results are run-to-run identical.
#include "ops.h"
#include "bf16.h"

namespace ssd {

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

static inline int grid_for(size_t n, int block = 256, int cap = 256 * 16) {
    size_t g = (n + block - 1) / block;
    if (g > (size_t)cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// =================================================================================
// max pooling
// =================================================================================
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(PoolDesc d, const T* __restrict__ x, T* __restrict__ y) {
    const int C4 = d.C >> 2;
    const size_t total = (size_t)d.B * d.Ho * d.Wo * C4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        size_t pix = idx / C4;
        const int ow = (int)(pix % d.Wo);
        pix /= d.Wo;
        const int oh = (int)(pix % d.Ho);
        const int b = (int)(pix / d.Ho);
        const int h0 = oh * d.stride - d.pad_h, w0 = ow * d.stride - d.pad_w;
        const float ninf = -__builtin_inff();
        f32x4 m = {ninf, ninf, ninf, ninf};
        for (int kh = 0; kh < d.k; ++kh) {
            const int h = h0 + kh;
            if ((unsigned)h >= (unsigned)d.Hi) continue;
            for (int kw = 0; kw < d.k; ++kw) {
                const int w = w0 + kw;
                if ((unsigned)w >= (unsigned)d.Wi) continue;
                const f32x4 v = ld4t(x + (((size_t)b * d.Hi + h) * d.Wi + w) * d.C + c4 * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
            }
        }
        st4t(y + idx * 4, m);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(PoolDesc d, const T* __restrict__ x,
                                                          const T* __restrict__ dy, T* __restrict__ dx,
                                                          int accumulate, int relu_mask) {
    const int C4 = d.C >> 2;
    const size_t total = (size_t)d.B * d.Hi * d.Wi * C4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        size_t pix = idx / C4;
        const int w = (int)(pix % d.Wi);
        pix /= d.Wi;
        const int h = (int)(pix % d.Hi);
        const int b = (int)(pix / d.Hi);
        const f32x4 self = ld4t(x + idx * 4);
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (relu_mask && !(self[0] > 0.f) && !(self[1] > 0.f) && !(self[2] > 0.f) && !(self[3] > 0.f)) {
            st4t(dx + idx * 4, g);                    // every component is masked whatever arrives
            continue;
        }
        int n = h + d.pad_h - d.k + 1;
        const int oh_lo = n <= 0 ? 0 : (n + d.stride - 1) / d.stride;
        const int oh_hi = min(d.Ho - 1, (h + d.pad_h) / d.stride);
        n = w + d.pad_w - d.k + 1;
        const int ow_lo = n <= 0 ? 0 : (n + d.stride - 1) / d.stride;
        const int ow_hi = min(d.Wo - 1, (w + d.pad_w) / d.stride);
        for (int oh = oh_lo; oh <= oh_hi; ++oh) {
            for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                const int h0 = oh * d.stride - d.pad_h, w0 = ow * d.stride - d.pad_w;
                bool first[4] = {true, true, true, true};
                for (int kh = 0; kh < d.k; ++kh) {
                    const int hh = h0 + kh;
                    if ((unsigned)hh >= (unsigned)d.Hi) continue;
                    for (int kw = 0; kw < d.k; ++kw) {
                        const int ww = w0 + kw;
                        if ((unsigned)ww >= (unsigned)d.Wi) continue;
                        if (hh == h && ww == w) continue;
                        const bool before = hh < h || (hh == h && ww < w);
                        const f32x4 v = ld4t(x + (((size_t)b * d.Hi + hh) * d.Wi + ww) * d.C + c4 * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (before ? v[e] >= self[e] : v[e] > self[e]) first[e] = false;
                    }
                }
                const f32x4 gy = ld4t(dy + (((size_t)b * d.Ho + oh) * d.Wo + ow) * d.C + c4 * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (first[e]) g[e] += gy[e];
            }
        }
        if (accumulate) g += ld4t(dx + idx * 4);
        if (relu_mask) {
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = self[e] > 0.f ? g[e] : 0.f;
        }
        st4t(dx + idx * 4, g);
    }
}

// ---- 2x2 stride-2 SAME pooling: never overlaps and never pads before the image -----------------------------------------
// One workgroup per output row (b, oh); a thread owns one window x V channels, V = 16 bytes' worth (4 fp32 / 8 bf16).
// All of a window's loads are issued up front, unconditionally, from clamped coordinates (a cell outside the image re-reads
// its in-image neighbour and is ignored by the `ok` test afterwards): a predicated load makes the loads wait for each other
// (s_waitcnt vmcnt(0) after each).  Index math is 32-bit, the row split is per workgroup (scalar).
template <typename T, int V> struct RawV;
template <> struct RawV<float, 4> { typedef f32x4 type; };
template <> struct RawV<bf16_t, 4> { typedef u32x2 type; };
template <> struct RawV<bf16_t, 8> { typedef u32x4 type; };
__device__ __forceinline__ void unpack(f32x4 r, float (&f)[4]) { f[0] = r[0]; f[1] = r[1]; f[2] = r[2]; f[3] = r[3]; }
__device__ __forceinline__ void unpack(u32x2 r, float (&f)[4]) { f[0] = lo2f(r[0]); f[1] = hi2f(r[0]); f[2] = lo2f(r[1]); f[3] = hi2f(r[1]); }
__device__ __forceinline__ void unpack(u32x4 r, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = lo2f(r[i]); f[2 * i + 1] = hi2f(r[i]); }
}
__device__ __forceinline__ void pack(const float (&f)[4], f32x4& r) { r = f32x4{f[0], f[1], f[2], f[3]}; }
__device__ __forceinline__ void pack(const float (&f)[4], u32x2& r) { r = u32x2{pack2(f[0], f[1]), pack2(f[2], f[3])}; }
__device__ __forceinline__ void pack(const float (&f)[8], u32x4& r) {
    r = u32x4{pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7])};
}

struct PoolRow {      // the output row of this workgroup
    int b, oh, h0, h1;
    bool okh;
    __device__ __forceinline__ PoolRow(const PoolDesc& d) {
        oh = blockIdx.x % d.Ho; b = blockIdx.x / d.Ho;
        h0 = oh * 2; okh = h0 + 1 < d.Hi; h1 = okh ? h0 + 1 : h0;
    }
};

template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(PoolDesc d, const T* __restrict__ x,
                                                             const T* __restrict__ dy, T* __restrict__ dx,
                                                             int accumulate, int relu_mask) {
    typedef typename RawV<T, V>::type raw_t;
    const PoolRow R(d);
    const unsigned CV = d.C / V, items = d.Wo * CV;
    const size_t in0 = ((size_t)R.b * d.Hi + R.h0) * d.Wi * d.C, in1 = ((size_t)R.b * d.Hi + R.h1) * d.Wi * d.C;
    const T* dyr = dy + (size_t)blockIdx.x * d.Wo * d.C;
    for (unsigned i = threadIdx.x; i < items; i += 256) {
        const unsigned ow = i / CV, cv = i - ow * CV;
        const int w0 = ow * 2;
        const bool okw = w0 + 1 < d.Wi;
        const int w1 = okw ? w0 + 1 : w0;
        const size_t o[4] = {in0 + (size_t)w0 * d.C + cv * V, in0 + (size_t)w1 * d.C + cv * V,
                             in1 + (size_t)w0 * d.C + cv * V, in1 + (size_t)w1 * d.C + cv * V};
        const bool ok[4] = {true, okw, R.okh, R.okh && okw};
        raw_t rx[4], ro[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) rx[q] = *reinterpret_cast<const raw_t*>(x + o[q]);
        const raw_t rg = *reinterpret_cast<const raw_t*>(dyr + (size_t)i * V);
        if (accumulate) {
#pragma unroll
            for (int q = 0; q < 4; ++q) ro[q] = *reinterpret_cast<const raw_t*>(dx + o[q]);
        }
        float v[4][V], gy[V], g[4][V];
#pragma unroll
        for (int q = 0; q < 4; ++q) unpack(rx[q], v[q]);
        unpack(rg, gy);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (accumulate) unpack(ro[q], g[q]);
            else {
#pragma unroll
                for (int e = 0; e < V; ++e) g[q][e] = 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            int a = 0;
            float m = v[0][e];                       // cell 0 is always inside the image
#pragma unroll
            for (int q = 1; q < 4; ++q)
                if (ok[q] && v[q][e] > m) { m = v[q][e]; a = q; }   // strict: the first maximum wins
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (a == q) g[q][e] += gy[e];
                if (relu_mask && !(v[q][e] > 0.f)) g[q][e] = 0.f;   // every component is masked whatever arrives
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!ok[q]) continue;
            raw_t out;
            pack(g[q], out);
            *reinterpret_cast<raw_t*>(dx + o[q]) = out;
        }
    }
}

// The same pooling with a 12-bit record per (window, 4 channels) written by the forward pass: per channel the
// first maximum's cell (2 bits) and whether that maximum is positive (1 bit).  Backward then needs neither the
// input tensor (argmax) nor its sign (relu mask of the producing conv): it reads record + dy and writes dx,
// 0.58x the bytes of the kernel above.  Valid when the pooled tensor has no other consumer (nothing to accumulate).
template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool2x2_fwd_rec_kernel(PoolDesc d, const T* __restrict__ x, T* __restrict__ y,
                                                                 unsigned short* __restrict__ rec) {
    typedef typename RawV<T, V>::type raw_t;
    const PoolRow R(d);
    const unsigned CV = d.C / V, items = d.Wo * CV;
    const T* x0 = x + ((size_t)R.b * d.Hi + R.h0) * d.Wi * d.C;
    const T* x1 = x + ((size_t)R.b * d.Hi + R.h1) * d.Wi * d.C;
    T* yr = y + (size_t)blockIdx.x * d.Wo * d.C;
    unsigned short* rr = rec + (size_t)blockIdx.x * d.Wo * (d.C / 4);
    for (unsigned i = threadIdx.x; i < items; i += 256) {
        const unsigned ow = i / CV, cv = i - ow * CV;
        const int w0 = ow * 2;
        const bool okw = w0 + 1 < d.Wi;
        const int w1 = okw ? w0 + 1 : w0;
        const bool ok[4] = {true, okw, R.okh, R.okh && okw};
        raw_t rx[4];
        rx[0] = *reinterpret_cast<const raw_t*>(x0 + (size_t)w0 * d.C + cv * V);
        rx[1] = *reinterpret_cast<const raw_t*>(x0 + (size_t)w1 * d.C + cv * V);
        rx[2] = *reinterpret_cast<const raw_t*>(x1 + (size_t)w0 * d.C + cv * V);
        rx[3] = *reinterpret_cast<const raw_t*>(x1 + (size_t)w1 * d.C + cv * V);
        float v[4][V], m[V];
#pragma unroll
        for (int q = 0; q < 4; ++q) unpack(rx[q], v[q]);
        unsigned r[V / 4];
#pragma unroll
        for (int gq = 0; gq < V / 4; ++gq) r[gq] = 0;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            unsigned a = 0;
            float mm = v[0][e];                      // cell 0 is always inside the image
#pragma unroll
            for (int q = 1; q < 4; ++q)
                if (ok[q] && v[q][e] > mm) { mm = v[q][e]; a = q; }   // strict: the first maximum wins
            m[e] = mm;
            r[e / 4] |= (a | (mm > 0.f ? 4u : 0u)) << (3 * (e & 3));
        }
        raw_t out;
        pack(m, out);
        *reinterpret_cast<raw_t*>(yr + (size_t)i * V) = out;
        if constexpr (V == 8) *reinterpret_cast<unsigned*>(rr + (size_t)i * 2) = r[0] | (r[1] << 16);
        else rr[i] = (unsigned short)r[0];
    }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool2x2_bwd_rec_kernel(PoolDesc d, const unsigned short* __restrict__ rec,
                                                                 const T* __restrict__ dy, T* __restrict__ dx, int relu_mask) {
    typedef typename RawV<T, V>::type raw_t;
    const PoolRow R(d);
    const unsigned CV = d.C / V, items = d.Wo * CV;
    T* d0 = dx + ((size_t)R.b * d.Hi + R.h0) * d.Wi * d.C;
    T* d1 = dx + ((size_t)R.b * d.Hi + R.h1) * d.Wi * d.C;
    const T* dyr = dy + (size_t)blockIdx.x * d.Wo * d.C;
    const unsigned short* rr = rec + (size_t)blockIdx.x * d.Wo * (d.C / 4);
    for (unsigned i = threadIdx.x; i < items; i += 256) {
        const unsigned ow = i / CV, cv = i - ow * CV;
        const int w0 = ow * 2;
        const bool okw = w0 + 1 < d.Wi;
        unsigned rw;
        if constexpr (V == 8) rw = *reinterpret_cast<const unsigned*>(rr + (size_t)i * 2);
        else rw = rr[i];
        const raw_t rg = *reinterpret_cast<const raw_t*>(dyr + (size_t)i * V);
        float gy[V];
        unpack(rg, gy);
        const bool ok[4] = {true, okw, R.okh, R.okh && okw};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!ok[q]) continue;
            float g[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const unsigned re = (rw >> (16 * (e / 4) + 3 * (e & 3))) & 7u;
                g[e] = ((re & 3u) == (unsigned)q && (!relu_mask || (re & 4u))) ? gy[e] : 0.f;
            }
            raw_t out;
            pack(g, out);
            *reinterpret_cast<raw_t*>((q >> 1 ? d1 : d0) + (size_t)(w0 + (q & 1)) * d.C + cv * V) = out;
        }
    }
}

// Overlapping pooling (3x3 stride 1, mod_pool5): pass A finds every window's first maximum once
// (its scan-order cell index, one byte per channel); pass B lets every input cell collect dy from
// the <= 9 windows whose recorded maximum it is.  27 loads per cell instead of 81.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_argmax_kernel(PoolDesc d, const T* __restrict__ x, unsigned* __restrict__ arg) {
    const int C4 = d.C >> 2;
    const size_t total = (size_t)d.B * d.Ho * d.Wo * C4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        size_t pix = idx / C4;
        const int ow = (int)(pix % d.Wo);
        pix /= d.Wo;
        const int oh = (int)(pix % d.Ho);
        const int b = (int)(pix / d.Ho);
        const int h0 = oh * d.stride - d.pad_h, w0 = ow * d.stride - d.pad_w;
        const float ninf = -__builtin_inff();
        f32x4 m = {ninf, ninf, ninf, ninf};
        unsigned a[4] = {255u, 255u, 255u, 255u};
        for (int kh = 0; kh < d.k; ++kh) {
            const int h = h0 + kh;
            if ((unsigned)h >= (unsigned)d.Hi) continue;
            for (int kw = 0; kw < d.k; ++kw) {
                const int w = w0 + kw;
                if ((unsigned)w >= (unsigned)d.Wi) continue;
                const f32x4 v = ld4t(x + (((size_t)b * d.Hi + h) * d.Wi + w) * d.C + c4 * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (v[e] > m[e] || a[e] == 255u) { m[e] = v[e]; a[e] = (unsigned)(kh * d.k + kw); }   // strict: first maximum
            }
        }
        arg[idx] = a[0] | (a[1] << 8) | (a[2] << 16) | (a[3] << 24);
    }
}

// K x K windows (K = 2, 3) with every tap's load issued before the first comparison: coordinates outside the image are
// clamped for the address and excluded by `ok` afterwards.  Writes the maxima (y != nullptr) and / or the first
// maximum's scan-order tap per channel (arg != nullptr: the record pass A of the backward below).  32-bit index math.
template <typename T, int K>
__global__ __launch_bounds__(256) void maxpool_taps_kernel(PoolDesc d, const T* __restrict__ x, T* __restrict__ y,
                                                           unsigned* __restrict__ arg) {
    typedef typename RawV<T, 4>::type raw_t;
    const unsigned C4 = d.C >> 2, total = (unsigned)d.B * d.Ho * d.Wo * C4;
    for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        unsigned pix = idx / C4;
        const unsigned c4 = idx - pix * C4;
        const int ow = (int)(pix % d.Wo);
        pix /= d.Wo;
        const int oh = (int)(pix % d.Ho);
        const int b = (int)(pix / d.Ho);
        const int h0 = oh * d.stride - d.pad_h, w0 = ow * d.stride - d.pad_w;
        raw_t r[K * K];
        bool ok[K * K];
#pragma unroll
        for (int kh = 0; kh < K; ++kh)
#pragma unroll
            for (int kw = 0; kw < K; ++kw) {
                const int h = h0 + kh, w = w0 + kw;
                ok[kh * K + kw] = (unsigned)h < (unsigned)d.Hi && (unsigned)w < (unsigned)d.Wi;
                const int hc = min(max(h, 0), d.Hi - 1), wc = min(max(w, 0), d.Wi - 1);
                r[kh * K + kw] = *reinterpret_cast<const raw_t*>(x + (((size_t)b * d.Hi + hc) * d.Wi + wc) * d.C + c4 * 4);
            }
        const float ninf = -__builtin_inff();
        float m[4] = {ninf, ninf, ninf, ninf};
        unsigned a[4] = {255u, 255u, 255u, 255u};
#pragma unroll
        for (int t = 0; t < K * K; ++t) {
            float v[4];
            unpack(r[t], v);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (ok[t] && (v[e] > m[e] || a[e] == 255u)) { m[e] = v[e]; a[e] = (unsigned)t; }   // strict: first maximum
        }
        if (y) {
            raw_t out;
            pack(m, out);
            *reinterpret_cast<raw_t*>(y + (size_t)idx * 4) = out;
        }
        if (arg) arg[idx] = a[0] | (a[1] << 8) | (a[2] << 16) | (a[3] << 24);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_arg_kernel(PoolDesc d, const T* __restrict__ x, const unsigned* __restrict__ arg,
                                                              const T* __restrict__ dy, T* __restrict__ dx,
                                                              int accumulate, int relu_mask) {
    const int C4 = d.C >> 2;
    const size_t total = (size_t)d.B * d.Hi * d.Wi * C4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        size_t pix = idx / C4;
        const int w = (int)(pix % d.Wi);
        pix /= d.Wi;
        const int h = (int)(pix % d.Hi);
        const int b = (int)(pix / d.Hi);
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        int n = h + d.pad_h - d.k + 1;
        const int oh_lo = n <= 0 ? 0 : (n + d.stride - 1) / d.stride;
        const int oh_hi = min(d.Ho - 1, (h + d.pad_h) / d.stride);
        n = w + d.pad_w - d.k + 1;
        const int ow_lo = n <= 0 ? 0 : (n + d.stride - 1) / d.stride;
        const int ow_hi = min(d.Wo - 1, (w + d.pad_w) / d.stride);
        for (int oh = oh_lo; oh <= oh_hi; ++oh)
            for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                const size_t o = (((size_t)b * d.Ho + oh) * d.Wo + ow) * C4 + c4;
                const unsigned me = (unsigned)((h - (oh * d.stride - d.pad_h)) * d.k + (w - (ow * d.stride - d.pad_w)));
                const unsigned a = arg[o];
                const f32x4 gy = ld4t(dy + o * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (((a >> (8 * e)) & 255u) == me) g[e] += gy[e];
            }
        if (accumulate) g += ld4t(dx + idx * 4);
        if (relu_mask) {
            const f32x4 self = ld4t(x + idx * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = self[e] > 0.f ? g[e] : 0.f;
        }
        st4t(dx + idx * 4, g);
    }
}

// Pass B for stride 1 (mod_pool5): input cell (h, w) is tap (j, i) of window (h + pad - j, w + pad - i).  The K x K records
// and gradients are loaded up front from clamped window coordinates, then summed in the order of the kernel above
// (windows ascending = taps descending).
template <typename T, int K>
__global__ __launch_bounds__(256) void maxpool_bwd_arg_s1_kernel(PoolDesc d, const T* __restrict__ x, const unsigned* __restrict__ arg,
                                                                 const T* __restrict__ dy, T* __restrict__ dx,
                                                                 int accumulate, int relu_mask) {
    typedef typename RawV<T, 4>::type raw_t;
    const unsigned C4 = d.C >> 2, total = (unsigned)d.B * d.Hi * d.Wi * C4;
    for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        unsigned pix = idx / C4;
        const unsigned c4 = idx - pix * C4;
        const int w = (int)(pix % d.Wi);
        pix /= d.Wi;
        const int h = (int)(pix % d.Hi);
        const int b = (int)(pix / d.Hi);
        raw_t rg[K * K], rself, rold;
        unsigned ra[K * K];
        bool ok[K * K];
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const int oh = h + d.pad_h - j, ow = w + d.pad_w - i;
                ok[j * K + i] = (unsigned)oh < (unsigned)d.Ho && (unsigned)ow < (unsigned)d.Wo;
                const int ohc = min(max(oh, 0), d.Ho - 1), owc = min(max(ow, 0), d.Wo - 1);
                const size_t o = (((size_t)b * d.Ho + ohc) * d.Wo + owc) * C4 + c4;
                ra[j * K + i] = arg[o];
                rg[j * K + i] = *reinterpret_cast<const raw_t*>(dy + o * 4);
            }
        if (relu_mask) rself = *reinterpret_cast<const raw_t*>(x + (size_t)idx * 4);
        if (accumulate) rold = *reinterpret_cast<const raw_t*>(dx + (size_t)idx * 4);
        float g[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = K * K - 1; t >= 0; --t) {
            float gy[4];
            unpack(rg[t], gy);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (ok[t] && ((ra[t] >> (8 * e)) & 255u) == (unsigned)t) g[e] += gy[e];
        }
        if (accumulate) {
            float old[4];
            unpack(rold, old);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] += old[e];
        }
        if (relu_mask) {
            float self[4];
            unpack(rself, self);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = self[e] > 0.f ? g[e] : 0.f;
        }
        raw_t out;
        pack(g, out);
        *reinterpret_cast<raw_t*>(dx + (size_t)idx * 4) = out;
    }
}

template <typename T>
static void maxpool_fwd_t(const PoolDesc& d, const T* x, T* y, hipStream_t s) {
    SSD_REQUIRE(d.C % 4 == 0, "maxpool: C must be a multiple of 4");
    const size_t total = (size_t)d.B * d.Ho * d.Wo * (d.C / 4);
    ProfScope prof("maxpool_fwd", 0.0, sizeof(T) * (double)d.C * d.B * ((double)d.Hi * d.Wi + (double)d.Ho * d.Wo), s);
    const bool small_idx = (double)d.B * d.Hi * d.Wi * d.C < 2.0e9;
    if (d.k == 3 && small_idx)
        hipLaunchKernelGGL((maxpool_taps_kernel<T, 3>), dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, d, x, y, (unsigned*)nullptr);
    else if (d.k == 2 && small_idx)
        hipLaunchKernelGGL((maxpool_taps_kernel<T, 2>), dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, d, x, y, (unsigned*)nullptr);
    else
        hipLaunchKernelGGL(maxpool_fwd_kernel<T>, dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, d, x, y);
    HIP_OK(hipGetLastError());
}

bool maxpool_rec_applicable(const PoolDesc& d) { return d.k == 2 && d.stride == 2 && d.pad_h == 0 && d.pad_w == 0 && d.C % 4 == 0; }
size_t maxpool_rec_bytes(const PoolDesc& d) { return (size_t)d.B * d.Ho * d.Wo * (d.C / 4) * sizeof(unsigned short); }

template <typename T>
static void maxpool_fwd_rec_t(const PoolDesc& d, const T* x, T* y, void* rec, hipStream_t s) {
    SSD_REQUIRE(maxpool_rec_applicable(d), "maxpool record: 2x2 stride-2 pooling without leading padding only");
    const size_t total = (size_t)d.B * d.Ho * d.Wo * (d.C / 4);
    ProfScope prof("maxpool_fwd", 0.0, sizeof(T) * (double)d.C * d.B * ((double)d.Hi * d.Wi + (double)d.Ho * d.Wo) + 2.0 * total, s);
    if (sizeof(T) == 2 && d.C % 8 == 0)
        hipLaunchKernelGGL((maxpool2x2_fwd_rec_kernel<T, sizeof(T) == 2 ? 8 : 4>), dim3(d.B * d.Ho), dim3(256), 0, s, d, x, y, (unsigned short*)rec);
    else
        hipLaunchKernelGGL((maxpool2x2_fwd_rec_kernel<T, 4>), dim3(d.B * d.Ho), dim3(256), 0, s, d, x, y, (unsigned short*)rec);
    HIP_OK(hipGetLastError());
}
void maxpool_fwd_rec(const PoolDesc& d, const float* x, float* y, void* rec, hipStream_t s) { maxpool_fwd_rec_t(d, x, y, rec, s); }
void maxpool_fwd_rec(const PoolDesc& d, const bf16_t* x, bf16_t* y, void* rec, hipStream_t s) { maxpool_fwd_rec_t(d, x, y, rec, s); }

template <typename T>
static void maxpool_bwd_rec_t(const PoolDesc& d, const void* rec, const T* dy, T* dx, bool relu_mask, hipStream_t s) {
    const size_t total = (size_t)d.B * d.Ho * d.Wo * (d.C / 4);
    ProfScope prof("maxpool_bwd", 0.0, sizeof(T) * (double)d.C * d.B * ((double)d.Hi * d.Wi + (double)d.Ho * d.Wo) + 2.0 * total, s);
    if (sizeof(T) == 2 && d.C % 8 == 0)
        hipLaunchKernelGGL((maxpool2x2_bwd_rec_kernel<T, sizeof(T) == 2 ? 8 : 4>), dim3(d.B * d.Ho), dim3(256), 0, s, d, (const unsigned short*)rec, dy,
                           dx, (int)relu_mask);
    else
        hipLaunchKernelGGL((maxpool2x2_bwd_rec_kernel<T, 4>), dim3(d.B * d.Ho), dim3(256), 0, s, d, (const unsigned short*)rec, dy, dx, (int)relu_mask);
    HIP_OK(hipGetLastError());
}
void maxpool_bwd_rec(const PoolDesc& d, const void* rec, const float* dy, float* dx, bool relu_mask, hipStream_t s) {
    maxpool_bwd_rec_t(d, rec, dy, dx, relu_mask, s);
}
void maxpool_bwd_rec(const PoolDesc& d, const void* rec, const bf16_t* dy, bf16_t* dx, bool relu_mask, hipStream_t s) {
    maxpool_bwd_rec_t(d, rec, dy, dx, relu_mask, s);
}

size_t maxpool_bwd_ws_bytes(const PoolDesc& d) {
    return (d.k == 2 && d.stride == 2) ? 0 : (size_t)d.B * d.Ho * d.Wo * (d.C / 4) * sizeof(unsigned);
}

void maxpool_fwd(const PoolDesc& d, const float* x, float* y, hipStream_t s) { maxpool_fwd_t(d, x, y, s); }
void maxpool_fwd(const PoolDesc& d, const bf16_t* x, bf16_t* y, hipStream_t s) { maxpool_fwd_t(d, x, y, s); }

// 3x3 stride-1 pooling (mod_pool5) whose forward pass keeps every window's first-maximum tap (the scratch of maxpool_bwd, 4
// bytes per window and 4 channels): backward then runs its second pass only -- the first one, which recomputes exactly this,
// sat on the data-gradient chain's critical path (28 of 51 us at batch 32, profiles/r05_l_timeline_merged_tail_bf16.txt)
bool maxpool_arg_applicable(const PoolDesc& d) { return d.k == 3 && d.stride == 1 && d.C % 4 == 0 && (double)d.B * d.Hi * d.Wi * d.C < 2.0e9; }
template <typename T>
static void maxpool_fwd_arg_t(const PoolDesc& d, const T* x, T* y, void* arg, hipStream_t s) {
    SSD_REQUIRE(maxpool_arg_applicable(d) && arg != nullptr, "maxpool_fwd_arg: 3x3 stride-1 pooling with a record buffer");
    const size_t total = (size_t)d.B * d.Ho * d.Wo * (d.C / 4);
    ProfScope prof("maxpool_fwd", 0.0, sizeof(T) * (double)d.C * d.B * ((double)d.Hi * d.Wi + (double)d.Ho * d.Wo) + 4.0 * total, s);
    hipLaunchKernelGGL((maxpool_taps_kernel<T, 3>), dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, d, x, y, (unsigned*)arg);
    HIP_OK(hipGetLastError());
}
template <typename T>
static void maxpool_bwd_arg_t(const PoolDesc& d, const T* x, const void* arg, const T* dy, T* dx, bool accumulate, bool relu_mask, hipStream_t s) {
    SSD_REQUIRE(maxpool_arg_applicable(d) && arg != nullptr, "maxpool_bwd_arg: 3x3 stride-1 pooling with the forward pass' record");
    const size_t total = (size_t)d.B * d.Hi * d.Wi * (d.C / 4);
    ProfScope prof("maxpool_bwd", 0.0, sizeof(T) * (double)d.C * d.B * (2.0 * d.Hi * d.Wi + (double)d.Ho * d.Wo), s);
    hipLaunchKernelGGL((maxpool_bwd_arg_s1_kernel<T, 3>), dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, d, x, (const unsigned*)arg, dy, dx,
                       (int)accumulate, (int)relu_mask);
    HIP_OK(hipGetLastError());
}
void maxpool_fwd_arg(const PoolDesc& d, const float* x, float* y, void* arg, hipStream_t s) { maxpool_fwd_arg_t(d, x, y, arg, s); }
void maxpool_fwd_arg(const PoolDesc& d, const bf16_t* x, bf16_t* y, void* arg, hipStream_t s) { maxpool_fwd_arg_t(d, x, y, arg, s); }
void maxpool_bwd_arg(const PoolDesc& d, const float* x, const void* arg, const float* dy, float* dx, bool accumulate, bool relu_mask, hipStream_t s) {
    maxpool_bwd_arg_t(d, x, arg, dy, dx, accumulate, relu_mask, s);
}
void maxpool_bwd_arg(const PoolDesc& d, const bf16_t* x, const void* arg, const bf16_t* dy, bf16_t* dx, bool accumulate, bool relu_mask, hipStream_t s) {
    maxpool_bwd_arg_t(d, x, arg, dy, dx, accumulate, relu_mask, s);
}

template <typename T>
static void maxpool_bwd_t(const PoolDesc& d, const T* x, const T* dy, T* dx, bool accumulate, bool relu_mask, void* ws,
                          hipStream_t s) {
    SSD_REQUIRE(d.C % 4 == 0, "maxpool: C must be a multiple of 4");
    const size_t total = (size_t)d.B * d.Hi * d.Wi * (d.C / 4);
    ProfScope prof("maxpool_bwd", 0.0, sizeof(T) * (double)d.C * d.B * (2.0 * d.Hi * d.Wi + (double)d.Ho * d.Wo), s);
    if (d.k == 2 && d.stride == 2 && d.pad_h == 0 && d.pad_w == 0) {
        if (sizeof(T) == 2 && d.C % 8 == 0)
            hipLaunchKernelGGL((maxpool2x2_bwd_kernel<T, sizeof(T) == 2 ? 8 : 4>), dim3(d.B * d.Ho), dim3(256), 0, s, d, x, dy, dx, (int)accumulate,
                               (int)relu_mask);
        else
            hipLaunchKernelGGL((maxpool2x2_bwd_kernel<T, 4>), dim3(d.B * d.Ho), dim3(256), 0, s, d, x, dy, dx, (int)accumulate, (int)relu_mask);
        HIP_OK(hipGetLastError());
        return;
    }
    if (ws) {
        const size_t nwin = (size_t)d.B * d.Ho * d.Wo * (d.C / 4);
        if (d.k == 3 && d.stride == 1 && (double)d.B * d.Hi * d.Wi * d.C < 2.0e9) {      // mod_pool5: every load up front
            hipLaunchKernelGGL((maxpool_taps_kernel<T, 3>), dim3(grid_for(nwin, 256, 256 * 32)), dim3(256), 0, s, d, x, (T*)nullptr, (unsigned*)ws);
            hipLaunchKernelGGL((maxpool_bwd_arg_s1_kernel<T, 3>), dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, d, x,
                               (const unsigned*)ws, dy, dx, (int)accumulate, (int)relu_mask);
        } else {
            hipLaunchKernelGGL(maxpool_argmax_kernel<T>, dim3(grid_for(nwin, 256, 256 * 32)), dim3(256), 0, s, d, x, (unsigned*)ws);
            hipLaunchKernelGGL(maxpool_bwd_arg_kernel<T>, dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, d, x,
                               (const unsigned*)ws, dy, dx, (int)accumulate, (int)relu_mask);
        }
        HIP_OK(hipGetLastError());
        return;
    }
    hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, d, x, dy, dx,
                       (int)accumulate, (int)relu_mask);
    HIP_OK(hipGetLastError());
}

void maxpool_bwd(const PoolDesc& d, const float* x, const float* dy, float* dx, bool accumulate, bool relu_mask, void* ws,
                 hipStream_t s) {
    maxpool_bwd_t(d, x, dy, dx, accumulate, relu_mask, ws, s);
}
void maxpool_bwd(const PoolDesc& d, const bf16_t* x, const bf16_t* dy, bf16_t* dx, bool accumulate, bool relu_mask, void* ws,
                 hipStream_t s) {
    maxpool_bwd_t(d, x, dy, dx, accumulate, relu_mask, ws, s);
}

// =================================================================================
// L2 normalisation over channels: one wave64 per pixel, each lane owns float4 chunks
// =================================================================================
constexpr int L2_MAXJ = 4;   // C <= 1024

// Four channels as they lie in memory (fp32: 16 bytes, bf16: 8 bytes).  The kernels below load RAW values for all their
// pixels first (unconditionally, from clamped addresses) and convert / mask them in a second pass: a conversion or a select
// on a loaded value inside the load group makes every load wait for the one before it (s_waitcnt vmcnt(0) each; the first
// version of l2norm_bwd ran its 8 loads per iteration as 8 dependent round trips: 80 us for 142 MB).
template <typename T> struct Raw4;
template <> struct Raw4<float> { typedef f32x4 type; };
template <> struct Raw4<bf16_t> { typedef u32x2 type; };
template <typename T>
__device__ __forceinline__ typename Raw4<T>::type ld4raw(const T* p) { return *reinterpret_cast<const typename Raw4<T>::type*>(p); }
__device__ __forceinline__ f32x4 cvt4(f32x4 r) { return r; }
__device__ __forceinline__ f32x4 cvt4(u32x2 w) { return f32x4{lo2f(w[0]), hi2f(w[0]), lo2f(w[1]), hi2f(w[1])}; }

template <typename T, int J>      // J = ceil(C / 256) chunks of 4 channels per lane
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(int npix, int C, const T* __restrict__ x,
                                                         const float* __restrict__ scale, T* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    constexpr int PX = 2;
    int cc[J];
    f32x4 sc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = lane * 4 + 256 * j;
        cc[j] = c < C ? c : 0;
        sc[j] = ld4(scale + cc[j]);
    }
    for (int pix0 = wave * PX; pix0 < npix; pix0 += nwaves * PX) {
        typename Raw4<T>::type raw[PX][J];
#pragma unroll
        for (int q = 0; q < PX; ++q) {
            const int pix = min(pix0 + q, npix - 1);
#pragma unroll
            for (int j = 0; j < J; ++j) raw[q][j] = ld4raw(x + (size_t)pix * C + cc[j]);
        }
        f32x4 v[PX][J];
        float ss[PX];
#pragma unroll
        for (int q = 0; q < PX; ++q) {
            ss[q] = 0.f;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                v[q][j] = cvt4(raw[q][j]);
                if (lane * 4 + 256 * j >= C) v[q][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                ss[q] += v[q][j][0] * v[q][j][0] + v[q][j][1] * v[q][j][1] + v[q][j][2] * v[q][j][2] + v[q][j][3] * v[q][j][3];
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int q = 0; q < PX; ++q) ss[q] += __shfl_xor(ss[q], o, 64);
#pragma unroll
        for (int q = 0; q < PX; ++q) {
            const int pix = pix0 + q;
            if (pix >= npix) continue;
            const float r = rsqrtf(fmaxf(ss[q], 1e-12f));
#pragma unroll
            for (int j = 0; j < J; ++j)
                if (lane * 4 + 256 * j < C) st4t(y + (size_t)pix * C + cc[j], sc[j] * v[q][j] * r);
        }
    }
}

// dx = scale*dy*r - x * (sum_c scale*dy*x) * r^3  (when sum x^2 > eps; else the norm is the
// constant sqrt(eps) and only the first term remains).  dscale partials per block -> ws.
template <typename T, int J>
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(int npix, int C, const T* __restrict__ x,
                                                         const float* __restrict__ scale, const T* __restrict__ dy,
                                                         T* __restrict__ dx, float* __restrict__ ws) {
    __shared__ float red[4][256 * J];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    constexpr int PX = J <= 2 ? 4 : 2;      // pixels per wave and iteration: 2 PX J loads in flight, their shuffle trees overlap
    int cc[J];
    f32x4 ds[J], sc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = lane * 4 + 256 * j;
        cc[j] = c < C ? c : 0;
        ds[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        sc[j] = ld4(scale + cc[j]);
        if (c >= C) sc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int pix0 = wave * PX; pix0 < npix; pix0 += nwaves * PX) {
        typename Raw4<T>::type rx[PX][J], rg[PX][J];
#pragma unroll
        for (int q = 0; q < PX; ++q) {
            const int pix = min(pix0 + q, npix - 1);
#pragma unroll
            for (int j = 0; j < J; ++j) {
                rx[q][j] = ld4raw(x + (size_t)pix * C + cc[j]);
                rg[q][j] = ld4raw(dy + (size_t)pix * C + cc[j]);
            }
        }
        f32x4 v[PX][J], g[PX][J];
        float ss[PX], t[PX];
#pragma unroll
        for (int q = 0; q < PX; ++q) {
            ss[q] = t[q] = 0.f;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                v[q][j] = cvt4(rx[q][j]);
                g[q][j] = cvt4(rg[q][j]);
                if (lane * 4 + 256 * j >= C) v[q][j] = g[q][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ss[q] += v[q][j][e] * v[q][j][e];
                    t[q] += sc[j][e] * g[q][j][e] * v[q][j][e];
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int q = 0; q < PX; ++q) {
                ss[q] += __shfl_xor(ss[q], o, 64);
                t[q] += __shfl_xor(t[q], o, 64);
            }
#pragma unroll
        for (int q = 0; q < PX; ++q) {
            const int pix = pix0 + q;
            if (pix >= npix) continue;
            const float r = rsqrtf(fmaxf(ss[q], 1e-12f));
            const float k = ss[q] > 1e-12f ? t[q] * r * r * r : 0.f;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (lane * 4 + 256 * j < C) st4t(dx + (size_t)pix * C + cc[j], sc[j] * g[q][j] * r - v[q][j] * k);
                ds[j] += g[q][j] * v[q][j] * r;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wib][lane * 4 + 256 * j + e] = ds[j][e];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x)
        ws[(size_t)blockIdx.x * C + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// column sums of ws[nrows][C] in a fixed order
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ ws, int nrows, int C, float* __restrict__ out) {
    // a workgroup = 16 columns x 16 row groups; a thread sums its rows (r = group, group + 16, ...) four independent loads at a
    // time (the first version walked 128 rows per wave with one dependent load each: 25 us for 1 MB), fixed order throughout
    __shared__ float red[16][17];
    const int col = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + col;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (c < C) {
        int r = rg;
        for (; r + 48 < nrows; r += 64) {
            const float a0 = ws[(size_t)r * C + c], a1 = ws[(size_t)(r + 16) * C + c];
            const float a2 = ws[(size_t)(r + 32) * C + c], a3 = ws[(size_t)(r + 48) * C + c];
            s0 += a0; s1 += a1; s2 += a2; s3 += a3;
        }
        for (; r < nrows; r += 16) s0 += ws[(size_t)r * C + c];
    }
    red[rg][col] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (rg == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += red[g][col];
        out[c] = t;
    }
}

static int l2_blocks(int npix) {      // (2048 workgroups were measured: the pixel loop gains nothing, the column sums lose)
    int b = (npix + 3) / 4;
    return b > 512 ? 512 : (b < 1 ? 1 : b);
}

template <typename T>
static void l2norm_fwd_t(int npix, int C, const T* x, const float* scale, T* y, hipStream_t s) {
    SSD_REQUIRE(C % 4 == 0 && C <= 1024, "l2norm: C must be a multiple of 4 and <= 1024");
    int b = (npix + 7) / 8;      // 4 waves x 2 pixels per workgroup and iteration
    if (b > 4096) b = 4096;
    ProfScope prof("l2norm_fwd", 0.0, 2.0 * sizeof(T) * npix * C, s);
    switch ((C + 255) / 256) {
    case 1: hipLaunchKernelGGL((l2norm_fwd_kernel<T, 1>), dim3(b), dim3(256), 0, s, npix, C, x, scale, y); break;
    case 2: hipLaunchKernelGGL((l2norm_fwd_kernel<T, 2>), dim3(b), dim3(256), 0, s, npix, C, x, scale, y); break;
    default: hipLaunchKernelGGL((l2norm_fwd_kernel<T, L2_MAXJ>), dim3(b), dim3(256), 0, s, npix, C, x, scale, y); break;
    }
    HIP_OK(hipGetLastError());
}
void l2norm_fwd(int npix, int C, const float* x, const float* scale, float* y, hipStream_t s) { l2norm_fwd_t(npix, C, x, scale, y, s); }
void l2norm_fwd(int npix, int C, const bf16_t* x, const float* scale, bf16_t* y, hipStream_t s) { l2norm_fwd_t(npix, C, x, scale, y, s); }

size_t l2norm_bwd_ws_floats(int npix, int C) { return (size_t)l2_blocks(npix) * C; }

template <typename T>
static void l2norm_bwd_t(int npix, int C, const T* x, const float* scale, const T* dy, T* dx, float* dscale, float* ws,
                         hipStream_t s) {
    SSD_REQUIRE(C % 4 == 0 && C <= 1024, "l2norm: C must be a multiple of 4 and <= 1024");
    const int nb = l2_blocks(npix);
    ProfScope prof("l2norm_bwd", 0.0, 3.0 * sizeof(T) * npix * C, s);
    switch ((C + 255) / 256) {
    case 1: hipLaunchKernelGGL((l2norm_bwd_kernel<T, 1>), dim3(nb), dim3(256), 0, s, npix, C, x, scale, dy, dx, ws); break;
    case 2: hipLaunchKernelGGL((l2norm_bwd_kernel<T, 2>), dim3(nb), dim3(256), 0, s, npix, C, x, scale, dy, dx, ws); break;
    default: hipLaunchKernelGGL((l2norm_bwd_kernel<T, L2_MAXJ>), dim3(nb), dim3(256), 0, s, npix, C, x, scale, dy, dx, ws); break;
    }
    hipLaunchKernelGGL(colsum_kernel, dim3((C + 15) / 16), dim3(256), 0, s, ws, nb, C, dscale);
    HIP_OK(hipGetLastError());
}
void l2norm_bwd(int npix, int C, const float* x, const float* scale, const float* dy, float* dx, float* dscale, float* ws,
                hipStream_t s) {
    l2norm_bwd_t(npix, C, x, scale, dy, dx, dscale, ws, s);
}
void l2norm_bwd(int npix, int C, const bf16_t* x, const float* scale, const bf16_t* dy, bf16_t* dx, float* dscale, float* ws,
                hipStream_t s) {
    l2norm_bwd_t(npix, C, x, scale, dy, dx, dscale, ws, s);
}

// =================================================================================
// multibox heads: anchor a of image b lives in map i at (box type j, cell hw):
//   a = off[i] + j*hw[i] + cell ;  source row (b*hw[i] + cell) of buf[i], columns j*nvars..
// =================================================================================
constexpr int MAXV = 32;   // nvars <= 32  (num_classes <= 27)

// ---- work decomposition of the head kernels ---------------------------------------------------------------
// One workgroup owns HCH consecutive cells of one feature map of one image, i.e. the HCH * nj anchors whose
// head outputs are the HCH contiguous rows [cell][ld] of the fused head buffer.  Every global access of the
// kernels below is then a contiguous run: the rows themselves (HCH*ld floats), and per box type j the HCH
// anchors' [nvars] records of result / labels (anchor a = off + j*hw + cell).  Tiles are staged through LDS
// with 16-byte loads; thread (cell = t & 31, j = t >> 5) works on one anchor from LDS at odd strides.
constexpr int HCH = 32;
constexpr int HTHREADS = 256;               // 32 cells x 8 type slots (nj <= 8)
constexpr int HSLOTS = HTHREADS / HCH;      // box type slots per workgroup
// Rows wider than MAXV (num_classes > 27) go to heads_wide_kernel on workgroups of hch = 16, 8 or 4 cells, the largest
// whose LDS tile fits HEAD_LDS_MAX; its HSLOTS * hch anchors then get HTHREADS / (HSLOTS * hch) = 2, 4 or 8 lanes each.
constexpr size_t HEAD_LDS_MAX = 64 * 1024;
struct HeadGrid {
    int blk_off[MAX_MAPS + 1];              // first workgroup of each map
    int nchunk[MAX_MAPS];                   // cell chunks per image
    int ldp_max, nj_max;
    int hch, lg_hch;                        // cells per workgroup (HCH for rows of <= MAXV values), its log2
};
static size_t heads_lds_floats(int hch, int ldp_max, int nj_max, int nv) {
    return (size_t)hch * ldp_max + (size_t)nj_max * hch * nv;
}
HeadLayout head_layout(int nmaps, const int* hw, const int* nj, int nvars) {
    SSD_REQUIRE(nmaps >= 1 && nmaps <= MAX_MAPS, "heads: 1..%d feature maps", MAX_MAPS);
    HeadLayout L{};
    L.nmaps = nmaps; L.nvars = nvars;
    int off = 0;
    for (int i = 0; i < nmaps; ++i) {
        SSD_REQUIRE(hw[i] >= 1 && nj[i] >= 1, "heads: map %d has no anchors", i);
        L.hw[i] = hw[i];
        L.nj[i] = nj[i];
        L.ld[i] = head_ld(nj[i], nvars);
        L.off[i] = off;
        off += nj[i] * hw[i];
    }
    L.off[nmaps] = L.A = off;
    return L;
}

static HeadGrid head_grid(const HeadLayout& L, int B) {
    HeadGrid g{};
    for (int i = 0; i < L.nmaps; ++i) {
        g.ldp_max = std::max(g.ldp_max, L.ld[i] + 1);
        g.nj_max = std::max(g.nj_max, L.nj[i]);
    }
    SSD_REQUIRE(g.nj_max <= HSLOTS, "heads: at most %d box types per map", HSLOTS);
    SSD_REQUIRE(L.nvars <= MAX_CLASSES + 5, "heads: num_classes + 5 must be <= %d", MAX_CLASSES + 5);
    g.hch = HCH;
    if (L.nvars > MAXV) {
        g.hch = HCH / 2;
        while (g.hch > 4 && heads_lds_floats(g.hch, g.ldp_max, g.nj_max, L.nvars) * sizeof(float) > HEAD_LDS_MAX) g.hch >>= 1;
        SSD_REQUIRE(heads_lds_floats(g.hch, g.ldp_max, g.nj_max, L.nvars) * sizeof(float) <= HEAD_LDS_MAX, "heads: tile too large");
    }
    g.lg_hch = __builtin_ctz(g.hch);
    int off = 0;
    for (int i = 0; i < L.nmaps; ++i) {
        g.blk_off[i] = off;
        g.nchunk[i] = (L.hw[i] + g.hch - 1) / g.hch;
        off += g.nchunk[i] * B;
    }
    for (int i = L.nmaps; i <= MAX_MAPS; ++i) g.blk_off[i] = off;
    return g;
}
struct HeadBlock {
    int map, b, cell0, ncell;
};
__device__ __forceinline__ HeadBlock head_block(const HeadLayout& L, const HeadGrid& G) {
    int i = 0;
#pragma unroll
    for (int k = 1; k < MAX_MAPS; ++k)
        if (k < L.nmaps && (int)blockIdx.x >= G.blk_off[k]) i = k;
    const int local = blockIdx.x - G.blk_off[i];
    HeadBlock r;
    r.map = i;
    r.b = local / G.nchunk[i];
    r.cell0 = (local - r.b * G.nchunk[i]) << G.lg_hch;
    r.ncell = min(G.hch, L.hw[i] - r.cell0);
    return r;
}

// contiguous global run (4-byte aligned) <-> LDS, 16-byte global accesses on the aligned middle
__device__ __forceinline__ void run_to_lds(float* dst, const float* __restrict__ src, int n) {
    const int pre = min(n, (int)((4u - (unsigned)(((size_t)src >> 2) & 3u)) & 3u));
    if ((int)threadIdx.x < pre) dst[threadIdx.x] = src[threadIdx.x];
    const int n4 = (n - pre) >> 2;
    for (int i = threadIdx.x; i < n4; i += HTHREADS) {
        const f32x4 v = ld4(src + pre + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[pre + 4 * i + e] = v[e];
    }
    for (int i = pre + 4 * n4 + threadIdx.x; i < n; i += HTHREADS) dst[i] = src[i];
}
__device__ __forceinline__ void lds_to_run(float* __restrict__ dst, const float* src, int n) {
    const int pre = min(n, (int)((4u - (unsigned)(((size_t)dst >> 2) & 3u)) & 3u));
    if ((int)threadIdx.x < pre) dst[threadIdx.x] = src[threadIdx.x];
    const int n4 = (n - pre) >> 2;
    for (int i = threadIdx.x; i < n4; i += HTHREADS) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = src[pre + 4 * i + e];
        st4(dst + pre + 4 * i, v);
    }
    for (int i = pre + 4 * n4 + threadIdx.x; i < n; i += HTHREADS) dst[i] = src[i];
}

// ---- generalized IoU box regression (Rezatofighi et al. 2019) on the encoded offsets -------------------------------------------------
// IoU and GIoU are ratios of areas, unchanged under a separate scaling and shift per axis, so the box of the offsets t is taken in
// units of its own anchor (centre (t0, t1) / 10, size exp((t2, t3) / 5)) and the ground truth of the same anchor from the label
// offsets g likewise: no anchor table.  Offsets are clamped to +-100 (no product overflows: exp(20)^2 ~ 2e17), so every width is
// >= exp(-20) > 0, U > 0 and C > 0, and no epsilon is added.  L = 1 - GIoU = (1 - I / U) + (1 - U / C), in [0, 2).
// Evaluated in the ground-truth box's frame (centre difference first: the one subtraction that cancels is then exact or rounds
// relative to its own result, not to |t|), with the rounding of t / 5 carried into the exponential (exp(q) * (1 + (t - 5 q) / 5),
// t - 5 q exact by fma), so every width is good to ~4 * 2^-24 relative instead of 20 * 2^-24.  No contraction: the order written
// here is the order evaluated, and the tie cases of the tests (unit boxes at multiples of 1/2) are exact ties.
// At a tie of a max / min the derivative goes to the predicted coordinate; boxes that only touch are not live.
// dt (GRAD): dL / dt, 0 on a clamped component.
constexpr int LOC_SMOOTH_L1 = 0, LOC_GIOU = 1;
__device__ __forceinline__ float giou_size(float t) {
    const float q = t / 5.f;
    const float e = expf(q);
    return fmaf(e, fmaf(-5.f, q, t) / 5.f, e);
}
template <bool GRAD>
__device__ __forceinline__ float giou_eval(const float* t, const float* g, float* dt) {
#pragma clang fp contract(off)
    float tc[4], gc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        tc[i] = fminf(fmaxf(t[i], -100.f), 100.f);
        gc[i] = fminf(fmaxf(g[i], -100.f), 100.f);
    }
    const float dx = (tc[0] - gc[0]) / 10.f, dy = (tc[1] - gc[1]) / 10.f;
    const float wp = giou_size(tc[2]), hp = giou_size(tc[3]), wg = giou_size(gc[2]), hg = giou_size(gc[3]);
    const float x0p = dx - 0.5f * wp, x1p = dx + 0.5f * wp, x0g = -0.5f * wg, x1g = 0.5f * wg;
    const float y0p = dy - 0.5f * hp, y1p = dy + 0.5f * hp, y0g = -0.5f * hg, y1g = 0.5f * hg;
    const float iw = fmaxf(fminf(x1p, x1g) - fmaxf(x0p, x0g), 0.f), ih = fmaxf(fminf(y1p, y1g) - fmaxf(y0p, y0g), 0.f);
    const float cw = fmaxf(x1p, x1g) - fminf(x0p, x0g), ch = fmaxf(y1p, y1g) - fminf(y0p, y0g);
    const float I = iw * ih, U = wp * hp + wg * hg - I, C = cw * ch;
    const float iou = I / U, uc = U / C;
    if constexpr (GRAD) {
        const float kA = iou / U - 1.f / C, kI = -1.f / U - kA, kC = uc / C;
        const bool live = iw > 0.f && ih > 0.f;
        const float gx0 = kI * ((live && x0p >= x0g) ? -ih : 0.f) - kA * hp + kC * (x0p <= x0g ? -ch : 0.f);
        const float gx1 = kI * ((live && x1p <= x1g) ? ih : 0.f) + kA * hp + kC * (x1p >= x1g ? ch : 0.f);
        const float gy0 = kI * ((live && y0p >= y0g) ? -iw : 0.f) - kA * wp + kC * (y0p <= y0g ? -cw : 0.f);
        const float gy1 = kI * ((live && y1p <= y1g) ? iw : 0.f) + kA * wp + kC * (y1p >= y1g ? cw : 0.f);
        dt[0] = fabsf(t[0]) > 100.f ? 0.f : (gx0 + gx1) / 10.f;
        dt[1] = fabsf(t[1]) > 100.f ? 0.f : (gy0 + gy1) / 10.f;
        dt[2] = fabsf(t[2]) > 100.f ? 0.f : (gx1 - gx0) * wp / 10.f;
        dt[3] = fabsf(t[3]) > 100.f ? 0.f : (gy1 - gy0) * hp / 10.f;
    }
    return fmaxf((1.f - iou) + (1.f - uc), 0.f);
}
// the localization weight of a kernel instantiation: the smooth-L1 ones take no such argument
__device__ __forceinline__ float loc_weight_arg() { return 1.f; }
__device__ __forceinline__ float loc_weight_arg(float w) { return w; }


// LOC (training): the localization term left in sl1_out, smooth-L1 (no further argument: the kernel and its arguments as they
// always were) or loc_weight * (1 - GIoU) (one more argument, the weight); only a positive anchor takes the GIoU branch.
template <bool TRAIN, int LOC = LOC_SMOOTH_L1, typename... LW>
__global__ __launch_bounds__(HTHREADS) void heads_kernel(HeadLayout L, HeadGrid G, int B, float* __restrict__ result,
                                                         const float* __restrict__ labels, float* __restrict__ ce_out,
                                                         float* __restrict__ sl1_out, unsigned char* __restrict__ pos_out, LW... loc_w) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    const HeadBlock k = head_block(L, G);
    const int nv = L.nvars, nc = nv - 4;
    const int ld = L.ld[k.map], ldp = ld + 1, nj = L.nj[k.map], hw = L.hw[k.map];
    float* hin = hsm;                         // [HCH][ldp]   raw head outputs, odd row pitch
    float* rec = hsm + HCH * G.ldp_max;       // [nj][HCH][nv] labels in, result out
    const size_t a0 = (size_t)k.b * L.A + L.off[k.map] + k.cell0;      // anchor of (type 0, first cell)
    const int nrec = k.ncell * nv;            // floats of one box type's run of [nv] records (<= 1024)
    // ---- every global load of the workgroup is issued before the first one is consumed ----------------------
    constexpr int HMAX = HCH * (MAXV * (HTHREADS / HCH) / 8 * 8) / 4 / HTHREADS + 1;     // float4 per thread, worst ld
    constexpr int RU = HCH * MAXV / HTHREADS;                                             // floats per thread and type
    const float* src = L.buf[k.map] + ((size_t)k.b * hw + k.cell0) * ld;                  // contiguous, 16-byte aligned rows
    const int n4 = (k.ncell * ld) >> 2;
    f32x4 hv[HMAX];
#pragma unroll
    for (int u = 0; u < HMAX; ++u) {
        const int i = threadIdx.x + HTHREADS * u;
        hv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < n4) hv[u] = ld4(src + 4 * i);
    }
    float lv[TRAIN ? HTHREADS / HCH : 1][RU];
    if constexpr (TRAIN) {
#pragma unroll
        for (int j = 0; j < HTHREADS / HCH; ++j) {
            const float* run = labels + (a0 + (size_t)j * hw) * nv;       // 4-byte aligned only: dword loads, 256 B per wave
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int i = threadIdx.x + HTHREADS * u;
                lv[j][u] = (j < nj && i < nrec) ? run[i] : 0.f;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < HMAX; ++u) {
        const int i = threadIdx.x + HTHREADS * u;
        if (i < n4) {
            const int row = (4 * i) / ld, col = 4 * i - row * ld;
#pragma unroll
            for (int e = 0; e < 4; ++e) hin[row * ldp + col + e] = hv[u][e];
        }
    }
    if constexpr (TRAIN) {
#pragma unroll
        for (int j = 0; j < HTHREADS / HCH; ++j)
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int i = threadIdx.x + HTHREADS * u;
                if (j < nj && i < nrec) rec[j * HCH * nv + i] = lv[j][u];
            }
    }
    __syncthreads();
    const int cell = threadIdx.x & (HCH - 1), j = threadIdx.x / HCH;
    if (cell < k.ncell && j < nj) {
        const float* zsrc = hin + cell * ldp + j * nv;
        float* r = rec + (j * HCH + cell) * nv;
        float z[MAXV], y[MAXV];
        float m = -__builtin_inff();
#pragma unroll
        for (int c = 0; c < MAXV; ++c) {
            z[c] = c < nv ? zsrc[c] : 0.f;
            y[c] = (TRAIN && c < nv) ? r[c] : 0.f;
            if (c < nc) m = fmaxf(m, z[c]);
        }
        // softmax = e_c / sum(e), e_c = exp(z_c - max) evaluated ONCE per class with the hardware exponential
        // (v_exp_f32 on (z - max) * log2 e: relative error ~ |z - max| * 2^-24 <= 1e-5 over the fp32 range, against
        // the 1e-3 bar); log once, accurately
        float e[MAXV];
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < MAXV; ++c) {
            e[c] = c < nc ? __expf(z[c] - m) : 0.f;
            se += e[c];
        }
        const float lse = m + logf(se);
        const float inv = 1.f / se;
#pragma unroll
        for (int c = 0; c < MAXV; ++c)
            if (c < nv) r[c] = c < nc ? e[c] * inv : z[c];
        if constexpr (TRAIN) {
            float ce = 0.f, sl = 0.f;
            const bool pos = y[nc - 1] == 0.f;
#pragma unroll
            for (int c = 0; c < MAXV; ++c) {
                if (c < nc) {
                    if (y[c] != 0.f) ce += y[c] * (lse - z[c]);
                } else if (LOC == LOC_SMOOTH_L1 && c < nv) {
                    const float d = z[c] - y[c];
                    const float ad = fabsf(d);
                    sl += ad < 1.f ? 0.5f * d * d : ad - 0.5f;
                }
            }
            if constexpr (LOC == LOC_GIOU) {
                if (pos) {
                    float gt[4];
#pragma unroll
                    for (int c = 1; c < MAXV; ++c)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (c == nc + i) gt[i] = y[c];
                    sl = loc_weight_arg(loc_w...) * giou_eval<false>(zsrc + nc, gt, nullptr);
                }
            }
            const size_t idx = a0 + (size_t)j * hw + cell;
            ce_out[idx] = ce;
            sl1_out[idx] = pos ? sl : 0.f;
            pos_out[idx] = pos ? 1 : 0;
        }
    }
    __syncthreads();
    // result: per box type one contiguous run of [nv] records; dword stores, 256 B per wave
#pragma unroll
    for (int jj = 0; jj < HTHREADS / HCH; ++jj) {
        float* run = result + (a0 + (size_t)jj * hw) * nv;
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int i = threadIdx.x + HTHREADS * u;
            if (jj < nj && i < nrec) run[i] = rec[jj * HCH * nv + i];
        }
    }
}

// heads_kernel for rows of more than MAXV values (num_classes 28..127): same results, same tiles and global runs, but
// G.hch (16, 8 or 4) cells per workgroup and a group of gl = HTHREADS / (HSLOTS * hch) lanes per anchor.  The lanes of a
// group stride the anchor's values in LDS (no per-value register arrays, so no spills at any width); max, sum of
// exponentials, cross-entropy and smooth-L1 meet by xor-shuffles inside the group (one wave holds whole groups).
template <bool TRAIN, int LOC = LOC_SMOOTH_L1, typename... LW>
__global__ __launch_bounds__(HTHREADS) void heads_wide_kernel(HeadLayout L, HeadGrid G, int B, float* __restrict__ result,
                                                              const float* __restrict__ labels, float* __restrict__ ce_out,
                                                              float* __restrict__ sl1_out, unsigned char* __restrict__ pos_out,
                                                              LW... loc_w) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    const HeadBlock k = head_block(L, G);
    const int hch = G.hch;
    const int nv = L.nvars, nc = nv - 4;
    const int ld = L.ld[k.map], ldp = ld + 1, nj = L.nj[k.map], hw = L.hw[k.map];
    float* hin = hsm;                         // [hch][ldp]   raw head outputs, odd row pitch
    float* rec = hsm + hch * G.ldp_max;       // [nj][hch][nv] labels in, result out
    const size_t a0 = (size_t)k.b * L.A + L.off[k.map] + k.cell0;
    const int nrec = k.ncell * nv;
    const float* src = L.buf[k.map] + ((size_t)k.b * hw + k.cell0) * ld;      // contiguous, 16-byte aligned rows
    const int n4 = (k.ncell * ld) >> 2;
#pragma unroll 4
    for (int i = threadIdx.x; i < n4; i += HTHREADS) {
        const f32x4 v = ld4(src + 4 * i);
        const int row = (4 * i) / ld, col = 4 * i - row * ld;
#pragma unroll
        for (int e = 0; e < 4; ++e) hin[row * ldp + col + e] = v[e];
    }
    if constexpr (TRAIN)
        for (int j = 0; j < nj; ++j) run_to_lds(rec + j * hch * nv, labels + (a0 + (size_t)j * hw) * nv, nrec);
    __syncthreads();
    const int lg_gl = __builtin_ctz(HTHREADS / HSLOTS) - G.lg_hch, gl = 1 << lg_gl;
    const int slot = threadIdx.x >> lg_gl, lane = threadIdx.x & (gl - 1);
    const int cell = slot & (hch - 1), j = slot >> G.lg_hch;
    if (cell < k.ncell && j < nj) {           // uniform over the lane group
        const float* z = hin + cell * ldp + j * nv;
        float* r = rec + (j * hch + cell) * nv;
        const bool pos = TRAIN && r[nc - 1] == 0.f;     // read before any lane of the group overwrites the record
        float m = -__builtin_inff();
        for (int c = lane; c < nc; c += gl) m = fmaxf(m, z[c]);
        for (int o = gl >> 1; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        // the exponential as in heads_kernel (hardware v_exp_f32 on z - max, log once)
        float se = 0.f;
        for (int c = lane; c < nc; c += gl) se += __expf(z[c] - m);
        for (int o = gl >> 1; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
        const float lse = m + logf(se);
        const float inv = 1.f / se;
        float ce = 0.f, sl = 0.f;
        for (int c = lane; c < nc; c += gl) {
            const float zc = z[c];
            if constexpr (TRAIN) {
                const float y = r[c];
                if (y != 0.f) ce += y * (lse - zc);
            }
            r[c] = __expf(zc - m) * inv;
        }
        if constexpr (LOC == LOC_GIOU) {          // every lane of a positive's group, from the record before the loop below overwrites it
            if (pos) {
                float gt[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) gt[i] = r[nc + i];
                sl = loc_weight_arg(loc_w...) * giou_eval<false>(z + nc, gt, nullptr);
            }
        }
        for (int c = nc + lane; c < nv; c += gl) {
            const float zc = z[c];
            if constexpr (TRAIN && LOC == LOC_SMOOTH_L1) {
                const float d = zc - r[c];
                const float ad = fabsf(d);
                sl += ad < 1.f ? 0.5f * d * d : ad - 0.5f;
            }
            r[c] = zc;
        }
        if constexpr (TRAIN) {
            for (int o = gl >> 1; o > 0; o >>= 1) {
                ce += __shfl_xor(ce, o, 64);
                if constexpr (LOC == LOC_SMOOTH_L1) sl += __shfl_xor(sl, o, 64);
            }
            if (lane == 0) {
                const size_t idx = a0 + (size_t)j * hw + cell;
                ce_out[idx] = ce;
                sl1_out[idx] = pos ? sl : 0.f;
                pos_out[idx] = pos ? 1 : 0;
            }
        }
    }
    __syncthreads();
    for (int jj = 0; jj < nj; ++jj) lds_to_run(result + (a0 + (size_t)jj * hw) * nv, rec + jj * hch * nv, nrec);
}

static size_t heads_lds_bytes(const HeadLayout& L, const HeadGrid& G) {
    return heads_lds_floats(G.hch, G.ldp_max, G.nj_max, L.nvars) * sizeof(float);
}

// Rows of <= MAXV values keep heads_kernel (one thread per anchor, the row in registers), the 20-class path as measured;
// wider rows, whose register arrays would spill, take heads_wide_kernel.  Chosen by L.nvars, fixed for a handle.
template <bool TRAIN>
static void launch_heads(const HeadLayout& L, const HeadGrid& G, int B, float* result, const float* labels, float* ce, float* sl1,
                         unsigned char* pos, hipStream_t s, LocLoss loc = {}) {
    if constexpr (TRAIN) {
        if (loc.kind == LOC_GIOU) {
            if (L.nvars <= MAXV)
                hipLaunchKernelGGL((heads_kernel<true, LOC_GIOU, float>), dim3(G.blk_off[MAX_MAPS]), dim3(HTHREADS), heads_lds_bytes(L, G), s,
                                   L, G, B, result, labels, ce, sl1, pos, loc.weight);
            else
                hipLaunchKernelGGL((heads_wide_kernel<true, LOC_GIOU, float>), dim3(G.blk_off[MAX_MAPS]), dim3(HTHREADS),
                                   heads_lds_bytes(L, G), s, L, G, B, result, labels, ce, sl1, pos, loc.weight);
            return;
        }
    }
    if (L.nvars <= MAXV)
        hipLaunchKernelGGL(heads_kernel<TRAIN>, dim3(G.blk_off[MAX_MAPS]), dim3(HTHREADS), heads_lds_bytes(L, G), s, L, G, B, result,
                           labels, ce, sl1, pos);
    else
        hipLaunchKernelGGL(heads_wide_kernel<TRAIN>, dim3(G.blk_off[MAX_MAPS]), dim3(HTHREADS), heads_lds_bytes(L, G), s, L, G, B,
                           result, labels, ce, sl1, pos);
}

void heads_result(const HeadLayout& L, int B, float* result, hipStream_t s) {
    const int total = B * L.A;
    const HeadGrid G = head_grid(L, B);
    ProfScope prof("heads_result", 0.0, 8.0 * total * L.nvars, s);
    launch_heads<false>(L, G, B, result, nullptr, nullptr, nullptr, nullptr, s);
    HIP_OK(hipGetLastError());
}

// ---- per-sample: counts, sums, hard-negative selection (top-k by radix select) ------
// One workgroup per sample holds the sample's A cross-entropy values in registers (PT per thread): every
// pass of the MSB-first radix select (8 bits per pass over the float bit pattern, values are >= 0) runs from
// registers into an LDS histogram, the bin holding the k-th largest is found by a parallel suffix scan.
constexpr int SUMSQ_BLOCKS = 1024;
constexpr int LS_THREADS = 1024;
constexpr int LS_WAVES = LS_THREADS / 64;

__device__ __forceinline__ void block_sum3_1024(float& a, float& b, float& c, float* red) {     // red[3 * LS_WAVES]
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = a; red[LS_WAVES + (threadIdx.x >> 6)] = b; red[2 * LS_WAVES + (threadIdx.x >> 6)] = c;
    }
    __syncthreads();
    float ta = 0.f, tb = 0.f, tc = 0.f;
#pragma unroll
    for (int i = 0; i < LS_WAVES; ++i) { ta += red[i]; tb += red[LS_WAVES + i]; tc += red[2 * LS_WAVES + i]; }
    a = ta; b = tb; c = tc;
}

// the four losses from the per-sample results and the l2 partial sums: run by the LAST workgroup of loss_sample_kernel
// to finish (an integer ticket), always in the same order, so the result does not depend on which one that is
__device__ void loss_final_block(int B, float bnorm, const float* sample, const float* partial, int npartial, float wd,
                                 float* losses, double* dred) {
    double ss = 0.0;
    for (int i = threadIdx.x; i < npartial; i += LS_THREADS) ss += (double)__builtin_nontemporal_load(partial + i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = ss;
    // the per-sample results: one load per thread (all in flight together), then summed in sample order
    __shared__ float s_conf[LS_THREADS / 2], s_loc[LS_THREADS / 2];
    if ((int)(threadIdx.x >> 1) < B)                        // B <= LS_THREADS / 2 (checked by the launcher)
        (threadIdx.x & 1 ? s_loc : s_conf)[threadIdx.x >> 1] = __builtin_nontemporal_load(sample + (threadIdx.x >> 1) * 4 + (threadIdx.x & 1));
    __syncthreads();
    if (threadIdx.x != 0) return;
    ss = 0.0;
    for (int i = 0; i < LS_WAVES; ++i) ss += dred[i];
    float conf = 0.f, loc = 0.f;
    for (int b = 0; b < B; ++b) {
        conf += s_conf[b];
        loc += s_loc[b];
    }
    conf /= bnorm;
    loc /= bnorm;
    const float l2 = wd * (float)(0.5 * ss);
    losses[0] = conf + loc + l2;
    losses[1] = loc;
    losses[2] = conf;
    losses[3] = l2;
    __threadfence_system();      // the executor's buffer is host memory
}

template <int PT>
__device__ __forceinline__ void loss_sample_body(int b, int A, float bnorm, const float* __restrict__ ce,
                                                 const float* __restrict__ sl1, const unsigned char* __restrict__ pos,
                                                 unsigned char* __restrict__ sel, float* __restrict__ sample) {
    __shared__ float red[3 * LS_WAVES];
    __shared__ unsigned hist[256];
    __shared__ unsigned sh_prefix, sh_k, sh_ties, sh_wsum[4], sh_wtot[LS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* cb = ce + (size_t)b * A;
    const float* lb = sl1 + (size_t)b * A;
    const unsigned char* pb = pos + (size_t)b * A;
    unsigned char* sb = sel + (size_t)b * A;

    // the sample's values, loaded once (coalesced, all loads in flight together)
    unsigned u[PT];          // negatives[a] = pos ? 0 : ce  (ssdvgg.py:459) as bit patterns
    unsigned pmask = 0, vmask = 0;
    float npos = 0.f, psum = 0.f, lsum = 0.f;
    {   // pass 1 issues every load, pass 2 consumes: a consumer between two loads would make each load wait in turn
        float cv[PT], lv[PT];
        unsigned char pv[PT];
#pragma unroll
        for (int r = 0; r < PT; ++r) {
            const int a = tid + LS_THREADS * r;
            const int ac = a < A ? a : 0;           // unconditional loads from a clamped index (a select on the loaded
            cv[r] = cb[ac];                         // value would be a consumer again); masked in pass 2
            lv[r] = lb[ac];
            pv[r] = pb[ac];
        }
#pragma unroll
        for (int r = 0; r < PT; ++r) {
            const int a = tid + LS_THREADS * r;
            u[r] = 0u;
            if (a < A) {
                const bool p = pv[r] != 0;
                lsum += lv[r];
                vmask |= 1u << r;
                if (p) { pmask |= 1u << r; npos += 1.f; psum += cv[r]; }
                else u[r] = __float_as_uint(cv[r]);
            }
        }
    }
    block_sum3_1024(npos, psum, lsum, red);
    const int pos_n = (int)npos;
    const int neg_n = A - pos_n;
    const int k = min(neg_n, 3 * pos_n);
    if (pos_n == 0) {   // ssdvgg.py:513-516,552-555: the sample contributes exactly 0
#pragma unroll
        for (int r = 0; r < PT; ++r)
            if (vmask >> r & 1u) sb[tid + LS_THREADS * r] = 0;
        if (tid == 0) {
            sample[b * 4 + 0] = 0.f; sample[b * 4 + 1] = 0.f; sample[b * 4 + 2] = 0.f; sample[b * 4 + 3] = 0.f;
        }
        return;
    }
    unsigned prefix = 0, kk = (unsigned)k;   // kk-th largest among entries matching prefix
    bool ties = false;
    if (k > 0) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const unsigned himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
#pragma unroll
            for (int r = 0; r < PT; ++r) {
                const bool in = (vmask >> r & 1u) && (u[r] & himask) == (prefix & himask);
                const unsigned digit = (u[r] >> shift) & 255u;
                const unsigned long long bal = __ballot(in);
                if (bal == 0ull) continue;
                // a wave whose entries all fall into one bin (the usual case for the exponent byte) adds once
                const unsigned d0 = __builtin_amdgcn_readlane(digit, __ffsll((long long)bal) - 1);
                if (__ballot(in && digit == d0) == bal) {
                    if (lane == __ffsll((long long)bal) - 1) atomicAdd(&hist[d0], (unsigned)__popcll(bal));
                } else if (in) {
                    atomicAdd(&hist[digit], 1u);
                }
            }
            __syncthreads();
            // bin of the kk-th largest: inclusive suffix sums over bins 255..0 by the first four waves
            unsigned h = 0, inc = 0;
            if (tid < 256) {
                h = hist[255 - tid];
                inc = h;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned t = __shfl_up(inc, o, 64);
                    if (lane >= o) inc += t;
                }
                if (lane == 63) sh_wsum[wv] = inc;
            }
            __syncthreads();
            if (tid < 256) {
                for (int i = 0; i < wv; ++i) inc += sh_wsum[i];
                const unsigned exc = inc - h;
                if (inc >= kk && exc < kk) {
                    sh_prefix = prefix | ((unsigned)(255 - tid) << shift);
                    sh_k = kk - exc;
                    sh_ties = h > kk - exc ? 1u : 0u;
                }
            }
            __syncthreads();
            prefix = sh_prefix;
            kk = sh_k;
            ties = sh_ties != 0u;          // meaningful after the last pass: more entries equal T than are taken
        }
    }
    // prefix = bit pattern of the threshold T; kk = how many entries == T are taken
    const float T = __uint_as_float(prefix);
    float tsum = 0.f, z0 = 0.f, z1 = 0.f;
    if (k > 0) {
#pragma unroll
        for (int r = 0; r < PT; ++r)
            if ((vmask >> r & 1u) && u[r] > prefix) tsum += __uint_as_float(u[r]);
    }
    block_sum3_1024(tsum, z0, z1, red);
    if (k > 0) tsum += (float)kk * T;
    // selection mask; ties at T go to the LOWER index first (tf.nn.top_k)
    if (!ties) {
#pragma unroll
        for (int r = 0; r < PT; ++r)
            if (vmask >> r & 1u) sb[tid + LS_THREADS * r] = ((pmask >> r & 1u) || (k > 0 && u[r] >= prefix)) ? 1 : 0;
    } else {
        unsigned base = 0;
#pragma unroll
        for (int r = 0; r < PT; ++r) {          // a = tid + 1024 r ascends with (r, tid)
            const bool in = vmask >> r & 1u;
            const bool eq = in && u[r] == prefix;      // positives hold 0: they tie with T == 0 like the reference's zeros
            const unsigned long long bal = __ballot(eq);
            const unsigned before = __popcll(bal & ((1ull << lane) - 1ull));
            __syncthreads();
            if (lane == 0) sh_wtot[wv] = __popcll(bal);
            __syncthreads();
            unsigned wbase = base, tot = 0;
#pragma unroll
            for (int i = 0; i < LS_WAVES; ++i) {
                if (i < wv) wbase += sh_wtot[i];
                tot += sh_wtot[i];
            }
            const bool take = u[r] > prefix || (eq && wbase + before < kk);
            if (in) sb[tid + LS_THREADS * r] = ((pmask >> r & 1u) || take) ? 1 : 0;
            base += tot;
        }
    }
    if (tid == 0) {
        sample[b * 4 + 0] = (psum + tsum) / (float)pos_n;
        sample[b * 4 + 1] = lsum / (float)pos_n;
        sample[b * 4 + 2] = 1.f / ((float)pos_n * bnorm);
        sample[b * 4 + 3] = (float)pos_n;
    }
}

// One workgroup per sample.  A step may run the samples in several launches (forward lanes, net.hip): b_off is this launch's
// first sample, B the step's total -- the workgroup that draws ticket B - 1, whichever launch it belongs to, finishes.
template <int PT>
__global__ __launch_bounds__(LS_THREADS) void loss_sample_kernel(int B, int b_off, int A, float bnorm, const float* __restrict__ ce,
                                                                 const float* __restrict__ sl1,
                                                                 const unsigned char* __restrict__ pos,
                                                                 unsigned char* __restrict__ sel,
                                                                 float* __restrict__ sample, const float* __restrict__ partial,
                                                                 int npartial, float wd, float* __restrict__ losses,
                                                                 unsigned* __restrict__ ticket) {
    __shared__ double dred[LS_WAVES];
    __shared__ unsigned sh_last;
    loss_sample_body<PT>((int)blockIdx.x + b_off, A, bnorm, ce, sl1, pos, sel, sample);
    // the workgroup that draws the last ticket reduces everything (loss_final_block); the ticket resets itself
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();                                   // this sample's results before the ticket
        const unsigned t = atomicAdd(ticket, 1u);
        sh_last = t == (unsigned)B - 1u ? 1u : 0u;
        if (sh_last) *ticket = 0u;
    }
    __syncthreads();
    if (!sh_last) return;
    __threadfence();
    loss_final_block(B, bnorm, sample, partial, npartial, wd, losses, dred);
}

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ w, size_t n, float* __restrict__ partial) {
    __shared__ float red[4];
    float s = 0.f;
    const size_t n4 = n >> 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 v = ld4(w + i * 4);
        s += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}


size_t loss_work_bytes(int B, int A) {
    const size_t n = (size_t)B * A;
    size_t bytes = 0;
    bytes += n * 4 * 2;                       // ce, sl1
    bytes += ((n + 15) / 16) * 16 * 2;        // pos, sel
    bytes += (size_t)B * 4 * 4 + SUMSQ_BLOCKS * 4 + 64 + 64;
    return bytes + 256;
}

void loss_work_carve(LossWork& w, void* base, int B, int A) {
    const size_t n = (size_t)B * A;
    char* p = (char*)base;
    w.ce = (float*)p; p += n * 4;
    w.sl1 = (float*)p; p += n * 4;
    w.pos = (unsigned char*)p; p += ((n + 15) / 16) * 16;
    w.sel = (unsigned char*)p; p += ((n + 15) / 16) * 16;
    w.sample = (float*)p; p += (size_t)B * 4 * 4;
    w.partial = (float*)p; p += SUMSQ_BLOCKS * 4;
    w.losses = (float*)p; p += 64;
    w.ticket = (unsigned*)p;          // zero at allocation, resets itself
}

void l2_partials(const float* filters, size_t nfilters, LossWork& w, hipStream_t s) {
    ProfScope prof("l2_partials", 0.0, 4.0 * nfilters, s);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(SUMSQ_BLOCKS), dim3(256), 0, s, filters, nfilters, w.partial);
    HIP_OK(hipGetLastError());
}

void multibox_loss(const HeadLayout& L, int B, int b_off, int B_total, const float* result, const float* labels, LossWork& w,
                   float weight_decay, float bnorm, hipStream_t s, LocLoss loc) {
    SSD_REQUIRE(L.A <= 32 * LS_THREADS, "loss: at most %d anchors", 32 * LS_THREADS);
    SSD_REQUIRE(B_total <= LS_THREADS / 2, "loss: at most %d images per step", LS_THREADS / 2);
    const int total = B * L.A;
    const HeadGrid G = head_grid(L, B);
    if (!(bnorm > 0.f)) bnorm = (float)B_total;          // reduce_mean over this step's own batch (ssdvgg.py:520,559)
    const size_t o = (size_t)b_off * L.A;                // this launch's slice of the per-anchor work arrays
    ProfScope prof("multibox_loss", 0.0, 12.0 * total * L.nvars, s);
    launch_heads<true>(L, G, B, const_cast<float*>(result), labels, w.ce + o, w.sl1 + o, w.pos + o, s, loc);
    const int pt = (L.A + LS_THREADS - 1) / LS_THREADS;
    if (pt <= 9)
        hipLaunchKernelGGL(loss_sample_kernel<9>, dim3(B), dim3(LS_THREADS), 0, s, B_total, b_off, L.A, bnorm, w.ce, w.sl1, w.pos, w.sel, w.sample,
                           w.partial, SUMSQ_BLOCKS, weight_decay, w.losses, w.ticket);
    else if (pt <= 24)
        hipLaunchKernelGGL(loss_sample_kernel<24>, dim3(B), dim3(LS_THREADS), 0, s, B_total, b_off, L.A, bnorm, w.ce, w.sl1, w.pos, w.sel, w.sample,
                           w.partial, SUMSQ_BLOCKS, weight_decay, w.losses, w.ticket);
    else
        hipLaunchKernelGGL(loss_sample_kernel<32>, dim3(B), dim3(LS_THREADS), 0, s, B_total, b_off, L.A, bnorm, w.ce, w.sl1, w.pos, w.sel, w.sample,
                           w.partial, SUMSQ_BLOCKS, weight_decay, w.losses, w.ticket);
    HIP_OK(hipGetLastError());
}

// d/d(logits) = sel * (softmax - labels) * w_b ; d/d(loc) = pos * clip(loc - gt, -1, 1) * w_b,
// w_b = 1 / (pos_n_b * B)  (reduce_mean over the batch of per-sample normalised sums).
// All but a few hundred anchors per image are neither selected nor positive: a workgroup zero-fills its
// [HCH][ld] tile of the gradient buffer in LDS, the few flagged anchors fetch their result / label records and
// fill their columns, and the tile leaves as one contiguous run of 16-byte stores (pad columns included).
// LOC_GIOU (one more argument, the weight): d/d(loc) = pos * loc_weight * w_b * dL/dt, the four derivatives of an anchor from
// all four offsets of its result and label records: lane 0 of the anchor's group computes and stores them.
template <typename T, int LOC = LOC_SMOOTH_L1, typename... LW>
__global__ __launch_bounds__(HTHREADS) void loss_grad_kernel(HeadLayout L, HeadGrid G, int B, int b_off, const float* __restrict__ result,
                                                             const float* __restrict__ labels,
                                                             const unsigned char* __restrict__ pos,
                                                             const unsigned char* __restrict__ sel,
                                                             const float* __restrict__ sample, LW... loc_w) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];      // [G.hch][ld]
    const HeadBlock k = head_block(L, G);
    const int nv = L.nvars, nc = nv - 4;
    const int ld = L.ld[k.map], nj = L.nj[k.map], hw = L.hw[k.map];
    const int n4 = (k.ncell * ld) >> 2;
    for (int i = threadIdx.x; i < n4; i += HTHREADS) *reinterpret_cast<f32x4*>(gsm + 4 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    // HSLOTS * G.hch anchors, gl lanes each striding its columns (gl = 1 at G.hch = HCH: one thread per anchor)
    const int lg_gl = __builtin_ctz(HTHREADS / HSLOTS) - G.lg_hch, gl = 1 << lg_gl;
    const int slot = threadIdx.x >> lg_gl, lane = threadIdx.x & (gl - 1);
    const int cell = slot & (G.hch - 1), j = slot >> G.lg_hch;
    if (cell < k.ncell && j < nj) {
        const size_t idx = (size_t)k.b * L.A + L.off[k.map] + (size_t)j * hw + k.cell0 + cell;
        const bool isel = sel[idx], ipos = pos[idx];
        if (isel || ipos) {
            const float wb = sample[(k.b + b_off) * 4 + 2];
            const float* r = result + idx * nv;
            const float* y = labels + idx * nv;
            float* dst = gsm + cell * ld + j * nv;
            if (isel)
                for (int c = lane; c < nc; c += gl) dst[c] = (r[c] - y[c]) * wb;
            if constexpr (LOC == LOC_GIOU) {
                if (ipos && lane == 0) {
                    float rt[4], gt[4], dt[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { rt[i] = r[nc + i]; gt[i] = y[nc + i]; }
                    giou_eval<true>(rt, gt, dt);
                    const float lw = loc_weight_arg(loc_w...) * wb;
#pragma unroll
                    for (int i = 0; i < 4; ++i) dst[nc + i] = lw * dt[i];
                }
            } else if (ipos)
                for (int c = nc + lane; c < nv; c += gl) dst[c] = fminf(fmaxf(r[c] - y[c], -1.f), 1.f) * wb;
        }
    }
    __syncthreads();
    T* out = static_cast<T*>(L.dbuf[k.map]) + ((size_t)k.b * hw + k.cell0) * ld;
    for (int i = threadIdx.x; i < n4; i += HTHREADS) st4t(out + 4 * i, *reinterpret_cast<const f32x4*>(gsm + 4 * i));
}

void multibox_loss_grad(const HeadLayout& L, int B, int b_off, const float* result, const float* labels, const LossWork& w,
                        hipStream_t s, LocLoss loc) {
    const int total = B * L.A;
    const HeadGrid G = head_grid(L, B);
    const size_t lds = (size_t)G.hch * (G.ldp_max - 1) * sizeof(float);
    const size_t o = (size_t)b_off * L.A;
    ProfScope prof("multibox_loss_grad", 0.0, (L.grad_bf16 ? 10.0 : 12.0) * total * L.nvars, s);
    if (loc.kind == LOC_GIOU) {
        if (L.grad_bf16)
            hipLaunchKernelGGL((loss_grad_kernel<bf16_t, LOC_GIOU, float>), dim3(G.blk_off[MAX_MAPS]), dim3(HTHREADS), lds, s, L, G, B, b_off,
                               result, labels, w.pos + o, w.sel + o, w.sample, loc.weight);
        else
            hipLaunchKernelGGL((loss_grad_kernel<float, LOC_GIOU, float>), dim3(G.blk_off[MAX_MAPS]), dim3(HTHREADS), lds, s, L, G, B, b_off,
                               result, labels, w.pos + o, w.sel + o, w.sample, loc.weight);
    } else if (L.grad_bf16)
        hipLaunchKernelGGL(loss_grad_kernel<bf16_t>, dim3(G.blk_off[MAX_MAPS]), dim3(HTHREADS), lds, s, L, G, B, b_off, result, labels,
                           w.pos + o, w.sel + o, w.sample);
    else
        hipLaunchKernelGGL(loss_grad_kernel<float>, dim3(G.blk_off[MAX_MAPS]), dim3(HTHREADS), lds, s, L, G, B, b_off, result, labels,
                           w.pos + o, w.sel + o, w.sample);
    HIP_OK(hipGetLastError());
}

// ---- focal loss (Lin et al. 2017), softmax form, on what the head kernels store per anchor -------------------------
// With ce = -log p_t from heads_kernel<true>:  p_t = exp(-ce),  q = 1 - p_t = -expm1(-ce)  (never 1 - exp(-ce): the small
// cross entropies of easy anchors would lose every digit),  alpha_t = alpha (positive) or 1 - alpha (background),
//   fl    = alpha_t * q^gamma * ce                                  exactly 0 at ce == 0 for every gamma, 0 included
//   kappa = alpha_t * q^gamma * (1 + gamma * p_t * ce / q)          d fl / d logit_c = kappa * (softmax_c - label_c)
// kappa is alpha_t * (q^gamma + gamma * p_t * ce * q^(gamma-1)) with q^gamma factored out: ce / q -> 1 as q -> 0, so no
// factor grows without bound for 0 < gamma < 1; q == 0 (ce == 0) is decided apart: alpha_t at gamma == 0, else 0.
// Every anchor contributes, nothing is selected; a sample is normalised by n_b = max(pos_n, 1), so a sample without
// positives still trains its background anchors (under mining it contributes exactly 0).
// gmode: gamma when it is 0, 1 or 2 (no powf on those), -1 otherwise.
__device__ __forceinline__ float focal_qpow(float q, float gamma, int gmode) {
    if (gmode == 0) return 1.f;
    if (gmode == 1) return q;
    if (gmode == 2) return q * q;
    return powf(q, gamma);
}
__device__ __forceinline__ float focal_term(float ce, bool pos, float gamma, float alpha, int gmode) {
    if (ce == 0.f) return 0.f;
    const float q = -expm1f(-ce);
    return (pos ? alpha : 1.f - alpha) * focal_qpow(q, gamma, gmode) * ce;
}
__device__ __forceinline__ float focal_kappa(float ce, bool pos, float gamma, float alpha, int gmode) {
    const float at = pos ? alpha : 1.f - alpha;
    const float q = -expm1f(-ce);
    if (!(q > 0.f)) return gmode == 0 ? at : 0.f;
    return at * focal_qpow(q, gamma, gmode) * (1.f + gamma * expf(-ce) * (ce / q));
}

// One workgroup per sample, the lanes and the completion ticket of loss_sample_kernel: three block sums (positives, focal
// terms, smooth-L1), sel = 1 on every valid anchor, sample = (sum fl / n_b, sum sl1 / n_b, 1 / (n_b * bnorm), pos_n).
template <int PT>
__global__ __launch_bounds__(LS_THREADS) void focal_sample_kernel(int B, int b_off, int A, float bnorm, float gamma, float alpha,
                                                                  int gmode, const float* __restrict__ ce,
                                                                  const float* __restrict__ sl1,
                                                                  const unsigned char* __restrict__ pos,
                                                                  unsigned char* __restrict__ sel, float* __restrict__ sample,
                                                                  const float* __restrict__ partial, int npartial, float wd,
                                                                  float* __restrict__ losses, unsigned* __restrict__ ticket) {
    __shared__ double dred[LS_WAVES];
    __shared__ unsigned sh_last;
    __shared__ float red[3 * LS_WAVES];
    const int tid = threadIdx.x, b = (int)blockIdx.x + b_off;
    const float* cb = ce + (size_t)b * A;
    const float* lb = sl1 + (size_t)b * A;
    const unsigned char* pb = pos + (size_t)b * A;
    unsigned char* sb = sel + (size_t)b * A;
    float npos = 0.f, fsum = 0.f, lsum = 0.f;
    // Pass 1 issues every load, pass 2 consumes (loss_sample_body).  PT = 32 (A > 24576, no preset) takes two such rounds of 16:
    // its 96 values in flight at once would need more of the 128 registers that 1024 threads leave than the consumers spare,
    // and spill.  The per-thread order of every sum is the same either way.
    constexpr int ROUNDS = PT > 24 ? 2 : 1, PR = PT / ROUNDS;
#pragma unroll
    for (int r0 = 0; r0 < PT; r0 += PR) {
        float cv[PR], lv[PR];
        unsigned char pv[PR];
#pragma unroll
        for (int r = 0; r < PR; ++r) {
            const int a = tid + LS_THREADS * (r0 + r);
            const int ac = a < A ? a : 0;           // unconditional loads from a clamped index, masked in pass 2
            cv[r] = cb[ac];
            lv[r] = lb[ac];
            pv[r] = pb[ac];
        }
#pragma unroll
        for (int r = 0; r < PR; ++r) {
            const int a = tid + LS_THREADS * (r0 + r);
            if (a < A) {
                const bool p = pv[r] != 0;
                npos += p ? 1.f : 0.f;
                lsum += lv[r];                      // stored as 0 off the positives
                fsum += focal_term(cv[r], p, gamma, alpha, gmode);
                sb[a] = 1;
            }
        }
        if (ROUNDS > 1) __builtin_amdgcn_sched_barrier(0);      // (keeps the next round's loads behind this round's consumers)
    }
    block_sum3_1024(npos, fsum, lsum, red);
    if (tid == 0) {
        const float nb = fmaxf(npos, 1.f);
        sample[b * 4 + 0] = fsum / nb;
        sample[b * 4 + 1] = lsum / nb;
        sample[b * 4 + 2] = 1.f / (nb * bnorm);
        sample[b * 4 + 3] = npos;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();                                   // this sample's results before the ticket
        const unsigned t = atomicAdd(ticket, 1u);
        sh_last = t == (unsigned)B - 1u ? 1u : 0u;
        if (sh_last) *ticket = 0u;
    }
    __syncthreads();
    if (!sh_last) return;
    __threadfence();
    loss_final_block(B, bnorm, sample, partial, npartial, wd, losses, dred);
}

static int focal_gmode(float gamma) { return gamma == 0.f ? 0 : gamma == 1.f ? 1 : gamma == 2.f ? 2 : -1; }

void multibox_focal_loss(const HeadLayout& L, int B, int b_off, int B_total, const float* result, const float* labels, LossWork& w,
                         float weight_decay, float bnorm, float gamma, float alpha, hipStream_t s, LocLoss loc) {
    SSD_REQUIRE(L.A <= 32 * LS_THREADS, "loss: at most %d anchors", 32 * LS_THREADS);
    SSD_REQUIRE(B_total <= LS_THREADS / 2, "loss: at most %d images per step", LS_THREADS / 2);
    const int total = B * L.A;
    const HeadGrid G = head_grid(L, B);
    if (!(bnorm > 0.f)) bnorm = (float)B_total;
    const size_t o = (size_t)b_off * L.A;
    const int gm = focal_gmode(gamma);
    ProfScope prof("multibox_focal_loss", 0.0, 12.0 * total * L.nvars, s);
    launch_heads<true>(L, G, B, const_cast<float*>(result), labels, w.ce + o, w.sl1 + o, w.pos + o, s, loc);
    const int pt = (L.A + LS_THREADS - 1) / LS_THREADS;
    if (pt <= 9)
        hipLaunchKernelGGL(focal_sample_kernel<9>, dim3(B), dim3(LS_THREADS), 0, s, B_total, b_off, L.A, bnorm, gamma, alpha, gm, w.ce,
                           w.sl1, w.pos, w.sel, w.sample, w.partial, SUMSQ_BLOCKS, weight_decay, w.losses, w.ticket);
    else if (pt <= 24)
        hipLaunchKernelGGL(focal_sample_kernel<24>, dim3(B), dim3(LS_THREADS), 0, s, B_total, b_off, L.A, bnorm, gamma, alpha, gm, w.ce,
                           w.sl1, w.pos, w.sel, w.sample, w.partial, SUMSQ_BLOCKS, weight_decay, w.losses, w.ticket);
    else
        hipLaunchKernelGGL(focal_sample_kernel<32>, dim3(B), dim3(LS_THREADS), 0, s, B_total, b_off, L.A, bnorm, gamma, alpha, gm, w.ce,
                           w.sl1, w.pos, w.sel, w.sample, w.partial, SUMSQ_BLOCKS, weight_decay, w.losses, w.ticket);
    HIP_OK(hipGetLastError());
}

// d/d(logits) = w_b * kappa * (softmax - labels) ; d/d(loc) = pos * clip(loc - gt, -1, 1) * w_b: every anchor has a gradient,
// so the kernel is dense and HBM-bound -- it reads the result and labels records and writes the head-shaped tile, the bytes
// heads_kernel<true> moves.  Tile geometry of head_block.  result and labels share one record layout, so per box type the
// two contiguous runs of [nv] records are read with dword loads at the same flat index i (heads_kernel's label reads),
// subtracted element by element and scaled by the factor of anchor i / nv, which one thread per anchor left in LDS from ce,
// pos and the sample weight.  The tile is built in LDS at pitch ld, pad columns zero, and leaves as one run of 16-byte
// stores.  WIDE (rows of more than MAXV values, G.hch < HCH): the runs are strided over the workgroup in a loop instead of
// held in registers.  No atomics: bitwise reproducible.
// LOC_GIOU (one more argument, the weight; four more anchor factors in LDS): the anchor's thread, on a positive, fetches the four
// offsets of its result and label records and leaves pos * loc_weight * w_b * dL/dt there for the element-wise stage.
template <typename T, bool WIDE, int LOC = LOC_SMOOTH_L1, typename... LW>
__global__ __launch_bounds__(HTHREADS) void focal_grad_kernel(HeadLayout L, HeadGrid G, int B, int b_off, float gamma, float alpha,
                                                              int gmode, const float* __restrict__ result,
                                                              const float* __restrict__ labels, const float* __restrict__ ce,
                                                              const unsigned char* __restrict__ pos,
                                                              const float* __restrict__ sample, LW... loc_w) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];      // [G.hch][ld] tile, then [HSLOTS * G.hch] x 2 (GIoU: x 6) anchor factors
    const HeadBlock k = head_block(L, G);
    const int hch = G.hch;
    const int nv = L.nvars, nc = nv - 4;
    const int ld = L.ld[k.map], nj = L.nj[k.map], hw = L.hw[k.map];
    float* fk = gsm + hch * (G.ldp_max - 1);      // w_b * kappa per (type, cell)
    float* fp = fk + HSLOTS * hch;                // w_b on positives, else 0
    float* fg = fp + HSLOTS * hch;                // LOC_GIOU: [4][HSLOTS * hch] gradients of the four offsets, 0 off the positives
    const size_t a0 = (size_t)k.b * L.A + L.off[k.map] + k.cell0;      // anchor of (type 0, first cell), local to this launch
    const int nrec = k.ncell * nv;
    const float rnv = 1.f / (float)nv;
    // ---- per-anchor loads first, then the records: nothing is consumed before every load is issued (narrow rows)
    const int acell = threadIdx.x & (hch - 1), aj = threadIdx.x >> G.lg_hch;
    const bool ahave = aj < nj && acell < k.ncell;        // aj >= HSLOTS >= nj for the threads beyond the anchors
    const size_t aidx = a0 + (size_t)(ahave ? aj : 0) * hw + (ahave ? acell : 0);
    const float ace = ce[aidx];
    const bool apos = pos[aidx] != 0;
    const float wb = sample[(k.b + b_off) * 4 + 2];
    constexpr int RU = WIDE ? 1 : HCH * MAXV / HTHREADS;
    float rv[WIDE ? 1 : HSLOTS][RU], yv[WIDE ? 1 : HSLOTS][RU];
    if constexpr (!WIDE) {
#pragma unroll
        for (int j = 0; j < HSLOTS; ++j) {
            const float* rrun = result + (a0 + (size_t)j * hw) * nv;
            const float* yrun = labels + (a0 + (size_t)j * hw) * nv;
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int i = threadIdx.x + HTHREADS * u;
                const bool in = j < nj && i < nrec;
                rv[j][u] = in ? rrun[i] : 0.f;
                yv[j][u] = in ? yrun[i] : 0.f;
            }
        }
    }
    if (ahave) {
        fk[aj * hch + acell] = wb * focal_kappa(ace, apos, gamma, alpha, gmode);
        fp[aj * hch + acell] = apos ? wb : 0.f;
        if constexpr (LOC == LOC_GIOU) {
            float dt[4] = {0.f, 0.f, 0.f, 0.f};
            if (apos) {
                float rt[4], gt[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { rt[i] = result[aidx * nv + nc + i]; gt[i] = labels[aidx * nv + nc + i]; }
                giou_eval<true>(rt, gt, dt);
            }
            const float lw = loc_weight_arg(loc_w...) * wb;
#pragma unroll
            for (int i = 0; i < 4; ++i) fg[i * HSLOTS * hch + aj * hch + acell] = lw * dt[i];
        }
    }
    const int npad = ld - nj * nv;
    for (int i = threadIdx.x; i < k.ncell * npad; i += HTHREADS) {
        const int row = i / npad;
        gsm[row * ld + nj * nv + (i - row * npad)] = 0.f;
    }
    __syncthreads();
    if constexpr (!WIDE) {
#pragma unroll
        for (int j = 0; j < HSLOTS; ++j)
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int i = threadIdx.x + HTHREADS * u;
                if (j < nj && i < nrec) {
                    const int cell = (int)(((float)i + 0.5f) * rnv), c = i - cell * nv;      // i < 1024: exact
                    const float d = rv[j][u] - yv[j][u];
                    if constexpr (LOC == LOC_GIOU)
                        gsm[cell * ld + j * nv + c] = c < nc ? d * fk[j * hch + cell] : fg[(c - nc) * HSLOTS * hch + j * hch + cell];
                    else
                        gsm[cell * ld + j * nv + c] = c < nc ? d * fk[j * hch + cell] : fminf(fmaxf(d, -1.f), 1.f) * fp[j * hch + cell];
                }
            }
    } else {
        for (int j = 0; j < nj; ++j) {
            const float* rrun = result + (a0 + (size_t)j * hw) * nv;
            const float* yrun = labels + (a0 + (size_t)j * hw) * nv;
            if constexpr (LOC == LOC_GIOU) {
                // the class columns alone are read (a record difference that only the columns c < nc use makes the compiler sink its
                // two loads under that condition, and the unrolled loop then waits for every pair of loads in turn); the loc columns
                // come from LDS
                const float rnc = 1.f / (float)nc;
                const int ncls = k.ncell * nc;
#pragma unroll 4
                for (int e = threadIdx.x; e < ncls; e += HTHREADS) {
                    const int cell = (int)(((float)e + 0.5f) * rnc), c = e - cell * nc;      // e < 16 * 128: exact
                    const int i = cell * nv + c;
                    gsm[cell * ld + j * nv + c] = (rrun[i] - yrun[i]) * fk[j * hch + cell];
                }
                for (int e = threadIdx.x; e < 4 * k.ncell; e += HTHREADS)
                    gsm[(e >> 2) * ld + j * nv + nc + (e & 3)] = fg[(e & 3) * HSLOTS * hch + j * hch + (e >> 2)];
            } else {
#pragma unroll 4
                for (int i = threadIdx.x; i < nrec; i += HTHREADS) {
                    const int cell = (int)(((float)i + 0.5f) * rnv), c = i - cell * nv;          // i < 16 * 132: exact
                    const float d = rrun[i] - yrun[i];
                    gsm[cell * ld + j * nv + c] = c < nc ? d * fk[j * hch + cell] : fminf(fmaxf(d, -1.f), 1.f) * fp[j * hch + cell];
                }
            }
        }
    }
    __syncthreads();
    const int n4 = (k.ncell * ld) >> 2;
    T* out = static_cast<T*>(L.dbuf[k.map]) + ((size_t)k.b * hw + k.cell0) * ld;
    for (int i = threadIdx.x; i < n4; i += HTHREADS) st4t(out + 4 * i, *reinterpret_cast<const f32x4*>(gsm + 4 * i));
}

void multibox_focal_loss_grad(const HeadLayout& L, int B, int b_off, const float* result, const float* labels, const LossWork& w,
                              float gamma, float alpha, hipStream_t s, LocLoss loc) {
    const int total = B * L.A;
    const HeadGrid G = head_grid(L, B);
    const bool giou = loc.kind == LOC_GIOU;
    const size_t lds = ((size_t)G.hch * (G.ldp_max - 1) + (giou ? 6 : 2) * (size_t)HSLOTS * G.hch) * sizeof(float);
    const size_t o = (size_t)b_off * L.A;
    const int gm = focal_gmode(gamma);
    const dim3 grid(G.blk_off[MAX_MAPS]), block(HTHREADS);
    ProfScope prof("multibox_focal_loss_grad", 0.0, (L.grad_bf16 ? 10.0 : 12.0) * total * L.nvars, s);
#define SSD_FOCAL_GRAD(T, WIDE)                                                                                                      \
    hipLaunchKernelGGL((focal_grad_kernel<T, WIDE>), grid, block, lds, s, L, G, B, b_off, gamma, alpha, gm, result, labels, w.ce + o, \
                       w.pos + o, w.sample)
#define SSD_FOCAL_GRAD_GIOU(T, WIDE)                                                                                                  \
    hipLaunchKernelGGL((focal_grad_kernel<T, WIDE, LOC_GIOU, float>), grid, block, lds, s, L, G, B, b_off, gamma, alpha, gm, result, \
                       labels, w.ce + o, w.pos + o, w.sample, loc.weight)
    if (giou) {
        if (L.nvars <= MAXV) {
            if (L.grad_bf16) SSD_FOCAL_GRAD_GIOU(bf16_t, false);
            else SSD_FOCAL_GRAD_GIOU(float, false);
        } else {
            if (L.grad_bf16) SSD_FOCAL_GRAD_GIOU(bf16_t, true);
            else SSD_FOCAL_GRAD_GIOU(float, true);
        }
    } else if (L.nvars <= MAXV) {
        if (L.grad_bf16) SSD_FOCAL_GRAD(bf16_t, false);
        else SSD_FOCAL_GRAD(float, false);
    } else {
        if (L.grad_bf16) SSD_FOCAL_GRAD(bf16_t, true);
        else SSD_FOCAL_GRAD(float, true);
    }
#undef SSD_FOCAL_GRAD
#undef SSD_FOCAL_GRAD_GIOU
    HIP_OK(hipGetLastError());
}

// =================================================================================
// optimizer
// =================================================================================
__global__ __launch_bounds__(256) void momentum_kernel(float* __restrict__ w, float* __restrict__ acc,
                                                       const float* __restrict__ g, size_t n4, float lr, float mom,
                                                       float gscale) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 a = mom * ld4(acc + i * 4) + gscale * ld4(g + i * 4);
        st4(acc + i * 4, a);
        st4(w + i * 4, ld4(w + i * 4) - lr * a);
    }
}

void momentum_update(float* w, float* acc, const float* g, size_t n, float lr, float momentum, float gscale,
                     hipStream_t s) {
    SSD_REQUIRE(n % 4 == 0, "momentum: arena size must be a multiple of 4");
    ProfScope prof("momentum_update", 0.0, 20.0 * n, s);
    hipLaunchKernelGGL(momentum_kernel, dim3(grid_for(n / 4, 256, 256 * 16)), dim3(256), 0, s, w, acc, g, n / 4, lr,
                       momentum, gscale);
    HIP_OK(hipGetLastError());
}

// ---- the same update with the gradient clipped by its global norm (ops.h; contract in include/ssdvgg_hip.h)
// Head of the workspace: ClipState (ops.h), what the finish kernel leaves for the update; the per-block partials follow it.

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the block's sum, valid in thread 0: lanes by the xor butterfly, the four waves through LDS in wave order
__device__ __forceinline__ double block_sum_256(double v) {
    __shared__ double red[4];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One read of the arena, 16 bytes per lane and trip: a float's square is exact in fp64 (48 bits of product), so the only
// rounding is the additions', and four chains per thread keep the fp64 adds off each other's latency.
__global__ __launch_bounds__(GRAD_NORM_BLOCK) void grad_norm_kernel(const float* __restrict__ g, size_t n4, double* __restrict__ partial) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
#define SSD_SQ_ACC(v)                   \
    a0 += (double)v[0] * (double)v[0];  \
    a1 += (double)v[1] * (double)v[1];  \
    a2 += (double)v[2] * (double)v[2];  \
    a3 += (double)v[3] * (double)v[3];
    // GRAD_NORM_UNROLL loads in flight per lane (a wave alone would wait out HBM's latency on every trip); added in index order, so
    // the sums are those of the plain loop below
    for (; i + (GRAD_NORM_UNROLL - 1) * stride < n4; i += GRAD_NORM_UNROLL * stride) {
        f32x4 v[GRAD_NORM_UNROLL];
#pragma unroll
        for (int u = 0; u < GRAD_NORM_UNROLL; ++u) v[u] = ld4(g + (i + u * stride) * 4);
#pragma unroll
        for (int u = 0; u < GRAD_NORM_UNROLL; ++u) { SSD_SQ_ACC(v[u]) }
    }
    for (; i < n4; i += stride) {
        const f32x4 v = ld4(g + i * 4);
        SSD_SQ_ACC(v)
    }
#undef SSD_SQ_ACC
    const double s = block_sum_256((a0 + a1) + (a2 + a3));
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One block: thread t takes partials t, t + 256, ... in index order, then the block's tree.  norm = |grad_scale| * sqrt(S) and
// the factor in fp64, each rounded to float once.
__global__ __launch_bounds__(GRAD_NORM_BLOCK) void grad_norm_finish_kernel(const double* __restrict__ partial, int nparts, float gscale,
                                                                          float max_norm, ClipState* __restrict__ st,
                                                                          float* __restrict__ report) {
    double a = 0.0;
    for (int i = threadIdx.x; i < nparts; i += GRAD_NORM_BLOCK) a += partial[i];
    const double S = block_sum_256(a);
    if (threadIdx.x != 0) return;
    const double norm = fabs((double)gscale) * sqrt(S);
    const bool finite = __builtin_isfinite(S);
    float f = 0.f;
    if (finite) f = norm <= (double)max_norm ? 1.f : (float)((double)max_norm / norm);
    st->gscale = gscale * f;
    st->skip = finite ? 0u : 1u;
    if (report) {
        report[0] = (float)norm;
        report[1] = f;
    }
}

// momentum_kernel's body; the scale comes from the finish kernel (one scalar load per wave: the pointer is a kernel argument)
__global__ __launch_bounds__(256) void momentum_clipped_kernel(float* __restrict__ w, float* __restrict__ acc,
                                                               const float* __restrict__ g, size_t n4, float lr, float mom,
                                                               const ClipState* __restrict__ st) {
    if (st->skip) return;
    const float gscale = st->gscale;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 a = mom * ld4(acc + i * 4) + gscale * ld4(g + i * 4);
        st4(acc + i * 4, a);
        st4(w + i * 4, ld4(w + i * 4) - lr * a);
    }
}

static inline int grad_norm_grid(size_t n) { return grid_for(n / 4, GRAD_NORM_BLOCK, GRAD_NORM_GRID_CAP); }
size_t grad_norm_ws_bytes(size_t n) { return sizeof(ClipState) + (size_t)grad_norm_grid(n) * sizeof(double); }

void grad_norm_pass(const float* g, size_t n, float gscale, float max_norm, void* ws, float* report, hipStream_t s) {
    SSD_REQUIRE(max_norm > 0.f, "gradient clipping: max_norm %g is neither 0 (off), a number > 0 nor +inf", (double)max_norm);
    SSD_REQUIRE(n % 4 == 0, "momentum: arena size must be a multiple of 4");
    SSD_REQUIRE(ws != nullptr && (uintptr_t)ws % 16 == 0, "gradient clipping: the workspace must be 16-byte aligned");
    ClipState* st = static_cast<ClipState*>(ws);
    double* partial = reinterpret_cast<double*>(st + 1);
    const int grid = grad_norm_grid(n);
    ProfScope prof("grad_norm", 2.0 * n, 4.0 * n, s);
    hipLaunchKernelGGL(grad_norm_kernel, dim3(grid), dim3(GRAD_NORM_BLOCK), 0, s, g, n / 4, partial);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(GRAD_NORM_BLOCK), 0, s, (const double*)partial, grid, gscale, max_norm,
                       st, report);
}

void momentum_update_clipped(float* w, float* acc, const float* g, size_t n, float lr, float momentum, float gscale, float max_norm,
                             void* ws, float* report, hipStream_t s) {
    if (max_norm == 0.f) return momentum_update(w, acc, g, n, lr, momentum, gscale, s);
    grad_norm_pass(g, n, gscale, max_norm, ws, report, s);
    ProfScope prof("momentum_update_clipped", 0.0, 20.0 * n, s);
    hipLaunchKernelGGL(momentum_clipped_kernel, dim3(grid_for(n / 4, 256, 256 * 16)), dim3(256), 0, s, w, acc, g, n / 4, lr, momentum,
                       (const ClipState*)ws);
    HIP_OK(hipGetLastError());
}

// Gradient range <-> bf16 message buffer of the data-parallel all-reduce (parallel.py, allreduce_dtype = 'bf16'): the payload
// that crosses xGMI is halved; masters, momentum and the local gradient arena stay fp32.  Round-to-nearest-even like every other
// bf16 store of the library; n need not be a multiple of anything.
__global__ __launch_bounds__(256) void grads_to_bf16_kernel(const float* __restrict__ g, unsigned short* __restrict__ out, size_t n) {
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 v = ld4(g + i * 4);
        *reinterpret_cast<u32x2*>(out + i * 4) = u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])};
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) out[n4 * 4 + threadIdx.x] = f2bf(g[n4 * 4 + threadIdx.x]);
}
__global__ __launch_bounds__(256) void grads_from_bf16_kernel(const unsigned short* __restrict__ in, float* __restrict__ g, size_t n) {
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const u32x2 w = *reinterpret_cast<const u32x2*>(in + i * 4);
        st4(g + i * 4, f32x4{lo2f(w[0]), hi2f(w[0]), lo2f(w[1]), hi2f(w[1])});
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) g[n4 * 4 + threadIdx.x] = lo2f((unsigned)in[n4 * 4 + threadIdx.x]);
}
void grads_to_bf16(const float* g, void* out, size_t n, hipStream_t s) {
    SSD_REQUIRE(((uintptr_t)g % 16 == 0) && ((uintptr_t)out % 8 == 0), "gradient range / message buffer must be 16- / 8-byte aligned");
    if (n == 0) return;
    hipLaunchKernelGGL(grads_to_bf16_kernel, dim3(grid_for(n / 4 + 1, 256, 256 * 16)), dim3(256), 0, s, g, (unsigned short*)out, n);
    HIP_OK(hipGetLastError());
}
void grads_from_bf16(const void* in, float* g, size_t n, hipStream_t s) {
    SSD_REQUIRE(((uintptr_t)g % 16 == 0) && ((uintptr_t)in % 8 == 0), "gradient range / message buffer must be 16- / 8-byte aligned");
    if (n == 0) return;
    hipLaunchKernelGGL(grads_from_bf16_kernel, dim3(grid_for(n / 4 + 1, 256, 256 * 16)), dim3(256), 0, s, (const unsigned short*)in, g, n);
    HIP_OK(hipGetLastError());
}

// gradient arena of a step without samples: d(l2_loss)/dw = wd * w on the filters, zero elsewhere
__global__ __launch_bounds__(256) void null_grads_kernel(const float* __restrict__ w, float* __restrict__ g, size_t nf4, size_t n4,
                                                         float wd) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x)
        st4(g + i * 4, i < nf4 ? wd * ld4(w + i * 4) : f32x4{0.f, 0.f, 0.f, 0.f});
}

void null_gradients(const float* w, float* g, size_t nfilters, size_t n, float wd, hipStream_t s) {
    SSD_REQUIRE(n % 4 == 0 && nfilters % 4 == 0, "arena sizes must be multiples of 4");
    hipLaunchKernelGGL(null_grads_kernel, dim3(grid_for(n / 4, 256, 256 * 16)), dim3(256), 0, s, w, g, nfilters / 4, n / 4, wd);
    HIP_OK(hipGetLastError());
}

// Shader-clock monitor (measurement aid, tools/power_probe.py): ONE wave spins next to whatever else runs on the GPU and
// records, every `period` ticks of the constant 100 MHz counter (s_memrealtime), how many shader-clock cycles
// (s_memtime) went by: out[i] = cycles per period -> MHz = out[i] / period * 100.
__global__ void clock_monitor_kernel(unsigned* __restrict__ out, int nsamples, unsigned period) {
    if (threadIdx.x != 0) return;
    for (int i = 0; i < nsamples; ++i) {
        const unsigned long long w0 = wall_clock64();
        const unsigned long long c0 = clock64();
        unsigned long long w1;
        do {
            __builtin_amdgcn_s_sleep(32);
            w1 = wall_clock64();
        } while (w1 - w0 < period);
        const unsigned long long c1 = clock64();
        // normalise to exactly `period` wall ticks
        out[i] = (unsigned)((double)(c1 - c0) * (double)period / (double)(w1 - w0));
    }
}

void clock_monitor(unsigned* out, int nsamples, unsigned period, hipStream_t s) {
    hipLaunchKernelGGL(clock_monitor_kernel, dim3(1), dim3(64), 0, s, out, nsamples, period);
    HIP_OK(hipGetLastError());
}

void fill_zero(void* p, size_t bytes, hipStream_t s) { HIP_OK(hipMemsetAsync(p, 0, bytes, s)); }

}  // namespace ssd
