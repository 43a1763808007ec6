// Box math of the SSD hot path for gfx950.  Integer / index results are bit-exact with the
// reference's numpy code (ssdutils.py, transforms.py, utils.py geometry) as it runs under
// numpy >= 2: the mixed f32/f64 arithmetic of decode_location / normalize_box is spelled out
// with explicitly rounded operations.  This file is compiled with -ffp-contract=off.
#include "boxes.h"
#include <cmath>
#include <climits>
#include <vector>

namespace ssd {

typedef unsigned long long u64;

// =================================================================================
// presets (ssdutils.py:36-62) and box sizes (ssdutils.py:83-99) -- host
// =================================================================================
static Preset make_preset(const char* name, int img, int nmaps, const int* sizes, const double* scales, int last_two,
                          double extra, int A) {
    Preset p{};
    p.name = name; p.image_w = p.image_h = img; p.nmaps = nmaps; p.extra_scale = extra; p.num_anchors = A;
    for (int k = 0; k < nmaps; ++k) {
        p.map_size[k] = sizes[k];
        p.scale[k] = scales[k];
        const bool two = (k == 0) || (k >= nmaps - last_two);
        if (two) {
            p.nratios[k] = 2; p.ratios[k][0] = 2; p.ratios[k][1] = 0.5;
        } else {
            p.nratios[k] = 4; p.ratios[k][0] = 2; p.ratios[k][1] = 3; p.ratios[k][2] = 0.5; p.ratios[k][3] = 1. / 3.;
        }
    }
    int off = 0;
    for (int k = 0; k < nmaps; ++k) {
        const double s = p.scale[k];
        int t = 0;
        double r = std::sqrt(1.0);
        p.bw[k][t] = s * r; p.bh[k][t] = s / r; ++t;
        for (int q = 0; q < p.nratios[k]; ++q) {
            r = std::sqrt(p.ratios[k][q]);
            p.bw[k][t] = s * r; p.bh[k][t] = s / r; ++t;
        }
        const double nxt = k < nmaps - 1 ? p.scale[k + 1] : extra;
        const double sp = std::sqrt(s * nxt);
        p.bw[k][t] = sp; p.bh[k][t] = sp; ++t;
        p.ntypes[k] = t;
        p.off[k] = off;
        off += t * sizes[k] * sizes[k];
    }
    p.off[nmaps] = off;
    if (off != A) fail("preset %s: anchor count %d != %d", name, off, A);
    return p;
}

const Preset& get_preset(const char* name) {
    static const int s300[] = {38, 19, 10, 5, 3, 1};
    static const double c300[] = {0.1, 0.2, 0.375, 0.55, 0.725, 0.9};
    static const int s512[] = {64, 32, 16, 8, 4, 2, 1};
    static const double c512[] = {0.07, 0.15, 0.3, 0.45, 0.6, 0.75, 0.9};
    static const Preset p300 = make_preset("vgg300", 300, 6, s300, c300, 2, 1.075, 8732);
    static const Preset p512 = make_preset("vgg512", 512, 7, s512, c512, 2, 1.05, 24564);
    if (name && !strcmp(name, "vgg300")) return p300;
    if (name && !strcmp(name, "vgg512")) return p512;
    fail("No such preset: %s", name ? name : "(null)");
    return p300;
}

// =================================================================================
// anchors (ssdutils.py:104-130): order map -> type -> row -> col
// =================================================================================
struct AnchorArgs {
    int nmaps, A;
    int fk[PRESET_MAX_MAPS], off[PRESET_MAX_MAPS + 1];
    double bw[PRESET_MAX_MAPS][PRESET_MAX_TYPES], bh[PRESET_MAX_MAPS][PRESET_MAX_TYPES];
};

// utils.py:100-108 in f64: int() truncates toward zero
__device__ __forceinline__ void prop2abs_f64(double cx, double cy, double w, double h, int* o) {
    const double w2 = __ddiv_rn(__dmul_rn(w, 1000.0), 2.0);
    const double h2 = __ddiv_rn(__dmul_rn(h, 1000.0), 2.0);
    const double ax = __dmul_rn(cx, 1000.0), ay = __dmul_rn(cy, 1000.0);
    o[0] = (int)(long long)__dsub_rn(ax, w2);
    o[1] = (int)(long long)__dadd_rn(ax, w2);
    o[2] = (int)(long long)__dsub_rn(ay, h2);
    o[3] = (int)(long long)__dadd_rn(ay, h2);
}

__global__ void anchors_kernel(AnchorArgs p, double* __restrict__ anchors, int* __restrict__ aabs) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= p.A) return;
    int k = 0;
    for (int q = 1; q < p.nmaps; ++q)
        if (a >= p.off[q]) k = q;
    const int fk = p.fk[k];
    const int al = a - p.off[k];
    const int t = al / (fk * fk);
    const int cell = al - t * fk * fk;
    const int j = cell / fk, i = cell - j * fk;
    const double x = __ddiv_rn((double)i + 0.5, (double)fk);
    const double y = __ddiv_rn((double)j + 0.5, (double)fk);
    const double w = p.bw[k][t], h = p.bh[k][t];
    anchors[a * 4 + 0] = x; anchors[a * 4 + 1] = y; anchors[a * 4 + 2] = w; anchors[a * 4 + 3] = h;
    if (aabs) prop2abs_f64(x, y, w, h, aabs + a * 4);
}

void anchors_device(const Preset& p, double* anchors, int* anchors_abs, hipStream_t s) {
    AnchorArgs a{};
    a.nmaps = p.nmaps; a.A = p.num_anchors;
    for (int k = 0; k < p.nmaps; ++k) {
        a.fk[k] = p.map_size[k];
        a.off[k] = p.off[k];
        for (int t = 0; t < PRESET_MAX_TYPES; ++t) { a.bw[k][t] = p.bw[k][t]; a.bh[k][t] = p.bh[k][t]; }
    }
    a.off[p.nmaps] = p.off[p.nmaps];
    hipLaunchKernelGGL(anchors_kernel, dim3((a.A + 255) / 256), dim3(256), 0, s, a, anchors, anchors_abs);
    HIP_OK(hipGetLastError());
}

// =================================================================================
// label encoding (transforms.py:57-114).  IoU uses the +1 pixel convention on integer
// boxes (ssdutils.py:138-152); ratios are compared exactly by cross-multiplication.
// =================================================================================
__device__ __forceinline__ void iou_terms(const int* g, long long areab, const int* a, long long* inter, long long* uni) {
    const long long areaa = (long long)(a[1] - a[0] + 1) * (a[3] - a[2] + 1);
    const int w = max(0, min(g[1], a[1]) - max(g[0], a[0]) + 1);
    const int h = max(0, min(g[3], a[3]) - max(g[2], a[2]) + 1);
    *inter = (long long)w * h;
    *uni = areab + areaa - *inter;
}

// one workgroup per GT box: its best anchor (np.argmax: first maximum), ssdutils.py:159-165
__global__ __launch_bounds__(256) void gt_best_kernel(int A, const int* __restrict__ aabs, const double* __restrict__ gt,
                                                      int ntot, int* __restrict__ gabs, int* __restrict__ best_a,
                                                      int* __restrict__ best_i, int* __restrict__ best_u) {
    __shared__ long long s_i[256], s_u[256];
    __shared__ int s_a[256];
    __shared__ int gb[4];
    const int g = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        prop2abs_f64(gt[g * 4 + 0], gt[g * 4 + 1], gt[g * 4 + 2], gt[g * 4 + 3], gb);
        for (int e = 0; e < 4; ++e) gabs[g * 4 + e] = gb[e];
    }
    __syncthreads();
    const int box[4] = {gb[0], gb[1], gb[2], gb[3]};
    const long long areab = (long long)(box[1] - box[0] + 1) * (box[3] - box[2] + 1);
    long long bi = -1, bu = 1;
    int ba = INT_MAX;
    for (int a = tid; a < A; a += 256) {
        long long in, un;
        iou_terms(box, areab, aabs + a * 4, &in, &un);
        if (in * bu > bi * un) { bi = in; bu = un; ba = a; }     // strict: the earlier index keeps a tie
    }
    s_i[tid] = bi; s_u[tid] = bu; s_a[tid] = ba;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            const long long i2 = s_i[tid + st], u2 = s_u[tid + st];
            const int a2 = s_a[tid + st];
            const long long l = i2 * s_u[tid], r = s_i[tid] * u2;
            if (l > r || (l == r && a2 < s_a[tid])) { s_i[tid] = i2; s_u[tid] = u2; s_a[tid] = a2; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool ok = 2 * s_i[0] > s_u[0];                      // iou > 0.5
        best_a[g] = ok ? s_a[0] : -1;
        best_i[g] = (int)s_i[0];
        best_u[g] = (int)s_u[0];
    }
}

// one thread per (image, anchor): the winning GT box (pass 1: every 'good' overlap, higher IoU
// wins, earlier box keeps a tie; pass 2: 'best' matches override, same rule among them) and
// the encoded row (ssdutils.py:173-179, transforms.py:47-55).  match_out (may be null): the winner's index within its image, -1: none.
// Behind match_bipartite_kernel (match = paper) best_a holds at most one box per anchor: pass 1 is the per-anchor stage, pass 2
// keeps the bipartite matches on top.
__global__ __launch_bounds__(256) void label_rows_kernel(int A, int C, int B, const double* __restrict__ anchors,
                                                         const int* __restrict__ aabs, const double* __restrict__ gt,
                                                         const int* __restrict__ cls, const int* __restrict__ offsets,
                                                         const int* __restrict__ gabs, const int* __restrict__ best_a,
                                                         float* __restrict__ vec, int* __restrict__ match_out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * A) return;
    const int b = idx / A, a = idx - b * A;
    const int an[4] = {aabs[a * 4], aabs[a * 4 + 1], aabs[a * 4 + 2], aabs[a * 4 + 3]};
    int w1 = -1, w2 = -1;
    long long i1 = 0, u1 = 1, i2 = 0, u2 = 1;
    for (int g = offsets[b]; g < offsets[b + 1]; ++g) {
        const int box[4] = {gabs[g * 4], gabs[g * 4 + 1], gabs[g * 4 + 2], gabs[g * 4 + 3]};
        const long long areab = (long long)(box[1] - box[0] + 1) * (box[3] - box[2] + 1);
        long long in, un;
        iou_terms(box, areab, an, &in, &un);
        if (2 * in > un) {
            if (w1 < 0 || in * u1 > i1 * un) { w1 = g; i1 = in; u1 = un; }
        }
        if (best_a[g] == a) {
            if (w2 < 0 || in * u2 > i2 * un) { w2 = g; i2 = in; u2 = un; }
        }
    }
    const int win = w2 >= 0 ? w2 : w1;
    if (match_out) match_out[idx] = win >= 0 ? win - offsets[b] : -1;      // the box's index within its image
    float* row = vec + (size_t)idx * (C + 5);
    for (int c = 0; c < C + 5; ++c) row[c] = 0.f;
    if (win < 0) {
        row[C] = 1.f;
        return;
    }
    row[cls[win]] = 1.f;
    const double acx = anchors[a * 4], acy = anchors[a * 4 + 1], aw = anchors[a * 4 + 2], ah = anchors[a * 4 + 3];
    const double bcx = gt[win * 4], bcy = gt[win * 4 + 1], bw = gt[win * 4 + 2], bh = gt[win * 4 + 3];
    row[C + 1] = (float)__dmul_rn(__ddiv_rn(__dsub_rn(bcx, acx), aw), 10.0);
    row[C + 2] = (float)__dmul_rn(__ddiv_rn(__dsub_rn(bcy, acy), ah), 10.0);
    row[C + 3] = (float)__dmul_rn(log(__ddiv_rn(bw, aw)), 5.0);
    row[C + 4] = (float)__dmul_rn(log(__ddiv_rn(bh, ah)), 5.0);
}

// jaccard_overlap (ssdutils.py:138-152) of one box against n boxes, all (xmin, xmax, ymin, ymax) f64
__global__ void jaccard_kernel(const double* __restrict__ box, const double* __restrict__ arr, int n, double* __restrict__ iou) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double b0 = box[0], b1 = box[1], b2 = box[2], b3 = box[3];
    const double a0 = arr[i * 4], a1 = arr[i * 4 + 1], a2 = arr[i * 4 + 2], a3 = arr[i * 4 + 3];
    const double areaa = __dmul_rn(__dadd_rn(__dsub_rn(a1, a0), 1.0), __dadd_rn(__dsub_rn(a3, a2), 1.0));
    const double areab = __dmul_rn(__dadd_rn(__dsub_rn(b1, b0), 1.0), __dadd_rn(__dsub_rn(b3, b2), 1.0));
    const double w = fmax(0.0, __dadd_rn(__dsub_rn(fmin(b1, a1), fmax(b0, a0)), 1.0));
    const double h = fmax(0.0, __dadd_rn(__dsub_rn(fmin(b3, a3), fmax(b2, a2)), 1.0));
    const double inter = __dmul_rn(w, h);
    iou[i] = __ddiv_rn(inter, __dsub_rn(__dadd_rn(areab, areaa), inter));
}

void jaccard_device(const double* box, const double* arr, int n, double* iou, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(jaccard_kernel, dim3((n + 255) / 256), dim3(256), 0, s, box, arr, n, iou);
    HIP_OK(hipGetLastError());
}

// ---------------------------------------------------------------------------------
// match = paper: the bipartite stage of the SSD paper's matching.  Greedy and one-to-one: among all pairs
// (box not yet matched, anchor not yet taken) that intersect, the pair of greatest IoU is matched, exact ties going to
// the lower anchor and then to the lower box; repeated until every box is matched or no pair is left.
// One workgroup per image.  Every live box caches its best free anchor (greatest IoU, lowest anchor on a tie): the
// pair to match is then the best of the cached ones under (IoU, lower anchor, lower box), and a box looks at the A
// anchors again only when the anchor it cached has been taken.  A rescan is one wave's work (the 16 waves rescan 16
// boxes side by side); box j of a chunk of 1024 belongs to lane j / 16 of wave j % 16, so neighbouring boxes -- the
// ones that compete for the same anchors -- spread over the waves.  The first MATCH_LDS_BOXES boxes of the image keep
// their state in LDS, the rest in the workspace: no limit on the boxes of an image.  The taken anchors are a bitmap
// in LDS.  No atomics; the result does not depend on any execution order.
// It leaves gabs and best_a (the anchor a box won, -1: none) as gt_best_kernel does: label_rows_kernel's pass 1 is the
// per-anchor stage, and its pass 2 -- now at most one box per anchor -- keeps the bipartite matches on top.
constexpr int MATCH_THREADS = 1024;
constexpr int MATCH_WAVES = MATCH_THREADS / 64;
constexpr int MATCH_LDS_BOXES = 32;
constexpr int MATCH_MAX_ANCHORS = 24576;      // bitmap capacity (vgg512: 24564)
constexpr int MATCH_BATCH = 8;                // anchor rows a lane has in flight during a rescan
constexpr int MATCH_STALE = -2, MATCH_NONE = -1;

// is (i1 / u1, a1, g1) ahead of (i2 / u2, a2, g2): greater IoU, then lower anchor, then lower box
__device__ __forceinline__ bool match_ahead(long long i1, long long u1, int a1, int g1, long long i2, long long u2, int a2, int g2) {
    const long long l = i1 * u2, r = i2 * u1;
    return l > r || (l == r && (a1 < a2 || (a1 == a2 && g1 < g2)));
}

__global__ __launch_bounds__(MATCH_THREADS) void match_bipartite_kernel(int A, const int* __restrict__ aabs, const double* __restrict__ gt,
                                                                        const int* __restrict__ offsets, int* __restrict__ gabs,
                                                                        int* best_a, int* c_in, int* c_un, int* c_a) {
    __shared__ unsigned taken[MATCH_MAX_ANCHORS / 32];
    __shared__ int l_box[MATCH_LDS_BOXES][4], l_in[MATCH_LDS_BOXES], l_un[MATCH_LDS_BOXES], l_a[MATCH_LDS_BOXES], l_best[MATCH_LDS_BOXES];
    __shared__ long long r_i[MATCH_WAVES], r_u[MATCH_WAVES];
    __shared__ int r_a[MATCH_WAVES], r_g[MATCH_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g0 = offsets[blockIdx.x], n = offsets[blockIdx.x + 1] - g0;
    if (n <= 0) return;                                  // workgroup uniform
    for (int i = tid; i < MATCH_MAX_ANCHORS / 32; i += MATCH_THREADS) taken[i] = 0u;
    for (int j = tid; j < n; j += MATCH_THREADS) {
        const int g = g0 + j;
        int o[4];
        prop2abs_f64(gt[g * 4 + 0], gt[g * 4 + 1], gt[g * 4 + 2], gt[g * 4 + 3], o);
        for (int e = 0; e < 4; ++e) gabs[g * 4 + e] = o[e];
        best_a[g] = -1;
        if (j < MATCH_LDS_BOXES) {
            for (int e = 0; e < 4; ++e) l_box[j][e] = o[e];
            l_best[j] = -1; l_a[j] = MATCH_STALE;
        } else {
            c_a[g] = MATCH_STALE;
        }
    }
    __syncthreads();
    const int nchunk = (n + MATCH_THREADS - 1) / MATCH_THREADS;
    for (int round = 0; round < n; ++round) {
        long long bi = -1, bu = 1;                       // this thread's best cached pair; (-1, 1): none, behind every real one
        int ba = INT_MAX, bg = INT_MAX;
        for (int c = 0; c < nchunk; ++c) {
            const int j = c * MATCH_THREADS + lane * MATCH_WAVES + wave;
            const bool lds = j < MATCH_LDS_BOXES;
            bool live = false;
            int ca = MATCH_NONE, ci = 0, cu = 1;
            if (j < n) {
                live = (lds ? l_best[j] : best_a[g0 + j]) < 0;
                if (live) {
                    ca = lds ? l_a[j] : c_a[g0 + j];
                    if (ca >= 0) { ci = lds ? l_in[j] : c_in[g0 + j]; cu = lds ? l_un[j] : c_un[g0 + j]; }
                }
            }
            const bool stale = live && (ca == MATCH_STALE || (ca >= 0 && ((taken[ca >> 5] >> (ca & 31)) & 1u)));
            u64 todo = __ballot(stale);
            while (todo) {                               // wave uniform: one rescan per stale box of this wave
                const int l = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int jj = c * MATCH_THREADS + l * MATCH_WAVES + wave;
                int box[4];
                for (int e = 0; e < 4; ++e) box[e] = jj < MATCH_LDS_BOXES ? l_box[jj][e] : gabs[(g0 + jj) * 4 + e];
                const long long areab = (long long)(box[1] - box[0] + 1) * (box[3] - box[2] + 1);
                long long si = 0, su = 1;                // (0, 1): only an anchor with a positive intersection gets ahead
                int sa = INT_MAX;
                // MATCH_BATCH rows of the table (L2) are in flight before the first is used (index clamped, not predicated);
                // iou_terms' 64-bit products only for the anchors that touch the box.  What is left is instruction issue:
                // A / 64 passes of ~40 instructions, ~2.3 us of the CU per rescan for vgg300 (profiles/label_match_rate.txt).
                for (int a0 = lane; a0 < A; a0 += 64 * MATCH_BATCH) {
                    int4 an[MATCH_BATCH];
#pragma unroll
                    for (int k = 0; k < MATCH_BATCH; ++k)      // (tables come from hipMalloc: 16-byte aligned)
                        an[k] = *reinterpret_cast<const int4*>(aabs + (size_t)min(a0 + 64 * k, A - 1) * 4);
#pragma unroll
                    for (int k = 0; k < MATCH_BATCH; ++k) {
                        const int a = a0 + 64 * k;
                        const int w = min(box[1], an[k].y) - max(box[0], an[k].x) + 1;
                        const int h = min(box[3], an[k].w) - max(box[2], an[k].z) + 1;
                        if (a < A && w > 0 && h > 0 && !((taken[a >> 5] >> (a & 31)) & 1u)) {
                            const long long in = (long long)w * h;
                            const long long un = areab + (long long)(an[k].y - an[k].x + 1) * (an[k].w - an[k].z + 1) - in;
                            if (in * su > si * un) { si = in; su = un; sa = a; }         // strict: the lower anchor keeps a tie
                        }
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const long long oi = __shfl_xor(si, o, 64), ou = __shfl_xor(su, o, 64);
                    const int oa = __shfl_xor(sa, o, 64);
                    if (match_ahead(oi, ou, oa, 0, si, su, sa, 0)) { si = oi; su = ou; sa = oa; }
                }
                if (lane == l) { ca = sa == INT_MAX ? MATCH_NONE : sa; ci = (int)si; cu = (int)su; }
            }
            if (stale) {
                if (lds) { l_a[j] = ca; l_in[j] = ci; l_un[j] = cu; }
                else { c_a[g0 + j] = ca; c_in[g0 + j] = ci; c_un[g0 + j] = cu; }
            }
            if (live && ca >= 0 && match_ahead(ci, cu, ca, j, bi, bu, ba, bg)) { bi = ci; bu = cu; ba = ca; bg = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long oi = __shfl_xor(bi, o, 64), ou = __shfl_xor(bu, o, 64);
            const int oa = __shfl_xor(ba, o, 64), og = __shfl_xor(bg, o, 64);
            if (match_ahead(oi, ou, oa, og, bi, bu, ba, bg)) { bi = oi; bu = ou; ba = oa; bg = og; }
        }
        if (lane == 0) { r_i[wave] = bi; r_u[wave] = bu; r_a[wave] = ba; r_g[wave] = bg; }
        __syncthreads();
        bi = r_i[0]; bu = r_u[0]; ba = r_a[0]; bg = r_g[0];
        for (int w = 1; w < MATCH_WAVES; ++w)
            if (match_ahead(r_i[w], r_u[w], r_a[w], r_g[w], bi, bu, ba, bg)) { bi = r_i[w]; bu = r_u[w]; ba = r_a[w]; bg = r_g[w]; }
        if (ba == INT_MAX) break;                        // workgroup uniform: no pair with a positive intersection is left
        if (tid == 0) {
            taken[ba >> 5] |= 1u << (ba & 31);
            best_a[g0 + bg] = ba;
            if (bg < MATCH_LDS_BOXES) l_best[bg] = ba;
        }
        __syncthreads();                                 // also: every thread has read r_* before the next round writes them
    }
}

size_t encode_labels_ws_bytes(int ntot) { return (size_t)(ntot > 0 ? ntot : 1) * 7 * sizeof(int) + 64; }

void encode_labels(const Preset& p, int num_classes, const double* anchors, const int* anchors_abs, const double* gt,
                   const int* cls, const int* offsets, int B, int ntot, float* vec, void* ws, hipStream_t s) {
    encode_labels_ex(p, num_classes, anchors, anchors_abs, gt, cls, offsets, B, ntot, vec, nullptr, MATCH_REFERENCE, ws, s);
}

void require_match(int match) {
    if (match != MATCH_REFERENCE && match != MATCH_PAPER) fail("match must be 0 (reference) or 1 (paper), got %d", match);
}

size_t encode_labels_ws_bytes_ex(int ntot, int B, int match) {
    require_match(match);
    (void)B;                                             // the bipartite stage keeps nothing per image outside LDS
    return (size_t)(ntot > 0 ? ntot : 1) * (match == MATCH_PAPER ? 8 : 7) * sizeof(int) + 64;
}

void encode_labels_ex(const Preset& p, int num_classes, const double* anchors, const int* anchors_abs, const double* gt,
                      const int* cls, const int* offsets, int B, int ntot, float* vec, int* match_out, int match, void* ws,
                      hipStream_t s) {
    require_match(match);
    const size_t nt = ntot > 0 ? ntot : 1;
    int* gabs = (int*)ws;
    int* best_a = gabs + nt * 4;
    int* best_i = best_a + nt;
    int* best_u = best_i + nt;
    const int A = p.num_anchors;
    if (match == MATCH_PAPER) {
        if (A > MATCH_MAX_ANCHORS) fail("match = paper: %d anchors exceed the kernel's bitmap of %d", A, MATCH_MAX_ANCHORS);
        if (ntot > 0)
            hipLaunchKernelGGL(match_bipartite_kernel, dim3(B), dim3(MATCH_THREADS), 0, s, A, anchors_abs, gt, offsets, gabs, best_a,
                               best_i, best_u, best_u + nt);
    } else if (ntot > 0) {
        hipLaunchKernelGGL(gt_best_kernel, dim3(ntot), dim3(256), 0, s, A, anchors_abs, gt, ntot, gabs, best_a, best_i, best_u);
    }
    hipLaunchKernelGGL(label_rows_kernel, dim3((B * A + 255) / 256), dim3(256), 0, s, A, num_classes, B, anchors, anchors_abs,
                       gt, cls, offsets, gabs, best_a, vec, match_out);
    HIP_OK(hipGetLastError());
}

// =================================================================================
// decode (ssdutils.py:192-229) + per-class greedy NMS (ssdutils.py:232-318)
// =================================================================================
// Pass 1, HBM-bound: every anchor row [C+5] f32 is read exactly once through LDS (coalesced
// float4 loads, all issued before the first is consumed; rows are then read at an odd stride:
// conflict-free).  Every anchor whose confidence reaches thr becomes one 64-bit sort key
//   conf bits << 32 | (32767 - anchor) << 8 | 0x80 | class   (descending sort == conf desc, anchor asc)
// (class in bits 0-6: up to MAX_CLASSES = 127 classes; below the per-image unique anchor bits, so it never orders keys)
// A workgroup compacts the keys of its 256 rows in place: ballot prefix per wave, wave totals through LDS,
// the survivors stored from the first row of the segment on, their number in `bcount`.  A workgroup's rows
// belong to at most two images (A >= 256): two segments, the second one starting at the image boundary.
// No atomics (a per-image counter serialises in L2: 137 waves hit each address), no memset, deterministic.
constexpr int SCAN_ROWS = 256;
constexpr int SCAN_MAXV = 32;                       // nv <= 32
constexpr int SCAN_LOADS = SCAN_ROWS * SCAN_MAXV / 4 / 256;   // float4 per thread, worst case

// One scan block = SCAN_ROWS rows, worked by the 256 threads t = 0..255 of a (half) workgroup; `rows` and `s_cnt` are that
// half's LDS.  blk past the last block: nothing to do, but every barrier is still passed.
__device__ __forceinline__ void detect_scan_block(const int blk, const int t, float* __restrict__ rows, int (*s_cnt)[4], int A, int nv,
                                                  int B, const float* __restrict__ pred, float thr, u64* __restrict__ dense,
                                                  int* __restrict__ bcount) {
    const int total_rows = B * A;
    const int r0 = blk * SCAN_ROWS;
    const int nrows = max(0, min(SCAN_ROWS, total_rows - r0));
    const int nfl = nrows * nv;
    const float* src = pred + (size_t)r0 * nv;           // r0*nv*4 bytes: 256*nv*4*block -> 16-byte aligned
    const int n4 = nfl >> 2;
    // all of this thread's loads are issued before the first one is consumed
    float4 v[SCAN_LOADS];
#pragma unroll
    for (int j = 0; j < SCAN_LOADS; ++j) {
        const int i = t + 256 * j;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < n4) v[j] = *reinterpret_cast<const float4*>(src + (size_t)i * 4);
    }
#pragma unroll
    for (int j = 0; j < SCAN_LOADS; ++j) {
        const int i = t + 256 * j;
        if (i < n4) *reinterpret_cast<float4*>(rows + (size_t)i * 4) = v[j];
    }
    for (int i = (n4 << 2) + t; i < nfl; i += 256) rows[i] = src[i];
    __syncthreads();
    const int lane = t & 63, wv = t >> 6;
    const int img_first = r0 / A;
    const int boundary = (img_first + 1) * A;            // first row of the next image (may lie beyond this workgroup)
    u64 key = 0ull;
    int half = 0;
    if ((int)t < nrows) {
        const float* r = rows + (size_t)t * nv;
        const int nfg = nv - 5;                  // argmax excludes the background class
        int best = 0;
        float conf = r[0];
        for (int c = 1; c < nfg; ++c)
            if (r[c] > conf) { conf = r[c]; best = c; }     // first maximum wins (np.argmax)
        const int row = r0 + t;
        half = row >= boundary ? 1 : 0;
        const int a = row - (img_first + half) * A;
        if (!(conf < thr))                        // the reference breaks at the first conf < thr
            key = ((u64)__float_as_uint(conf) << 32) | ((u64)(32767 - a) << 8) | (u64)best | (1ull << 7);
    }
    const u64 bal0 = __ballot(key != 0ull && half == 0), bal1 = __ballot(key != 0ull && half == 1);
    if (lane == 0) { s_cnt[0][wv] = __popcll(bal0); s_cnt[1][wv] = __popcll(bal1); }
    __syncthreads();
    int base = 0, tot0 = 0, tot1 = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wv) base += s_cnt[half][w];
        tot0 += s_cnt[0][w]; tot1 += s_cnt[1][w];
    }
    if (key != 0ull) {
        const u64 bal = half ? bal1 : bal0;
        __hip_atomic_store(dense + (size_t)(half ? boundary : r0) + base + __popcll(bal & ((1ull << lane) - 1ull)), key, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    if (t == 0 && nrows > 0) {
        __hip_atomic_store(bcount + blk * 2, tot0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(bcount + blk * 2 + 1, tot1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this lane's stores have left before the workgroup's barrier
}

__global__ __launch_bounds__(256) void detect_scan_kernel(int A, int nv, int B, const float* __restrict__ pred, float thr,
                                                          u64* __restrict__ dense, int* __restrict__ bcount) {
    extern __shared__ __attribute__((aligned(16))) float rows[];
    __shared__ int s_cnt[2][4];
    detect_scan_block(blockIdx.x, threadIdx.x, rows, s_cnt, A, nv, B, pred, thr, dense, bcount);
}

// The same pass for rows of more than SCAN_MAXV values (28..127 classes), where SCAN_ROWS rows would need up to 135 KB of
// LDS: the workgroup's SCAN_ROWS rows go through LDS in SCANW_CHUNKS chunks of SCANW_ROWS, the next chunk's float4 loads in
// flight while the current one is ranked, 4 lanes per row.  Each lane takes the first maximum of every 4th class, the 4
// lanes then keep the larger value, on ties the lower class: the first maximum of the row (a NaN in class 0 wins, as
// in detect_scan_block).  The dense keys and the per-segment counts are those of detect_scan_kernel (a segment's keys
// in another order, which the per-image sort does not see).
constexpr int SCANW_ROWS = 64;
constexpr int SCANW_CHUNKS = SCAN_ROWS / SCANW_ROWS;
constexpr int SCANW_MAXV = MAX_CLASSES + 5;
constexpr int SCANW_LOADS = (SCANW_ROWS * SCANW_MAXV / 4 + 255) / 256;      // float4 per thread and chunk, worst case

__global__ __launch_bounds__(256) void detect_scan_wide_kernel(int A, int nv, int B, const float* __restrict__ pred, float thr,
                                                               u64* __restrict__ dense, int* __restrict__ bcount) {
    extern __shared__ __attribute__((aligned(16))) float rows[];      // [SCANW_ROWS][nv]
    __shared__ int s_cnt[2][4];
    const int t = threadIdx.x, blk = blockIdx.x;
    const int r0 = blk * SCAN_ROWS;
    const int nrows = max(0, min(SCAN_ROWS, B * A - r0));
    const int lane = t & 63, wv = t >> 6, sub = t & 3, rl = t >> 2;
    const int img_first = r0 / A;
    const int boundary = (img_first + 1) * A;
    const int nfg = nv - 5;
    float4 v[SCANW_LOADS];
    auto issue = [&](int q) {             // chunk q's rows start at (r0 + 64 q) * nv floats: 16-byte aligned
        const int n4 = (max(0, min(SCANW_ROWS, nrows - q * SCANW_ROWS)) * nv) >> 2;
        const float* src = pred + (size_t)(r0 + q * SCANW_ROWS) * nv;
#pragma unroll
        for (int j = 0; j < SCANW_LOADS; ++j) {
            const int i = t + 256 * j;
            v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < n4) v[j] = *reinterpret_cast<const float4*>(src + (size_t)i * 4);
        }
    };
    issue(0);
    int tot0 = 0, tot1 = 0;               // keys stored so far per segment (workgroup uniform)
    for (int q = 0; q < SCANW_CHUNKS; ++q) {
        const int c0 = q * SCANW_ROWS;
        const int nr = max(0, min(SCANW_ROWS, nrows - c0));
        const int nfl = nr * nv, n4 = nfl >> 2;
        const float* src = pred + (size_t)(r0 + c0) * nv;
#pragma unroll
        for (int j = 0; j < SCANW_LOADS; ++j) {
            const int i = t + 256 * j;
            if (i < n4) *reinterpret_cast<float4*>(rows + (size_t)i * 4) = v[j];
        }
        for (int i = (n4 << 2) + t; i < nfl; i += 256) rows[i] = src[i];
        __syncthreads();
        if (q + 1 < SCANW_CHUNKS) issue(q + 1);
        u64 key = 0ull;
        int half = 0;
        if (rl < nr) {                    // uniform over the row's 4 lanes
            const float* r = rows + (size_t)rl * nv;
            float conf = -__builtin_inff();
            int best = sub;
            for (int c = sub; c < nfg; c += 4)
                if (r[c] > conf) { conf = r[c]; best = c; }
#pragma unroll
            for (int o = 1; o <= 2; o <<= 1) {
                const float oc = __shfl_xor(conf, o, 64);
                const int ob = __shfl_xor(best, o, 64);
                if (oc > conf || (oc == conf && ob < best)) { conf = oc; best = ob; }
            }
            if (r[0] != r[0]) { conf = r[0]; best = 0; }
            const int row = r0 + c0 + rl;
            half = row >= boundary ? 1 : 0;
            const int a = row - (img_first + half) * A;
            if (sub == 0 && !(conf < thr))
                key = ((u64)__float_as_uint(conf) << 32) | ((u64)(32767 - a) << 8) | (u64)best | (1ull << 7);
        }
        const u64 bal0 = __ballot(key != 0ull && half == 0), bal1 = __ballot(key != 0ull && half == 1);
        if (lane == 0) { s_cnt[0][wv] = __popcll(bal0); s_cnt[1][wv] = __popcll(bal1); }
        __syncthreads();
        int base = half ? tot1 : tot0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wv) base += s_cnt[half][w];
        }
        if (key != 0ull) {
            const u64 bal = half ? bal1 : bal0;
            __hip_atomic_store(dense + (size_t)(half ? boundary : r0) + base + __popcll(bal & ((1ull << lane) - 1ull)), key, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) { tot0 += s_cnt[0][w]; tot1 += s_cnt[1][w]; }
        __syncthreads();                  // rows and s_cnt are rewritten by the next chunk
    }
    if (t == 0 && nrows > 0) {
        __hip_atomic_store(bcount + blk * 2, tot0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(bcount + blk * 2 + 1, tot1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}


// descending bitonic sort of n2 (power of two) keys by one workgroup; keys may live in LDS or global
__device__ void bitonic_desc(u64* keys, int n2) {
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const u64 a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if (up ? (a < b) : (a > b)) { keys[i] = b; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// decode_location under numpy>=2 promotion (x, y float32; w, h float64) followed by
// normalize_box's integer box (utils.py:118-135; centre*1000 in f32, half extent cast to f32).
__device__ __forceinline__ void decode_box(const float* loc, const double* an, int* o) {
    float l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) l[e] = loc[e] > 100.f ? 100.f : loc[e];      // ssdutils.py:183
    const double acx = an[0], acy = an[1], aw = an[2], ah = an[3];
    const float x = __fadd_rn(__fmul_rn(__fdiv_rn(l[0], 10.f), (float)aw), (float)acx);
    const float y = __fadd_rn(__fmul_rn(__fdiv_rn(l[1], 10.f), (float)ah), (float)acy);
    const double w = __dmul_rn(exp((double)__fdiv_rn(l[2], 5.f)), aw);
    const double h = __dmul_rn(exp((double)__fdiv_rn(l[3], 5.f)), ah);
    if (!(isfinite(x) && isfinite(y) && isfinite(w) && isfinite(h))) {
        // the reference passes such a box through un-normalised and then fails in NMS's int();
        // here it becomes an empty corner box
        o[0] = o[1] = o[2] = o[3] = 0;
        return;
    }
    const float w2 = (float)__ddiv_rn(__dmul_rn(w, 1000.0), 2.0);
    const float h2 = (float)__ddiv_rn(__dmul_rn(h, 1000.0), 2.0);
    const float cx = __fmul_rn(x, 1000.f), cy = __fmul_rn(y, 1000.f);
    const float fx0 = __fsub_rn(cx, w2), fx1 = __fadd_rn(cx, w2), fy0 = __fsub_rn(cy, h2), fy1 = __fadd_rn(cy, h2);
    const float big = 9.0e18f;
    long long xmin = (long long)fminf(fmaxf(fx0, -big), big), xmax = (long long)fminf(fmaxf(fx1, -big), big);
    long long ymin = (long long)fminf(fmaxf(fy0, -big), big), ymax = (long long)fminf(fmaxf(fy1, -big), big);
    xmin = xmin > 0 ? xmin : 0; xmax = xmax < 999 ? xmax : 999;
    ymin = ymin > 0 ? ymin : 0; ymax = ymax < 999 ? ymax : 999;
    xmin = xmin < xmax ? xmin : xmax;
    ymin = ymin < ymax ? ymin : ymax;
    const long long lo = -(1LL << 30);
    o[0] = (int)(xmin > lo ? xmin : lo); o[1] = (int)(xmax > lo ? xmax : lo);
    o[2] = (int)(ymin > lo ? ymin : lo); o[3] = (int)(ymax > lo ? ymax : lo);
}

// prop2abs(abs2prop(ints)) as non_maximum_suppression recomputes it (not the identity)
__device__ __forceinline__ void nms_roundtrip(const int* b, int* o) {
    const double width = (double)(b[1] - b[0]), height = (double)(b[3] - b[2]);
    const double cx = __ddiv_rn(__dadd_rn((double)b[0], __ddiv_rn(width, 2.0)), 1000.0);
    const double cy = __ddiv_rn(__dadd_rn((double)b[2], __ddiv_rn(height, 2.0)), 1000.0);
    prop2abs_f64(cx, cy, __ddiv_rn(width, 1000.0), __ddiv_rn(height, 1000.0), o);
}

// IoU(+1) > 0.45 without a division: 20*inter > 9*union (exact for the integer areas of the 1000 grid)
__device__ __forceinline__ bool overlaps45(int x0, int x1, int y0, int y1, int area_i, int4 bj) {
    const int w = max(0, min(x1, bj.y) - max(x0, bj.x) + 1);
    const int h = max(0, min(y1, bj.w) - max(y0, bj.z) + 1);
    const int inter = w * h;
    const int uni = area_i + (bj.y - bj.x + 1) * (bj.w - bj.z + 1) - inter;
    return 20 * inter > 9 * uni;
}

// Greedy NMS of one class segment (boxes in descending confidence) by one wave.  Segments of up to 64 boxes
// live in registers: lane j holds box j, the pivot is broadcast with v_readlane, the survivors are a 64-bit
// mask; no memory traffic in the loop.  Longer segments walk the boxes in LDS / global.
// `al` is a plain LDS pointer on purpose: a `volatile` one degrades to a generic pointer whose byte stores compile to
// `flat_store_byte ... sc0 sc1` + `s_waitcnt vmcnt(0)` -- a system-scope store that took ~2 us EACH (three per wave here:
// 6.3 of this kernel's 13.7 us at batch 128, SSD_DETECT_STAMPS=1); only the long-segment walk below, where lanes read flags
// other lanes have just cleared, goes through a volatile alias.
__device__ __forceinline__ void nms_segment(const int4* nbox, unsigned char* al_plain, int s0, int len, int lane) {
    // The segment bounds come out of LDS, i.e. in vector registers: left there, the compiler treats the pivot loop as
    // divergent (exec-mask bookkeeping, 64-bit vector shifts for the survivor mask, a v_readfirstlane per v_readlane) --
    // ~420 cycles per pivot, 7.8 us of the 23 us this kernel took at batch 128 (phase clocks of workgroup 0, a measurement aid of round 3).  They are wave
    // uniform, so say so: the loop counter, the survivor mask and the pivot's coordinates then live in scalar registers.
    s0 = __builtin_amdgcn_readfirstlane(s0);
    len = __builtin_amdgcn_readfirstlane(len);
    if (len <= 64) {
        int4 me = make_int4(0, 0, 0, 0);
        if (lane < len) me = nbox[s0 + lane];
        // Phase A, no dependence between iterations, no branch: lane j collects the set of EARLIER boxes that overlap it
        // (bit i of lo / hi).  The greedy walk "pivot i suppresses what it overlaps, if it is still alive itself" spent
        // ~340 cycles per pivot on its serial chain (survivor mask -> branch -> 4 v_readlane -> compare -> ballot -> mask).
        unsigned lo = 0u, hi = 0u;
        const int n_lo = len < 32 ? len : 32;
        for (int i = 0; i < n_lo; ++i) {
            const int x0 = __builtin_amdgcn_readlane(me.x, i), x1 = __builtin_amdgcn_readlane(me.y, i);
            const int y0 = __builtin_amdgcn_readlane(me.z, i), y1 = __builtin_amdgcn_readlane(me.w, i);
            const bool ov = overlaps45(x0, x1, y0, y1, (x1 - x0 + 1) * (y1 - y0 + 1), me) & (lane > i);
            lo |= ov ? (1u << i) : 0u;
        }
        for (int i = 32; i < len; ++i) {
            const int x0 = __builtin_amdgcn_readlane(me.x, i), x1 = __builtin_amdgcn_readlane(me.y, i);
            const int y0 = __builtin_amdgcn_readlane(me.z, i), y1 = __builtin_amdgcn_readlane(me.w, i);
            const bool ov = overlaps45(x0, x1, y0, y1, (x1 - x0 + 1) * (y1 - y0 + 1), me) & (lane > i);
            hi |= ov ? (1u << (i - 32)) : 0u;
        }
        // Phase B: only boxes that overlap an earlier one can die.  In ascending order (the survivor bits below j are final
        // when j's turn comes): j dies iff one of its earlier overlappers is alive.
        u64 alive = len == 64 ? ~0ull : ((1ull << len) - 1ull);
        u64 cand = __ballot(((lo | hi) != 0u) & (lane < len));
        while (cand) {
            const int j = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            const u64 killers = ((u64)(unsigned)__builtin_amdgcn_readlane((int)hi, j) << 32) | (u64)(unsigned)__builtin_amdgcn_readlane((int)lo, j);
            if (killers & alive) alive &= ~(1ull << j);
        }
        if (lane < len) al_plain[s0 + lane] = (alive >> lane) & 1ull ? 1 : 0;
        return;
    }
    volatile unsigned char* al = al_plain;
    for (int i = 0; i < len; ++i) {
        if (!al[s0 + i]) continue;
        const int4 bi = nbox[s0 + i];
        const int area_i = (bi.y - bi.x + 1) * (bi.w - bi.z + 1);
        for (int j = i + 1 + lane; j < len; j += 64) {
            if (!al[s0 + j]) continue;
            if (overlaps45(bi.x, bi.y, bi.z, bi.w, area_i, nbox[s0 + j])) al[s0 + j] = 0;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// =================================================================================
// Soft-NMS: a neighbour's score is decayed, the picks re-ranked after every decay
// =================================================================================
// exp(x) for x <= 0 as a fixed sequence of singly rounded fp32 operations (this file is compiled with -ffp-contract=off), so
// that numpy float32 restates it bit for bit (tests/softnms_ref.py expw): Cody-Waite reduction by ln 2 in two parts, a degree-6
// polynomial, the scale by an exact power of two.  x < -87 gives 0; the smallest other value, 2^-126 * y, is a normal number.
__device__ __forceinline__ float soft_expw(float x) {
    if (x < -87.f) return 0.f;
    const float n = rintf(__fmul_rn(x, 1.44269504088896341f));
    const float r = __fsub_rn(__fsub_rn(x, __fmul_rn(n, 0.693359375f)), __fmul_rn(n, -2.12194440e-4f));
    float p = 1.9875691500e-4f;
    p = __fadd_rn(__fmul_rn(p, r), 1.3981999507e-3f);
    p = __fadd_rn(__fmul_rn(p, r), 8.3334519073e-3f);
    p = __fadd_rn(__fmul_rn(p, r), 4.1665795894e-2f);
    p = __fadd_rn(__fmul_rn(p, r), 1.6666665459e-1f);
    p = __fadd_rn(__fmul_rn(p, r), 5.0000001201e-1f);
    const float y = __fadd_rn(__fadd_rn(__fmul_rn(p, __fmul_rn(r, r)), r), 1.f);
    return __fmul_rn(y, __uint_as_float((unsigned)((int)n + 127) << 23));
}

constexpr int SOFT_LINEAR = 1, SOFT_GAUSSIAN = 2;      // ssd_nms_params.kind (0 = hard: nms_segment)
constexpr int SOFT_MAX = 1024;                         // candidates of one list
constexpr int SOFT_PER = SOFT_MAX / 64;                // per lane

struct SoftNmsArgs {
    float iou_thr, sigma, min_score;
    int max_picks;      // a class gives the image at most keep_top_k rows: the walk stops there
};

// Soft-NMS of one list of m <= 1024 candidates by one wave, where nms_segment runs for the hard rule.  keys[q] = score bits
// << 32 | a unique low word that ranks equal scores (any order of q: the rule always takes the largest remaining key), nbox[q]
// the round-tripped box.  Lane l owns candidates l, l + 64, ...: their keys live in registers (hi = score bits, lo = the low
// word; 0 / 0 = picked or absent -- a live key is never 0, its anchor field is at least 1 << 8), their boxes are read from LDS
// for every pivot.  Per pick: the lane's largest key, a 64-bit wave maximum (six __shfl_xor steps), the owner by ballot,
// the pivot's slot and box made scalar with readfirstlane (see nms_segment about vector loop state), then every remaining
// score times the weight of its overlap with the pivot.  Scores are non-negative floats, so their bit patterns order as their
// values and a product that is a denormal stays one (the kernels run with fp32 denormals on).  Picks leave as newkey[i] (the
// decayed key) and order[i] (the pivot's q), i < the returned count; the keys are strictly descending.  No atomics, no spin,
// every loop bounded by m, LDS the only memory touched.
template <int KIND>
__device__ __forceinline__ int soft_nms_segment(const u64* keys, const int4* nbox, int m, int lane, SoftNmsArgs sp, u64* newkey,
                                                unsigned short* order) {
    m = __builtin_amdgcn_readfirstlane(m);
    const int rows = (m + 63) >> 6;            // uniform: the slots any lane uses
    unsigned hi[SOFT_PER], lo[SOFT_PER];
#pragma unroll
    for (int t = 0; t < SOFT_PER; ++t) {
        const int q = lane + 64 * t;
        const u64 key = q < m ? keys[q] : 0ull;
        hi[t] = (unsigned)(key >> 32);
        lo[t] = (unsigned)key;
    }
    const int limit = __builtin_amdgcn_readfirstlane(min(m, sp.max_picks));
    int picks = 0;
    for (; picks < limit; ++picks) {
        // the lane's largest key and its slot
        u64 best = 0ull;
        int bt = 0;
#pragma unroll
        for (int t = 0; t < SOFT_PER; ++t) {
            if (t < rows) {
                const u64 key = ((u64)hi[t] << 32) | (u64)lo[t];
                if (key > best) { best = key; bt = t; }
            }
        }
        u64 top = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 other = __shfl_xor(top, o, 64);
            top = other > top ? other : top;
        }
        const unsigned top_hi = __builtin_amdgcn_readfirstlane((unsigned)(top >> 32));
        const unsigned top_lo = __builtin_amdgcn_readfirstlane((unsigned)top);
        if ((top_hi | top_lo) == 0u) break;                            // nothing remains (cannot happen before `limit`)
        if (__uint_as_float(top_hi) < sp.min_score) break;             // the rest is below it too
        const u64 own = __ballot(best == (((u64)top_hi << 32) | (u64)top_lo));      // exactly one lane: keys are unique
        const int owner = __builtin_ctzll(own);
        const int pt = __builtin_amdgcn_readlane(bt, owner);
        const int pq = owner + 64 * pt;
        if (lane == 0) {
            newkey[picks] = ((u64)top_hi << 32) | (u64)top_lo;
            order[picks] = (unsigned short)pq;
        }
#pragma unroll
        for (int t = 0; t < SOFT_PER; ++t)
            if (t == pt && lane == owner) { hi[t] = 0u; lo[t] = 0u; }
        const int4 pv = nbox[pq];
        const int x0 = __builtin_amdgcn_readfirstlane(pv.x), x1 = __builtin_amdgcn_readfirstlane(pv.y);
        const int y0 = __builtin_amdgcn_readfirstlane(pv.z), y1 = __builtin_amdgcn_readfirstlane(pv.w);
        const int area_i = (x1 - x0 + 1) * (y1 - y0 + 1);
#pragma unroll
        for (int t = 0; t < SOFT_PER; ++t) {
            if (t < rows) {
                const int q = min(lane + 64 * t, m - 1);               // (a clamped read; an absent slot's product stays 0)
                const int4 bj = nbox[q];
                const int w = max(0, min(x1, bj.y) - max(x0, bj.x) + 1);      // as overlaps45 computes them
                const int h = max(0, min(y1, bj.w) - max(y0, bj.z) + 1);
                const int inter = w * h;
                const int uni = area_i + (bj.y - bj.x + 1) * (bj.w - bj.z + 1) - inter;
                const float iou = uni > 0 ? __fdiv_rn((float)inter, (float)uni) : 0.f;
                float wgt;
                if constexpr (KIND == SOFT_LINEAR) wgt = iou > sp.iou_thr ? __fsub_rn(1.f, iou) : 1.f;
                else wgt = soft_expw(-__fdiv_rn(__fmul_rn(iou, iou), sp.sigma));
                hi[t] = __float_as_uint(__fmul_rn(__uint_as_float(hi[t]), wgt));
            }
        }
    }
    return picks;
}

constexpr int DET_THREADS = 512;
constexpr int DET_WAVES = DET_THREADS / 64;
constexpr int DET_FAST = 1024;           // up to this many candidates the whole image is handled in LDS
constexpr int DET_LDS_KEYS = 2048;       // general path: sort in LDS up to this many keys, else in (L2-resident) global
constexpr int DET_MAX_ALIVE = 32768;
constexpr int DET_MAX_SEGS = DET_MAX_ALIVE / SCAN_ROWS + 2;      // scan workgroups touching one image
constexpr int DET_SMEM = 50 * 1024;      // carved per path (general: 16 KB keys + 32 KB flags; fast: 49 KB)
static_assert(DET_SMEM >= DET_FAST * (8 + 8 + 16 + 16 + 1) && DET_SMEM >= DET_LDS_KEYS * 8 + DET_MAX_ALIVE, "LDS carve");

struct DetectArgs {
    int A, A2, nv, B;
    const double* anchors;
    const float* pred;
    int cap, max_out, out_cap, do_nms;
    const int* bcount;  // [scan workgroups][2] candidates per (workgroup, image) segment
    const u64* dense;   // [B*A] the segments' keys, compacted at each segment's first row
    u64* keys1;         // [B][A2] general path: the image's candidates gathered for the sort
    u64* keys2;
    int* box;       // [B][A][4]
    int* nbox;      // [B][A][4]
    DetectOut out;
};
// survivors in order -> the caller's arrays, clipped to [:max_out] / out_cap
template <int NCLS, typename KeyAt, typename BoxAt>
__device__ __forceinline__ void detect_emit(const DetectArgs& p, int b, int m, const unsigned char* alive, KeyAt key_at,
                                            BoxAt box_at, int* s_wtot) {
    const int tid = threadIdx.x;
    int limit = p.out_cap;
    if (p.max_out >= 0 && p.max_out < limit) limit = p.max_out;
    const int lane = tid & 63, wv = tid >> 6;
    int total = 0;
    for (int q0 = 0; q0 < m; q0 += DET_THREADS) {
        const int q = q0 + tid;
        const bool keep = q < m && alive[q];
        const u64 bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wtot[wv] = __popcll(bal);
        __syncthreads();
        int wbase = total, tot = 0;
#pragma unroll
        for (int i = 0; i < DET_WAVES; ++i) {
            if (i < wv) wbase += s_wtot[i];
            tot += s_wtot[i];
        }
        const int o = wbase + before;
        if (keep && o < limit) {
            const u64 key = key_at(q);
            const size_t dst = (size_t)b * p.out_cap + o;
            p.out.conf[dst] = __uint_as_float((unsigned)(key >> 32));
            p.out.cls[dst] = (int)(key & (u64)(NCLS - 1));
            p.out.idx[dst] = 32767 - (int)((key >> 8) & 0xFFFFull);
            *reinterpret_cast<int4*>(p.out.box + dst * 4) = box_at(q);
        }
        total += tot;
        __syncthreads();
    }
    if (tid == 0) p.out.count[b] = p.max_out >= 0 ? min(total, p.max_out) : total;
}

// The per-image phase: rank, decode, NMS and ordered emit of image b by one workgroup of DET_THREADS threads; `smem` = DET_SMEM
// bytes of the caller's LDS.  Called by detect_image_kernel (one workgroup per image).  NCLS, the class capacity of the
// per-class tables and of the key's class field (a power of two): 32 up to 27 classes, 128 up to MAX_CLASSES.
template <int NCLS>
__device__ __forceinline__ void detect_image_body(const DetectArgs& p, const int b, unsigned char* smem) {
    static_assert(NCLS == 32 || NCLS == 128, "class capacity");
    constexpr u64 CMASK = NCLS - 1;
    constexpr int CLANES = NCLS > 64 ? NCLS : 64;        // threads of the one-lane-per-class steps (whole waves)
    __shared__ int firstpos[NCLS], crank[NCLS], ccount[NCLS], segstart[NCLS + 1], order_cls[NCLS];
    __shared__ int s_npresent, s_wtot[DET_WAVES];
    __shared__ u64 cmax[NCLS];
    __shared__ int bstart[NCLS];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    u64* g1 = p.keys1 + (size_t)b * p.A2;
    // ---- the image's candidate segments (one per scan workgroup that touched the image) ----------------
    __shared__ int seg_off[DET_MAX_SEGS + 1], seg_base[DET_MAX_SEGS];
    __shared__ int s_pos[DET_FAST], s_cpos[DET_FAST];
    const int row_lo = b * p.A, row_hi = row_lo + p.A;
    const int first_blk = row_lo / SCAN_ROWS, nseg = (row_hi - 1) / SCAN_ROWS - first_blk + 1;
    if (tid < nseg) {
        const int blk = first_blk + tid;
        const bool tail_of_prev = blk * SCAN_ROWS < row_lo;      // the workgroup started in the previous image
        seg_base[tid] = tail_of_prev ? row_lo : blk * SCAN_ROWS;
        seg_off[tid + 1] = __hip_atomic_load(p.bcount + blk * 2 + (tail_of_prev ? 1 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (nseg <= 64) {                       // inclusive scan of the segment counts by one wave
        if (tid < 64) {
            int v = tid < nseg ? seg_off[tid + 1] : 0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(v, o, 64);
                if (lane >= o) v += t;
            }
            if (tid < nseg) seg_off[tid + 1] = v;
            if (tid == 0) seg_off[0] = 0;
        }
    } else if (tid == 0) {
        int acc = 0;
        seg_off[0] = 0;
        for (int i = 1; i <= nseg; ++i) { acc += seg_off[i]; seg_off[i] = acc; }
    }
    __syncthreads();
    const int n = seg_off[nseg];
    auto candidate = [&](int f) {            // f-th candidate of the image (any order: the keys are unique and get sorted)
        int lo = 0, hi = nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (seg_off[mid] <= f) lo = mid; else hi = mid - 1;
        }
        return __hip_atomic_load(p.dense + (size_t)seg_base[lo] + (f - seg_off[lo]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };

    if (n <= DET_FAST) {
        // ================= everything in LDS: rank sort, decode, NMS, emit =================
        u64* skey = reinterpret_cast<u64*>(smem);                       // candidates as listed
        u64* okey = skey + DET_FAST;                                    // candidates in output order
        int4* box = reinterpret_cast<int4*>(okey + DET_FAST);
        int4* nbox = box + DET_FAST;
        unsigned char* alive = reinterpret_cast<unsigned char*>(nbox + DET_FAST);      // (not volatile: see nms_segment)
        // every candidate's key, then (addressed by the key's anchor) its offsets and anchor: all global loads of the
        // workgroup are in flight together and land while the ranking sweep below runs.  Indices are clamped instead of
        // predicated: a select on a loaded value would make each load wait in turn.
        constexpr int PER = DET_FAST / DET_THREADS;
        u64 mykey[PER];
        float loc[PER][4];
        double anc[PER][4];
        int pos[PER], cpos[PER];
        if (n > 0) {
#pragma unroll
            for (int r = 0; r < PER; ++r) mykey[r] = candidate(min(tid + DET_THREADS * r, n - 1));
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int a = 32767 - (int)((mykey[r] >> 8) & 0xFFFFull);
                const float* lp = p.pred + ((size_t)b * p.A + a) * p.nv + (p.nv - 4);
                const double* ap = p.anchors + (size_t)a * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) { loc[r][e] = lp[e]; anc[r][e] = ap[e]; }
            }
        }
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int i = tid + DET_THREADS * r;
            if (i < n) skey[i] = mykey[r];
            else mykey[r] = ~0ull;
            s_pos[i] = 0; s_cpos[i] = 0;
        }
        if (tid < NCLS) { firstpos[tid] = INT_MAX; ccount[tid] = 0; }
        __syncthreads();
        const int m = p.cap >= 0 ? min(n, p.cap) : n;          // detections_cap (ssdutils.py:207-210)
        // The output order is: class groups in first-appearance order of the confidence-sorted list (defaultdict,
        // ssdutils.py:311-314) = classes by their best key, and inside a group by key.  When no cap bites (m == n, the
        // inference setting infer.py:233-234; training's cap of 200 only above 200 candidates) the GLOBAL rank of a
        // candidate is never needed: a counting sort by class and a rank inside the class' bucket (~n / 20 comparisons per
        // candidate instead of n) replace the n x n sweep, which was 9.6 of this kernel's 23 us at batch 128.
        const bool by_class = p.do_nms && m == n;
        if (by_class) {
            int myslot[PER];
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int i = tid + DET_THREADS * r;
                myslot[r] = i < n ? atomicAdd(&ccount[(int)(mykey[r] & CMASK)], 1) : 0;      // any order inside the bucket
                pos[r] = 0;
            }
            __syncthreads();
            if constexpr (NCLS <= 64) {
            if (tid < 64) {         // exclusive prefix of the class counts (raw class ids): where each bucket starts
                const int v = tid < NCLS ? ccount[tid] : 0;
                int inc = v;
#pragma unroll
                for (int o = 1; o < NCLS; o <<= 1) {
                    const int t = __shfl_up(inc, o, 64);
                    if (lane >= o) inc += t;
                }
                if (tid < NCLS) bstart[tid] = inc - v;
            }
            } else {
            if (tid < 64) {         // the same with NCLS / 64 consecutive classes per lane
                constexpr int K = NCLS / 64;
                int v[K], sum = 0;
#pragma unroll
                for (int e = 0; e < K; ++e) { v[e] = ccount[K * tid + e]; sum += v[e]; }
                int inc = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int t = __shfl_up(inc, o, 64);
                    if (lane >= o) inc += t;
                }
                int acc = inc - sum;
#pragma unroll
                for (int e = 0; e < K; ++e) { bstart[K * tid + e] = acc; acc += v[e]; }
            }
            }
            __syncthreads();
            u64* bkey = reinterpret_cast<u64*>(nbox);       // (nbox is written by the placement phase, two barriers on)
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int i = tid + DET_THREADS * r;
                if (i < n) bkey[bstart[(int)(mykey[r] & CMASK)] + myslot[r]] = mykey[r];
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int i = tid + DET_THREADS * r;
                cpos[r] = 0;
                if (i < n) {
                    const u64 key = mykey[r];
                    const int c = (int)(key & CMASK);
                    const u64* bk = bkey + bstart[c];
                    const int cnt = ccount[c];
                    int cp = 0;
                    for (int j = 0; j < cnt; ++j) cp += bk[j] > key ? 1 : 0;
                    cpos[r] = cp;
                    if (cp == 0) cmax[c] = key;      // the class' best key: one writer per class
                }
            }
            __syncthreads();
            if (tid < CLANES) {     // one lane per class: its rank among the present classes and where its segment starts
                const bool present = tid < NCLS && ccount[tid & (NCLS - 1)] > 0;
                const u64 mine = present ? cmax[tid & (NCLS - 1)] : 0ull;
                int r = 0, start = 0, npc = 0;
                for (int c = 0; c < NCLS; ++c) {
                    const bool before = ccount[c] > 0 && cmax[c] > mine;
                    r += before ? 1 : 0;
                    start += before ? ccount[c] : 0;
                    if constexpr (NCLS > 64) npc += ccount[c] > 0 ? 1 : 0;
                }
                int np;
                if constexpr (NCLS > 64) np = npc;
                else np = __popcll(__ballot(present));
                if (tid < NCLS) crank[tid] = r;
                if (present) segstart[r] = start;
                if (tid == 0) { s_npresent = np; segstart[np] = m; }
            }
        } else {
        // Rank of every candidate among all (confidence descending, anchor ascending: keys are unique) and among those of
        // its own class: an n x n comparison, spread over ALL thread
        // slots -- with n candidates rounded up to n2 (a power of two) each candidate gets 1024 / n2 slots, each sweeping
        // its share of the list (every read an LDS broadcast); the partial counts meet in LDS.
        {
            const int n2 = next_pow2(n > 1 ? n : 1);
            const int lg = 31 - __builtin_clz(n2);
            const int nsweep = (DET_THREADS * PER) >> lg;
            const int jchunk = (n + nsweep - 1) / nsweep;
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int slot = tid + DET_THREADS * r;
                const int i = slot & (n2 - 1), sw = slot >> lg;
                if (i >= n) continue;
                const u64 ki = skey[i];
                const int j0 = sw * jchunk, j1 = min(n, j0 + jchunk);
                int gt = 0, cgt = 0;
#pragma unroll 4
                for (int j = j0; j < j1; ++j) {
                    const u64 kj = skey[j];
                    const bool g = kj > ki;
                    gt += g ? 1 : 0;
                    cgt += (g && ((kj ^ ki) & CMASK) == 0ull) ? 1 : 0;
                }
                if (gt) atomicAdd(&s_pos[i], gt);
                if (cgt) atomicAdd(&s_cpos[i], cgt);
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int i = tid + DET_THREADS * r;
            pos[r] = s_pos[i]; cpos[r] = s_cpos[i];
        }
        // class groups in first-appearance order (defaultdict, ssdutils.py:311-314)
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int i = tid + DET_THREADS * r;
            if (i < n && pos[r] < m) {
                const int c = (int)(mykey[r] & CMASK);
                atomicMin(&firstpos[c], pos[r]);
                atomicAdd(&ccount[c], 1);
            }
        }
        __syncthreads();
        if (tid < CLANES) {     // one lane per class: its rank among the present classes and where its segment starts
            const int mine = tid < NCLS ? firstpos[tid] : INT_MAX;
            int r = 0, start = 0, npc = 0;
            for (int c = 0; c < NCLS; ++c) {
                const bool before = firstpos[c] < mine;
                r += before ? 1 : 0;
                start += before ? ccount[c] : 0;
                if constexpr (NCLS > 64) npc += firstpos[c] != INT_MAX ? 1 : 0;
            }
            int np;
            if constexpr (NCLS > 64) np = npc;
            else np = __popcll(__ballot(mine != INT_MAX));
            if (tid < NCLS) crank[tid] = r;
            if (p.do_nms && mine != INT_MAX) segstart[r] = start;
            if (tid == 0) {     // decode-only mode: one group in confidence order, no suppression
                s_npresent = p.do_nms ? np : 0;
                segstart[p.do_nms ? np : 0] = m;
            }
        }
        }
        __syncthreads();
        // place, decode
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int i = tid + DET_THREADS * r;
            if (i < n && pos[r] < m) {
                const u64 key = mykey[r];
                const int q = p.do_nms ? segstart[crank[(int)(key & CMASK)]] + cpos[r] : pos[r];
                const int a = 32767 - (int)((key >> 8) & 0xFFFFull);
                int bx[4], nb[4];
                decode_box(loc[r], anc[r], bx);
                nms_roundtrip(bx, nb);
                okey[q] = key;
                box[q] = make_int4(bx[0], bx[1], bx[2], bx[3]);
                nbox[q] = make_int4(nb[0], nb[1], nb[2], nb[3]);
                alive[q] = 1;
            }
        }
        __syncthreads();
        for (int r = wave; r < s_npresent; r += DET_WAVES) nms_segment(nbox, alive, segstart[r], segstart[r + 1] - segstart[r], lane);
        __syncthreads();
        detect_emit<NCLS>(p, b, m, alive, [&](int q) { return okey[q]; }, [&](int q) { return box[q]; }, s_wtot);
        return;
    }

    // ================= general path: bitonic sorts, boxes in (L2-resident) global memory =================
    u64* lkeys = reinterpret_cast<u64*>(smem);
    unsigned char* alive = smem + DET_LDS_KEYS * 8;
    u64* g2 = p.keys2 + (size_t)b * p.A2;
    int4* box = reinterpret_cast<int4*>(p.box + (size_t)b * p.A * 4);
    int4* nbox = reinterpret_cast<int4*>(p.nbox + (size_t)b * p.A * 4);

    // ---- sort 1: confidence descending, anchor ascending ------------------------------
    const int n2 = next_pow2(n > 1 ? n : 1);
    if (n2 <= DET_LDS_KEYS) {
        for (int i = tid; i < n2; i += DET_THREADS) lkeys[i] = i < n ? candidate(i) : 0ull;
        __syncthreads();
        bitonic_desc(lkeys, n2);
        for (int i = tid; i < n; i += DET_THREADS) g1[i] = lkeys[i];
    } else {
        for (int i = tid; i < n2; i += DET_THREADS) g1[i] = i < n ? candidate(i) : 0ull;
        __syncthreads();
        bitonic_desc(g1, n2);
    }
    __syncthreads();
    const int m = p.cap >= 0 ? min(n, p.cap) : n;          // detections_cap (ssdutils.py:207-210)

    // ---- class groups in first-appearance order (defaultdict, ssdutils.py:311-314) ----
    if (tid < NCLS) { firstpos[tid] = INT_MAX; ccount[tid] = 0; }
    __syncthreads();
    for (int i = tid; i < m; i += DET_THREADS) {
        const int c = (int)(g1[i] & CMASK);
        atomicMin(&firstpos[c], i);
        atomicAdd(&ccount[c], 1);
    }
    __syncthreads();
    if (tid < NCLS) {
        int r = 0;
        for (int c = 0; c < NCLS; ++c)
            if (firstpos[c] < firstpos[tid]) ++r;
        crank[tid] = (firstpos[tid] == INT_MAX) ? NCLS - 1 : (p.do_nms ? r : 0);
    }
    __syncthreads();
    if (tid == 0) {
        int np = 0;
        if (p.do_nms) {     // decode-only mode: one group in confidence order, no suppression
            for (int c = 0; c < NCLS; ++c)
                if (firstpos[c] != INT_MAX) { order_cls[crank[c]] = c; ++np; }
            int acc = 0;
            for (int r = 0; r < np; ++r) { segstart[r] = acc; acc += ccount[order_cls[r]]; }
            segstart[np] = acc;
        }
        s_npresent = np;
    }
    __syncthreads();

    // ---- sort 2: (class rank, position) ascending == descending of the complement -----
    const int m2 = next_pow2(m > 1 ? m : 1);
    u64* k2 = m2 <= DET_LDS_KEYS ? lkeys : g2;
    for (int i = tid; i < m2; i += DET_THREADS) {
        u64 key = ~0ull;
        if (i < m) key = ((u64)crank[(int)(g1[i] & CMASK)] << 32) | (u64)i;
        k2[i] = ~key;
    }
    __syncthreads();
    bitonic_desc(k2, m2);

    // ---- decode every candidate in class-grouped order ----------------------------------
    for (int q = tid; q < m; q += DET_THREADS) {
        const int pos = (int)((~k2[q]) & 0xFFFFFFFFull);
        const u64 key = g1[pos];
        const int a = 32767 - (int)((key >> 8) & 0xFFFFull);
        int bx[4], nb[4];
        decode_box(p.pred + ((size_t)b * p.A + a) * p.nv + (p.nv - 4), p.anchors + (size_t)a * 4, bx);
        nms_roundtrip(bx, nb);
        box[q] = make_int4(bx[0], bx[1], bx[2], bx[3]);
        nbox[q] = make_int4(nb[0], nb[1], nb[2], nb[3]);
        if (q < DET_MAX_ALIVE) alive[q] = 1;
    }
    __syncthreads();

    // ---- greedy NMS: one wave per class segment ---
    for (int r = wave; r < s_npresent; r += DET_WAVES) nms_segment(nbox, alive, segstart[r], segstart[r + 1] - segstart[r], lane);
    __syncthreads();

    // ---- compact survivors in order; the caller's [:max_out] -------------------------------
    detect_emit<NCLS>(p, b, m, alive, [&](int q) { return g1[(int)((~k2[q]) & 0xFFFFFFFFull)]; }, [&](int q) { return box[q]; }, s_wtot);
}

template <int NCLS>
__global__ __launch_bounds__(DET_THREADS) void detect_image_kernel(DetectArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[DET_SMEM];
    detect_image_body<NCLS>(p, blockIdx.x, smem);
}

// (Round 4 also built the pass as ONE launch -- scan workgroups taking a ticket per image, the last arriver running that image's
// per-image phase beside the scan: bit-identical and slower, 92 us against 17.6 + 26.6 us (profiles/r04_y_detect_fused_probe.txt:
// the scan half alone took 34 us in that form, and a chain of dependent loads beside an HBM-bound scan pays the loaded memory
// system's latency at every link).  Removed in round 5.)

static int pow2_ge(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

static size_t det_bcount_bytes(int B, int A) {      // bcount [scan workgroups][2]
    const size_t blocks = ((size_t)B * A + SCAN_ROWS - 1) / SCAN_ROWS;
    return (blocks * 8 + 255) / 256 * 256 + 256;
}
constexpr int DET_MAX_BATCH = 4096;
static size_t det_head_bytes(int B, int A) { return det_bcount_bytes(B, A); }

size_t detect_ws_bytes(int B, int A) {
    const size_t A2 = pow2_ge(A);
    return det_head_bytes(B, A) + ((size_t)B * A * 8 + 255) / 256 * 256 + 2 * (size_t)B * A2 * 8 + 2 * (size_t)B * A * 16;
}

void detect(int A, int num_classes, const double* anchors, const float* pred, int B, float conf_thr, int cap, int max_out,
            int out_cap, bool nms, const DetectOut& out, void* ws, hipStream_t s) {
    SSD_REQUIRE(A <= 32767 && A <= DET_MAX_ALIVE, "detect: at most 32767 anchors (got %d)", A);
    require_num_classes(num_classes);
    SSD_REQUIRE(A >= SCAN_ROWS, "detect: at least %d anchors", SCAN_ROWS);
    SSD_REQUIRE(out_cap >= 1, "detect: out_cap must be >= 1");
    SSD_REQUIRE((long long)B * A < (1LL << 31), "detect: batch * anchors must stay below 2^31");
    const int nv = num_classes + 5;
    const int A2 = pow2_ge(A);
    SSD_REQUIRE(B <= DET_MAX_BATCH, "detect: at most %d images per pass (got %d)", DET_MAX_BATCH, B);
    char* base = (char*)ws;
    int* bcount = (int*)base; base += det_head_bytes(B, A);
    u64* dense = (u64*)base; base += ((size_t)B * A * 8 + 255) / 256 * 256;
    u64* keys1 = (u64*)base; base += (size_t)B * A2 * 8;
    u64* keys2 = (u64*)base; base += (size_t)B * A2 * 8;
    int* box = (int*)base; base += (size_t)B * A * 16;
    int* nbox = (int*)base;
    const size_t rows = (size_t)B * A;
    const int blocks = (int)((rows + SCAN_ROWS - 1) / SCAN_ROWS);
    // Up to 27 classes the kernels measured on the 20-class workload (a thread per row, 32-entry class tables); wider rows
    // take the chunked scan and the 128-entry tables, which the narrow path would outgrow in LDS (scan) and key bits.
    const bool wide = nv > SCAN_MAXV;
    {
        ProfScope prof("detect_scan", 0.0, (double)rows * nv * 4.0, s);
        if (wide)
            hipLaunchKernelGGL(detect_scan_wide_kernel, dim3(blocks), dim3(256), (size_t)SCANW_ROWS * nv * sizeof(float), s, A, nv, B,
                               pred, conf_thr, dense, bcount);
        else
            hipLaunchKernelGGL(detect_scan_kernel, dim3(blocks), dim3(256), (size_t)SCAN_ROWS * nv * sizeof(float), s, A, nv, B, pred,
                               conf_thr, dense, bcount);
    }
    DetectArgs a{};
    a.A = A; a.A2 = A2; a.nv = nv; a.B = B; a.anchors = anchors; a.pred = pred;
    a.cap = cap; a.max_out = max_out; a.out_cap = out_cap; a.do_nms = nms ? 1 : 0; a.bcount = bcount; a.dense = dense;
    a.keys1 = keys1; a.keys2 = keys2; a.box = box; a.nbox = nbox; a.out = out;
    {
        ProfScope prof("detect_image", 0.0, 0.0, s);
        if (wide)
            hipLaunchKernelGGL(detect_image_kernel<128>, dim3(B), dim3(DET_THREADS), 0, s, a);
        else
            hipLaunchKernelGGL(detect_image_kernel<32>, dim3(B), dim3(DET_THREADS), 0, s, a);
    }
    HIP_OK(hipGetLastError());
}

// =================================================================================
// tiled detection: the boxes of a picture's tiles merged into one detection list
// =================================================================================
// One workgroup per picture.  Its tiles' decode_boxes records (ssd_decode_nms_dev with nms = 0: confidence order, integer
// boxes on the tile's 1000 grid) are gathered, records that an interior tile edge has cut are dropped, and every survivor becomes
//   pre-key = order(conf) << 30 | (255 - tile) << 22 | (32767 - anchor) << 7 | class      (62 bits)
// stored densely (ballot prefix, no atomics on memory) with its source slot beside it.  A class' place among the groups
// is the place of its best record in the confidence-sorted union (defaultdict, ssdutils.py:311-314), i.e. the rank of
// max(pre-key) per class, which an LDS atomicMax finds without a sort.  ONE descending sort of
//   key = (127 - class rank) << 55 | pre-key >> 7
// then yields the output order: class groups in first-appearance order, inside a group confidence descending, equal
// confidences by tile, then anchor.  The sorted records are mapped into the picture's 1000 grid, suppressed per class by
// nms_segment (one wave per class) and emitted in order.  Up to MRG_LDS_KEYS candidates sort in LDS, more in the picture's
// (L2-resident) workspace region.
__device__ __forceinline__ unsigned float_order_bits(float f);      // (defined with nms_boxes_kernel below)
constexpr int MRG_THREADS = 512;
constexpr int MRG_WAVES = MRG_THREADS / 64;
constexpr int MRG_NCLS = 128;
static_assert(MERGE_MAX_TILES <= 256 && MAX_CLASSES < MRG_NCLS, "key fields");

struct MergeArgs {
    const MergeTile* tiles;     // [n_tiles]
    const int* img_first;       // [n_images + 1] first tile of every picture
    const int* reg_off;         // [n_images] first workspace element of every picture
    int tile_cap, edge_margin, max_out, out_cap;
    const int* count; const float* conf; const int* cls; const int* idx; const int* box;
    u64* keys; unsigned* vals; int4* mbox; int4* nbox;
    int* count_out; float* conf_out; int* cls_out; int* idx_out; int* tile_out; int* box_out;
};

// descending bitonic sort of n2 (power of two) unique keys with a 32-bit payload by one workgroup
__device__ __forceinline__ void merge_sort_desc(u64* keys, unsigned* vals, int n2) {
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += MRG_THREADS) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const u64 a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if (up ? (a < b) : (a > b)) {
                        const unsigned va = vals[i], vb = vals[ixj];
                        keys[i] = b; keys[ixj] = a;
                        vals[i] = vb; vals[ixj] = va;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// a tile-grid coordinate (0..999) on the picture's 1000 grid: floor((1000 * origin + v * extent) / picture), at most 999.
// origin + extent <= picture <= MERGE_MAX_SIDE keeps the numerator below 2^31.
__device__ __forceinline__ int merge_map(int v, int origin, int extent, int picture) {
    const unsigned num = 1000u * (unsigned)origin + (unsigned)min(max(v, 0), 999) * (unsigned)extent;
    return min((int)(num / (unsigned)picture), 999);
}

__global__ __launch_bounds__(MRG_THREADS) void merge_tiles_kernel(MergeArgs p) {
    __shared__ __attribute__((aligned(16))) u64 lkeys[MERGE_LDS_KEYS];
    __shared__ unsigned lvals[MERGE_LDS_KEYS];
    __shared__ unsigned char alive[MERGE_MAX_CAND];
    __shared__ int s_tcnt[MERGE_MAX_TILES];
    __shared__ u64 cmax[MRG_NCLS];
    __shared__ int ccount[MRG_NCLS], crank[MRG_NCLS], segstart[MRG_NCLS + 1];
    __shared__ int s_npresent, s_wtot[MRG_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int T0 = p.img_first[b], nt = p.img_first[b + 1] - T0;
    const int cap = p.tile_cap;
    const int slots = nt * cap;                              // <= MERGE_MAX_CAND (checked on the host)
    const size_t R = (size_t)p.reg_off[b];
    u64* gkeys = p.keys + R;
    unsigned* gvals = p.vals + R;
    int4* mbox = p.mbox + R;
    int4* nbox = p.nbox + R;
    const int4* box_in = reinterpret_cast<const int4*>(p.box);

    for (int t = tid; t < nt; t += MRG_THREADS) s_tcnt[t] = min(max(p.count[T0 + t], 0), cap);      // count may exceed the cap
    if (tid < MRG_NCLS) { cmax[tid] = 0ull; ccount[tid] = 0; }
    __syncthreads();

    // ---- gather, edge drop, dense pre-keys ------------------------------------------------------------
    int n = 0;
    for (int f0 = 0; f0 < slots; f0 += MRG_THREADS) {
        const int f = f0 + tid;
        bool ok = false;
        u64 pre = 0ull;
        if (f < slots) {
            const int t = f / cap, j = f - t * cap;
            if (j < s_tcnt[t]) {
                const size_t src = (size_t)(T0 + t) * cap + j;
                const int4 bx = box_in[src];                  // xmin, xmax, ymin, ymax
                const int in = p.tiles[T0 + t].interior, m = p.edge_margin;
                const bool cut = m >= 0 && (((in & 1) && bx.x <= m) || ((in & 2) && bx.y >= 999 - m) || ((in & 4) && bx.z <= m) ||
                                            ((in & 8) && bx.w >= 999 - m));
                if (!cut) {
                    ok = true;
                    const float cf = p.conf[src] + 0.f;       // -0 orders as +0: by float value
                    pre = ((u64)float_order_bits(cf) << 30) | ((u64)(255 - t) << 22) | ((u64)(32767 - (p.idx[src] & 32767)) << 7) |
                          (u64)(p.cls[src] & (MRG_NCLS - 1));
                }
            }
        }
        const u64 bal = __ballot(ok);
        if (lane == 0) s_wtot[wave] = __popcll(bal);
        __syncthreads();
        int wbase = n, tot = 0;
#pragma unroll
        for (int i = 0; i < MRG_WAVES; ++i) {
            if (i < wave) wbase += s_wtot[i];
            tot += s_wtot[i];
        }
        if (ok) {
            const int g = wbase + __popcll(bal & ((1ull << lane) - 1ull));
            const int c = (int)(pre & (u64)(MRG_NCLS - 1));
            gkeys[g] = pre;
            gvals[g] = (unsigned)f;
            atomicMax(reinterpret_cast<unsigned long long*>(&cmax[c]), (unsigned long long)pre);
            atomicAdd(&ccount[c], 1);
        }
        n += tot;
        __syncthreads();
    }

    // ---- class groups in first-appearance order of the sorted union = by their best record ------------
    if (tid < MRG_NCLS) {
        const bool present = ccount[tid] > 0;
        const u64 mine = cmax[tid];
        int r = 0, np = 0;
        for (int c = 0; c < MRG_NCLS; ++c) {
            const bool pc = ccount[c] > 0;
            r += (pc && cmax[c] > mine) ? 1 : 0;
            np += pc ? 1 : 0;
        }
        crank[tid] = present ? r : MRG_NCLS - 1;
        if (tid == 0) { s_npresent = np; segstart[np] = n; }
    }
    __syncthreads();

    // ---- the one sort -----------------------------------------------------------------------------------
    const int n2 = next_pow2(n > 1 ? n : 1);
    const bool in_lds = n2 <= MERGE_LDS_KEYS;
    if (in_lds) {
        for (int i = tid; i < n2; i += MRG_THREADS) {
            u64 k = 0ull;                                     // padding sorts last: a real key's rank field is >= 1
            if (i < n) {
                const u64 pre = gkeys[i];
                k = ((u64)(MRG_NCLS - 1 - crank[(int)(pre & (u64)(MRG_NCLS - 1))]) << 55) | (pre >> 7);
                lvals[i] = gvals[i];
            } else {
                lvals[i] = 0u;
            }
            lkeys[i] = k;
        }
        __syncthreads();
        merge_sort_desc(lkeys, lvals, n2);
        for (int i = tid; i < n; i += MRG_THREADS) { gkeys[i] = lkeys[i]; gvals[i] = lvals[i]; }
    } else {
        for (int i = tid; i < n2; i += MRG_THREADS) {         // n2 <= the region's size, a power of two >= slots
            u64 k = 0ull;
            if (i < n) {
                const u64 pre = gkeys[i];
                k = ((u64)(MRG_NCLS - 1 - crank[(int)(pre & (u64)(MRG_NCLS - 1))]) << 55) | (pre >> 7);
            } else {
                gvals[i] = 0u;
            }
            gkeys[i] = k;
        }
        __syncthreads();
        merge_sort_desc(gkeys, gvals, n2);
    }
    __syncthreads();

    // ---- segment starts, boxes on the picture's grid ----------------------------------------------------
    for (int q = tid; q < n; q += MRG_THREADS) {
        const int r = MRG_NCLS - 1 - (int)(gkeys[q] >> 55);
        if (q == 0 || (MRG_NCLS - 1 - (int)(gkeys[q - 1] >> 55)) != r) segstart[r] = q;
        const int f = (int)gvals[q];
        const int t = f / cap, j = f - t * cap;
        const MergeTile tl = p.tiles[T0 + t];
        const int4 bx = box_in[(size_t)(T0 + t) * cap + j];
        int o[4], nb[4];
        o[0] = merge_map(bx.x, tl.x0, tl.w, tl.img_w); o[1] = merge_map(bx.y, tl.x0, tl.w, tl.img_w);
        o[2] = merge_map(bx.z, tl.y0, tl.h, tl.img_h); o[3] = merge_map(bx.w, tl.y0, tl.h, tl.img_h);
        nms_roundtrip(o, nb);
        mbox[q] = make_int4(o[0], o[1], o[2], o[3]);
        nbox[q] = make_int4(nb[0], nb[1], nb[2], nb[3]);
        alive[q] = 1;
    }
    __syncthreads();

    // ---- greedy NMS: one wave per class segment ---------------------------------------------------------
    for (int r = wave; r < s_npresent; r += MRG_WAVES) nms_segment(nbox, alive, segstart[r], segstart[r + 1] - segstart[r], lane);
    __syncthreads();

    // ---- survivors in order; the caller's [:max_out] ----------------------------------------------------
    int limit = p.out_cap;
    if (p.max_out >= 0 && p.max_out < limit) limit = p.max_out;
    int total = 0;
    for (int q0 = 0; q0 < n; q0 += MRG_THREADS) {
        const int q = q0 + tid;
        const bool keep = q < n && alive[q];
        const u64 bal = __ballot(keep);
        if (lane == 0) s_wtot[wave] = __popcll(bal);
        __syncthreads();
        int wbase = total, tot = 0;
#pragma unroll
        for (int i = 0; i < MRG_WAVES; ++i) {
            if (i < wave) wbase += s_wtot[i];
            tot += s_wtot[i];
        }
        const int o = wbase + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && o < limit) {
            const int f = (int)gvals[q];
            const int t = f / cap, j = f - t * cap;
            const size_t src = (size_t)(T0 + t) * cap + j;
            const size_t dst = (size_t)b * p.out_cap + o;
            if (p.conf_out) p.conf_out[dst] = p.conf[src];
            p.cls_out[dst] = p.cls[src] & (MRG_NCLS - 1);
            if (p.idx_out) p.idx_out[dst] = p.idx[src];
            if (p.tile_out) p.tile_out[dst] = t;
            *reinterpret_cast<int4*>(p.box_out + dst * 4) = mbox[q];
        }
        total += tot;
        __syncthreads();
    }
    if (tid == 0) p.count_out[b] = p.max_out >= 0 ? min(total, p.max_out) : total;
}

// workspace: the tile table and the per-picture offsets, then per picture a region of pow2(tiles * tile_cap) elements of
// each of keys (8 B), payload (4 B), mapped box (16 B) and NMS box (16 B); the regions sum to < 2 * n_tiles * tile_cap.
static size_t merge_head_bytes(int n_tiles) {
    return ((size_t)n_tiles * sizeof(MergeTile) + (size_t)(2 * n_tiles + 2) * sizeof(int) + 255) / 256 * 256;
}

size_t merge_tiles_ws_bytes(int n_tiles, int tile_cap) {
    SSD_REQUIRE(n_tiles >= 1 && tile_cap >= 1, "merge_tiles: n_tiles and tile_cap must be >= 1 (got %d, %d)", n_tiles, tile_cap);
    SSD_REQUIRE((long long)n_tiles * tile_cap < (1LL << 28), "merge_tiles: n_tiles * tile_cap must stay below 2^28");
    return merge_head_bytes(n_tiles) + 2 * (size_t)n_tiles * tile_cap * (8 + 4 + 16 + 16) + 256;
}

// every limit of merge_tiles; fills the table that goes to the device: the tiles, then img_first [n_tiles + 1] and reg_off [n_tiles + 1]
static void merge_plan(const MergeTile* tiles, int n_tiles, int n_images, int tile_cap, int out_cap, std::vector<int>& head) {
    SSD_REQUIRE(tiles != nullptr, "merge_tiles: null argument");
    SSD_REQUIRE(n_tiles >= 1 && n_images >= 1, "merge_tiles: at least one tile and one picture (got %d, %d)", n_tiles, n_images);
    SSD_REQUIRE(tile_cap >= 1, "merge_tiles: tile_cap must be >= 1 (got %d)", tile_cap);
    SSD_REQUIRE(out_cap >= 1, "merge_tiles: out_cap must be >= 1 (got %d)", out_cap);
    SSD_REQUIRE((long long)n_tiles * tile_cap < (1LL << 28), "merge_tiles: n_tiles * tile_cap must stay below 2^28");
    SSD_REQUIRE(tiles[0].image == 0 && tiles[n_tiles - 1].image == n_images - 1,
                "merge_tiles: image indices must ascend from 0 to n_images - 1 = %d (first %d, last %d)", n_images - 1, tiles[0].image,
                tiles[n_tiles - 1].image);
    head.assign((size_t)n_tiles * 8 + 2 * (size_t)n_tiles + 2, 0);
    MergeTile* ht = reinterpret_cast<MergeTile*>(head.data());
    int* first = head.data() + (size_t)n_tiles * 8;
    int* reg = first + n_tiles + 1;
    size_t off = 0;
    for (int t = 0, img = -1; t < n_tiles; ++t) {
        const MergeTile& tl = tiles[t];
        const int im = tl.image;
        SSD_REQUIRE(im == img || im == img + 1, "merge_tiles: image indices must ascend without gaps (tile %d: image %d after %d)", t, im,
                    img);
        SSD_REQUIRE(tl.img_w >= 1 && tl.img_h >= 1 && tl.img_w <= MERGE_MAX_SIDE && tl.img_h <= MERGE_MAX_SIDE,
                    "merge_tiles: tile %d: picture of %d x %d outside 1..%d", t, tl.img_w, tl.img_h, MERGE_MAX_SIDE);
        SSD_REQUIRE(tl.x0 >= 0 && tl.y0 >= 0 && tl.w >= 1 && tl.h >= 1 && tl.x0 <= tl.img_w - tl.w && tl.y0 <= tl.img_h - tl.h,
                    "merge_tiles: tile %d (%d, %d, %d x %d) leaves its %d x %d picture", t, tl.x0, tl.y0, tl.w, tl.h, tl.img_w, tl.img_h);
        SSD_REQUIRE(tl.interior >= 0 && tl.interior <= 15, "merge_tiles: tile %d: interior = %d outside 0..15", t, tl.interior);
        if (im != img) {
            img = im;
            first[img] = t;
        } else {
            SSD_REQUIRE(tl.img_w == tiles[t - 1].img_w && tl.img_h == tiles[t - 1].img_h,
                        "merge_tiles: tile %d: the tiles of picture %d disagree about its size", t, im);
        }
        ht[t] = tl;
    }
    first[n_images] = n_tiles;
    for (int i = 0; i < n_images; ++i) {
        const int nt = first[i + 1] - first[i];
        SSD_REQUIRE(nt <= MERGE_MAX_TILES, "merge_tiles: picture %d has %d tiles, at most %d", i, nt, MERGE_MAX_TILES);
        SSD_REQUIRE((long long)nt * tile_cap <= MERGE_MAX_CAND, "merge_tiles: picture %d: %d tiles x tile_cap %d exceeds %d candidates", i,
                    nt, tile_cap, MERGE_MAX_CAND);
        reg[i] = (int)off;
        off += (size_t)pow2_ge(nt * tile_cap);
    }
}

void merge_tiles_check(const MergeTile* tiles, int n_tiles, int n_images, int tile_cap, int out_cap) {
    std::vector<int> head;
    merge_plan(tiles, n_tiles, n_images, tile_cap, out_cap, head);
}

void merge_tiles(const MergeTile* tiles, int n_tiles, int n_images, int tile_cap, const int* count, const float* conf, const int* cls,
                 const int* idx, const int* box, int edge_margin, int max_out, int out_cap, int* count_out, float* conf_out,
                 int* cls_out, int* idx_out, int* tile_out, int* box_out, void* ws, hipStream_t s) {
    // every limit is checked before anything is enqueued
    SSD_REQUIRE(tiles && count && conf && cls && idx && box && count_out && cls_out && box_out && ws, "merge_tiles: null argument");
    std::vector<int> head;
    merge_plan(tiles, n_tiles, n_images, tile_cap, out_cap, head);
    const size_t total = 2 * (size_t)n_tiles * tile_cap;      // the regions end below it: each is below twice its slots
    char* base = (char*)ws;
    MergeArgs a{};
    a.tiles = reinterpret_cast<const MergeTile*>(base);
    a.img_first = reinterpret_cast<const int*>(base) + (size_t)n_tiles * 8;
    a.reg_off = a.img_first + n_tiles + 1;
    HIP_OK(hipMemcpyAsync(base, head.data(), head.size() * sizeof(int), hipMemcpyHostToDevice, s));      // (pageable: copied by the call)
    base += merge_head_bytes(n_tiles);
    a.keys = (u64*)base; base += total * 8;
    a.mbox = (int4*)base; base += total * 16;
    a.nbox = (int4*)base; base += total * 16;
    a.vals = (unsigned*)base;
    a.tile_cap = tile_cap; a.edge_margin = edge_margin; a.max_out = max_out; a.out_cap = out_cap;
    a.count = count; a.conf = conf; a.cls = cls; a.idx = idx; a.box = box;
    a.count_out = count_out; a.conf_out = conf_out; a.cls_out = cls_out; a.idx_out = idx_out; a.tile_out = tile_out; a.box_out = box_out;
    {
        ProfScope prof("merge_tiles", 0.0, 0.0, s);
        hipLaunchKernelGGL(merge_tiles_kernel, dim3(n_images), dim3(MRG_THREADS), 0, s, a);
    }
    HIP_OK(hipGetLastError());
}

// =================================================================================
// non_maximum_suppression / suppress_overlaps on an arbitrary box list (ssdutils.py:232-318)
// =================================================================================
// One workgroup: sort by (group ascending, confidence descending, input index ascending), greedy NMS per group
// (one wave per group, IoU as the reference's f64 quotient against an arbitrary threshold), survivors in order.
constexpr int NMSB_THREADS = 512;

__device__ __forceinline__ unsigned float_order_bits(float f) {      // monotone map float -> unsigned (any sign)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(NMSB_THREADS) void nms_boxes_kernel(int n, int n2, int ngroups, const int4* __restrict__ boxes,
                                                                 const float* __restrict__ conf, const int* __restrict__ group,
                                                                 double thr, u64* __restrict__ keys, int* __restrict__ gstart,
                                                                 unsigned char* __restrict__ alive, int* __restrict__ keep) {
    __shared__ int s_wtot[NMSB_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < n2; i += NMSB_THREADS) {
        u64 k = 0ull;        // padding sorts last
        if (i < n) {
            // -0.0 == +0.0 by value: both take +0.0's bits, so that the input index alone orders them (the earlier box first)
            const float c = conf[i] == 0.f ? 0.f : conf[i];
            k = ((u64)(65535 - group[i]) << 48) | ((u64)float_order_bits(c) << 16) | (u64)(65535 - i);
        }
        keys[i] = k;
        if (i < n) alive[i] = 1;
    }
    for (int g = tid; g <= ngroups; g += NMSB_THREADS) gstart[g] = n;
    __syncthreads();
    bitonic_desc(keys, n2);
    // segment starts: first sorted position of every group (groups without boxes keep the next start)
    for (int q = tid; q < n; q += NMSB_THREADS) {
        const int g = 65535 - (int)(keys[q] >> 48);
        if (q == 0 || (65535 - (int)(keys[q - 1] >> 48)) != g) gstart[g] = q;
    }
    __syncthreads();
    if (tid == 0)
        for (int g = ngroups - 1; g >= 0; --g)
            if (gstart[g] == n) gstart[g] = gstart[g + 1];
    __syncthreads();
    volatile unsigned char* al = alive;
    for (int g = wave; g < ngroups; g += NMSB_THREADS / 64) {
        const int s0 = gstart[g], len = gstart[g + 1] - s0;
        for (int i = 0; i < len; ++i) {
            if (!al[s0 + i]) continue;
            const int4 bi = boxes[65535 - (int)(keys[s0 + i] & 0xFFFFull)];
            const long long area_i = (long long)(bi.y - bi.x + 1) * (bi.w - bi.z + 1);
            for (int j = i + 1 + lane; j < len; j += 64) {
                if (!al[s0 + j]) continue;
                const int4 bj = boxes[65535 - (int)(keys[s0 + j] & 0xFFFFull)];
                const long long w = max(0, min(bi.y, bj.y) - max(bi.x, bj.x) + 1);
                const long long h = max(0, min(bi.w, bj.w) - max(bi.z, bj.z) + 1);
                const long long inter = w * h;
                const long long uni = area_i + (long long)(bj.y - bj.x + 1) * (bj.w - bj.z + 1) - inter;
                // intersection / union as numpy divides two int64 arrays: IEEE f64 quotient (ssdutils.py:290-292)
                if (__ddiv_rn((double)inter, (double)uni) > thr) al[s0 + j] = 0;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    int total = 0;
    for (int q0 = 0; q0 < n; q0 += NMSB_THREADS) {
        const int q = q0 + tid;
        const bool kp = q < n && alive[q];
        const u64 bal = __ballot(kp);
        if (lane == 0) s_wtot[wave] = __popcll(bal);
        __syncthreads();
        int wbase = total, tot = 0;
#pragma unroll
        for (int i = 0; i < NMSB_THREADS / 64; ++i) {
            if (i < wave) wbase += s_wtot[i];
            tot += s_wtot[i];
        }
        if (kp) keep[1 + wbase + __popcll(bal & ((1ull << lane) - 1ull))] = 65535 - (int)(keys[q] & 0xFFFFull);
        total += tot;
        __syncthreads();
    }
    if (tid == 0) keep[0] = total;
}

size_t nms_boxes_ws_bytes(int n, int ngroups) {
    const size_t n2 = pow2_ge(n > 1 ? n : 1);
    return n2 * 8 + ((size_t)(ngroups + 2) * 4 + 15) / 16 * 16 + (size_t)n + 64;
}

void nms_boxes_device(int n, int ngroups, const int* boxes, const float* conf, const int* group, double thr, int* keep, void* ws,
                      hipStream_t s) {
    SSD_REQUIRE(n >= 1 && n <= 65535 && ngroups >= 1 && ngroups <= 65535, "nms_boxes: 1..65535 boxes and groups");
    const int n2 = pow2_ge(n);
    char* base = (char*)ws;
    u64* keys = (u64*)base; base += (size_t)n2 * 8;
    int* gstart = (int*)base; base += ((size_t)(ngroups + 2) * 4 + 15) / 16 * 16;
    unsigned char* alive = (unsigned char*)base;
    hipLaunchKernelGGL(nms_boxes_kernel, dim3(1), dim3(NMSB_THREADS), 0, s, n, n2, ngroups, reinterpret_cast<const int4*>(boxes), conf,
                       group, thr, keys, gstart, alive, keep);
    HIP_OK(hipGetLastError());
}

// =================================================================================
// DetectionOutput: every (anchor, class) pair that reaches the threshold is a candidate
// =================================================================================
// The SSD paper's decode: per class the best nms_top_k candidates, greedy suppression per class, then the best keep_top_k of the
// image across classes.  Two launches, no atomics on memory, no host wait:
//   detout_class_kernel   one workgroup per (image, class), the classes of an image adjacent in launch order (their rows stay
//                         in L2).  The class' column of `pred` is read ONCE into registers (PER values per thread, thread t
//                         holding anchors t*PER .. t*PER+PER-1), so the b*A*C list of keys is never materialised.  With more than
//                         nms_top_k candidates the bit pattern of the k-th largest confidence is found by a bitwise search
//                         over the registers (32 workgroup-wide counts); everything above it and the first (by anchor) k - n_above
//                         values equal to it are compacted by one prefix scan, sorted in LDS (bitonic_desc), decoded (decode_box)
//                         and suppressed (nms_segment).  The survivors go to the class' [nms_top_k] slot of the workspace.
//   detout_merge_kernel   one workgroup per image: the keep_top_k largest keys of its C sorted survivor lists.  The key
//                           conf bits << 32 | (32767 - anchor) << 8 | (127 - class)
//                         is unique in the image and orders by (confidence desc, anchor asc, class asc); the k-th largest key is
//                         found by a bitwise search in which every list answers "how many of my keys are >= t" by bisection.
// Candidates satisfy !(conf < thr) with thr >= 0: confidences are non-negative floats, whose bit patterns order as their
// values.  Negative zero and NaN in the class columns are outside the contract (inputs are softmax outputs); they cannot make
// the kernels leave their bounds.
constexpr int DOUT_MAX_K = 1024;           // nms_top_k and keep_top_k: one LDS slot each

struct DetOutArgs {
    int A, nv, C, B;
    const double* anchors;
    const float* pred;
    float thr;
    int nms_top_k, keep_top_k, out_cap;
    int* cls_count;     // [B][C] survivors of every class
    u64* cls_keys;      // [B][C][nms_top_k] their keys, descending
    int4* cls_box;      // [B][C][nms_top_k] their boxes
    DetectOut out;
};

// sum of v over the workgroup (WAVES waves), the same value in every thread; two barriers
template <int WAVES>
__device__ __forceinline__ int dout_block_sum(int v, int* s_red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) t += s_red[i];
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(t);
}

// The tile stage of tiled DetectionOutput is this kernel with TILE = true: image = the b-th network input of
// the call = tile tp.first + b of the table, the lists are the tiles' [C][nms_top_k] slots (p.cls_* point at tile tp.first), the
// survivor predicate is "not cut by an interior edge" instead of "survived NMS", and a record leaves with its box on the
// picture's 1000 grid and its tile (index inside the picture) in bits 24..31 of the key.
struct DetTileArgs {
    const MergeTile* tiles;     // [n_tiles] the whole table
    const int* img_first;       // [n_images + 1] first tile of every picture
    int first, edge_margin;
};

// NMS = SOFT_LINEAR / SOFT_GAUSSIAN (never with TILE): soft_nms_segment in the place of nms_segment; the picks
// leave in pick order with their decayed keys.
template <int DOUT_THREADS, int PER, bool TILE, int NMS = 0>
__device__ __forceinline__ void detout_class_body(DetOutArgs p, DetTileArgs tp, SoftNmsArgs sp = SoftNmsArgs{}) {
    static_assert(!(TILE && NMS != 0), "the tile stage suppresses nothing");
    constexpr int DOUT_WAVES = DOUT_THREADS / 64;
    __shared__ __attribute__((aligned(16))) u64 skey[DOUT_MAX_K];
    __shared__ int4 sbox[DOUT_MAX_K], snbox[DOUT_MAX_K];
    __shared__ unsigned char alive[DOUT_MAX_K];
    __shared__ int s_red[DOUT_WAVES], s_sc[2][DOUT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x / p.C, c = blockIdx.x - b * p.C;
    const int k = p.nms_top_k;
    const float* col = p.pred + (size_t)b * p.A * p.nv + c;
    const int a0 = tid * PER;
    // the column, all loads in flight together (indices clamped, not predicated); u = 0: no candidate, else conf bits + 1
    float v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j)           // (a 32-bit byte offset from a uniform base: A * nv * 4 < 2^25)
        v[j] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(col) + (unsigned)min(a0 + j, p.A - 1) * (unsigned)p.nv * 4u);
    const int nvalid = p.A - a0;             // this thread's anchors are j < nvalid
    // (the empty asm statements of this kernel pin a value in its register: without them the compiler keeps the lane mask
    // of every comparison of one unrolled loop alive for the next loop that asks the same question -- 2 scalar registers per
    // value, which it then has to park in vector lanes)
    unsigned u[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const bool cand = j < nvalid && !(v[j] < p.thr);         // the argmax path's comparison
        u[j] = cand ? min(__float_as_uint(v[j]), 0xFFFFFFFEu) + 1u : 0u;
        asm volatile("" : "+v"(u[j]));
    }
    int mine = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) mine += u[j] != 0u ? 1 : 0;
    const int n = dout_block_sum<DOUT_WAVES>(mine, s_red);
    // more than k: T = the k-th largest u, the largest t with count(u >= t) >= k, built from the top bit down
    unsigned T = 0u;
    int need_eq = 0;
    if (n > k) {
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned trial = T | (1u << bit);
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j) cnt += u[j] >= trial ? 1 : 0;
            if (dout_block_sum<DOUT_WAVES>(cnt, s_red) >= k) T = trial;
        }
        int above = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) above += u[j] > T ? 1 : 0;
        need_eq = k - dout_block_sum<DOUT_WAVES>(above, s_red);       // >= 1
    }
    // compaction: everything above T from slot 0 on, then the first need_eq values equal to T in anchor order (= thread order)
    int g = 0, e = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        g += u[j] > T ? 1 : 0;
        e += (need_eq > 0 && u[j] == T) ? 1 : 0;
    }
    int gi = g, ei = e;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int tg = __shfl_up(gi, o, 64), te = __shfl_up(ei, o, 64);
        if (lane >= o) { gi += tg; ei += te; }
    }
    if (lane == 63) { s_sc[0][wave] = gi; s_sc[1][wave] = ei; }
    __syncthreads();
    int gbase = 0, ebase = 0, n_above = 0;
#pragma unroll
    for (int w = 0; w < DOUT_WAVES; ++w) {
        if (w < wave) { gbase += s_sc[0][w]; ebase += s_sc[1][w]; }
        n_above += s_sc[0][w];
    }
    const int m = min(n, k);                 // n_above + min(need_eq, equals) == m
    asm volatile("" : "+s"(T));
    int gpos = gbase + gi - g, epos = n_above + ebase + ei - e;
    const u64 low = (u64)(127 - c);
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const u64 key = ((u64)(u[j] - 1u) << 32) | ((u64)(32767 - (a0 + j)) << 8) | low;
        const bool isg = u[j] > T, ise = need_eq > 0 && u[j] == T;
        const int pos = isg ? gpos : epos;
        if ((isg || ise) && pos < m) skey[pos] = key;      // (an equal past the first need_eq has pos >= m)
        gpos += isg ? 1 : 0;
        epos += ise ? 1 : 0;
    }
    const int m2 = next_pow2(m > 1 ? m : 1);
    for (int i = m + tid; i < m2; i += DOUT_THREADS) skey[i] = 0ull;
    __syncthreads();
    bitonic_desc(skey, m2);
    for (int q = tid; q < m; q += DOUT_THREADS) {
        const int a = min(32767 - (int)((skey[q] >> 8) & 0xFFFFull), p.A - 1);
        int bx[4], nb[4];
        decode_box(p.pred + ((size_t)b * p.A + a) * p.nv + (p.nv - 4), p.anchors + (size_t)a * 4, bx);
        if constexpr (TILE) {
            const MergeTile tl = tp.tiles[tp.first + b];
            const int in = tl.interior, mg = tp.edge_margin;      // merge_tiles_kernel's rule, on the tile-grid box
            const bool cut = mg >= 0 && (((in & 1) && bx[0] <= mg) || ((in & 2) && bx[1] >= 999 - mg) || ((in & 4) && bx[2] <= mg) ||
                                         ((in & 8) && bx[3] >= 999 - mg));
            sbox[q] = make_int4(merge_map(bx[0], tl.x0, tl.w, tl.img_w), merge_map(bx[1], tl.x0, tl.w, tl.img_w),
                                merge_map(bx[2], tl.y0, tl.h, tl.img_h), merge_map(bx[3], tl.y0, tl.h, tl.img_h));
            alive[q] = cut ? 0 : 1;
        } else {
            nms_roundtrip(bx, nb);
            sbox[q] = make_int4(bx[0], bx[1], bx[2], bx[3]);
            snbox[q] = make_int4(nb[0], nb[1], nb[2], nb[3]);
            alive[q] = 1;
        }
    }
    __syncthreads();
    if constexpr (NMS != 0) {
        __shared__ __attribute__((aligned(16))) u64 newkey[DOUT_MAX_K];
        __shared__ unsigned short order[DOUT_MAX_K];
        if (wave == 0) {
            const int picks = soft_nms_segment<NMS>(skey, snbox, m, lane, sp, newkey, order);
            if (lane == 0) s_red[0] = picks;
        }
        __syncthreads();
        const int picks = s_red[0];
        const size_t slot = (size_t)blockIdx.x * k;
        for (int i = tid; i < picks; i += DOUT_THREADS) {
            p.cls_keys[slot + i] = newkey[i];
            p.cls_box[slot + i] = sbox[order[i]];
        }
        if (tid == 0) p.cls_count[blockIdx.x] = picks;
        return;
    }
    if constexpr (!TILE) {
        if (wave == 0) nms_segment(snbox, alive, 0, m, lane);
        __syncthreads();
    }
    u64 tile_bits = 0ull;
    if constexpr (TILE) {
        const int g = tp.first + b;
        tile_bits = (u64)(255 - (g - tp.img_first[tp.tiles[g].image])) << 24;
    }
    // survivors, in order, into the class' slot
    const size_t slot = (size_t)blockIdx.x * k;
    int total = 0;
    for (int q0 = 0; q0 < m; q0 += DOUT_THREADS) {
        const int q = q0 + tid;
        const bool keep = q < m && alive[q];
        const u64 bal = __ballot(keep);
        if (lane == 0) s_red[wave] = __popcll(bal);
        __syncthreads();
        int wbase = total, tot = 0;
#pragma unroll
        for (int i = 0; i < DOUT_WAVES; ++i) {
            if (i < wave) wbase += s_red[i];
            tot += s_red[i];
        }
        if (keep) {
            const int o = wbase + __popcll(bal & ((1ull << lane) - 1ull));
            if constexpr (TILE) p.cls_keys[slot + o] = skey[q] | tile_bits;
            else p.cls_keys[slot + o] = skey[q];
            p.cls_box[slot + o] = sbox[q];
        }
        total += tot;
        __syncthreads();
    }
    if (tid == 0) p.cls_count[blockIdx.x] = total;
}

template <int DOUT_THREADS, int PER>
__global__ __launch_bounds__(DOUT_THREADS) void detout_class_kernel(DetOutArgs p) {
    detout_class_body<DOUT_THREADS, PER, false>(p, DetTileArgs{});
}

template <int DOUT_THREADS, int PER, int NMS>
__global__ __launch_bounds__(DOUT_THREADS) void detout_class_soft_kernel(DetOutArgs p, SoftNmsArgs sp) {
    detout_class_body<DOUT_THREADS, PER, false, NMS>(p, DetTileArgs{}, sp);
}

template <int DOUT_THREADS, int PER>
__global__ __launch_bounds__(DOUT_THREADS) void detout_tile_kernel(DetOutArgs p, DetTileArgs tp) {
    detout_class_body<DOUT_THREADS, PER, true>(p, tp);
}

// TILE = true is the picture merge of tiled DetectionOutput: the lists are a picture's classes, the key carries the tile in bits
// 24..31 (so the anchor field is read with 15 bits), `tile_out` receives it, and conf / idx / tile_out may be null.
template <bool TILE>
__device__ __forceinline__ void detout_merge_body(DetOutArgs p, int* tile_out) {
    __shared__ __attribute__((aligned(16))) u64 lkeys[DOUT_MAX_K];
    __shared__ unsigned lvals[DOUT_MAX_K];
    __shared__ int s_off[MRG_NCLS + 1], s_red[MRG_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int C = p.C, k = p.nms_top_k, K = p.keep_top_k;
    const size_t img = (size_t)b * C * k;
    const u64* kc = p.cls_keys + img + (size_t)min(tid, C - 1) * k;       // thread c < C: the list of class c
    const int cnt = tid < C ? min(max(p.cls_count[b * C + tid], 0), k) : 0;
    const int N = dout_block_sum<MRG_WAVES>(cnt, s_red);
    // more than K survivors: T = the K-th largest key.  The number of this list's keys >= T stays inside [lo, hi]: an accepted
    // trial lowers hi, a rejected one (every later trial is smaller) raises lo.
    int lo = 0, hi = cnt;
    if (N > K) {
        u64 T = 0ull;
        for (int bit = 63; bit >= 0; --bit) {
            const u64 trial = T | (1ull << bit);
            int l = lo, h = hi;
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (kc[mid] >= trial) l = mid + 1; else h = mid;
            }
            if (dout_block_sum<MRG_WAVES>(l, s_red) >= K) { T = trial; hi = l; }
            else lo = l;
        }
    }
    const int sel = hi;                       // this list's share of the output
    if (tid < MRG_NCLS) s_off[tid + 1] = sel;
    if (tid == 0) s_off[0] = 0;
    __syncthreads();
    if (tid == 0)
        for (int i = 1; i <= MRG_NCLS; ++i) s_off[i] += s_off[i - 1];
    __syncthreads();
    const int total = min(s_off[MRG_NCLS], K);      // (== s_off[MRG_NCLS]: the keys are unique)
    const int n2 = next_pow2(total > 1 ? total : 1);
    for (int f = tid; f < n2; f += MRG_THREADS) {
        u64 key = 0ull;
        unsigned src = 0u;
        if (f < total) {
            int l = 0, h = MRG_NCLS - 1;      // the list that holds the f-th selected record
            while (l < h) {
                const int mid = (l + h + 1) >> 1;
                if (s_off[mid] <= f) l = mid; else h = mid - 1;
            }
            src = (unsigned)(l * k + (f - s_off[l]));
            key = p.cls_keys[img + src];
        }
        lkeys[f] = key;
        lvals[f] = src;
    }
    __syncthreads();
    merge_sort_desc(lkeys, lvals, n2);
    for (int f = tid; f < total && f < p.out_cap; f += MRG_THREADS) {
        const u64 key = lkeys[f];
        const size_t dst = (size_t)b * p.out_cap + f;
        if constexpr (TILE) {
            if (p.out.conf) p.out.conf[dst] = __uint_as_float((unsigned)(key >> 32));
            p.out.cls[dst] = 127 - (int)(key & 127ull);
            if (p.out.idx) p.out.idx[dst] = 32767 - (int)((key >> 8) & 0x7FFFull);
            if (tile_out) tile_out[dst] = 255 - (int)((key >> 24) & 0xFFull);
        } else {
            p.out.conf[dst] = __uint_as_float((unsigned)(key >> 32));
            p.out.cls[dst] = 127 - (int)(key & 127ull);
            p.out.idx[dst] = 32767 - (int)((key >> 8) & 0xFFFFull);
        }
        const int4 bx = p.cls_box[img + lvals[f]];
        int* ob = p.out.box + dst * 4;      // (four stores: with out_cap = keep_top_k the caller's rows need not be 16-byte aligned)
        ob[0] = bx.x; ob[1] = bx.y; ob[2] = bx.z; ob[3] = bx.w;
    }
    if (tid == 0) p.out.count[b] = total;
}

__global__ __launch_bounds__(MRG_THREADS) void detout_merge_kernel(DetOutArgs p) { detout_merge_body<false>(p, nullptr); }

__global__ __launch_bounds__(MRG_THREADS) void detout_tile_picture_kernel(DetOutArgs p, int* tile_out) {
    detout_merge_body<true>(p, tile_out);
}

// Class merge of tiled DetectionOutput: one workgroup per (picture, class).  Thread t owns the sorted list that tile t of the
// picture wrote for the class; the nms_top_k-th largest key of their union is found as detout_merge_kernel finds its cut (a
// bitwise search over the key, every list answering "how many of my keys are >= trial" by bisection), so the up to
// 256 * nms_top_k records of the picture are never sorted.  The <= nms_top_k selected records are gathered into LDS, sorted,
// suppressed (nms_segment on the picture-grid boxes) and written, in order, to the picture's [C][nms_top_k] slot.
struct DetTileMergeArgs {
    const int* img_first;       // [n_images + 1]
    int C, k;
    const int* tcount; const u64* tkeys; const int4* tbox;      // [n_tiles][C] and [n_tiles][C][k]: the tile stage's lists
    int* pcount; u64* pkeys; int4* pbox;                        // [n_images][C] and [n_images][C][k]
};

// NMS = SOFT_LINEAR / SOFT_GAUSSIAN: soft_nms_segment in the place of nms_segment.  The kernel itself is the
// template (NMS = 0 never reads sp): behind a wrapper the compiler schedules the hard instantiation differently.
template <int NMS>
__global__ __launch_bounds__(MRG_THREADS) void detout_tile_class_kernel(DetTileMergeArgs p, SoftNmsArgs sp) {
    __shared__ __attribute__((aligned(16))) u64 lkeys[DOUT_MAX_K];
    __shared__ unsigned lvals[DOUT_MAX_K];
    __shared__ int4 sbox[DOUT_MAX_K], snbox[DOUT_MAX_K];
    __shared__ unsigned char alive[DOUT_MAX_K];
    __shared__ int s_off[MERGE_MAX_TILES + 1], s_red[MRG_WAVES];
    static_assert(MERGE_MAX_TILES <= MRG_THREADS && DOUT_MAX_K <= 1024, "a thread per list; 10 bits of the payload for the record");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, k = p.k;
    const int img = blockIdx.x / C, c = blockIdx.x - img * C;
    const int T0 = p.img_first[img], nt = p.img_first[img + 1] - T0;      // 1..MERGE_MAX_TILES (checked on the host)
    const size_t mylist = (size_t)(T0 + min(tid, nt - 1)) * C + c;
    const u64* kc = p.tkeys + mylist * k;
    const int cnt = tid < nt ? min(max(p.tcount[mylist], 0), k) : 0;
    const int N = dout_block_sum<MRG_WAVES>(cnt, s_red);
    int lo = 0, hi = cnt;                     // (as in detout_merge_body)
    if (N > k) {
        u64 T = 0ull;
        for (int bit = 63; bit >= 0; --bit) {
            const u64 trial = T | (1ull << bit);
            int l = lo, h = hi;
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (kc[mid] >= trial) l = mid + 1; else h = mid;
            }
            if (dout_block_sum<MRG_WAVES>(l, s_red) >= k) { T = trial; hi = l; }
            else lo = l;
        }
    }
    // exclusive prefix of the lists' shares
    int inc = hi;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_red[wave] = inc;
    __syncthreads();
    int wbase0 = 0;
#pragma unroll
    for (int w = 0; w < MRG_WAVES; ++w)
        if (w < wave) wbase0 += s_red[w];
    if (tid < MERGE_MAX_TILES) s_off[tid + 1] = wbase0 + inc;
    if (tid == 0) s_off[0] = 0;
    __syncthreads();
    const int total = min(s_off[MERGE_MAX_TILES], k);      // (== s_off[MERGE_MAX_TILES]: the keys are unique)
    const int n2 = next_pow2(total > 1 ? total : 1);
    for (int f = tid; f < n2; f += MRG_THREADS) {
        u64 key = 0ull;
        unsigned src = 0u;
        if (f < total) {
            int l = 0, h = MERGE_MAX_TILES - 1;      // the list that holds the f-th selected record
            while (l < h) {
                const int mid = (l + h + 1) >> 1;
                if (s_off[mid] <= f) l = mid; else h = mid - 1;
            }
            const int j = f - s_off[l];
            src = ((unsigned)l << 10) | (unsigned)j;
            key = p.tkeys[((size_t)(T0 + l) * C + c) * k + j];
        }
        lkeys[f] = key;
        lvals[f] = src;
    }
    __syncthreads();
    merge_sort_desc(lkeys, lvals, n2);
    for (int q = tid; q < total; q += MRG_THREADS) {
        const unsigned src = lvals[q];
        const int4 bx = p.tbox[((size_t)(T0 + (int)(src >> 10)) * C + c) * k + (src & 1023u)];
        int o[4] = {bx.x, bx.y, bx.z, bx.w}, nb[4];
        nms_roundtrip(o, nb);
        sbox[q] = bx;
        snbox[q] = make_int4(nb[0], nb[1], nb[2], nb[3]);
        alive[q] = 1;
    }
    __syncthreads();
    if constexpr (NMS != 0) {      //  the picks in pick order, their keys decayed
        __shared__ __attribute__((aligned(16))) u64 newkey[DOUT_MAX_K];
        __shared__ unsigned short order[DOUT_MAX_K];
        if (wave == 0) {
            const int picks = soft_nms_segment<NMS>(lkeys, snbox, total, lane, sp, newkey, order);
            if (lane == 0) s_red[0] = picks;
        }
        __syncthreads();
        const int picks = s_red[0];
        const size_t slot = (size_t)blockIdx.x * k;
        for (int i = tid; i < picks; i += MRG_THREADS) {
            p.pkeys[slot + i] = newkey[i];
            p.pbox[slot + i] = sbox[order[i]];
        }
        if (tid == 0) p.pcount[blockIdx.x] = picks;
        return;
    }
    if (wave == 0) nms_segment(snbox, alive, 0, total, lane);
    __syncthreads();
    const size_t slot = (size_t)blockIdx.x * k;
    int kept = 0;
    for (int q0 = 0; q0 < total; q0 += MRG_THREADS) {
        const int q = q0 + tid;
        const bool keep = q < total && alive[q];
        const u64 bal = __ballot(keep);
        if (lane == 0) s_red[wave] = __popcll(bal);
        __syncthreads();
        int wbase = kept, tot = 0;
#pragma unroll
        for (int i = 0; i < MRG_WAVES; ++i) {
            if (i < wave) wbase += s_red[i];
            tot += s_red[i];
        }
        if (keep) {
            const int o = wbase + __popcll(bal & ((1ull << lane) - 1ull));
            p.pkeys[slot + o] = lkeys[q];
            p.pbox[slot + o] = sbox[q];
        }
        kept += tot;
        __syncthreads();
    }
    if (tid == 0) p.pcount[blockIdx.x] = kept;
}

// The rule alone on one list (ssd_soft_nms_boxes): boxes [n] on the 1000 grid, conf [n] non-negative; the key's anchor field
// is the input index.  One workgroup; order_out / conf_out [n] receive the picks, *n_keep their number.
constexpr int SOFTB_THREADS = 256;

template <int NMS>
__global__ __launch_bounds__(SOFTB_THREADS) void soft_nms_boxes_kernel(int n, const int4* __restrict__ boxes, const float* __restrict__ conf,
                                                                       SoftNmsArgs sp, int* __restrict__ order_out,
                                                                       float* __restrict__ conf_out, int* __restrict__ n_keep) {
    __shared__ __attribute__((aligned(16))) u64 skey[SOFT_MAX], newkey[SOFT_MAX];
    __shared__ int4 snbox[SOFT_MAX];
    __shared__ unsigned short order[SOFT_MAX];
    __shared__ int s_picks;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    n = min(n, SOFT_MAX);
    for (int q = tid; q < n; q += SOFTB_THREADS) {
        const int4 bx = boxes[q];
        int o[4] = {bx.x, bx.y, bx.z, bx.w}, nb[4];
        nms_roundtrip(o, nb);
        snbox[q] = make_int4(nb[0], nb[1], nb[2], nb[3]);
        skey[q] = ((u64)__float_as_uint(conf[q]) << 32) | ((u64)(32767 - q) << 8) | 127ull;
    }
    __syncthreads();
    if (wave == 0) {
        const int picks = soft_nms_segment<NMS>(skey, snbox, n, lane, sp, newkey, order);
        if (lane == 0) s_picks = picks;
    }
    __syncthreads();
    const int picks = s_picks;
    for (int i = tid; i < picks; i += SOFTB_THREADS) {
        order_out[i] = (int)order[i];
        conf_out[i] = __uint_as_float((unsigned)(newkey[i] >> 32));
    }
    if (tid == 0) *n_keep = picks;
}

static size_t align256(size_t n) { return (n + 255) / 256 * 256; }

void detection_output_check(int A, int num_classes, int B, float conf_thr, int nms_top_k, int keep_top_k, int out_cap) {
    SSD_REQUIRE(A >= 1 && A <= 32767, "detection_output: at most 32767 anchors (got %d)", A);
    require_num_classes(num_classes);
    SSD_REQUIRE(B >= 1 && B <= DET_MAX_BATCH, "detection_output: 1..%d images per pass (got %d)", DET_MAX_BATCH, B);
    SSD_REQUIRE(std::isfinite(conf_thr) && conf_thr >= 0.f, "detection_output: the confidence threshold must be finite and >= 0");
    SSD_REQUIRE(nms_top_k >= 1 && nms_top_k <= DOUT_MAX_K, "detection_output: nms_top_k must be in 1..%d (got %d)", DOUT_MAX_K, nms_top_k);
    SSD_REQUIRE(keep_top_k >= 1 && keep_top_k <= DOUT_MAX_K, "detection_output: keep_top_k must be in 1..%d (got %d)", DOUT_MAX_K, keep_top_k);
    SSD_REQUIRE(out_cap >= 1, "detection_output: out_cap must be >= 1");
}

void nms_params_check(const char* who, const NmsParams* nms) {
    SSD_REQUIRE(nms != nullptr, "%s: the nms parameters are null", who);
    SSD_REQUIRE(nms->kind == NMS_HARD || nms->kind == NMS_SOFT_LINEAR || nms->kind == NMS_SOFT_GAUSSIAN,
                "%s: nms kind must be 0 (hard), 1 (soft, linear) or 2 (soft, gaussian) (got %d)", who, nms->kind);
    if (nms->kind == NMS_HARD) return;      // the other fields are not read
    if (nms->kind == NMS_SOFT_LINEAR)
        SSD_REQUIRE(std::isfinite(nms->iou_thr) && nms->iou_thr >= 0.f && nms->iou_thr <= 1.f, "%s: soft nms iou_thr must be finite and in [0, 1]",
                    who);
    if (nms->kind == NMS_SOFT_GAUSSIAN)
        SSD_REQUIRE(std::isfinite(nms->sigma) && nms->sigma > 0.f, "%s: soft nms sigma must be finite and > 0", who);
    SSD_REQUIRE(std::isfinite(nms->min_score) && nms->min_score >= 0.f, "%s: soft nms min_score must be finite and >= 0", who);
}

static SoftNmsArgs soft_args(const NmsParams& nms, int max_picks) {
    return SoftNmsArgs{nms.iou_thr, nms.sigma, nms.min_score + 0.f, max_picks};      // (+ 0.f: a -0.0 min_score compares like +0.0 anyway)
}

size_t detection_output_ws_bytes(int B, int num_classes, int nms_top_k) {
    const size_t lists = (size_t)B * num_classes;
    return align256(lists * 4) + align256(lists * nms_top_k * 8) + lists * nms_top_k * 16;
}

void detection_output(int A, int num_classes, const double* anchors, const float* pred, int B, float conf_thr, int nms_top_k,
                      int keep_top_k, int out_cap, const DetectOut& out, void* ws, size_t ws_bytes, hipStream_t s, const NmsParams& nms) {
    nms_params_check("detection_output", &nms);
    detection_output_check(A, num_classes, B, conf_thr, nms_top_k, keep_top_k, out_cap);
    SSD_REQUIRE(anchors && pred && ws && out.count && out.conf && out.cls && out.idx && out.box, "detection_output: null argument");
    const size_t need = detection_output_ws_bytes(B, num_classes, nms_top_k);
    SSD_REQUIRE(ws_bytes >= need, "detection_output: the workspace holds %zu bytes, %zu are needed", ws_bytes, need);
    const size_t lists = (size_t)B * num_classes;
    DetOutArgs a{};
    a.A = A; a.nv = num_classes + 5; a.C = num_classes; a.B = B; a.anchors = anchors; a.pred = pred; a.thr = conf_thr;
    a.nms_top_k = nms_top_k; a.keep_top_k = keep_top_k; a.out_cap = out_cap; a.out = out;
    char* base = (char*)ws;
    a.cls_count = (int*)base; base += align256(lists * 4);
    a.cls_keys = (u64*)base; base += align256(lists * nms_top_k * 8);
    a.cls_box = (int4*)base;
    {
        ProfScope prof(nms.kind == NMS_HARD ? "detout_class" : "detout_class_soft", 0.0, (double)B * A * a.nv * 4.0, s);
        const dim3 grid((unsigned)lists);
        const SoftNmsArgs sp = soft_args(nms, keep_top_k);
        if (nms.kind == NMS_SOFT_LINEAR) {
            if (A <= 256 * 35) hipLaunchKernelGGL((detout_class_soft_kernel<256, 35, SOFT_LINEAR>), grid, dim3(256), 0, s, a, sp);
            else if (A <= 512 * 48) hipLaunchKernelGGL((detout_class_soft_kernel<512, 48, SOFT_LINEAR>), grid, dim3(512), 0, s, a, sp);
            else hipLaunchKernelGGL((detout_class_soft_kernel<512, 64, SOFT_LINEAR>), grid, dim3(512), 0, s, a, sp);
        } else if (nms.kind == NMS_SOFT_GAUSSIAN) {
            if (A <= 256 * 35) hipLaunchKernelGGL((detout_class_soft_kernel<256, 35, SOFT_GAUSSIAN>), grid, dim3(256), 0, s, a, sp);
            else if (A <= 512 * 48) hipLaunchKernelGGL((detout_class_soft_kernel<512, 48, SOFT_GAUSSIAN>), grid, dim3(512), 0, s, a, sp);
            else hipLaunchKernelGGL((detout_class_soft_kernel<512, 64, SOFT_GAUSSIAN>), grid, dim3(512), 0, s, a, sp);
        } else if (A <= 256 * 35) hipLaunchKernelGGL((detout_class_kernel<256, 35>), grid, dim3(256), 0, s, a);     // vgg300: 8732
        else if (A <= 512 * 48) hipLaunchKernelGGL((detout_class_kernel<512, 48>), grid, dim3(512), 0, s, a);       // vgg512: 24564
        else hipLaunchKernelGGL((detout_class_kernel<512, 64>), grid, dim3(512), 0, s, a);
    }
    {
        ProfScope prof("detout_merge", 0.0, 0.0, s);
        hipLaunchKernelGGL(detout_merge_kernel, dim3(B), dim3(MRG_THREADS), 0, s, a);
    }
    HIP_OK(hipGetLastError());
}

// =================================================================================
// tiled DetectionOutput: every tile decoded per class, one NMS per class over the picture's tiles
// =================================================================================
// workspace: the tile table and img_first, then the tile lists (count, key, box per (tile, class)) and the picture lists
// (the same per (picture, class)); detout_tiles_add and detout_tiles_merge carve it alike from (n_tiles, n_images, C, k).
struct DetTilesWs {
    MergeTile* tiles; int* img_first;
    int* tcount; u64* tkeys; int4* tbox;
    int* pcount; u64* pkeys; int4* pbox;
    size_t head_ints, bytes;
};

static DetTilesWs detout_tiles_carve(void* ws, int n_tiles, int n_images, int C, int k) {
    DetTilesWs w{};
    char* base = (char*)ws;
    const size_t tl = (size_t)n_tiles * C, pl = (size_t)n_images * C;
    w.head_ints = (size_t)n_tiles * 8 + (size_t)n_images + 1;
    w.tiles = (MergeTile*)base; w.img_first = (int*)base + (size_t)n_tiles * 8; base += align256(w.head_ints * 4);
    w.tcount = (int*)base; base += align256(tl * 4);
    w.tkeys = (u64*)base; base += align256(tl * k * 8);
    w.tbox = (int4*)base; base += align256(tl * k * 16);
    w.pcount = (int*)base; base += align256(pl * 4);
    w.pkeys = (u64*)base; base += align256(pl * k * 8);
    w.pbox = (int4*)base; base += align256(pl * k * 16);
    w.bytes = (size_t)(base - (char*)ws);
    return w;
}

// every limit of the tile table; fills the head that goes to the device: the tiles, then img_first [n_images + 1]
static void detout_tiles_plan(const char* who, const MergeTile* tiles, int n_tiles, int n_images, std::vector<int>& head) {
    SSD_REQUIRE(tiles != nullptr, "%s: null argument", who);
    SSD_REQUIRE(n_tiles >= 1 && n_tiles <= DET_MAX_BATCH, "%s: 1..%d tiles (got %d)", who, DET_MAX_BATCH, n_tiles);
    SSD_REQUIRE(n_images >= 1 && n_images <= n_tiles, "%s: 1..n_tiles pictures (got %d for %d tiles)", who, n_images, n_tiles);
    SSD_REQUIRE(tiles[0].image == 0 && tiles[n_tiles - 1].image == n_images - 1,
                "%s: image indices must ascend from 0 to n_images - 1 = %d (first %d, last %d)", who, n_images - 1, tiles[0].image,
                tiles[n_tiles - 1].image);
    head.assign((size_t)n_tiles * 8 + (size_t)n_images + 1, 0);
    MergeTile* ht = reinterpret_cast<MergeTile*>(head.data());
    int* first = head.data() + (size_t)n_tiles * 8;
    for (int t = 0, img = -1; t < n_tiles; ++t) {
        const MergeTile& tl = tiles[t];
        const int im = tl.image;
        SSD_REQUIRE(im == img || im == img + 1, "%s: image indices must ascend without gaps (tile %d: image %d after %d)", who, t, im, img);
        SSD_REQUIRE(tl.img_w >= 1 && tl.img_h >= 1 && tl.img_w <= MERGE_MAX_SIDE && tl.img_h <= MERGE_MAX_SIDE,
                    "%s: tile %d: picture of %d x %d outside 1..%d", who, t, tl.img_w, tl.img_h, MERGE_MAX_SIDE);
        SSD_REQUIRE(tl.x0 >= 0 && tl.y0 >= 0 && tl.w >= 1 && tl.h >= 1 && tl.x0 <= tl.img_w - tl.w && tl.y0 <= tl.img_h - tl.h,
                    "%s: tile %d (%d, %d, %d x %d) leaves its %d x %d picture", who, t, tl.x0, tl.y0, tl.w, tl.h, tl.img_w, tl.img_h);
        SSD_REQUIRE(tl.interior >= 0 && tl.interior <= 15, "%s: tile %d: interior = %d outside 0..15", who, t, tl.interior);
        if (im != img) {
            img = im;
            first[img] = t;
        } else {
            SSD_REQUIRE(tl.img_w == tiles[t - 1].img_w && tl.img_h == tiles[t - 1].img_h,
                        "%s: tile %d: the tiles of picture %d disagree about its size", who, t, im);
        }
        ht[t] = tl;
    }
    first[n_images] = n_tiles;
    for (int i = 0; i < n_images; ++i)
        SSD_REQUIRE(first[i + 1] - first[i] <= MERGE_MAX_TILES, "%s: picture %d has %d tiles, at most %d", who, i, first[i + 1] - first[i],
                    MERGE_MAX_TILES);
}

static void detout_tiles_sizes(const char* who, int A, int num_classes, int nms_top_k) {
    SSD_REQUIRE(A >= 1 && A <= 32767, "%s: at most 32767 anchors (got %d)", who, A);
    SSD_REQUIRE(num_classes >= 1 && num_classes <= MAX_CLASSES, "%s: num_classes must be in 1..%d (got %d)", who, MAX_CLASSES, num_classes);
    SSD_REQUIRE(nms_top_k >= 1 && nms_top_k <= DOUT_MAX_K, "%s: nms_top_k must be in 1..%d (got %d)", who, DOUT_MAX_K, nms_top_k);
}

size_t detout_tiles_ws_bytes(int A, int num_classes, int n_tiles, int n_images, int nms_top_k) {
    const char* who = "detout_tiles_ws_bytes";
    detout_tiles_sizes(who, A, num_classes, nms_top_k);
    SSD_REQUIRE(n_tiles >= 1 && n_tiles <= DET_MAX_BATCH, "%s: 1..%d tiles (got %d)", who, DET_MAX_BATCH, n_tiles);
    SSD_REQUIRE(n_images >= 1 && n_images <= n_tiles, "%s: 1..n_tiles pictures (got %d for %d tiles)", who, n_images, n_tiles);
    return detout_tiles_carve(nullptr, n_tiles, n_images, num_classes, nms_top_k).bytes;
}

void detout_tiles_add_check(const char* who, int A, int num_classes, const MergeTile* tiles, int n_tiles, int first, int b, float conf_thr,
                            int nms_top_k, std::vector<int>& head) {
    detout_tiles_sizes(who, A, num_classes, nms_top_k);
    SSD_REQUIRE(std::isfinite(conf_thr) && conf_thr >= 0.f, "%s: the confidence threshold must be finite and >= 0", who);
    SSD_REQUIRE(tiles != nullptr && n_tiles >= 1, "%s: at least one tile", who);
    detout_tiles_plan(who, tiles, n_tiles, tiles[n_tiles - 1].image + 1, head);
    SSD_REQUIRE(first >= 0 && b >= 1 && b <= n_tiles - first, "%s: tiles %d .. %d + %d outside the %d tiles of the table", who, first, first, b,
                n_tiles);
}

void detout_tiles_merge_check(const char* who, int num_classes, const MergeTile* tiles, int n_tiles, int n_images, int nms_top_k,
                              int keep_top_k, int out_cap, std::vector<int>& head) {
    detout_tiles_sizes(who, 1, num_classes, nms_top_k);
    SSD_REQUIRE(keep_top_k >= 1 && keep_top_k <= DOUT_MAX_K, "%s: keep_top_k must be in 1..%d (got %d)", who, DOUT_MAX_K, keep_top_k);
    SSD_REQUIRE(out_cap >= 1, "%s: out_cap must be >= 1 (got %d)", who, out_cap);
    detout_tiles_plan(who, tiles, n_tiles, n_images, head);
}

static void detout_tiles_ws_check(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    SSD_REQUIRE(ws != nullptr && ((uintptr_t)ws & 15) == 0, "%s: the workspace must be a 16-byte aligned device pointer", who);
    SSD_REQUIRE(ws_bytes >= need, "%s: the workspace holds %zu bytes, %zu are needed", who, ws_bytes, need);
}

void detout_tiles_add(const char* who, int A, int num_classes, const double* anchors, const float* pred, const MergeTile* tiles,
                      int n_tiles, int first, int b, float conf_thr, int nms_top_k, int edge_margin, void* ws, size_t ws_bytes,
                      hipStream_t s) {
    std::vector<int> head;
    detout_tiles_add_check(who, A, num_classes, tiles, n_tiles, first, b, conf_thr, nms_top_k, head);
    SSD_REQUIRE(anchors && pred, "%s: null argument", who);
    const int n_images = tiles[n_tiles - 1].image + 1;
    const DetTilesWs w = detout_tiles_carve(ws, n_tiles, n_images, num_classes, nms_top_k);
    detout_tiles_ws_check(who, ws, ws_bytes, w.bytes);
    HIP_OK(hipMemcpyAsync(ws, head.data(), head.size() * sizeof(int), hipMemcpyHostToDevice, s));      // (pageable: copied by the call)
    const size_t l0 = (size_t)first * num_classes;
    DetOutArgs a{};
    a.A = A; a.nv = num_classes + 5; a.C = num_classes; a.B = b; a.anchors = anchors; a.pred = pred; a.thr = conf_thr;
    a.nms_top_k = nms_top_k;
    a.cls_count = w.tcount + l0; a.cls_keys = w.tkeys + l0 * nms_top_k; a.cls_box = w.tbox + l0 * nms_top_k;
    DetTileArgs t{w.tiles, w.img_first, first, edge_margin};
    {
        ProfScope prof("detout_tile", 0.0, (double)b * A * a.nv * 4.0, s);
        const dim3 grid((unsigned)((size_t)b * num_classes));
        if (A <= 256 * 35) hipLaunchKernelGGL((detout_tile_kernel<256, 35>), grid, dim3(256), 0, s, a, t);
        else if (A <= 512 * 48) hipLaunchKernelGGL((detout_tile_kernel<512, 48>), grid, dim3(512), 0, s, a, t);
        else hipLaunchKernelGGL((detout_tile_kernel<512, 64>), grid, dim3(512), 0, s, a, t);
    }
    HIP_OK(hipGetLastError());
}

void detout_tiles_merge(const char* who, int num_classes, const MergeTile* tiles, int n_tiles, int n_images, int nms_top_k, int keep_top_k,
                        int out_cap, int* count_out, float* conf_out, int* cls_out, int* idx_out, int* tile_out, int* box_out, void* ws,
                        size_t ws_bytes, hipStream_t s, const NmsParams& nms) {
    nms_params_check(who, &nms);
    std::vector<int> head;
    detout_tiles_merge_check(who, num_classes, tiles, n_tiles, n_images, nms_top_k, keep_top_k, out_cap, head);
    SSD_REQUIRE(count_out && cls_out && box_out, "%s: null argument", who);
    const DetTilesWs w = detout_tiles_carve(ws, n_tiles, n_images, num_classes, nms_top_k);
    detout_tiles_ws_check(who, ws, ws_bytes, w.bytes);
    HIP_OK(hipMemcpyAsync(ws, head.data(), head.size() * sizeof(int), hipMemcpyHostToDevice, s));      // (pageable: copied by the call)
    DetTileMergeArgs m{};
    m.img_first = w.img_first; m.C = num_classes; m.k = nms_top_k;
    m.tcount = w.tcount; m.tkeys = w.tkeys; m.tbox = w.tbox; m.pcount = w.pcount; m.pkeys = w.pkeys; m.pbox = w.pbox;
    {
        ProfScope prof(nms.kind == NMS_HARD ? "detout_tile_class" : "detout_tile_class_soft", 0.0, 0.0, s);
        const dim3 grid((unsigned)((size_t)n_images * num_classes));
        const SoftNmsArgs sp = soft_args(nms, keep_top_k);
        if (nms.kind == NMS_SOFT_LINEAR) hipLaunchKernelGGL(detout_tile_class_kernel<SOFT_LINEAR>, grid, dim3(MRG_THREADS), 0, s, m, sp);
        else if (nms.kind == NMS_SOFT_GAUSSIAN) hipLaunchKernelGGL(detout_tile_class_kernel<SOFT_GAUSSIAN>, grid, dim3(MRG_THREADS), 0, s, m, sp);
        else hipLaunchKernelGGL(detout_tile_class_kernel<0>, grid, dim3(MRG_THREADS), 0, s, m, sp);
    }
    DetOutArgs a{};
    a.C = num_classes; a.B = n_images; a.nms_top_k = nms_top_k; a.keep_top_k = keep_top_k; a.out_cap = out_cap;
    a.cls_count = w.pcount; a.cls_keys = w.pkeys; a.cls_box = w.pbox;
    a.out = DetectOut{count_out, conf_out, cls_out, idx_out, box_out};
    {
        ProfScope prof("detout_tile_picture", 0.0, 0.0, s);
        hipLaunchKernelGGL(detout_tile_picture_kernel, dim3(n_images), dim3(MRG_THREADS), 0, s, a, tile_out);
    }
    HIP_OK(hipGetLastError());
}

// one list through soft_nms_segment; every pointer in device memory, n in 1..1024, nms.kind soft (checked by the caller)
void soft_nms_boxes_device(int n, const int* boxes, const float* conf, const NmsParams& nms, int* order_out, float* conf_out, int* n_keep,
                           hipStream_t s) {
    SSD_REQUIRE(n >= 1 && n <= SOFT_MAX, "soft_nms_boxes: 1..%d boxes (got %d)", SOFT_MAX, n);
    SSD_REQUIRE(nms.kind == NMS_SOFT_LINEAR || nms.kind == NMS_SOFT_GAUSSIAN, "soft_nms_boxes: a soft nms kind (got %d)", nms.kind);
    const SoftNmsArgs sp = soft_args(nms, n);
    const int4* b4 = reinterpret_cast<const int4*>(boxes);
    if (nms.kind == NMS_SOFT_LINEAR)
        hipLaunchKernelGGL(soft_nms_boxes_kernel<SOFT_LINEAR>, dim3(1), dim3(SOFTB_THREADS), 0, s, n, b4, conf, sp, order_out, conf_out, n_keep);
    else
        hipLaunchKernelGGL(soft_nms_boxes_kernel<SOFT_GAUSSIAN>, dim3(1), dim3(SOFTB_THREADS), 0, s, n, b4, conf, sp, order_out, conf_out, n_keep);
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
