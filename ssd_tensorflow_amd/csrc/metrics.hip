// Average precision per class on gfx950: the reference's VOC07 11-point form (average_precision.py:84-176), the devkit's VOC07
// with difficult objects, and the VOC2010+ all-point area; and the accumulator that keeps a run's detections in HBM.
// Three kernels per computation:
//   count  one workgroup per class: its detections, its ground truth, its unflagged ground truth (npos).  The host turns the
//          counts into offsets: the sort keys of class k take pow2(n_k) slots, not pow2(n_det).
//   sort   one workgroup per class: compact the class's detections into keys, bitonic sort by confidence (L2 resident).
//   walk   one wave per (class, IoU threshold): ONE lane walks the sorted detections -- the greedy matching of a detection
//          against the still-unmatched ground truth of its image is inherently sequential -- with matched bytes of its own, so
//          the walks of a threshold list run side by side.
// COCO's box evaluation (AP / AR over thresholds, area ranges and detection caps) reuses count and sort and has a walk of its
// own, one wave per class with the combinations as lanes: see "COCO" below.
// All arithmetic in IEEE f64 with explicit round-to-nearest operations: bit-exact with numpy.
#include "metrics.h"
#include "boxmath.h"
#include <climits>
#include <numeric>

namespace ssd {

typedef unsigned long long u64;

struct APArgs {
    APInput in;
    int protocol, n_thr;
    double minoverlap[AP_MAX_THRESHOLDS];
    int* counts;               // [3][ncls]: detections, ground truth, unflagged ground truth
    const long long* koff;     // [ncls] first key of the class
    const long long* toff;     // [ncls] first true-positive slot of the class (VOC12)
    long long tp_stride;       // true-positive slots per threshold
    u64* keys;
    unsigned char* matched;    // [n_thr][n_gt], zeroed
    double* tp_prec;           // [n_thr][tp_stride] (VOC12)
    double* ap;                // [n_thr][ncls]
    int* present;              // [ncls]: 1 if the class is part of the mAP
};

__device__ static int block_sum(int c, int* s_w) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __syncthreads();
    if (lane == 0) s_w[wv] = c;
    __syncthreads();
    return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(256) void ap_count_kernel(APArgs p) {
    __shared__ int s_w[4];
    const int k = blockIdx.x, tid = threadIdx.x;
    int nd = 0, ng = 0, np = 0;
    for (int d = tid; d < p.in.n_det; d += 256) nd += p.in.det_cls[d] == k;
    for (int g = tid; g < p.in.n_gt; g += 256) {
        const bool mine = p.in.gt_cls[g] == k;
        ng += mine;
        np += mine && !p.in.gt_flags[g];
    }
    nd = block_sum(nd, s_w);
    ng = block_sum(ng, s_w);
    np = block_sum(np, s_w);
    if (tid == 0) {
        p.counts[k] = nd;
        p.counts[p.in.ncls + k] = ng;
        p.counts[2 * p.in.ncls + k] = np;
    }
}

__device__ static void bitonic_desc_u64(u64* keys, int n2) {
    for (int k = 2; k <= n2; k <<= 1)
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

// the class's denominator: every ground-truth box for the reference's protocol, the unflagged ones for the devkit's
__device__ static int ap_denominator(const APArgs& p, int k) { return p.counts[(p.protocol == AP_REFERENCE ? 1 : 2) * p.in.ncls + k]; }

__global__ __launch_bounds__(256) void ap_sort_kernel(APArgs p) {
    __shared__ int s_w[4];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (ap_denominator(p, k) == 0) return;
    u64* keys = p.keys + p.koff[k];
    // ---- this class's detections: key = order-preserving confidence bits << 32 | ~index --------
    int n = 0;
    for (int d0 = 0; d0 < p.in.n_det; d0 += 256) {
        const int d = d0 + tid;
        const bool mine = d < p.in.n_det && p.in.det_cls[d] == k;
        const u64 bal = __ballot(mine);
        if (lane == 0) s_w[wv] = __popcll(bal);
        __syncthreads();
        int base = n, tot = 0;
        for (int i = 0; i < 4; ++i) { if (i < wv) base += s_w[i]; tot += s_w[i]; }
        if (mine) {
            unsigned u = __float_as_uint(p.in.det_conf[d]);
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
            keys[base + __popcll(bal & ((1ull << lane) - 1ull))] = ((u64)u << 32) | (u64)(0xFFFFFFFFu - (unsigned)d);
        }
        n += tot;
        __syncthreads();
    }
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = n + tid; i < n2; i += 256) keys[i] = 0ull;
    __syncthreads();
    bitonic_desc_u64(keys, n2);
}

__global__ __launch_bounds__(64) void ap_walk_kernel(APArgs p) {
    if (threadIdx.x != 0) return;
    const int k = blockIdx.x, t = blockIdx.y, ncls = p.in.ncls, n_gt = p.in.n_gt;
    const int count = ap_denominator(p, k);
    if (t == 0) p.present[k] = count > 0;
    if (count == 0) { p.ap[t * ncls + k] = 0.0; return; }
    const int n = p.counts[k];
    const u64* keys = p.keys + p.koff[k];
    const bool devkit = p.protocol != AP_REFERENCE, area = p.protocol == AP_VOC12;
    const double minoverlap = p.minoverlap[t];
    unsigned char* matched = p.matched + (size_t)t * (n_gt > 0 ? n_gt : 1);
    double* tp_prec = area ? p.tp_prec + (size_t)t * p.tp_stride + p.toff[k] : nullptr;
    const float* det_box = p.in.det_box;
    const double* gt_box = p.in.gt_box;
    // ---- greedy matching in confidence order (average_precision.py:130-161; VOCevaldet.m with difficult objects) ----------
    double tp = 0.0, fp = 0.0, best[11];
    bool any[11];
    int ntp = 0;
    for (int j = 0; j < 11; ++j) { best[j] = 0.0; any[j] = false; }
    for (int i = 0; i < n; ++i) {
        const int d = (int)(0xFFFFFFFFu - (unsigned)(keys[i] & 0xFFFFFFFFull));
        const int s = p.in.det_sample[d];
        int lo = 0, hi = n_gt;                       // first ground-truth row of sample s
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (p.in.gt_sample[mid] < s) lo = mid + 1; else hi = mid; }
        const double b0 = det_box[(size_t)d * 4], b1 = det_box[(size_t)d * 4 + 1], b2 = det_box[(size_t)d * 4 + 2], b3 = det_box[(size_t)d * 4 + 3];
        const double areab = __dmul_rn(__dadd_rn(__dsub_rn(b1, b0), 1.0), __dadd_rn(__dsub_rn(b3, b2), 1.0));
        int arg = -1;
        double iou_max = 0.0;
        for (int g = lo; g < n_gt && p.in.gt_sample[g] == s; ++g) {
            if (p.in.gt_cls[g] != k) continue;
            const double a0 = gt_box[(size_t)g * 4], a1 = gt_box[(size_t)g * 4 + 1], a2 = gt_box[(size_t)g * 4 + 2], a3 = gt_box[(size_t)g * 4 + 3];
            const double areaa = __dmul_rn(__dadd_rn(__dsub_rn(a1, a0), 1.0), __dadd_rn(__dsub_rn(a3, a2), 1.0));
            const double w = fmax(0.0, __dadd_rn(__dsub_rn(fmin(b1, a1), fmax(b0, a0)), 1.0));
            const double h = fmax(0.0, __dadd_rn(__dsub_rn(fmin(b3, a3), fmax(b2, a2)), 1.0));
            const double inter = __dmul_rn(w, h);
            const double iou = __ddiv_rn(inter, __dsub_rn(__dadd_rn(areab, areaa), inter));
            if (arg < 0 || iou > iou_max) { iou_max = iou; arg = g; }    // np.argmax: first maximum
        }
        bool hit = false;
        if (arg < 0 || iou_max < minoverlap) fp += 1.0;
        else if (devkit && p.in.gt_flags[arg]) continue;                 // a difficult object: the detection counts neither way
        else if (matched[arg]) fp += 1.0;
        else { tp += 1.0; matched[arg] = 1; hit = true; }
        const double recall = __ddiv_rn(tp, (double)count);
        const double prec = __ddiv_rn(tp, __dadd_rn(tp, fp));
        if (area) {
            // Only true positives are kept: recall moves only there, and a false positive's precision never exceeds that of
            // the counted point before it (same tp, larger tp + fp; a correctly rounded quotient is monotonic), so the
            // devkit's maximum over all later points is the maximum over the later true positives.
            if (hit) tp_prec[ntp++] = prec;
            continue;
        }
        for (int j = 0; j < 11; ++j)
            if (recall >= __dmul_rn((double)j, 0.1)) {                     // np.arange(0, 1.1, 0.1)[j]
                if (!any[j] || prec > best[j]) best[j] = prec;
                any[j] = true;
            }
    }
    double ap = 0.0;
    if (area) {
        // VOCevaldet.m / voc_eval: mrec = [0, recall, 1], mpre = [0, precision, 0], mpre made non-increasing from the back, then the
        // sum over ascending i with mrec[i+1] != mrec[i] of (mrec[i+1] - mrec[i]) * mpre[i+1].  The closing term is (1 - r) * 0.
        double m = 0.0;
        for (int i = ntp - 1; i >= 0; --i) {
            if (tp_prec[i] > m) m = tp_prec[i];
            tp_prec[i] = m;
        }
        double prev = 0.0;
        for (int i = 0; i < ntp; ++i) {
            const double rec = __ddiv_rn((double)(i + 1), (double)count);
            ap = __dadd_rn(ap, __dmul_rn(__dsub_rn(rec, prev), tp_prec[i]));
            prev = rec;
        }
    } else {
        for (int j = 0; j < 11; ++j)
            if (any[j]) ap = __dadd_rn(ap, best[j]);
        ap = __ddiv_rn(ap, 11.0);
    }
    p.ap[t * ncls + k] = ap;
}

// HIP events around the count, sort and walk stages of a computation, while ap_kernel_times has switched them on (measurements).
// The switch and the last times are process-wide and unguarded: for a tool that computes from one thread.
static bool g_stage_timing = false;
static double g_stage_ms[3] = {0.0, 0.0, 0.0};

struct StageTimer {
    hipStream_t s;
    bool on;
    hipEvent_t ev[5] = {};
    explicit StageTimer(hipStream_t stream) : s(stream), on(g_stage_timing) {
        for (int i = 0; on && i < 5; ++i) HIP_OK(hipEventCreate(&ev[i]));
    }
    ~StageTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    void mark(int i) { if (on) HIP_OK(hipEventRecord(ev[i], s)); }      // 0 | count | 1 ... 2 | sort | 3 | walk | 4
    void finish() {                                                      // (after the stream has been waited for)
        if (!on) return;
        const int from[3] = {0, 2, 3};
        for (int i = 0; i < 3; ++i) {
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, ev[from[i]], ev[from[i] + 1]));
            g_stage_ms[i] = ms;
        }
    }
};

void ap_kernel_times(int enable, double* ms_out) {
    if (ms_out) for (int i = 0; i < 3; ++i) ms_out[i] = g_stage_ms[i];
    g_stage_timing = enable != 0;
}

static long long pow2_at_least(long long n) {
    long long n2 = 1;
    while (n2 < n) n2 <<= 1;
    return n2;
}

void average_precision_run(const APInput& in, int protocol, int n_thr, const double* minoverlaps, double* ap_out, int* present_out,
                           hipStream_t s) {
    require_num_classes(in.ncls);
    SSD_REQUIRE(protocol >= AP_REFERENCE && protocol <= AP_VOC12, "AP protocol must be 0 (reference), 1 (voc07) or 2 (voc12), got %d", protocol);
    SSD_REQUIRE(n_thr >= 1 && n_thr <= AP_MAX_THRESHOLDS && minoverlaps, "1..%d IoU thresholds (got %d)", AP_MAX_THRESHOLDS, n_thr);
    SSD_REQUIRE(in.n_det >= 0 && in.n_gt >= 0 && ap_out && present_out, "bad sizes");
    const int ncls = in.ncls;
    APArgs a{};
    a.in = in;
    a.protocol = protocol;
    a.n_thr = n_thr;
    for (int t = 0; t < n_thr; ++t) a.minoverlap[t] = minoverlaps[t];
    const size_t ng = in.n_gt ? in.n_gt : 1;
    DevBuf counts((size_t)ncls * 12), offs((size_t)ncls * 16), matched(ng * n_thr), ap((size_t)n_thr * ncls * 8), present((size_t)ncls * 4);
    a.counts = counts.as<int>();
    StageTimer timer(s);
    timer.mark(0);
    hipLaunchKernelGGL(ap_count_kernel, dim3(ncls), dim3(256), 0, s, a);
    HIP_OK(hipGetLastError());
    timer.mark(1);
    std::vector<int> h_counts((size_t)ncls * 3);
    HIP_OK(hipMemcpyAsync(h_counts.data(), counts.p, h_counts.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    std::vector<long long> h_offs((size_t)ncls * 2);
    long long nkeys = 0, ntp = 0;
    for (int k = 0; k < ncls; ++k) {
        h_offs[k] = nkeys;
        h_offs[ncls + k] = ntp;
        nkeys += pow2_at_least(h_counts[k]);
        ntp += h_counts[2 * ncls + k];
    }
    DevBuf keys((size_t)nkeys * 8), tp_prec(protocol == AP_VOC12 ? (size_t)ntp * n_thr * 8 : 0);
    HIP_OK(hipMemcpyAsync(offs.p, h_offs.data(), h_offs.size() * 8, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemsetAsync(matched.p, 0, ng * n_thr, s));
    a.koff = offs.as<long long>();
    a.toff = offs.as<long long>() + ncls;
    a.tp_stride = ntp;
    a.keys = keys.as<u64>();
    a.matched = matched.as<unsigned char>();
    a.tp_prec = tp_prec.as<double>();
    a.ap = ap.as<double>();
    a.present = present.as<int>();
    timer.mark(2);
    hipLaunchKernelGGL(ap_sort_kernel, dim3(ncls), dim3(256), 0, s, a);
    HIP_OK(hipGetLastError());
    timer.mark(3);
    hipLaunchKernelGGL(ap_walk_kernel, dim3(ncls, n_thr), dim3(64), 0, s, a);
    HIP_OK(hipGetLastError());
    timer.mark(4);
    HIP_OK(hipMemcpyAsync(ap_out, ap.p, (size_t)n_thr * ncls * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(present_out, present.p, (size_t)ncls * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    timer.finish();
}

// ------------------------------------------------------------------------------------------------------------------- COCO
// COCO's box evaluation (include/ssdvgg_hip.h, "COCO box evaluation").  ap_count_kernel and ap_sort_kernel as above; then
//   npig   one workgroup per class: its unflagged ground truth inside each of the four area ranges.
//   walk   one WAVE per class, one LANE per (IoU threshold, area range, maxDet) combination -- at most 10 x (4 + 2) = 60.  All
//          combinations walk the same detections against the same boxes and differ only in their matched state, so the
//          control flow is the wave's: the detection, its rank in its image (one counter per sample, kept by lane 0), its
//          image's boxes of the class and their IoUs (each computed by ONE lane, shared through LDS) are common; a lane owns
//          its matched bytes, its tp / fp counts and its true-positive precisions, and ends with the 101-point sampling.
constexpr int COCO_MAX_DET = 100;

struct COCOArgs {
    COCOInput c;
    int n_thr, n_combo;                // lanes in use: 6 * n_thr
    double thr[AP_MAX_THRESHOLDS];     // min(t, 1 - 1e-10)
    double tmin;                       // the smallest of them: a box below it matches in no lane
    const int* counts;                 // ap_count_kernel's [3][ncls]
    int* npig;                         // [4][ncls]
    const long long* koff;             // [ncls] first key of the class
    const long long* toff;             // [ncls] first true-positive row of the class (a row = 64 lanes)
    const u64* keys;
    unsigned char* matched;            // [n_gt][64], zeroed
    unsigned char* rank;               // [ncls][n_samples], zeroed: detections of the (image, class) seen so far, up to 100
    double* tp_prec;                   // [rows][64]
    double* ap;                        // [4][n_thr][ncls]
    double* ar;                        // [6][n_thr][ncls]
    int* present;                      // [4][ncls]
};

__device__ static double coco_area_lo(int a) { return a == 2 ? 1024.0 : (a == 3 ? 9216.0 : 0.0); }
__device__ static double coco_area_hi(int a) { return a == 1 ? 1024.0 : (a == 2 ? 9216.0 : 1e10); }

__global__ __launch_bounds__(256) void coco_npig_kernel(COCOArgs p) {
    __shared__ int s_w[4];
    const int k = blockIdx.x, tid = threadIdx.x;
    int n[COCO_AREAS] = {0, 0, 0, 0};
    for (int g = tid; g < p.c.in.n_gt; g += 256) {
        if (p.c.in.gt_cls[g] != k || p.c.in.gt_flags[g]) continue;
        const double area = p.c.gt_area[g];
        for (int a = 0; a < COCO_AREAS; ++a) n[a] += !(area < coco_area_lo(a) || area > coco_area_hi(a));
    }
    for (int a = 0; a < COCO_AREAS; ++a) {
        const int v = block_sum(n[a], s_w);
        if (tid == 0) p.npig[a * p.c.in.ncls + k] = v;
    }
}

__global__ __launch_bounds__(64) void coco_walk_kernel(COCOArgs p) {
    __shared__ int s_g[64];                // the image's boxes of the class (a chunk of 64 rows of the image): row,
    __shared__ double s_iou[64];           // IoU with the detection,
    __shared__ unsigned char s_fl[64];     // bit a = ignored under area range a, bit 4 = crowd
    const int k = blockIdx.x, lane = threadIdx.x, ncls = p.c.in.ncls;
    const bool live = lane < p.n_combo;
    const int grp = live ? lane / p.n_thr : 0, t = live ? lane % p.n_thr : 0;
    const int a = grp < COCO_AREAS ? grp : 0, maxdet = grp == 4 ? 1 : (grp == 5 ? 10 : COCO_MAX_DET);
    if (lane < COCO_AREAS) p.present[lane * ncls + k] = p.npig[lane * ncls + k] > 0;
    const int npos = p.counts[2 * ncls + k], npig = p.npig[a * ncls + k];
    double* ap_out = grp < COCO_AREAS ? p.ap + ((size_t)grp * p.n_thr + t) * ncls + k : nullptr;
    double* ar_out = p.ar + ((size_t)grp * p.n_thr + t) * ncls + k;
    if (npos == 0) {                       // (the wave's: no unflagged box, the class is present under no range; nothing was sorted)
        if (live) { *ar_out = -1.0; if (ap_out) *ap_out = -1.0; }
        return;
    }
    const int n = p.counts[k];
    const u64* keys = p.keys + p.koff[k];
    double* tpp = p.tp_prec + (size_t)p.toff[k] * 64 + lane;
    unsigned char* rank = p.rank + (size_t)k * p.c.n_samples;
    const float* det_box = p.c.in.det_box;
    const double* gt_box = p.c.in.gt_box;
    const double thr = p.thr[t], lo = coco_area_lo(a), hi = coco_area_hi(a);
    double tp = 0.0, fp = 0.0;
    int ntp = 0;
    for (int i = 0; i < n; ++i) {
        const int d = (int)(0xFFFFFFFFu - (unsigned)(keys[i] & 0xFFFFFFFFull));
        const int s = p.c.in.det_sample[d];
        int r = 0;
        if (lane == 0) {                   // one lane reads and writes the counter: no cross-lane ordering is relied on
            r = rank[s];
            if (r < COCO_MAX_DET) rank[s] = (unsigned char)(r + 1);
        }
        r = __shfl(r, 0, 64);
        if (r >= COCO_MAX_DET) continue;   // the 101st detection of an (image, class) takes no part
        const double b0 = det_box[(size_t)d * 4], b1 = det_box[(size_t)d * 4 + 1], b2 = det_box[(size_t)d * 4 + 2], b3 = det_box[(size_t)d * 4 + 3];
        const double aread = __dmul_rn(__dsub_rn(b1, b0), __dsub_rn(b3, b2));
        const int g_lo = p.c.gt_first[s], g_hi = p.c.gt_first[s + 1];
        const bool act = live && r < maxdet, single = g_hi - g_lo <= 64;
        double best = thr;
        int m = -1, cnt = 0;
        bool m_ign = false;
        // COCO walks the non-ignored boxes first, then the ignored ones (which boxes those are depends on the lane's area range):
        // two passes over the boxes in arrival order, pass 1 skipped by a lane that holds a non-ignored match
        for (int pass = 0; pass < 2; ++pass)
            for (int c0 = g_lo; c0 < g_hi; c0 += 64) {
                if (!(single && pass == 1)) {
                    __syncthreads();
                    const int g = c0 + lane;
                    const bool mine = g < g_hi && p.c.in.gt_cls[g] == k;
                    const u64 bal = __ballot(mine);
                    cnt = __popcll(bal);
                    if (mine) {
                        const int pos = __popcll(bal & ((1ull << lane) - 1ull));
                        const double a0 = gt_box[(size_t)g * 4], a1 = gt_box[(size_t)g * 4 + 1], a2 = gt_box[(size_t)g * 4 + 2], a3 = gt_box[(size_t)g * 4 + 3];
                        const int fl = p.c.in.gt_flags[g];
                        const double ga = p.c.gt_area[g];
                        const double w = __dsub_rn(fmin(b1, a1), fmax(b0, a0)), h = __dsub_rn(fmin(b3, a3), fmax(b2, a2));
                        double iou = 0.0;
                        if (w > 0.0 && h > 0.0) {
                            const double inter = __dmul_rn(w, h);
                            const double uni = (fl & 2) ? aread
                                                        : __dsub_rn(__dadd_rn(aread, __dmul_rn(__dsub_rn(a1, a0), __dsub_rn(a3, a2))), inter);
                            iou = __ddiv_rn(inter, uni);
                        }
                        int bits = (fl & 2) ? 16 : 0;
                        for (int q = 0; q < COCO_AREAS; ++q) bits |= (fl != 0 || ga < coco_area_lo(q) || ga > coco_area_hi(q)) ? (1 << q) : 0;
                        s_g[pos] = g; s_iou[pos] = iou; s_fl[pos] = (unsigned char)bits;
                    }
                    __syncthreads();
                }
                for (int j = 0; j < cnt; ++j) {
                    const double iou = s_iou[j];
                    if (iou < p.tmin) continue;                           // (the wave's) below every lane's threshold
                    const int gi = s_g[j], fl = s_fl[j];
                    const bool ign = (fl >> a) & 1;
                    if (!act || ign != (pass == 1) || (pass == 1 && m >= 0 && !m_ign)) continue;
                    if (p.matched[(size_t)gi * 64 + lane] && !(fl & 16)) continue;      // taken, and not a crowd box
                    if (iou < best) continue;
                    best = iou; m = gi; m_ign = ign;                       // >=: among equal IoUs the last one wins
                }
            }
        const double area = __dmul_rn(aread, p.c.sample_scale[s]);
        // ignored: matched to an ignored box, or unmatched and outside the area range itself
        const bool counted = act && !(m >= 0 ? m_ign : (area < lo || area > hi));
        if (act && m >= 0) p.matched[(size_t)m * 64 + lane] = 1;
        if (counted && m >= 0) {
            tp += 1.0;
            // only the true positives' precisions are kept (see ap_walk_kernel: the 2^-52 term keeps the quotient monotonic in fp)
            if (ntp < npos) tpp[(size_t)ntp * 64] = __ddiv_rn(tp, __dadd_rn(__dadd_rn(fp, tp), 0x1p-52));
            ++ntp;
        } else if (counted) {
            fp += 1.0;
        }
    }
    if (!live) return;
    if (npig == 0) { *ar_out = -1.0; if (ap_out) *ap_out = -1.0; return; }
    *ar_out = __ddiv_rn(tp, (double)npig);
    if (!ap_out) return;
    if (ntp > npos) ntp = npos;
    double mx = 0.0;
    for (int i = ntp - 1; i >= 0; --i) {                                  // the precisions made non-increasing from the back
        const double v = tpp[(size_t)i * 64];
        if (v > mx) mx = v;
        tpp[(size_t)i * 64] = mx;
    }
    // q_j: the precision at the first point with recall >= j * 0.01 -- the first true positive nn with nn / npig >= j * 0.01
    double sum = 0.0;
    int nn = 1;
    for (int j = 0; j <= 100; ++j) {
        const double rj = __dmul_rn((double)j, 0.01);
        while (nn <= ntp && !(__ddiv_rn((double)nn, (double)npig) >= rj)) ++nn;
        if (nn <= ntp) sum = __dadd_rn(sum, tpp[(size_t)(nn - 1) * 64]);
    }
    *ap_out = __ddiv_rn(sum, 101.0);
}

void coco_eval_run(const COCOInput& c, const int* gt_sample_host, int n_thr, const double* thresholds, double* ap_out, double* ar_out,
                   int* present_out, hipStream_t s) {
    const APInput& in = c.in;
    require_num_classes(in.ncls);
    SSD_REQUIRE(n_thr >= 1 && n_thr <= AP_MAX_THRESHOLDS && thresholds, "1..%d IoU thresholds (got %d)", AP_MAX_THRESHOLDS, n_thr);
    SSD_REQUIRE(in.n_det >= 0 && in.n_gt >= 0 && c.n_samples >= 0, "bad sizes");
    SSD_REQUIRE(ap_out && ar_out && present_out, "null output array");
    SSD_REQUIRE(in.n_gt == 0 || gt_sample_host, "null ground truth");
    const int ncls = in.ncls, ns = c.n_samples;
    std::vector<int> first((size_t)ns + 1, 0);
    for (int g = 0; g < in.n_gt; ++g) {
        SSD_REQUIRE(gt_sample_host[g] >= 0 && gt_sample_host[g] < ns, "ground truth %d belongs to sample %d outside 0..%d", g, gt_sample_host[g], ns - 1);
        SSD_REQUIRE(g == 0 || gt_sample_host[g] >= gt_sample_host[g - 1], "ground truth must be grouped by ascending sample id");
        ++first[(size_t)gt_sample_host[g] + 1];
    }
    for (int i = 0; i < ns; ++i) first[i + 1] += first[i];
    APArgs a{};
    a.in = in;
    a.protocol = AP_VOC07;                 // the sort's denominator: the unflagged boxes
    COCOArgs q{};
    q.c = c;
    q.n_thr = n_thr;
    q.n_combo = COCO_GROUPS * n_thr;
    q.tmin = 1.0;
    for (int t = 0; t < n_thr; ++t) {
        q.thr[t] = std::min(thresholds[t], 1.0 - 1e-10);
        q.tmin = std::min(q.tmin, q.thr[t]);
    }
    const size_t ng = in.n_gt ? in.n_gt : 1;
    DevBuf counts((size_t)ncls * 12), npig((size_t)ncls * 16), offs((size_t)ncls * 16), gfirst(first.size() * 4), matched(ng * 64),
        rank((size_t)ncls * ns), ap((size_t)COCO_AREAS * n_thr * ncls * 8), ar((size_t)COCO_GROUPS * n_thr * ncls * 8),
        present((size_t)COCO_AREAS * ncls * 4);
    HIP_OK(hipMemcpyAsync(gfirst.p, first.data(), first.size() * 4, hipMemcpyHostToDevice, s));
    q.c.gt_first = gfirst.as<int>();
    a.counts = counts.as<int>();
    q.counts = a.counts;
    q.npig = npig.as<int>();
    StageTimer timer(s);
    timer.mark(0);
    hipLaunchKernelGGL(ap_count_kernel, dim3(ncls), dim3(256), 0, s, a);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(coco_npig_kernel, dim3(ncls), dim3(256), 0, s, q);
    HIP_OK(hipGetLastError());
    timer.mark(1);
    std::vector<int> h_counts((size_t)ncls * 3);
    HIP_OK(hipMemcpyAsync(h_counts.data(), counts.p, h_counts.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    std::vector<long long> h_offs((size_t)ncls * 2);
    long long nkeys = 0, ntp = 0;
    for (int k = 0; k < ncls; ++k) {
        h_offs[k] = nkeys;
        h_offs[ncls + k] = ntp;
        nkeys += pow2_at_least(h_counts[k]);
        ntp += h_counts[2 * ncls + k];      // a lane's true positives match distinct unflagged boxes of the class
    }
    DevBuf keys((size_t)nkeys * 8), tp_prec((size_t)ntp * 64 * 8);
    HIP_OK(hipMemcpyAsync(offs.p, h_offs.data(), h_offs.size() * 8, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemsetAsync(matched.p, 0, ng * 64, s));
    HIP_OK(hipMemsetAsync(rank.p, 0, (size_t)ncls * ns ? (size_t)ncls * ns : 1, s));
    a.koff = offs.as<long long>();
    a.keys = keys.as<u64>();
    q.koff = a.koff;
    q.toff = offs.as<long long>() + ncls;
    q.keys = a.keys;
    q.matched = matched.as<unsigned char>();
    q.rank = rank.as<unsigned char>();
    q.tp_prec = tp_prec.as<double>();
    q.ap = ap.as<double>();
    q.ar = ar.as<double>();
    q.present = present.as<int>();
    timer.mark(2);
    hipLaunchKernelGGL(ap_sort_kernel, dim3(ncls), dim3(256), 0, s, a);
    HIP_OK(hipGetLastError());
    timer.mark(3);
    hipLaunchKernelGGL(coco_walk_kernel, dim3(ncls), dim3(64), 0, s, q);
    HIP_OK(hipGetLastError());
    timer.mark(4);
    HIP_OK(hipMemcpyAsync(ap_out, ap.p, (size_t)COCO_AREAS * n_thr * ncls * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(ar_out, ar.p, (size_t)COCO_GROUPS * n_thr * ncls * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(present_out, present.p, (size_t)COCO_AREAS * ncls * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    timer.finish();
}

// ------------------------------------------------------------------------------------------------------------ accumulator
struct APStore { float* box; float* conf; int* cls; int* sample; };

// One workgroup appends a pass: min(count[i], out_cap) detections of image 0, then of image 1, ... behind the accumulator's end,
// in the order the host lists hold them (ties between equal confidences are broken by that order).  The boxes take the host
// path's round trip through the proportional form.  words[0] (the end) and words[1] (dropped class ids) are advanced with
// ordinary vector stores: the stream orders one append behind the other.
__global__ __launch_bounds__(256) void ap_append_kernel(int b, int out_cap, const int* __restrict__ count, const float* __restrict__ conf,
                                                         const int* __restrict__ cls, const int* __restrict__ box, int ncls, int sample0,
                                                         long long cap, APStore st, int* words) {
    __shared__ int s_w[4], s_bad[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int base = words[0];
    int total = 0, dropped = 0;
    __syncthreads();
    for (int i = 0; i < b; ++i) {
        int n = count[i];
        n = n < 0 ? 0 : (n > out_cap ? out_cap : n);
        for (int j0 = 0; j0 < n; j0 += 256) {
            const int j = j0 + tid;
            const size_t e = (size_t)i * out_cap + j;
            const int c = j < n ? cls[e] : -1;
            const bool ok = j < n && c >= 0 && c < ncls;
            const u64 bal = __ballot(ok), bad = __ballot(j < n && !ok);
            if (lane == 0) { s_w[wv] = __popcll(bal); s_bad[wv] = __popcll(bad); }
            __syncthreads();
            int at = total;
            for (int q = 0; q < 4; ++q) { if (q < wv) at += s_w[q]; total += s_w[q]; dropped += s_bad[q]; }
            const long long pos = (long long)base + at + __popcll(bal & ((1ull << lane) - 1ull));
            if (ok && pos < cap) {
                const int* r = box + e * 4;      // (a slot's boxes are 4-byte aligned only)
                int o[4];
                rect_on_image(r[0], r[1], r[2], r[3], 1000, 1000, o);
                *reinterpret_cast<float4*>(st.box + pos * 4) = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
                st.conf[pos] = conf[e];
                st.cls[pos] = c;
                st.sample[pos] = sample0 + i;
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        const long long end = (long long)base + total;
        words[0] = (int)(end < cap ? end : cap);
        words[1] += dropped + (int)(end > cap ? end - cap : 0);
    }
}

APAccumulator::APAccumulator(int device, int num_classes) : hip_(device), device_(device), ncls_(num_classes) {
    require_num_classes(num_classes);
    DeviceGuard g(device_);
    words_ = (int*)hip_.mem(16);
    HIP_OK(hipMemset(words_, 0, 16));
}

void APAccumulator::release_retired() {
    for (void* p : retired_) hip_.free_mem(p);
    retired_.clear();
}

void APAccumulator::sync() {
    HIP_OK(hipStreamSynchronize(last_));
    release_retired();
}

void APAccumulator::clear() {
    DeviceGuard g(device_);
    sync();
    HIP_OK(hipMemset(words_, 0, 16));
    bound_ = 0;
    samples_ = 0;
    gt_box_.clear(); gt_cls_.clear(); gt_sample_.clear(); gt_flags_.clear();
    gt_area_.clear(); sample_scale_.clear();
    plain_samples_ = 0;
}

// Room for `extra` more detections behind the host's bound.  The old buffers are copied on `s`, behind the appends already
// enqueued there, and freed at the next wait: growing never waits for the GPU.
void APAccumulator::reserve(long long extra, hipStream_t s) {
    const long long need = bound_ + extra;
    SSD_REQUIRE(need < INT_MAX, "the accumulator holds at most 2^31 - 1 detections");
    if (need <= cap_) return;
    const long long cap = std::max<long long>(std::max<long long>(2 * cap_, need), 1024);
    Store nw;
    nw.box = (float*)hip_.mem((size_t)cap * 16);
    nw.conf = (float*)hip_.mem((size_t)cap * 4);
    nw.cls = (int*)hip_.mem((size_t)cap * 4);
    nw.sample = (int*)hip_.mem((size_t)cap * 4);
    if (bound_ > 0) {
        HIP_OK(hipMemcpyAsync(nw.box, st_.box, (size_t)bound_ * 16, hipMemcpyDeviceToDevice, s));
        HIP_OK(hipMemcpyAsync(nw.conf, st_.conf, (size_t)bound_ * 4, hipMemcpyDeviceToDevice, s));
        HIP_OK(hipMemcpyAsync(nw.cls, st_.cls, (size_t)bound_ * 4, hipMemcpyDeviceToDevice, s));
        HIP_OK(hipMemcpyAsync(nw.sample, st_.sample, (size_t)bound_ * 4, hipMemcpyDeviceToDevice, s));
    }
    if (st_.box) {
        retired_.push_back(st_.box); retired_.push_back(st_.conf); retired_.push_back(st_.cls); retired_.push_back(st_.sample);
    }
    st_ = nw;
    cap_ = cap;
}

// gt_area / sample_scale: of a _coco append (both or neither).  Such rows keep their flag byte (bit 1 = crowd; the VOC kernels
// read nonzero as flagged); the rows of a plain append get area 0 and scale 1, which nothing reads: they bar compute_coco.
void APAccumulator::push_gt(int n_gt, const double* gt_box, const int* gt_cls, const int* gt_sample, const unsigned char* gt_flags,
                            int n_samples, const char* what, const double* gt_area, const double* sample_scale) {
    const bool coco = sample_scale != nullptr;
    SSD_REQUIRE(!coco || n_gt == 0 || gt_area, "%s: null gt_area", what);
    for (int i = 0; coco && i < n_samples; ++i)
        SSD_REQUIRE(sample_scale[i] > 0.0, "%s: sample_scale[%d] = %g must be positive (W*H/1e6 of the image)", what, i, sample_scale[i]);
    for (int g = 0; coco && g < n_gt; ++g) SSD_REQUIRE(gt_area[g] >= 0.0, "%s: gt_area[%d] = %g is negative", what, g, gt_area[g]);
    SSD_REQUIRE(n_gt >= 0 && (n_gt == 0 || (gt_box && gt_cls && gt_sample)), "%s: null ground truth", what);
    SSD_REQUIRE(samples_ + n_samples < INT_MAX, "%s: too many samples", what);
    for (int g = 0; g < n_gt; ++g) {
        SSD_REQUIRE(gt_sample[g] >= 0 && gt_sample[g] < n_samples, "%s: ground truth %d belongs to image %d outside 0..%d", what, g, gt_sample[g], n_samples - 1);
        SSD_REQUIRE(gt_cls[g] >= 0 && gt_cls[g] < ncls_, "%s: ground truth %d has class id %d outside 0..%d", what, g, gt_cls[g], ncls_ - 1);
    }
    std::vector<int> order(n_gt);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return gt_sample[x] < gt_sample[y]; });      // rows grouped by sample
    for (int g : order) {
        gt_box_.insert(gt_box_.end(), gt_box + (size_t)g * 4, gt_box + (size_t)g * 4 + 4);
        gt_cls_.push_back(gt_cls[g]);
        gt_sample_.push_back((int)samples_ + gt_sample[g]);
        gt_flags_.push_back(gt_flags ? (coco ? gt_flags[g] : (gt_flags[g] ? 1 : 0)) : 0);
        gt_area_.push_back(coco ? gt_area[g] : 0.0);
    }
    for (int i = 0; i < n_samples; ++i) sample_scale_.push_back(coco ? sample_scale[i] : 1.0);
    if (!coco) plain_samples_ += n_samples;
}

void APAccumulator::add_dev(int b, int out_cap, const int* count_dev, const float* conf_dev, const int* cls_dev, const int* box_dev,
                            int n_gt, const double* gt_box, const int* gt_cls, const int* gt_image, const unsigned char* gt_flags,
                            hipStream_t s) {
    add_dev_coco(b, out_cap, count_dev, conf_dev, cls_dev, box_dev, n_gt, gt_box, gt_cls, gt_image, gt_flags, nullptr, nullptr, s);
}

void APAccumulator::add_dev_coco(int b, int out_cap, const int* count_dev, const float* conf_dev, const int* cls_dev, const int* box_dev,
                                 int n_gt, const double* gt_box, const int* gt_cls, const int* gt_image, const unsigned char* gt_flags,
                                 const double* gt_area, const double* sample_scale, hipStream_t s) {
    const char* what = sample_scale ? "ssd_ap_add_dev_coco" : "ssd_ap_add_dev";
    SSD_REQUIRE(b >= 1 && out_cap >= 1 && (long long)b * out_cap < INT_MAX, "%s: b >= 1, out_cap >= 1", what);
    SSD_REQUIRE(count_dev && conf_dev && cls_dev && box_dev, "%s: null detection array", what);
    DeviceGuard g(device_);
    reserve((long long)b * out_cap, s);      // (before the ground truth is appended: a failed allocation leaves the accumulator as it was)
    push_gt(n_gt, gt_box, gt_cls, gt_image, gt_flags, b, what, gt_area, sample_scale);
    APStore st{st_.box, st_.conf, st_.cls, st_.sample};
    hipLaunchKernelGGL(ap_append_kernel, dim3(1), dim3(256), 0, s, b, out_cap, count_dev, conf_dev, cls_dev, box_dev, ncls_, (int)samples_,
                       cap_, st, words_);
    HIP_OK(hipGetLastError());
    bound_ += (long long)b * out_cap;
    samples_ += b;
    last_ = s;
}

void APAccumulator::counts(long long* n_det, long long* n_dropped) {
    DeviceGuard g(device_);
    sync();
    int w[2];
    HIP_OK(hipMemcpy(w, words_, 8, hipMemcpyDeviceToHost));
    bound_ = w[0];      // (the exact end: the bound is tight again)
    if (n_det) *n_det = w[0];
    if (n_dropped) *n_dropped = w[1];
}

void APAccumulator::add_host(int n_det, const float* det_box, const float* det_conf, const int* det_cls, const int* det_sample,
                             int n_samples, int n_gt, const double* gt_box, const int* gt_cls, const int* gt_sample,
                             const unsigned char* gt_flags) {
    add_host_coco(n_det, det_box, det_conf, det_cls, det_sample, n_samples, n_gt, gt_box, gt_cls, gt_sample, gt_flags, nullptr, nullptr);
}

void APAccumulator::add_host_coco(int n_det, const float* det_box, const float* det_conf, const int* det_cls, const int* det_sample,
                                  int n_samples, int n_gt, const double* gt_box, const int* gt_cls, const int* gt_sample,
                                  const unsigned char* gt_flags, const double* gt_area, const double* sample_scale) {
    const char* what = sample_scale ? "ssd_ap_add_host_coco" : "ssd_ap_add_host";
    SSD_REQUIRE(n_det >= 0 && n_samples >= 0 && (n_det == 0 || (det_box && det_conf && det_cls && det_sample)), "%s: bad detections", what);
    DeviceGuard g(device_);
    long long end, dropped;
    counts(&end, &dropped);
    std::vector<float> hb, hc;
    std::vector<int> hk, hs;
    for (int d = 0; d < n_det; ++d) {
        SSD_REQUIRE(det_sample[d] >= 0 && det_sample[d] < n_samples, "%s: detection %d belongs to sample %d outside 0..%d", what, d, det_sample[d], n_samples - 1);
        if (det_cls[d] < 0 || det_cls[d] >= ncls_) { ++dropped; continue; }
        hb.insert(hb.end(), det_box + (size_t)d * 4, det_box + (size_t)d * 4 + 4);
        hc.push_back(det_conf[d]); hk.push_back(det_cls[d]); hs.push_back((int)samples_ + det_sample[d]);
    }
    const long long n = (long long)hk.size();
    reserve(n, last_);      // (before the ground truth is appended, as in add_dev_coco)
    push_gt(n_gt, gt_box, gt_cls, gt_sample, gt_flags, n_samples, what, gt_area, sample_scale);
    HIP_OK(hipStreamSynchronize(last_));
    if (n) {
        HIP_OK(hipMemcpy(st_.box + end * 4, hb.data(), (size_t)n * 16, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(st_.conf + end, hc.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(st_.cls + end, hk.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(st_.sample + end, hs.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    }
    const int w[2] = {(int)(end + n), (int)dropped};
    HIP_OK(hipMemcpy(words_, w, 8, hipMemcpyHostToDevice));
    bound_ = end + n;
    samples_ += n_samples;
}

void APAccumulator::fetch(long long cap, float* det_box, float* det_conf, int* det_cls, int* det_sample, long long* n_det) {
    DeviceGuard g(device_);
    long long end;
    counts(&end, nullptr);
    if (n_det) *n_det = end;
    SSD_REQUIRE(cap >= end, "ssd_ap_fetch: room for %lld detections, the accumulator holds %lld", cap, end);
    if (end == 0) return;
    if (det_box) HIP_OK(hipMemcpy(det_box, st_.box, (size_t)end * 16, hipMemcpyDeviceToHost));
    if (det_conf) HIP_OK(hipMemcpy(det_conf, st_.conf, (size_t)end * 4, hipMemcpyDeviceToHost));
    if (det_cls) HIP_OK(hipMemcpy(det_cls, st_.cls, (size_t)end * 4, hipMemcpyDeviceToHost));
    if (det_sample) HIP_OK(hipMemcpy(det_sample, st_.sample, (size_t)end * 4, hipMemcpyDeviceToHost));
}

void APAccumulator::compute(int protocol, int n_thr, const double* minoverlaps, double* ap_out, int* present_out, long long* n_det,
                            long long* n_dropped) {
    DeviceGuard g(device_);
    long long end;
    counts(&end, n_dropped);
    if (n_det) *n_det = end;
    const size_t ng = gt_cls_.size();
    DevBuf gbox(ng * 32), gcls(ng * 4), gsmp(ng * 4), gflg(ng);
    if (ng) {
        HIP_OK(hipMemcpy(gbox.p, gt_box_.data(), ng * 32, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(gcls.p, gt_cls_.data(), ng * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(gsmp.p, gt_sample_.data(), ng * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(gflg.p, gt_flags_.data(), ng, hipMemcpyHostToDevice));
    }
    APInput in{(int)end, (int)ng, ncls_, st_.box, st_.conf, st_.cls, st_.sample, gbox.as<double>(), gcls.as<int>(), gsmp.as<int>(),
               gflg.as<unsigned char>()};
    average_precision_run(in, protocol, n_thr, minoverlaps, ap_out, present_out, last_);
}

void APAccumulator::compute_coco(int n_thr, const double* thresholds, double* ap_out, double* ar_out, int* present_out, long long* n_det,
                                 long long* n_dropped) {
    SSD_REQUIRE(plain_samples_ == 0, "ssd_ap_compute_coco: %lld of the accumulator's %lld samples were added without areas and image "
                "scales (ssd_ap_add_dev / ssd_ap_add_host); use the _coco calls for every pass", plain_samples_, samples_);
    SSD_REQUIRE(n_thr >= 1 && n_thr <= AP_MAX_THRESHOLDS && thresholds, "1..%d IoU thresholds (got %d)", AP_MAX_THRESHOLDS, n_thr);
    SSD_REQUIRE(ap_out && ar_out && present_out, "ssd_ap_compute_coco: null output array");
    DeviceGuard g(device_);
    long long end;
    counts(&end, n_dropped);
    if (n_det) *n_det = end;
    const size_t ng = gt_cls_.size(), ns = sample_scale_.size();
    DevBuf gbox(ng * 32), gcls(ng * 4), gsmp(ng * 4), gflg(ng), garea(ng * 8), scale(ns * 8);
    if (ng) {
        HIP_OK(hipMemcpy(gbox.p, gt_box_.data(), ng * 32, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(gcls.p, gt_cls_.data(), ng * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(gsmp.p, gt_sample_.data(), ng * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(gflg.p, gt_flags_.data(), ng, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(garea.p, gt_area_.data(), ng * 8, hipMemcpyHostToDevice));
    }
    if (ns) HIP_OK(hipMemcpy(scale.p, sample_scale_.data(), ns * 8, hipMemcpyHostToDevice));
    COCOInput c{{(int)end, (int)ng, ncls_, st_.box, st_.conf, st_.cls, st_.sample, gbox.as<double>(), gcls.as<int>(), gsmp.as<int>(),
                 gflg.as<unsigned char>()}, (int)ns, garea.as<double>(), scale.as<double>(), nullptr};
    coco_eval_run(c, gt_sample_.data(), n_thr, thresholds, ap_out, ar_out, present_out, last_);
}

}  // namespace ssd
