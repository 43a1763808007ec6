// Detections drawn on images where both already lie: the reference's draw_box (utils.py:138-148) restated so
// that it can be checked bit for bit -- a 3-pixel outline ring, a filled tag above the box, the label in a built-in 5 x 7 font
// (2 x 2 pixels per font pixel), each box blended 0.8 : 0.2 over what the boxes before it left (cv2.addWeighted).  Parity with
// OpenCV's rasteriser and its Hershey font is unpinned; the pixel rectangle of a box is the reference's own float64 arithmetic.
//
// Two launches per call:
//   annotate_boxes_kernel: one workgroup per image reads the detection arrays ONCE (they may be mapped pinned host memory,
//                          across PCIe) and leaves one record per box in HBM: pixel rectangle, influence rectangle, style row.
//   annotate_draw_kernel:  a pure gather.  An image is a linear run of pixels; a thread owns 16 consecutive ones (48 bytes of
//                          uint8, three aligned 16-byte stores; 192 bytes of float32), a workgroup 4096.  The workgroup walks the
//                          image's records 256 at a time and compacts, IN LIST ORDER (ballot + prefix), those whose influence
//                          meets its rows into LDS with their colour and label; every thread then applies that list in order to
//                          the pixels it holds in registers.  No atomics, no read-modify-write of the destination: the output
//                          does not depend on scheduling.  A tile no box touches is a copy (a resize / convert for float32).
// Compiled with -ffp-contract=off: every product and sum of the blend and of the bilinear taps is rounded on its own.
#include "annotate.h"
#include "boxmath.h"
#include <memory>

namespace ssd {

constexpr int ANN_THREADS = 256;
constexpr int ANN_PPT = 16;                          // pixels per thread
constexpr int ANN_TILE = ANN_THREADS * ANN_PPT;      // pixels per workgroup
constexpr int ANN_MAX_LABEL = 31;
constexpr int ANN_MAX_DIM = 32768;                   // image width / height
constexpr int ANN_COORD = 1 << 24;                   // box coordinates are clamped here: far outside any image either way

// THE font: 5 x 7, ASCII 32..126, one byte per row, column 0 = bit 4.  The kernel and ssd_annotate_glyph both read it here;
// any other byte is drawn as '?'.
__host__ __device__ inline unsigned glyph_row(int ch, int r) {
    constexpr unsigned char FONT[95][7] = {
        {0x00,0x00,0x00,0x00,0x00,0x00,0x00}, {0x04,0x04,0x04,0x04,0x04,0x00,0x04}, {0x0A,0x0A,0x0A,0x00,0x00,0x00,0x00}, {0x0A,0x0A,0x1F,0x0A,0x1F,0x0A,0x0A},   //   ! " #
        {0x04,0x0F,0x14,0x0E,0x05,0x1E,0x04}, {0x18,0x19,0x02,0x04,0x08,0x13,0x03}, {0x08,0x14,0x14,0x08,0x15,0x12,0x0D}, {0x06,0x06,0x04,0x08,0x00,0x00,0x00},   // $ % & '
        {0x02,0x04,0x08,0x08,0x08,0x04,0x02}, {0x08,0x04,0x02,0x02,0x02,0x04,0x08}, {0x04,0x15,0x0E,0x1F,0x0E,0x15,0x04}, {0x00,0x04,0x04,0x1F,0x04,0x04,0x00},   // ( ) * +
        {0x00,0x00,0x00,0x00,0x0C,0x04,0x08}, {0x00,0x00,0x00,0x1F,0x00,0x00,0x00}, {0x00,0x00,0x00,0x00,0x00,0x06,0x06}, {0x00,0x01,0x02,0x04,0x08,0x10,0x00},   // , - . /
        {0x0E,0x11,0x13,0x15,0x19,0x11,0x0E}, {0x04,0x0C,0x04,0x04,0x04,0x04,0x0E}, {0x0E,0x11,0x01,0x0E,0x10,0x10,0x1F}, {0x1F,0x01,0x02,0x06,0x01,0x11,0x0E},   // 0 1 2 3
        {0x02,0x06,0x0A,0x12,0x1F,0x02,0x02}, {0x1F,0x10,0x1E,0x01,0x01,0x11,0x0E}, {0x07,0x08,0x10,0x1E,0x11,0x11,0x0E}, {0x1F,0x01,0x01,0x02,0x04,0x08,0x10},   // 4 5 6 7
        {0x0E,0x11,0x11,0x0E,0x11,0x11,0x0E}, {0x0E,0x11,0x11,0x0F,0x01,0x02,0x1C}, {0x00,0x00,0x04,0x00,0x04,0x00,0x00}, {0x00,0x00,0x04,0x00,0x04,0x04,0x08},   // 8 9 : ;
        {0x01,0x02,0x04,0x08,0x04,0x02,0x01}, {0x00,0x00,0x1F,0x00,0x1F,0x00,0x00}, {0x08,0x04,0x02,0x01,0x02,0x04,0x08}, {0x0E,0x11,0x01,0x06,0x04,0x00,0x04},   // < = > ?
        {0x0E,0x11,0x15,0x17,0x16,0x10,0x0F}, {0x04,0x0A,0x11,0x11,0x1F,0x11,0x11}, {0x1E,0x11,0x11,0x1E,0x11,0x11,0x1E}, {0x0E,0x11,0x10,0x10,0x10,0x11,0x0E},   // @ A B C
        {0x1E,0x11,0x11,0x11,0x11,0x11,0x1E}, {0x1F,0x10,0x10,0x1E,0x10,0x10,0x1F}, {0x1F,0x10,0x10,0x1E,0x10,0x10,0x10}, {0x0F,0x11,0x10,0x10,0x13,0x11,0x0F},   // D E F G
        {0x11,0x11,0x11,0x1F,0x11,0x11,0x11}, {0x0E,0x04,0x04,0x04,0x04,0x04,0x0E}, {0x07,0x02,0x02,0x02,0x02,0x12,0x0C}, {0x11,0x12,0x14,0x18,0x14,0x12,0x11},   // H I J K
        {0x10,0x10,0x10,0x10,0x10,0x10,0x1F}, {0x11,0x1B,0x15,0x15,0x15,0x11,0x11}, {0x11,0x11,0x19,0x15,0x13,0x11,0x11}, {0x0E,0x11,0x11,0x11,0x11,0x11,0x0E},   // L M N O
        {0x1E,0x11,0x11,0x1E,0x10,0x10,0x10}, {0x0E,0x11,0x11,0x11,0x15,0x12,0x0D}, {0x1E,0x11,0x11,0x1E,0x14,0x12,0x11}, {0x0E,0x11,0x10,0x0E,0x01,0x11,0x0E},   // P Q R S
        {0x1F,0x15,0x04,0x04,0x04,0x04,0x04}, {0x11,0x11,0x11,0x11,0x11,0x11,0x0E}, {0x11,0x11,0x11,0x11,0x11,0x0A,0x04}, {0x11,0x11,0x11,0x15,0x15,0x15,0x0A},   // T U V W
        {0x11,0x11,0x0A,0x04,0x0A,0x11,0x11}, {0x11,0x11,0x0A,0x04,0x04,0x04,0x04}, {0x1F,0x01,0x02,0x0E,0x08,0x10,0x1F}, {0x0F,0x08,0x08,0x08,0x08,0x08,0x0F},   // X Y Z [
        {0x00,0x10,0x08,0x04,0x02,0x01,0x00}, {0x0F,0x01,0x01,0x01,0x01,0x01,0x0F}, {0x04,0x0A,0x11,0x00,0x00,0x00,0x00}, {0x00,0x00,0x00,0x00,0x00,0x00,0x1F},   // backslash ] ^ _
        {0x0C,0x0C,0x04,0x02,0x00,0x00,0x00}, {0x00,0x00,0x0C,0x02,0x0E,0x12,0x0F}, {0x10,0x10,0x16,0x19,0x11,0x19,0x16}, {0x00,0x00,0x0E,0x11,0x10,0x11,0x0E},   // ` a b c
        {0x01,0x01,0x0D,0x13,0x11,0x13,0x0D}, {0x00,0x00,0x0E,0x11,0x1F,0x10,0x0E}, {0x02,0x05,0x04,0x0E,0x04,0x04,0x04}, {0x00,0x0F,0x11,0x11,0x0F,0x01,0x0E},   // d e f g
        {0x10,0x10,0x16,0x19,0x11,0x11,0x11}, {0x04,0x00,0x0C,0x04,0x04,0x04,0x0E}, {0x02,0x00,0x02,0x02,0x02,0x12,0x0C}, {0x10,0x10,0x12,0x14,0x18,0x14,0x12},   // h i j k
        {0x0C,0x04,0x04,0x04,0x04,0x04,0x0E}, {0x00,0x00,0x1A,0x15,0x15,0x15,0x15}, {0x00,0x00,0x16,0x19,0x11,0x11,0x11}, {0x00,0x00,0x0E,0x11,0x11,0x11,0x0E},   // l m n o
        {0x00,0x00,0x1E,0x11,0x1E,0x10,0x10}, {0x00,0x00,0x0D,0x13,0x0F,0x01,0x01}, {0x00,0x00,0x16,0x19,0x10,0x10,0x10}, {0x00,0x00,0x0F,0x10,0x0E,0x01,0x1E},   // p q r s
        {0x04,0x04,0x1F,0x04,0x04,0x05,0x02}, {0x00,0x00,0x11,0x11,0x11,0x13,0x0D}, {0x00,0x00,0x11,0x11,0x11,0x0A,0x04}, {0x00,0x00,0x11,0x11,0x15,0x15,0x0A},   // t u v w
        {0x00,0x00,0x11,0x0A,0x04,0x0A,0x11}, {0x00,0x00,0x11,0x11,0x0F,0x01,0x0E}, {0x00,0x00,0x1F,0x02,0x04,0x08,0x1F}, {0x02,0x04,0x04,0x08,0x04,0x04,0x02},   // x y z {
        {0x04,0x04,0x04,0x00,0x04,0x04,0x04}, {0x08,0x04,0x04,0x02,0x04,0x04,0x08}, {0x08,0x15,0x02,0x00,0x00,0x00,0x00},   // | } ~
    };
    return FONT[(ch >= 32 && ch <= 126) ? ch - 32 : '?' - 32][r];
}

__host__ __device__ inline int clamp_coord(int v) { return v < -ANN_COORD ? -ANN_COORD : (v > ANN_COORD ? ANN_COORD : v); }

struct alignas(4) StyleEntry {      // row num_classes: white, "?" (a class id outside 0..num_classes-1)
    unsigned char bgr[3];
    unsigned char len;
    unsigned char text[32];
};
static_assert(sizeof(StyleEntry) == 36, "StyleEntry layout");

struct AnnotateStyle {
    HipOwner hip;
    int device, num_classes;
    StyleEntry* dev = nullptr;
    AnnotateStyle(int d, int nc) : hip(d), device(d), num_classes(nc) {}
};

struct alignas(16) BoxRec {
    int xmin, xmax, ymin, ymax;      // pixel rectangle
    int ix0, ix1, iy0, iy1;          // everything the box can touch: outline ring, tag, text
    int cls, pad[3];
};
struct DevImage {
    unsigned long long src_off, dst_off;
    int src_w, src_h, dst_w, dst_h;
    int tile0, pad;
};
struct Item {                        // one box of a tile's list, in LDS
    int xmin, xmax, ymin, ymax, ix1, iy1;
    unsigned head;                   // b | g << 8 | r << 16 | label length << 24
    unsigned text[8];
};

__global__ __launch_bounds__(ANN_THREADS) void annotate_boxes_kernel(const DevImage* __restrict__ imgs, const int* __restrict__ count,
                                                                      const int* __restrict__ cls, const int* __restrict__ box, int out_cap,
                                                                      int grid1000, int num_classes, const StyleEntry* __restrict__ style,
                                                                      int* __restrict__ nbox, BoxRec* __restrict__ recs) {
    const int i = blockIdx.x;
    int n = count[i];
    n = n < 0 ? 0 : (n > out_cap ? out_cap : n);
    if (threadIdx.x == 0) nbox[i] = n;
    const int W = imgs[i].dst_w, H = imgs[i].dst_h;
    for (int k = threadIdx.x; k < n; k += ANN_THREADS) {
        const size_t e = (size_t)i * out_cap + k;
        int r[4];
        for (int q = 0; q < 4; ++q) r[q] = clamp_coord(box[e * 4 + q]);
        if (grid1000) rect_on_image(r[0], r[1], r[2], r[3], W, H, r);
        int c = cls[e];
        if (c < 0 || c >= num_classes) c = num_classes;
        const int len = style[c].len;
        BoxRec o;
        o.xmin = r[0]; o.xmax = r[1]; o.ymin = r[2]; o.ymax = r[3];
        o.ix0 = r[0] - 1;
        o.ix1 = max(r[1] + 1, r[0] + 4 + 12 * len);
        o.iy0 = r[2] - 20;
        o.iy1 = max(r[3] + 1, r[2]);
        o.cls = c; o.pad[0] = o.pad[1] = o.pad[2] = 0;
        recs[e] = o;
    }
}

// cv2's float INTER_LINEAR tap of destination coordinate d (source extent s, destination extent dn)
__device__ inline void linear_tap(int d, int s, int dn, int* i0, int* i1, float* f) {
    const float fx = (float)((d + 0.5) * ((double)s / (double)dn) - 0.5);
    int sx = (int)floorf(fx);
    float fr = fx - (float)sx;
    if (sx < 0) { sx = 0; fr = 0.f; }
    if (sx >= s - 1) { sx = s - 1; fr = 0.f; }
    *i0 = sx; *i1 = sx + 1 < s - 1 ? sx + 1 : s - 1; *f = fr;
}

template <bool SF, bool DF>
__global__ __launch_bounds__(ANN_THREADS) void annotate_draw_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                     const DevImage* __restrict__ imgs, int b, const int* __restrict__ nbox,
                                                                     const BoxRec* __restrict__ recs, int out_cap,
                                                                     const StyleEntry* __restrict__ style, int rgb_out) {
    __shared__ Item items[ANN_THREADS];
    __shared__ int s_wtot[ANN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int lo = 0, hi = b - 1;
    while (lo < hi) {      // the image this tile belongs to
        const int mid = (lo + hi + 1) >> 1;
        if (imgs[mid].tile0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const DevImage im = imgs[lo];
    const int W = im.dst_w, H = im.dst_h, npix = W * H;
    const int P0 = ((int)blockIdx.x - im.tile0) * ANN_TILE;
    const int p0 = P0 + t * ANN_PPT;
    const int nv = npix - p0 <= 0 ? 0 : (npix - p0 < ANN_PPT ? npix - p0 : ANN_PPT);
    const int x0 = nv ? p0 % W : 0, y0 = nv ? p0 / W : 0;

    // ---- the thread's pixels: copy / convert / resize
    float v[ANN_PPT * 3];
#pragma unroll
    for (int j = 0; j < ANN_PPT * 3; ++j) v[j] = 0.f;
    if constexpr (!SF) {
        const unsigned char* sp = src + im.src_off + (size_t)p0 * 3;
        if (nv == ANN_PPT) {
            unsigned wd[12];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 u = reinterpret_cast<const uint4*>(sp)[q];
                wd[4 * q] = u.x; wd[4 * q + 1] = u.y; wd[4 * q + 2] = u.z; wd[4 * q + 3] = u.w;
            }
#pragma unroll
            for (int j = 0; j < ANN_PPT * 3; ++j) v[j] = (float)((wd[j >> 2] >> ((j & 3) * 8)) & 255u);
        } else {
#pragma unroll
            for (int j = 0; j < ANN_PPT * 3; ++j)
                if (j < nv * 3) v[j] = (float)sp[j];
        }
    } else if (im.src_w == W && im.src_h == H) {
        const float* sp = reinterpret_cast<const float*>(src + im.src_off) + (size_t)p0 * 3;
        if (nv == ANN_PPT) {
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                const float4 u = reinterpret_cast<const float4*>(sp)[q];
                v[4 * q] = u.x; v[4 * q + 1] = u.y; v[4 * q + 2] = u.z; v[4 * q + 3] = u.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < ANN_PPT * 3; ++j)
                if (j < nv * 3) v[j] = sp[j];
        }
    } else {
        const float* sp = reinterpret_cast<const float*>(src + im.src_off);
        const int sw = im.src_w, sh = im.src_h;
        int x = x0, y = y0;
#pragma unroll
        for (int i = 0; i < ANN_PPT; ++i) {
            if (i < nv) {
                int xa, xb, ya, yb;
                float fx, fy;
                linear_tap(x, sw, W, &xa, &xb, &fx);
                linear_tap(y, sh, H, &ya, &yb, &fy);
                const float gx = 1.f - fx, gy = 1.f - fy;
                const float* ra = sp + (size_t)ya * sw * 3;
                const float* rb = sp + (size_t)yb * sw * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {      // the horizontal pass on both rows, then the vertical one
                    const float top = ra[xa * 3 + c] * gx + ra[xb * 3 + c] * fx;
                    const float bot = rb[xa * 3 + c] * gx + rb[xb * 3 + c] * fx;
                    v[3 * i + c] = top * gy + bot * fy;
                }
            }
            if (++x == W) { x = 0; ++y; }
        }
    }

    // ---- the boxes, in list order
    const int n = nbox[lo];
    const BoxRec* rb = recs + (size_t)lo * out_cap;
    const int P1 = (P0 + ANN_TILE < npix ? P0 + ANN_TILE : npix) - 1;
    const int ty0 = P0 / W, ty1 = P1 / W;
    const int pl = p0 + (nv ? nv - 1 : 0);
    const int my1 = nv ? pl / W : 0;
    const bool one_row = my1 == y0;
    const int mx1 = x0 + nv - 1;      // (meaningful when one_row)
    for (int base = 0; base < n; base += ANN_THREADS) {
        const int k = base + t;
        bool hit = false;
        BoxRec r;
        if (k < n) {
            r = rb[k];
            hit = r.iy1 >= ty0 && r.iy0 <= ty1 && r.ix1 >= 0 && r.ix0 < W;
        }
        const unsigned long long bal = __ballot(hit);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wtot[wv] = __popcll(bal);
        __syncthreads();
        int wbase = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < ANN_THREADS / 64; ++w) {
            const int c = s_wtot[w];
            if (w < wv) wbase += c;
            tot += c;
        }
        if (hit) {
            Item& it = items[wbase + before];
            it.xmin = r.xmin; it.xmax = r.xmax; it.ymin = r.ymin; it.ymax = r.ymax; it.ix1 = r.ix1; it.iy1 = r.iy1;
            const unsigned* se = reinterpret_cast<const unsigned*>(style + r.cls);
            it.head = se[0];
#pragma unroll
            for (int q = 0; q < 8; ++q) it.text[q] = se[1 + q];
        }
        __syncthreads();
        if (nv > 0) {
            for (int q = 0; q < tot; ++q) {
                const Item& it = items[q];
                const int xmin = it.xmin, xmax = it.xmax, ymin = it.ymin, ymax = it.ymax;
                if (it.iy1 < y0 || ymin - 20 > my1) continue;
                if (one_row && (it.ix1 < x0 || xmin - 1 > mx1)) continue;
                const unsigned head = it.head;
                const int len = (int)(head >> 24);
                const float dw = 0.8f * 255.f;
                float dc[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) dc[c] = 0.8f * (float)((head >> (8 * c)) & 255u);
                int x = x0, y = y0;
#pragma unroll
                for (int i = 0; i < ANN_PPT; ++i) {
                    if (i < nv) {
                        const bool in_x = x >= xmin - 1 && x <= xmax + 1;
                        const bool outline = in_x && y >= ymin - 1 && y <= ymax + 1 &&
                                             !(x >= xmin + 2 && x <= xmax - 2 && y >= ymin + 2 && y <= ymax - 2);
                        const bool tag = in_x && y >= ymin - 20 && y <= ymin;
                        bool text = false;
                        const int ty = y - (ymin - 18), tx = x - (xmin + 5);
                        if (ty >= 0 && ty < 14 && tx >= 0 && tx < 12 * len) {
                            const int ci = tx / 12, rem = tx - 12 * ci;
                            if (rem < 10) {
                                const int ch = (int)((it.text[ci >> 2] >> ((ci & 3) * 8)) & 255u);
                                text = ((glyph_row(ch, ty >> 1) >> (4 - (rem >> 1))) & 1u) != 0u;
                            }
                        }
                        if (outline || tag || text) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                const float d8 = text ? dw : dc[c];
                                const float sum = d8 + 0.2f * v[3 * i + c];
                                if constexpr (SF) v[3 * i + c] = sum;
                                else v[3 * i + c] = fminf(fmaxf(rintf(sum), 0.f), 255.f);      // saturate_cast<uchar>(cvRound)
                            }
                        }
                    }
                    if (++x == W) { x = 0; ++y; }
                }
            }
        }
        __syncthreads();      // the next chunk rewrites the list
    }

    // ---- out
    if (nv == 0) return;
    if (rgb_out) {
#pragma unroll
        for (int i = 0; i < ANN_PPT; ++i) {
            const float s = v[3 * i];
            v[3 * i] = v[3 * i + 2];
            v[3 * i + 2] = s;
        }
    }
    if constexpr (DF) {
        float* dp = reinterpret_cast<float*>(dst + im.dst_off) + (size_t)p0 * 3;
        if (nv == ANN_PPT) {
#pragma unroll
            for (int q = 0; q < 12; ++q) reinterpret_cast<float4*>(dp)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < ANN_PPT * 3; ++j)
                if (j < nv * 3) dp[j] = v[j];
        }
    } else {
        unsigned by[ANN_PPT * 3];
#pragma unroll
        for (int j = 0; j < ANN_PPT * 3; ++j) {
            float f = v[j];
            if constexpr (SF) f = f > 255.f ? 255.f : (f < 0.f ? 0.f : f);      // ImageSummary.push: clamp, then astype(uint8) truncates
            by[j] = (unsigned)(int)f;
        }
        unsigned char* dp = dst + im.dst_off + (size_t)p0 * 3;
        if (nv == ANN_PPT) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                unsigned wd[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 16 * q + 4 * e;
                    wd[e] = by[j] | (by[j + 1] << 8) | (by[j + 2] << 16) | (by[j + 3] << 24);
                }
                reinterpret_cast<uint4*>(dp)[q] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < ANN_PPT * 3; ++j)
                if (j < nv * 3) dp[j] = (unsigned char)by[j];
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
void annotate_rect(const int box1000[4], int w, int h, int out[4]) {
    SSD_REQUIRE(box1000 && out, "null argument");
    SSD_REQUIRE(w >= 1 && h >= 1 && w <= ANN_MAX_DIM && h <= ANN_MAX_DIM, "annotate: image size %d x %d outside 1..%d", w, h, ANN_MAX_DIM);
    rect_on_image(clamp_coord(box1000[0]), clamp_coord(box1000[1]), clamp_coord(box1000[2]), clamp_coord(box1000[3]), w, h, out);
}

void annotate_glyph(int ch, unsigned char rows[7]) {
    SSD_REQUIRE(rows != nullptr, "null argument");
    for (int r = 0; r < 7; ++r) rows[r] = (unsigned char)glyph_row(ch, r);
}

AnnotateStyle* annotate_style_create(int device, int num_classes, const unsigned char* colors_bgr, const char* names32) {
    require_num_classes(num_classes);
    SSD_REQUIRE(colors_bgr && names32, "null argument");
    std::vector<StyleEntry> tab(num_classes + 1);
    for (int c = 0; c <= num_classes; ++c) {
        StyleEntry& e = tab[c];
        memset(&e, 0, sizeof e);
        if (c == num_classes) {
            e.bgr[0] = e.bgr[1] = e.bgr[2] = 255;
            e.len = 1; e.text[0] = '?';
            continue;
        }
        for (int k = 0; k < 3; ++k) e.bgr[k] = colors_bgr[c * 3 + k];
        const char* nm = names32 + (size_t)c * 32;
        int len = 0;
        while (len < ANN_MAX_LABEL && nm[len]) ++len;      // labels are cut at 31 characters
        e.len = (unsigned char)len;
        memcpy(e.text, nm, len);
    }
    auto s = std::make_unique<AnnotateStyle>(device, num_classes);
    s->dev = static_cast<StyleEntry*>(s->hip.mem(tab.size() * sizeof(StyleEntry)));
    HIP_OK(hipMemcpy(s->dev, tab.data(), tab.size() * sizeof(StyleEntry), hipMemcpyHostToDevice));
    return s.release();
}

void annotate_style_destroy(AnnotateStyle* s) { delete s; }
int annotate_style_device(const AnnotateStyle* s) { return s->device; }

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

size_t annotate_ws_bytes(int b, int out_cap) {
    if (b < 1 || out_cap < 1) return 0;
    return up256((size_t)b * sizeof(DevImage)) + up256((size_t)b * sizeof(int)) + (size_t)b * out_cap * sizeof(BoxRec);
}

void annotate_batch(const void* src_dev, bool src_f32, const ssd_annotate_image* images_host, int b, const int* count_dev,
                    const int* cls_dev, const int* box_dev, int out_cap, bool grid1000, const AnnotateStyle* style, bool rgb_out,
                    void* dst_dev, bool dst_f32, void* ws, hipStream_t s) {
    SSD_REQUIRE(b >= 1, "annotate: batch %d must be >= 1", b);
    SSD_REQUIRE(out_cap >= 1, "annotate: out_cap must be >= 1");
    SSD_REQUIRE(src_dev && images_host && count_dev && cls_dev && box_dev && style && dst_dev && ws, "annotate: null argument");
    SSD_REQUIRE(src_f32 || !dst_f32, "annotate: a float32 destination needs a float32 source");
    SSD_REQUIRE((uintptr_t)src_dev % 16 == 0 && (uintptr_t)dst_dev % 16 == 0 && (uintptr_t)ws % 16 == 0, "annotate: src, dst and ws must be 16-byte aligned");
    std::vector<DevImage> imgs(b);
    long long tiles = 0;
    for (int i = 0; i < b; ++i) {
        const ssd_annotate_image& p = images_host[i];
        SSD_REQUIRE(p.src_w >= 1 && p.src_h >= 1 && p.dst_w >= 1 && p.dst_h >= 1, "annotate: image %d has zero size", i);
        SSD_REQUIRE(p.src_w <= ANN_MAX_DIM && p.src_h <= ANN_MAX_DIM && p.dst_w <= ANN_MAX_DIM && p.dst_h <= ANN_MAX_DIM,
                    "annotate: image %d is larger than %d pixels a side", i, ANN_MAX_DIM);
        SSD_REQUIRE(src_f32 || (p.src_w == p.dst_w && p.src_h == p.dst_h), "annotate: image %d: a resize needs a float32 source", i);
        SSD_REQUIRE(p.src_off % 16 == 0 && p.dst_off % 16 == 0, "annotate: image %d: offsets must be multiples of 16 bytes", i);
        DevImage& d = imgs[i];
        d.src_off = p.src_off; d.dst_off = p.dst_off;
        d.src_w = p.src_w; d.src_h = p.src_h; d.dst_w = p.dst_w; d.dst_h = p.dst_h;
        d.tile0 = (int)tiles; d.pad = 0;
        tiles += cdiv((long long)p.dst_w * p.dst_h, ANN_TILE);
        SSD_REQUIRE(tiles < (1ll << 30), "annotate: too many pixels in one call");
    }
    char* base = static_cast<char*>(ws);
    DevImage* imgs_dev = reinterpret_cast<DevImage*>(base);
    int* nbox = reinterpret_cast<int*>(base + up256((size_t)b * sizeof(DevImage)));
    BoxRec* recs = reinterpret_cast<BoxRec*>(base + up256((size_t)b * sizeof(DevImage)) + up256((size_t)b * sizeof(int)));
    HIP_OK(hipMemcpyAsync(imgs_dev, imgs.data(), (size_t)b * sizeof(DevImage), hipMemcpyHostToDevice, s));      // (pageable: copied by the call)
    {
        ProfScope prof("annotate_boxes", 0.0, (double)b * out_cap * (20 + sizeof(BoxRec)), s);
        hipLaunchKernelGGL(annotate_boxes_kernel, dim3(b), dim3(ANN_THREADS), 0, s, imgs_dev, count_dev, cls_dev, box_dev, out_cap,
                           grid1000 ? 1 : 0, style->num_classes, style->dev, nbox, recs);
    }
    {
        ProfScope prof("annotate_draw", 0.0, (double)tiles * ANN_TILE * 3 * ((src_f32 ? 4 : 1) + (dst_f32 ? 4 : 1)), s);
        const unsigned char* sp = static_cast<const unsigned char*>(src_dev);
        unsigned char* dp = static_cast<unsigned char*>(dst_dev);
        const dim3 grid((unsigned)tiles), block(ANN_THREADS);
        if (!src_f32)
            hipLaunchKernelGGL((annotate_draw_kernel<false, false>), grid, block, 0, s, sp, dp, imgs_dev, b, nbox, recs, out_cap, style->dev, rgb_out ? 1 : 0);
        else if (!dst_f32)
            hipLaunchKernelGGL((annotate_draw_kernel<true, false>), grid, block, 0, s, sp, dp, imgs_dev, b, nbox, recs, out_cap, style->dev, rgb_out ? 1 : 0);
        else
            hipLaunchKernelGGL((annotate_draw_kernel<true, true>), grid, block, 0, s, sp, dp, imgs_dev, b, nbox, recs, out_cap, style->dev, rgb_out ? 1 : 0);
    }
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
