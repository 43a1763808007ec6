// Baseline JPEG encode, bit-exact with libjpeg-turbo's default path: cv2.imwrite(<name>.jpg) of the reference's
// infer.py:247 and detect.py:124.  The decoder's split (jpeg.hip) mirrored.
//
// Device half: one launch per batch.
//   jpeg_fdct_kernel     16-bit fixed-point BGR -> YCbCr, h2v1 / h2v2 chroma downsampling with edge replication, libjpeg's "islow"
//                        8 x 8 forward DCT in int32, rounded division by the quantiser -> int16 coefficients in natural order,
//                        one [64] block after the other, per component plane padded to whole MCUs (the layout of ssd_jpeg_desc)
// It walks all images of the batch through a per-image prefix table of workgroups; nothing synchronises per image.
//
// Host half: Huffman coding with the Annex K tables + the file framing, native, batched and multi-threaded, one image per task.
// (jpeg_huff.hip is the same half on the GPU; it shares the header writer, the code tables and the descriptor rules below.)
// Every write is bounds-checked against the capacity the caller states.
#include "jpeg_enc.h"
#include <atomic>
#include <mutex>
#include <thread>

namespace ssd {

namespace {

const unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ISO 10918-1 Annex K.1, natural order
const unsigned char STD_LUMA_Q[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                      14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                      18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const unsigned char STD_CHROMA_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                        99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// ISO 10918-1 Annex K.3: code counts per length 1..16, then the symbols in code order
const unsigned char DC_LUMA_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const unsigned char DC_CHROMA_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const unsigned char DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char AC_LUMA_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const unsigned char AC_LUMA_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const unsigned char AC_CHROMA_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const unsigned char AC_CHROMA_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

bool sampling_ok(int hs, int vs) { return (hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2); }

size_t blocks_of(int w, int h, int hs, int vs) {
    const size_t mx = (size_t)(w + 8 * hs - 1) / (8 * hs), my = (size_t)(h + 8 * vs - 1) / (8 * vs);
    return mx * my * ((size_t)hs * vs + 2);
}

void require_shape(const int* shapes, int i) {
    const int h = shapes[2 * i], w = shapes[2 * i + 1];
    SSD_REQUIRE(w >= 1 && h >= 1 && w <= 16384 && h <= 16384, "jpeg: image %d: size %d x %d", i, w, h);
}

void require_batch(const int* shapes, int n, int sampling) {
    SSD_REQUIRE(n >= 1 && shapes, "jpeg: empty batch");
    SSD_REQUIRE(sampling == 0x11 || sampling == 0x21 || sampling == 0x22, "jpeg: sampling 0x%02x is not 0x11 (4:4:4), 0x21 (4:2:2) or 0x22 (4:2:0)", sampling);
    for (int i = 0; i < n; ++i) require_shape(shapes, i);
}

}  // namespace

void jpeg_quant_tables(int quality, unsigned short* luma, unsigned short* chroma) {
    SSD_REQUIRE(quality >= 1 && quality <= 100, "jpeg: quality must be in 1..100 (got %d)", quality);
    SSD_REQUIRE(luma && chroma, "jpeg: null argument");
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;          // jcparam.c jpeg_quality_scaling
    for (int k = 0; k < 64; ++k) {
        const int l = (STD_LUMA_Q[k] * scale + 50) / 100, c = (STD_CHROMA_Q[k] * scale + 50) / 100;
        luma[k] = (unsigned short)std::min(std::max(l, 1), 255);                  // (force_baseline)
        chroma[k] = (unsigned short)std::min(std::max(c, 1), 255);
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------------------------------
struct EncImage {
    int w, h, hs, vs;
    int rbw, rbh;                        // the luma plane's real blocks: libjpeg transforms these, the others up to whole MCUs are dummies
    int bw[3], bh[3];                    // component planes in 8 x 8 blocks (whole MCUs)
    int blk_pre[4];                      // prefix of the planes' block counts
    unsigned long long coef_off[3];      // int16 elements
    unsigned long long src_off;          // bytes
};

struct EncTables {                       // [0] luma, [1] chroma; natural order
    unsigned short q[2][64];
    unsigned recip[2][64];               // floor(2^32 / (8 q)) + 1: umulhi(n, recip) == n / (8 q) for n < 2^21
};

constexpr int FDCT_BLOCKS = 32;          // 8 x 8 blocks per workgroup of 256 (8 lanes per block)

// jfdctint.c (libjpeg's "islow" transform), one dimension, before the descale.  int32 is exact for 8-bit samples.
__device__ __forceinline__ void fdct_1d(const int* d, int* even04, int* o) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    even04[0] = t10 + t11;
    even04[1] = t10 - t11;
    int z1 = (t12 + t13) * 4433;
    o[2] = z1 + t13 * 6270;
    o[6] = z1 + t12 * -15137;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    o[7] = a4 + z1 + z3; o[5] = a5 + z2 + z4; o[3] = a6 + z2 + z3; o[1] = a7 + z1 + z4;      // (this order of sums is the one DESIGN.md 14 bounds)
}

// the image a workgroup belongs to: the last i with start[i] <= wg (wave-uniform)
__device__ __forceinline__ int enc_find_image(const int* __restrict__ start, int n, int wg) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= wg) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// jccolor.c rgb_ycc_convert, one component of the pixel at p (B, G, R)
__device__ __forceinline__ int ycc_at(const unsigned char* __restrict__ p, int comp) {
    const int B = p[0], G = p[1], R = p[2];
    if (comp == 0) return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    if (comp == 1) return (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    return (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
}

// 8 lanes per block.  Lane (block, i) converts (and, for chroma, downsamples) the 8 samples of row i straight from the packed
// pixels, transforms ROW i, then COLUMN i after a trip through LDS, quantises, and after a second trip stores the 8 coefficients
// of row i as one 16-byte vector (a wave writes 1 KiB of contiguous coefficients).
__global__ __launch_bounds__(256) void jpeg_fdct_kernel(const unsigned char* __restrict__ src, const EncImage* __restrict__ imgs,
                                                        const EncTables* __restrict__ tabs, const int* __restrict__ wg_start, int n,
                                                        short* __restrict__ coef) {
    __shared__ __attribute__((aligned(16))) int sw[FDCT_BLOCKS * 72];      // 72: the column pass's 64 lanes hit 64 different banks
    __shared__ __attribute__((aligned(16))) short sc[FDCT_BLOCKS * 64];
    const int img = enc_find_image(wg_start, n, blockIdx.x);
    const EncImage& D = imgs[img];
    const int tid = threadIdx.x, slot = tid >> 3, i = tid & 7;
    const int lb = (blockIdx.x - wg_start[img]) * FDCT_BLOCKS + slot;
    const bool valid = lb < D.blk_pre[3];
    const int comp = valid ? (lb >= D.blk_pre[1]) + (lb >= D.blk_pre[2]) : 0;
    const int b = lb - D.blk_pre[comp];
    const int w = D.w, h = D.h;
    bool dummy = false;
    if (valid) {
        const int bw = D.bw[comp];
        int by = b / bw, bx = b - by * bw;
        const unsigned char* base = src + D.src_off;
        int d[8];
        if (comp == 0) {
            // jccoefct.c compress_data: a luma block beyond the real ones has AC 0 and the DC of the block before it in the
            // MCU's order -- the block to its left, or for a whole dummy row the right block of the row above (itself possibly
            // a copy of its left neighbour).  So it transforms that block and keeps the DC.
            if (by >= D.rbh) { dummy = true; by -= 1; bx |= 1; }
            if (bx >= D.rbw) { dummy = true; bx = D.rbw - 1; }
            const int y = min(by * 8 + i, h - 1);
            const unsigned char* row = base + (size_t)y * w * 3;
#pragma unroll
            for (int c = 0; c < 8; ++c) d[c] = ycc_at(row + (size_t)min(bx * 8 + c, w - 1) * 3, 0) - 128;
        } else {
            // jcsample.c: the right edge is replicated in the full-size samples, the bottom edge in the full-size samples up to
            // a whole row group and in the DOWNSAMPLED rows from there on (jcprepct.c); the bias alternates along the output row.
            const int hs = D.hs, vs = D.vs;
            const int oy = min(by * 8 + i, (h + vs - 1) / vs - 1);
            const int shift = (hs == 2) + (vs == 2);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int ox = bx * 8 + c;
                int sum = hs == 1 ? 0 : (vs == 1 ? (c & 1) : 1 + (c & 1));
                for (int dy = 0; dy < vs; ++dy) {
                    const unsigned char* row = base + (size_t)min(oy * vs + dy, h - 1) * w * 3;
                    for (int dx = 0; dx < hs; ++dx) sum += ycc_at(row + (size_t)min(ox * hs + dx, w - 1) * 3, comp);
                }
                d[c] = (sum >> shift) - 128;
            }
        }
        int e[2], o[8];
        fdct_1d(d, e, o);
        int* r = sw + slot * 72 + i * 8;
        r[0] = e[0] << 2; r[4] = e[1] << 2;
        r[1] = (o[1] + 1024) >> 11; r[2] = (o[2] + 1024) >> 11; r[3] = (o[3] + 1024) >> 11;
        r[5] = (o[5] + 1024) >> 11; r[6] = (o[6] + 1024) >> 11; r[7] = (o[7] + 1024) >> 11;
    }
    __syncthreads();
    if (valid) {
        int d[8], e[2], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = sw[slot * 72 + r * 8 + i];
        fdct_1d(d, e, o);
        o[0] = (e[0] + 2) >> 2; o[4] = (e[1] + 2) >> 2;
        o[1] = (o[1] + 16384) >> 15; o[2] = (o[2] + 16384) >> 15; o[3] = (o[3] + 16384) >> 15;
        o[5] = (o[5] + 16384) >> 15; o[6] = (o[6] + 16384) >> 15; o[7] = (o[7] + 16384) >> 15;
        const int t = comp ? 1 : 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            // jcdctmgr.c quantize: divisor 8 q, half of it added to the magnitude, truncating division, sign restored
            const int k = r * 8 + i, v = o[r];
            const unsigned mag = (unsigned)(v < 0 ? -v : v) + ((unsigned)tabs->q[t][k] << 2);
            const int qv = (int)__umulhi(mag, tabs->recip[t][k]);
            sc[slot * 64 + k] = (short)((dummy && k) ? 0 : (v < 0 ? -qv : qv));
        }
    }
    __syncthreads();
    if (valid) *reinterpret_cast<uint4*>(coef + D.coef_off[comp] + (size_t)b * 64 + i * 8) = *reinterpret_cast<const uint4*>(sc + slot * 64 + i * 8);
}

namespace {
struct EncLayout {
    size_t tab_off, img_off, wg_off, total;
};
EncLayout enc_layout(int n) {
    EncLayout l;
    l.tab_off = 0;
    l.img_off = (sizeof(EncTables) + 255) / 256 * 256;
    l.wg_off = l.img_off + ((size_t)n * sizeof(EncImage) + 255) / 256 * 256;
    l.total = l.wg_off + ((size_t)(n + 1) * sizeof(int) + 255) / 256 * 256;
    return l;
}
}  // namespace

size_t jpeg_enc_coef_bytes(const int* shapes, int n, int sampling) {
    require_batch(shapes, n, sampling);
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += blocks_of(shapes[2 * i + 1], shapes[2 * i], sampling >> 4, sampling & 15) * 64 * sizeof(short);
    return total;
}

size_t jpeg_enc_ws_bytes(const int* shapes, int n, int sampling) {
    require_batch(shapes, n, sampling);
    return enc_layout(n).total;
}

void jpeg_encode_batch(const unsigned char* src_dev, size_t src_bytes, const unsigned long long* src_offs, const int* shapes, int n,
                       int quality, int sampling, short* coef_dev, size_t coef_bytes, ssd_jpeg_desc* descs_out, void* ws,
                       size_t ws_bytes, hipStream_t s) {
    require_batch(shapes, n, sampling);
    SSD_REQUIRE(src_dev && src_offs && coef_dev && descs_out && ws, "jpeg: null argument");
    SSD_REQUIRE(((uintptr_t)coef_dev | (uintptr_t)ws) % 16 == 0, "jpeg: coef_dev and ws_dev must be 16-byte aligned");
    const EncLayout l = enc_layout(n);
    SSD_REQUIRE(ws_bytes >= l.total, "jpeg: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    const size_t need = jpeg_enc_coef_bytes(shapes, n, sampling);
    SSD_REQUIRE(coef_bytes >= need, "jpeg: the coefficient buffer holds %zu bytes, the batch needs %zu", coef_bytes, need);
    // (the staging block outlives the call: the copy below reads it)
    static thread_local std::vector<unsigned char> staging;
    staging.assign(l.total, 0);
    EncTables* T = reinterpret_cast<EncTables*>(staging.data() + l.tab_off);
    EncImage* imgs = reinterpret_cast<EncImage*>(staging.data() + l.img_off);
    int* wg = reinterpret_cast<int*>(staging.data() + l.wg_off);
    jpeg_quant_tables(quality, T->q[0], T->q[1]);
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) T->recip[t][k] = (unsigned)((1ull << 32) / ((unsigned)T->q[t][k] << 3)) + 1;
    const int hs = sampling >> 4, vs = sampling & 15;
    long long n1 = 0;
    size_t co = 0;
    double blocks = 0, pixels = 0;
    for (int i = 0; i < n; ++i) {
        const int h = shapes[2 * i], w = shapes[2 * i + 1];
        const size_t bytes = (size_t)w * h * 3;
        SSD_REQUIRE(src_offs[i] <= src_bytes && bytes <= src_bytes - src_offs[i], "jpeg: image %d: %zu bytes at offset %llu outside the %zu-byte source", i,
                    bytes, src_offs[i], src_bytes);
        ssd_jpeg_desc& d = descs_out[i];
        memset(&d, 0, sizeof d);
        d.width = w; d.height = h; d.components = 3; d.hs = hs; d.vs = vs;
        d.mcus_x = (w + 8 * hs - 1) / (8 * hs);
        d.mcus_y = (h + 8 * vs - 1) / (8 * vs);
        d.dst_off = src_offs[i];
        EncImage& D = imgs[i];
        D.w = w; D.h = h; D.hs = hs; D.vs = vs;
        D.rbw = (w + 7) / 8; D.rbh = (h + 7) / 8;
        D.src_off = src_offs[i];
        D.blk_pre[0] = 0;
        for (int c = 0; c < 3; ++c) {
            D.bw[c] = d.mcus_x * (c == 0 ? hs : 1);
            D.bh[c] = d.mcus_y * (c == 0 ? vs : 1);
            const size_t nb = (size_t)D.bw[c] * D.bh[c];
            D.blk_pre[c + 1] = D.blk_pre[c] + (int)nb;
            D.coef_off[c] = d.coef_off[c] = co;
            co += nb * 64;
            memcpy(d.qt[c], T->q[c ? 1 : 0], sizeof d.qt[c]);
        }
        wg[i] = (int)n1;
        n1 += cdiv(D.blk_pre[3], FDCT_BLOCKS);
        blocks += D.blk_pre[3];
        pixels += (double)w * h;
    }
    SSD_REQUIRE(n1 < (1ll << 30), "jpeg: batch too large for one launch");
    wg[n] = (int)n1;
    char* base = static_cast<char*>(ws);
    HIP_OK(hipMemcpyAsync(base, staging.data(), l.total, hipMemcpyHostToDevice, s));
    {
        ProfScope prof("jpeg_fdct", 0.0, pixels * 3 + blocks * 128, s);
        hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)n1), dim3(256), 0, s, src_dev, reinterpret_cast<const EncImage*>(base + l.img_off),
                           reinterpret_cast<const EncTables*>(base + l.tab_off), reinterpret_cast<const int*>(base + l.wg_off), n, coef_dev);
    }
    HIP_OK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------------------------------
// host: Huffman coder + file framing
// ------------------------------------------------------------------------------------------------------------------------
namespace {

struct EncHuff {
    unsigned short code[256];
    unsigned char len[256];          // 0: the symbol has no code
};

void build_enc_huffman(EncHuff& h, const unsigned char* counts, const unsigned char* vals) {
    memset(&h, 0, sizeof h);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < counts[l - 1]; ++i, ++k) {
            h.code[vals[k]] = (unsigned short)code++;
            h.len[vals[k]] = (unsigned char)l;
        }
        code <<= 1;
    }
}

struct EncTablesHost {
    EncHuff dc[2], ac[2];
    EncTablesHost() {
        build_enc_huffman(dc[0], DC_LUMA_BITS, DC_VALS);
        build_enc_huffman(dc[1], DC_CHROMA_BITS, DC_VALS);
        build_enc_huffman(ac[0], AC_LUMA_BITS, AC_LUMA_VALS);
        build_enc_huffman(ac[1], AC_CHROMA_BITS, AC_CHROMA_VALS);
    }
};
const EncTablesHost& enc_tables() {
    static const EncTablesHost t;
    return t;
}

constexpr size_t HEADER_BYTES = 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 14;
constexpr size_t BLOCK_BYTES = 416;          // (11 + 11 + 63 * (16 + 10)) bits = 208 bytes, every one of them stuffed

struct Writer {
    unsigned char* p;
    unsigned char* end;
    uint64_t acc = 0;
    int cnt = 0;                     // bits waiting in acc (< 8 between calls)

    void need(size_t k) const {
        if ((size_t)(end - p) < k) fail("jpeg: the output buffer is too small for the file");
    }
    void byte(int v) { need(1); *p++ = (unsigned char)v; }
    void be16(int v) { byte(v >> 8); byte(v & 255); }
    void bytes(const unsigned char* v, size_t k) { need(k); memcpy(p, v, k); p += k; }
    template <bool CHECKED> void bits(unsigned code, int len) {        // len <= 32
        acc = (acc << len) | code;
        cnt += len;
        while (cnt >= 8) {
            const unsigned char c = (unsigned char)(acc >> (cnt - 8));
            if (CHECKED) need(c == 0xFF ? 2 : 1);
            *p++ = c;
            if (c == 0xFF) *p++ = 0;
            cnt -= 8;
        }
    }
    void flush() {
        if (cnt) bits<true>((1u << (8 - cnt)) - 1, 8 - cnt);           // the last byte is padded with 1-bits
        acc = 0;
    }
};

inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// jchuff.c encode_one_block
template <bool CHECKED> void encode_block(Writer& W, const short* blk, int& pred, const EncHuff& dc, const EncHuff& ac) {
    int diff = (int)blk[0] - pred;
    pred = blk[0];
    int mag = diff < 0 ? -diff : diff, low = diff < 0 ? diff - 1 : diff;
    int nb = bit_length((unsigned)mag);
    if (nb > 11) fail("jpeg: DC difference %d needs %d bits, baseline Huffman codes 11", diff, nb);
    W.bits<CHECKED>(((unsigned)dc.code[nb] << nb) | ((unsigned)low & ((1u << nb) - 1)), dc.len[nb] + nb);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[ZIGZAG[k]];
        if (v == 0) { ++run; continue; }
        while (run > 15) { W.bits<CHECKED>(ac.code[0xF0], ac.len[0xF0]); run -= 16; }
        mag = v < 0 ? -v : v;
        low = v < 0 ? v - 1 : v;
        nb = bit_length((unsigned)mag);
        if (nb > 10) fail("jpeg: AC coefficient %d needs %d bits, baseline Huffman codes 10", v, nb);
        const int sym = (run << 4) | nb;
        W.bits<CHECKED>(((unsigned)ac.code[sym] << nb) | ((unsigned)low & ((1u << nb) - 1)), ac.len[sym] + nb);
        run = 0;
    }
    if (run) W.bits<CHECKED>(ac.code[0], ac.len[0]);
}

void require_enc_desc(const ssd_jpeg_desc& d, size_t coef_bytes, int i) {
    SSD_REQUIRE(d.width >= 1 && d.height >= 1 && d.width <= 16384 && d.height <= 16384, "jpeg: image %d: size %d x %d", i, d.width, d.height);
    SSD_REQUIRE(d.components == 3, "jpeg: image %d: %d components, the encoder writes 3", i, d.components);
    SSD_REQUIRE(sampling_ok(d.hs, d.vs), "jpeg: image %d: luma sampling %dx%d", i, d.hs, d.vs);
    SSD_REQUIRE(d.mcus_x == (d.width + 8 * d.hs - 1) / (8 * d.hs) && d.mcus_y == (d.height + 8 * d.vs - 1) / (8 * d.vs),
                "jpeg: image %d: %d x %d MCUs do not match its %d x %d pixels", i, d.mcus_x, d.mcus_y, d.width, d.height);
    for (int c = 0; c < 3; ++c) {
        const size_t nb = (size_t)d.mcus_x * d.mcus_y * (c == 0 ? d.hs * d.vs : 1);
        SSD_REQUIRE(d.coef_off[c] <= coef_bytes / 2 && nb * 64 <= coef_bytes / 2 - d.coef_off[c],
                    "jpeg: image %d: coefficient plane %d (offset %llu, %zu blocks) outside the %zu-byte buffer", i, c, d.coef_off[c], nb, coef_bytes);
        for (int k = 0; k < 64; ++k)
            SSD_REQUIRE(d.qt[c][k] >= 1 && d.qt[c][k] <= 255, "jpeg: image %d: quantiser %d outside 1..255 (baseline)", i, d.qt[c][k]);
    }
    SSD_REQUIRE(memcmp(d.qt[1], d.qt[2], sizeof d.qt[1]) == 0, "jpeg: image %d: Cb and Cr must share one quantisation table", i);
}

void write_dht(Writer& W, int tc_th, const unsigned char* counts, const unsigned char* vals, int total) {
    W.be16(0xFFC4); W.be16(2 + 1 + 16 + total); W.byte(tc_th);
    W.bytes(counts, 16); W.bytes(vals, (size_t)total);
}

// jcmarker.c: write_file_header, write_frame_header, write_scan_header -- the HEADER_BYTES in front of the scan
void write_header(Writer& W, const ssd_jpeg_desc& d) {
    static const unsigned char APP0[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    W.be16(0xFFD8);
    W.bytes(APP0, sizeof APP0);
    for (int t = 0; t < 2; ++t) {
        W.be16(0xFFDB); W.be16(67); W.byte(t);
        for (int k = 0; k < 64; ++k) W.byte(d.qt[t][ZIGZAG[k]]);
    }
    W.be16(0xFFC0); W.be16(17); W.byte(8); W.be16(d.height); W.be16(d.width); W.byte(3);
    W.byte(1); W.byte(d.hs * 16 + d.vs); W.byte(0);
    W.byte(2); W.byte(0x11); W.byte(1);
    W.byte(3); W.byte(0x11); W.byte(1);
    write_dht(W, 0x00, DC_LUMA_BITS, DC_VALS, 12);
    write_dht(W, 0x10, AC_LUMA_BITS, AC_LUMA_VALS, 162);
    write_dht(W, 0x01, DC_CHROMA_BITS, DC_VALS, 12);
    write_dht(W, 0x11, AC_CHROMA_BITS, AC_CHROMA_VALS, 162);
    static const unsigned char SOS[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    W.bytes(SOS, sizeof SOS);
}

size_t entropy_encode(const short* coef, const ssd_jpeg_desc& d, unsigned char* out, size_t out_cap) {
    Writer W{out, out + out_cap};
    write_header(W, d);
    const EncTablesHost& T = enc_tables();
    int pred[3] = {0, 0, 0};
    for (int y = 0; y < d.mcus_y; ++y)
        for (int x = 0; x < d.mcus_x; ++x) {
            const bool fast = (size_t)(W.end - W.p) >= BLOCK_BYTES * 6 + 8;
            for (int ci = 0; ci < 3; ++ci) {
                const int h = ci == 0 ? d.hs : 1, v = ci == 0 ? d.vs : 1, t = ci ? 1 : 0;
                const size_t bw = (size_t)d.mcus_x * h;
                for (int by = 0; by < v; ++by)
                    for (int bx = 0; bx < h; ++bx) {
                        const short* blk = coef + d.coef_off[ci] + (((size_t)y * v + by) * bw + (size_t)x * h + bx) * 64;
                        if (fast) encode_block<false>(W, blk, pred[ci], T.dc[t], T.ac[t]);
                        else encode_block<true>(W, blk, pred[ci], T.dc[t], T.ac[t]);
                    }
            }
        }
    W.flush();
    W.be16(0xFFD9);
    return (size_t)(W.p - out);
}

}  // namespace

static_assert(HEADER_BYTES == SSD_JPEG_HEADER_BYTES, "the header the host stage writes");

void jpeg_require_enc_desc(const ssd_jpeg_desc& d, size_t coef_bytes, int i) { require_enc_desc(d, coef_bytes, i); }

void jpeg_file_header(const ssd_jpeg_desc& d, unsigned char* out) {
    SSD_REQUIRE(out, "jpeg: null argument");
    require_enc_desc(d, (size_t)-1, 0);
    Writer W{out, out + HEADER_BYTES};
    write_header(W, d);
}

void jpeg_huff_code_tables(unsigned dc[2][16], unsigned ac[2][256]) {
    const EncTablesHost& T = enc_tables();
    for (int t = 0; t < 2; ++t) {
        for (int k = 0; k < 16; ++k) dc[t][k] = T.dc[t].code[k] | ((unsigned)T.dc[t].len[k] << 16);
        for (int k = 0; k < 256; ++k) ac[t][k] = T.ac[t].code[k] | ((unsigned)T.ac[t].len[k] << 16);
    }
}

size_t jpeg_file_bound(const ssd_jpeg_desc& d) {
    SSD_REQUIRE(d.width >= 1 && d.height >= 1 && d.width <= 16384 && d.height <= 16384, "jpeg: size %d x %d", d.width, d.height);
    SSD_REQUIRE(sampling_ok(d.hs, d.vs), "jpeg: luma sampling %dx%d", d.hs, d.vs);
    return HEADER_BYTES + blocks_of(d.width, d.height, d.hs, d.vs) * BLOCK_BYTES + 16;
}

size_t jpeg_entropy_encode(const short* coef, size_t coef_bytes, const ssd_jpeg_desc& d, unsigned char* out, size_t out_cap) {
    SSD_REQUIRE(coef && out, "jpeg: null argument");
    require_enc_desc(d, coef_bytes, 0);
    return entropy_encode(coef, d, out, out_cap);
}

void jpeg_entropy_encode_batch(const short* coef, size_t coef_bytes, const ssd_jpeg_desc* descs, int n, int threads,
                               unsigned char* out, size_t out_bytes, const unsigned long long* out_offsets,
                               unsigned long long* out_sizes) {
    SSD_REQUIRE(n >= 1 && coef && descs && out && out_offsets && out_sizes, "jpeg: null argument or empty batch");
    SSD_REQUIRE(threads >= 1 && threads <= 64, "jpeg: threads must be in 1..64 (got %d)", threads);
    for (int i = 0; i < n; ++i) {
        SSD_REQUIRE(out_offsets[i] <= out_offsets[i + 1], "jpeg: output offsets must ascend (image %d)", i);
        require_enc_desc(descs[i], coef_bytes, i);
    }
    SSD_REQUIRE(out_offsets[n] <= out_bytes, "jpeg: the last output offset %llu is past the %zu-byte buffer", out_offsets[n], out_bytes);
    std::atomic<int> next{0};
    std::mutex mu;
    int first_bad = n;
    std::string first_msg;
    auto work = [&]() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n) return;
            try {
                out_sizes[i] = entropy_encode(coef, descs[i], out + out_offsets[i], (size_t)(out_offsets[i + 1] - out_offsets[i]));
            } catch (const std::exception& e) {
                out_sizes[i] = 0;
                std::lock_guard<std::mutex> lock(mu);
                if (i < first_bad) { first_bad = i; first_msg = e.what(); }
            }
        }
    };
    const int nt = threads < n ? threads : n;
    if (nt <= 1) work();
    else {
        std::vector<std::thread> pool;
        for (int t = 0; t < nt; ++t) pool.emplace_back(work);
        for (auto& t : pool) t.join();
    }
    if (first_bad < n) fail("image %d: %s", first_bad, first_msg.c_str());
}

}  // namespace ssd
