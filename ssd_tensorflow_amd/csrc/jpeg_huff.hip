// Baseline JPEG Huffman coding and file framing on the GPU: what jchuff.c encode_one_block and jcmarker.c do, from
// the int16 coefficients jpeg_fdct_kernel (jpeg_enc.hip) leaves to complete JFIF files in one device buffer.  The bytes equal the
// host stage's (jpeg_enc.hip entropy_encode), which equal libjpeg-turbo's.
//
// A block's code depends on its own 64 coefficients and on the DC of its predecessor of the same component, which index
// arithmetic finds; bit positions are a prefix sum.  Seven launches per batch on the caller's stream, the kernel boundary the only
// synchronisation between workgroups; all images of a batch walk through per-image prefix tables of workgroups:
//   jpeg_huff_count    bits of every run of HUFF_BLOCKS blocks in scan order; a value baseline Huffman cannot code -> status
//   jpeg_huff_scan     per image: exclusive 64-bit prefix of those sums; zeroes the stream words two workgroups will share
//   jpeg_huff_emit     the codes again, assembled in LDS at the run's bit position, whole words to the unstuffed stream
//   jpeg_huff_ffcount  FF bytes per STUFF_CHUNK of the stream (the last byte padded with 1-bits first)
//   jpeg_huff_ffscan   per image: exclusive prefix of those counts, the file's size
//   jpeg_huff_offsets  file i starts at the sum of the sizes before it, each rounded up to 16; the records
//   jpeg_huff_write    header, stuffed scan, EOI
// An image with status != 0 is skipped by every pass after the first (decided per workgroup from the status word).
//
// Lane k of a wave holds zigzag position k of one block: __ballot(v != 0) is the block's nonzero map, the run in front of a
// coefficient comes from that mask, and a lane's whole contribution -- up to three ZRL codes, its run / size code and the value
// bits: 3 * 11 + 16 + 10 = 59 bits -- fits one 64-bit word that goes to LDS with at most three 32-bit ORs.
#include "jpeg_huff.h"
#include "jpeg_enc.h"

namespace ssd {

namespace {
constexpr int HUFF_BLOCKS = 32;                      // blocks per workgroup of 256: 8 lanes load a block, a wave codes 8 of them
constexpr int BLOCK_MAX_BITS = 1660;                 // >= 9 + 11 + 63 * (16 + 10) bits of a codeable block
constexpr int BLOCK_MAX_BYTES = 208;
constexpr int EMIT_WORDS = (31 + HUFF_BLOCKS * BLOCK_MAX_BITS + 31) / 32 + 3;      // a run at any bit phase (+ a lane's reach)
constexpr int STUFF_CHUNK = 4096;                    // stream bytes per workgroup of 256: one 16-byte vector per lane
constexpr int HEADER_STRIDE = 640;                   // SSD_JPEG_HEADER_BYTES rounded up
}  // namespace

struct HuffImage {
    int hs, vs, mcus_x, nblocks;                     // nblocks in scan order: MCUs of hs * vs luma blocks, Cb, Cr
    int bpm, nluma, bw0, pad;                        // blocks per MCU, luma blocks per MCU, luma plane's width in blocks
    unsigned long long coef_off[3];                  // int16 elements
    unsigned long long stream_off, stream_cap;       // the unstuffed stream inside the workspace, bytes (16-byte aligned)
};

struct HuffArgs {
    const unsigned* tabs;                            // [2][16] DC by category, [2][256] AC by run << 4 | size: code | length << 16
    const HuffImage* imgs;
    const int* wg_start;                             // [n + 1] prefix of the images' workgroups of HUFF_BLOCKS
    const int* ck_start;                             // [n + 1] prefix of the images' workgroups of STUFF_CHUNK
    const unsigned char* headers;                    // [n][HEADER_STRIDE]
    int* status;                                     // [n]
    unsigned long long* total_bits;                  // [n]
    unsigned long long* sizes;                       // [n]
    unsigned* wg_bits;                               // per count workgroup
    unsigned long long* wg_pos;
    unsigned* ck_ff;                                 // per stuff workgroup
    unsigned* ck_pos;
    unsigned char* ws;
    int n;
};

__constant__ unsigned char HUFF_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the image a workgroup belongs to: the last i with start[i] <= wg (wave-uniform)
__device__ __forceinline__ int huff_find_image(const int* __restrict__ start, int n, int wg) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= wg) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// first coefficient of block s of the scan, and its table (0 luma, 1 chroma)
__device__ __forceinline__ unsigned long long huff_block_elem(const HuffImage& D, int s, int* table) {
    const int mcu = s / D.bpm, j = s - mcu * D.bpm;
    if (j < D.nluma) {
        const int my = mcu / D.mcus_x, mx = mcu - my * D.mcus_x;
        const int by = j >> (D.hs - 1), bx = j & (D.hs - 1);
        *table = 0;
        return D.coef_off[0] + ((unsigned long long)(my * D.vs + by) * D.bw0 + (unsigned)(mx * D.hs + bx)) * 64;
    }
    *table = 1;
    return D.coef_off[j - D.nluma + 1] + (unsigned long long)mcu * 64;
}

// the block before s in its component, -1 for the component's first
__device__ __forceinline__ int huff_pred_block(const HuffImage& D, int s) {
    const int mcu = s / D.bpm, j = s - mcu * D.bpm;
    if (j > 0 && j < D.nluma) return s - 1;
    if (mcu == 0) return -1;
    return j == 0 ? s - 3 : s - D.bpm;
}

// 8 lanes per block: the 64 coefficients of the workgroup's blocks as 16-byte vectors into LDS, natural order, with each
// block's DC prediction and table
__device__ __forceinline__ void huff_load_blocks(const HuffImage& D, const short* __restrict__ coef, int first, short* sc, int* spred,
                                                 int* stab) {
    const int tid = threadIdx.x, slot = tid >> 3, i = tid & 7;
    const int s = first + slot;
    if (s < D.nblocks) {
        int t;
        const unsigned long long e = huff_block_elem(D, s, &t);
        *reinterpret_cast<uint4*>(sc + slot * 64 + i * 8) = *reinterpret_cast<const uint4*>(coef + e + i * 8);
        if (i == 0) {
            const int p = huff_pred_block(D, s);
            int tp;
            spred[slot] = p < 0 ? 0 : (int)coef[huff_block_elem(D, p, &tp)];
            stab[slot] = t;
        }
    }
}

__device__ __forceinline__ void huff_load_tables(const unsigned* __restrict__ tabs, unsigned* st) {
    for (int i = threadIdx.x; i < 2 * 16 + 2 * 256; i += 256) st[i] = tabs[i];
}

__device__ __forceinline__ int huff_bit_length(unsigned v) { return v ? 32 - __clz((int)v) : 0; }

struct LaneCode {
    unsigned long long val;          // the lane's bits, right-aligned
    int len;                         // 0..59 for a codeable block
    int flag;                        // 0, 1 (DC difference beyond 11 bits), 2 (AC beyond 10 bits)
};

// jchuff.c encode_one_block for the lane that holds zigzag position k; every lane of the wave calls it (ballot)
__device__ __forceinline__ LaneCode huff_lane_code(int v, int k, int pred, int t, const unsigned* st) {
    const unsigned long long nz = __ballot(v != 0);
    const unsigned* dc = st + t * 16;
    const unsigned* ac = st + 32 + t * 256;
    LaneCode r;
    r.val = 0; r.len = 0; r.flag = 0;
    if (k == 0) {
        const int diff = v - pred;
        const int nb = huff_bit_length((unsigned)(diff < 0 ? -diff : diff));
        const unsigned low = (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1);          // nb <= 17
        const unsigned e = dc[nb < 15 ? nb : 15];
        r.flag = nb > 11 ? 1 : 0;
        r.val = ((unsigned long long)(e & 0xffff) << nb) | low;
        r.len = (int)(e >> 16) + nb;
    } else if (v != 0) {
        const unsigned long long below = nz & ((1ull << k) - 1) & ~1ull;
        const int p = below ? 63 - __clzll((long long)below) : 0;
        const int run = k - 1 - p, z = run >> 4;
        const int nb = huff_bit_length((unsigned)(v < 0 ? -v : v));
        const unsigned low = (unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1);                   // nb <= 16
        const unsigned e = ac[((run & 15) << 4) | (nb < 15 ? nb : 15)];
        const unsigned zrl = ac[0xF0];
        const unsigned long long zc = zrl & 0xffff;
        const int zl = (int)(zrl >> 16), l = (int)(e >> 16) + nb;
        const unsigned long long z2 = (zc << zl) | zc;
        const unsigned long long zv = z == 0 ? 0 : (z == 1 ? zc : (z == 2 ? z2 : ((z2 << zl) | zc)));
        r.flag = nb > 10 ? 2 : 0;
        r.val = (zv << l) | ((unsigned long long)(e & 0xffff) << nb) | low;
        r.len = z * zl + l;
    } else if (k == 63) {
        const unsigned e = ac[0];                                                                // EOB: the block ends in zeros
        r.val = e & 0xffff;
        r.len = (int)(e >> 16);
    }
    return r;
}

__device__ __forceinline__ int wave_incl_scan(int x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// exclusive prefix over the workgroup's 256 values and their sum; sh: 4 values of LDS (free again on return)
template <class T> __device__ __forceinline__ T wg_excl_scan(T x, T* total, T* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const T v = sh[w];
        if (w < wave) before += v;
        all += v;
    }
    __syncthreads();
    *total = all;
    return before + incl - x;
}

// (a) bits per workgroup of HUFF_BLOCKS blocks; the image's status
__global__ __launch_bounds__(256) void jpeg_huff_count_kernel(const short* __restrict__ coef, HuffArgs A) {
    __shared__ __attribute__((aligned(16))) short sc[HUFF_BLOCKS * 64];
    __shared__ unsigned st[2 * 16 + 2 * 256];
    __shared__ int spred[HUFF_BLOCKS], stab[HUFF_BLOCKS], swave[4];
    const int img = huff_find_image(A.wg_start, A.n, blockIdx.x);
    const HuffImage& D = A.imgs[img];
    const int first = (blockIdx.x - A.wg_start[img]) * HUFF_BLOCKS;
    huff_load_tables(A.tabs, st);
    huff_load_blocks(D, coef, first, sc, spred, stab);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, zz = HUFF_ZIGZAG[lane];
    int bits = 0, flag = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int slot = wave * 8 + j;
        if (first + slot < D.nblocks) {                                  // (wave-uniform)
            const LaneCode c = huff_lane_code(sc[slot * 64 + zz], lane, spred[slot], stab[slot], st);
            bits += c.len;
            flag = max(flag, c.flag);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        bits += __shfl_xor(bits, d);
        flag = max(flag, __shfl_xor(flag, d));
    }
    if (lane == 0) {
        swave[wave] = bits;
        if (flag) atomicMax(A.status + img, flag);
    }
    __syncthreads();
    if (threadIdx.x == 0) A.wg_bits[blockIdx.x] = (unsigned)(swave[0] + swave[1] + swave[2] + swave[3]);
}

// (b) one workgroup per image: where every count workgroup's bits start; the two stream words each of them may share with a
// neighbour are cleared here, a launch ahead of the ORs
__global__ __launch_bounds__(256) void jpeg_huff_scan_kernel(HuffArgs A) {
    __shared__ unsigned long long sh[4];
    const int img = blockIdx.x, tid = threadIdx.x;
    if (A.status[img] != 0) {
        if (tid == 0) A.total_bits[img] = 0;
        return;
    }
    const HuffImage& D = A.imgs[img];
    const int w0 = A.wg_start[img], nwg = A.wg_start[img + 1] - w0;
    unsigned* words = reinterpret_cast<unsigned*>(A.ws + D.stream_off);
    const unsigned long long cap_words = D.stream_cap / 4;
    unsigned long long carry = 0;
    for (int base = 0; base < nwg; base += 256) {
        const bool valid = base + tid < nwg;
        const unsigned long long x = valid ? A.wg_bits[w0 + base + tid] : 0;
        unsigned long long total;
        const unsigned long long pos = carry + wg_excl_scan(x, &total, sh);
        if (valid) {
            A.wg_pos[w0 + base + tid] = pos;
            const unsigned long long a = pos >> 5, b = (pos + x - (x ? 1 : 0)) >> 5;
            if (a < cap_words) words[a] = 0;
            if (b < cap_words) words[b] = 0;
        }
        carry += total;
    }
    if (tid == 0) A.total_bits[img] = carry;
}

// (c) every block's codes at its bit position of the unstuffed stream (bit 0 = the MSB of byte 0)
__global__ __launch_bounds__(256) void jpeg_huff_emit_kernel(const short* __restrict__ coef, HuffArgs A) {
    __shared__ __attribute__((aligned(16))) short sc[HUFF_BLOCKS * 64];
    __shared__ unsigned st[2 * 16 + 2 * 256];
    __shared__ int spred[HUFF_BLOCKS], stab[HUFF_BLOCKS], sblk[HUFF_BLOCKS];
    __shared__ unsigned sbits[EMIT_WORDS];                               // big-endian words: stream bit 32 w + i = bit 31 - i of word w
    const int img = huff_find_image(A.wg_start, A.n, blockIdx.x);
    if (A.status[img] != 0) return;
    const HuffImage& D = A.imgs[img];
    const int first = (blockIdx.x - A.wg_start[img]) * HUFF_BLOCKS;
    huff_load_tables(A.tabs, st);
    huff_load_blocks(D, coef, first, sc, spred, stab);
    for (int i = threadIdx.x; i < EMIT_WORDS; i += 256) sbits[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, zz = HUFF_ZIGZAG[lane];
    unsigned long long val[8];
    int len[8], off[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int slot = wave * 8 + j;
        val[j] = 0; len[j] = 0; off[j] = 0;
        int total = 0;
        if (first + slot < D.nblocks) {                                  // (wave-uniform)
            const LaneCode c = huff_lane_code(sc[slot * 64 + zz], lane, spred[slot], stab[slot], st);
            const int incl = wave_incl_scan(c.len, lane);
            val[j] = c.val; len[j] = c.len; off[j] = incl - c.len;
            total = __shfl(incl, 63);
        }
        if (lane == 0) sblk[slot] = total;
    }
    __syncthreads();
    const unsigned long long start = A.wg_pos[blockIdx.x];
    const int phase = (int)(start & 31);
    const int mine = lane < HUFF_BLOCKS ? sblk[lane] : 0;
    const int incl = wave_incl_scan(mine, lane);
    const int all = __shfl(incl, 63);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int at = __shfl(incl - mine, wave * 8 + j);
        if (len[j] > 0) {
            const int p = phase + at + off[j], w = p >> 5, sh = p & 31;
            if (w + 2 < EMIT_WORDS) {                                    // (always, for the codeable blocks this pass is run on)
                const unsigned long long hi = val[j] << (64 - len[j]);   // left-aligned; its low 5 bits are 0
                const unsigned long long a = hi >> sh;
                const unsigned w0 = (unsigned)(a >> 32), w1 = (unsigned)a, w2 = sh ? (unsigned)hi << (32 - sh) : 0u;
                if (w0) atomicOr(sbits + w, w0);
                if (w1) atomicOr(sbits + w + 1, w1);
                if (w2) atomicOr(sbits + w + 2, w2);
            }
        }
    }
    __syncthreads();
    int nwords = (phase + all + 31) >> 5;
    nwords = nwords < EMIT_WORDS ? nwords : EMIT_WORDS;
    unsigned* words = reinterpret_cast<unsigned*>(A.ws + D.stream_off);
    const unsigned long long g0 = start >> 5, cap_words = D.stream_cap / 4;
    for (int i = threadIdx.x; i < nwords; i += 256) {
        if (g0 + i >= cap_words) break;
        const unsigned v = __builtin_bswap32(sbits[i]);
        if (i == 0 || i == nwords - 1) atomicOr(words + g0 + i, v);      // shared with the neighbour; cleared by jpeg_huff_scan_kernel
        else words[g0 + i] = v;
    }
}

// 16 bytes of the stream at b0 (a multiple of 16 below `bytes`), the last byte of the stream padded with 1-bits
__device__ __forceinline__ uint4 huff_load16(const unsigned char* __restrict__ stream, unsigned long long b0, unsigned long long bytes,
                                             unsigned pad) {
    uint4 v = *reinterpret_cast<const uint4*>(stream + b0);
    const unsigned long long last = bytes - 1;
    if (last >= b0 && last < b0 + 16) {
        const unsigned q = (unsigned)(last - b0), m = pad << ((q & 3) * 8);
        if ((q >> 2) == 0) v.x |= m;
        else if ((q >> 2) == 1) v.y |= m;
        else if ((q >> 2) == 2) v.z |= m;
        else v.w |= m;
    }
    return v;
}

__device__ __forceinline__ unsigned huff_byte(const uint4& v, int q) {
    const unsigned w = (q >> 2) == 0 ? v.x : ((q >> 2) == 1 ? v.y : ((q >> 2) == 2 ? v.z : v.w));
    return (w >> ((q & 3) * 8)) & 255u;
}

// (d) FF bytes per chunk
__global__ __launch_bounds__(256) void jpeg_huff_ffcount_kernel(HuffArgs A) {
    __shared__ unsigned sh[4];
    const int img = huff_find_image(A.ck_start, A.n, blockIdx.x);
    if (A.status[img] != 0) return;
    const HuffImage& D = A.imgs[img];
    const unsigned long long bits = A.total_bits[img], bytes = (bits + 7) >> 3;
    const unsigned long long c0 = (unsigned long long)(blockIdx.x - A.ck_start[img]) * STUFF_CHUNK;
    if (c0 >= bytes || bytes > (unsigned long long)D.nblocks * BLOCK_MAX_BYTES) return;
    const unsigned pad = (bits & 7) ? (1u << (8 - (bits & 7))) - 1 : 0;
    const unsigned long long b0 = c0 + threadIdx.x * 16;
    unsigned cnt = 0;
    if (b0 < bytes) {
        const uint4 v = huff_load16(A.ws + D.stream_off, b0, bytes, pad);
        const int nv = bytes - b0 < 16 ? (int)(bytes - b0) : 16;
#pragma unroll
        for (int q = 0; q < 16; ++q) cnt += (q < nv && huff_byte(v, q) == 0xFF) ? 1 : 0;
    }
    unsigned total;
    wg_excl_scan(cnt, &total, sh);
    if (threadIdx.x == 0) A.ck_ff[blockIdx.x] = total;
}

// one workgroup per image: stuffed bytes in front of every chunk; the file's size
__global__ __launch_bounds__(256) void jpeg_huff_ffscan_kernel(HuffArgs A) {
    __shared__ unsigned long long sh[4];
    const int img = blockIdx.x, tid = threadIdx.x;
    const HuffImage& D = A.imgs[img];
    const unsigned long long bytes = (A.total_bits[img] + 7) >> 3;
    if (A.status[img] != 0 || bytes > (unsigned long long)D.nblocks * BLOCK_MAX_BYTES) {      // (the second: never)
        if (tid == 0) A.sizes[img] = 0;
        return;
    }
    const int k0 = A.ck_start[img];
    const int nck = (int)((bytes + STUFF_CHUNK - 1) / STUFF_CHUNK);      // <= ck_start[img + 1] - k0
    unsigned long long carry = 0;
    for (int base = 0; base < nck; base += 256) {
        const bool valid = base + tid < nck;
        const unsigned long long x = valid ? A.ck_ff[k0 + base + tid] : 0;
        unsigned long long total;
        const unsigned long long pos = carry + wg_excl_scan(x, &total, sh);
        if (valid) A.ck_pos[k0 + base + tid] = (unsigned)pos;
        carry += total;
    }
    if (tid == 0) A.sizes[img] = SSD_JPEG_HEADER_BYTES + bytes + carry + 2;
}

// one workgroup: file offsets and the records
__global__ __launch_bounds__(256) void jpeg_huff_offsets_kernel(HuffArgs A, ssd_jpeg_file_rec* __restrict__ files) {
    __shared__ unsigned long long sh[4];
    const int tid = threadIdx.x;
    unsigned long long carry = 0;
    for (int base = 0; base < A.n; base += 256) {
        const int i = base + tid;
        const unsigned long long size = i < A.n ? A.sizes[i] : 0, x = (size + 15) / 16 * 16;
        unsigned long long total;
        const unsigned long long pos = carry + wg_excl_scan(x, &total, sh);
        if (i < A.n) {
            ssd_jpeg_file_rec r;
            r.offset = pos; r.size = size; r.status = A.status[i]; r.reserved = 0;
            files[i] = r;
        }
        carry += total;
    }
}

// (e) header, stuffed scan, EOI
__global__ __launch_bounds__(256) void jpeg_huff_write_kernel(HuffArgs A, const ssd_jpeg_file_rec* __restrict__ files,
                                                              unsigned char* __restrict__ out) {
    __shared__ unsigned sh[4];
    __shared__ unsigned char sout[2 * STUFF_CHUNK + 16];
    const int img = huff_find_image(A.ck_start, A.n, blockIdx.x);
    const ssd_jpeg_file_rec rec = files[img];
    if (rec.status != 0 || rec.size == 0) return;
    const HuffImage& D = A.imgs[img];
    const unsigned long long bits = A.total_bits[img], bytes = (bits + 7) >> 3;
    const unsigned long long c0 = (unsigned long long)(blockIdx.x - A.ck_start[img]) * STUFF_CHUNK;
    if (c0 >= bytes) return;
    const int tid = threadIdx.x;
    unsigned char* file = out + rec.offset;
    if (c0 == 0)
        for (int i = tid; i < SSD_JPEG_HEADER_BYTES; i += 256) file[i] = A.headers[(size_t)img * HEADER_STRIDE + i];
    const unsigned pad = (bits & 7) ? (1u << (8 - (bits & 7))) - 1 : 0;
    const unsigned long long b0 = c0 + tid * 16;
    uint4 v = make_uint4(0, 0, 0, 0);
    int nv = 0;
    unsigned mine = 0;
    if (b0 < bytes) {
        v = huff_load16(A.ws + D.stream_off, b0, bytes, pad);
        nv = bytes - b0 < 16 ? (int)(bytes - b0) : 16;
#pragma unroll
        for (int q = 0; q < 16; ++q) mine += (q < nv && huff_byte(v, q) == 0xFF) ? 1 : 0;
        mine += nv;
    }
    unsigned total;
    unsigned p = wg_excl_scan(mine, &total, sh);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (q < nv) {
            const unsigned b = huff_byte(v, q);
            sout[p++] = (unsigned char)b;
            if (b == 0xFF) sout[p++] = 0;
        }
    }
    if (tid == 0 && c0 + STUFF_CHUNK >= bytes) {                         // the image's last chunk
        sout[total] = 0xFF;
        sout[total + 1] = 0xD9;
    }
    __syncthreads();
    if (c0 + STUFF_CHUNK >= bytes) total += 2;
    unsigned char* dst = file + SSD_JPEG_HEADER_BYTES + c0 + A.ck_pos[blockIdx.x];
    if (rec.size < SSD_JPEG_HEADER_BYTES + c0 + A.ck_pos[blockIdx.x] + total) return;       // (never: the size is the sum of these)
    for (unsigned i = tid; i < total; i += 256) dst[i] = sout[i];
}

namespace {
size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct HuffLayout {
    size_t tab_off, img_off, wg_off, ck_off, hdr_off, status_off, upload;      // [0, upload) is written by the host-to-device copy
    size_t bits_off, size_off, wgbits_off, wgpos_off, ckff_off, ckpos_off, stream_off, total;
    long long nwg, nck;
};

size_t huff_blocks(const ssd_jpeg_desc& d) { return (size_t)d.mcus_x * d.mcus_y * ((size_t)d.hs * d.vs + 2); }
size_t huff_stream_cap(const ssd_jpeg_desc& d) { return (huff_blocks(d) * BLOCK_MAX_BYTES + 16 + 15) / 16 * 16; }

void require_huff_descs(const ssd_jpeg_desc* descs, int n, size_t coef_bytes) {
    SSD_REQUIRE(n >= 1 && descs, "jpeg: empty batch");
    for (int i = 0; i < n; ++i) {
        jpeg_require_enc_desc(descs[i], coef_bytes, i);
        for (int c = 0; c < 3; ++c)
            SSD_REQUIRE(descs[i].coef_off[c] % 8 == 0, "jpeg: image %d: coefficient plane %d is not 16-byte aligned", i, c);
    }
}

HuffLayout huff_layout(const ssd_jpeg_desc* descs, int n) {
    HuffLayout l;
    l.nwg = l.nck = 0;
    size_t streams = 0;
    for (int i = 0; i < n; ++i) {
        l.nwg += (long long)((huff_blocks(descs[i]) + HUFF_BLOCKS - 1) / HUFF_BLOCKS);
        l.nck += (long long)((huff_blocks(descs[i]) * BLOCK_MAX_BYTES + STUFF_CHUNK - 1) / STUFF_CHUNK);
        streams += huff_stream_cap(descs[i]);
    }
    SSD_REQUIRE(l.nwg < (1ll << 30) && l.nck < (1ll << 30), "jpeg: batch too large for one launch");
    l.tab_off = 0;
    l.img_off = up256((2 * 16 + 2 * 256) * sizeof(unsigned));
    l.wg_off = l.img_off + up256((size_t)n * sizeof(HuffImage));
    l.ck_off = l.wg_off + up256((size_t)(n + 1) * sizeof(int));
    l.hdr_off = l.ck_off + up256((size_t)(n + 1) * sizeof(int));
    l.status_off = l.hdr_off + up256((size_t)n * HEADER_STRIDE);
    l.upload = l.status_off + up256((size_t)n * sizeof(int));
    l.bits_off = l.upload;
    l.size_off = l.bits_off + up256((size_t)n * 8);
    l.wgbits_off = l.size_off + up256((size_t)n * 8);
    l.wgpos_off = l.wgbits_off + up256((size_t)l.nwg * 4);
    l.ckff_off = l.wgpos_off + up256((size_t)l.nwg * 8);
    l.ckpos_off = l.ckff_off + up256((size_t)l.nck * 4);
    l.stream_off = l.ckpos_off + up256((size_t)l.nck * 4);
    l.total = l.stream_off + up256(streams);
    return l;
}
}  // namespace

size_t jpeg_huff_ws_bytes(const ssd_jpeg_desc* descs, int n) {
    require_huff_descs(descs, n, (size_t)-1);
    return huff_layout(descs, n).total;
}

size_t jpeg_huff_out_bytes(const ssd_jpeg_desc* descs, int n) {
    require_huff_descs(descs, n, (size_t)-1);
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (jpeg_file_bound(descs[i]) + 15) / 16 * 16;
    return total;
}

void jpeg_huffman_batch(const short* coef_dev, size_t coef_bytes, const ssd_jpeg_desc* descs, int n, unsigned char* out_dev,
                        size_t out_bytes, ssd_jpeg_file_rec* files_dev, void* ws, size_t ws_bytes, hipStream_t s) {
    SSD_REQUIRE(n >= 1 && descs, "jpeg: empty batch");
    SSD_REQUIRE(coef_dev && out_dev && files_dev && ws, "jpeg: null argument");
    SSD_REQUIRE(((uintptr_t)coef_dev | (uintptr_t)out_dev | (uintptr_t)files_dev | (uintptr_t)ws) % 16 == 0,
                "jpeg: coef_dev, out_dev, files_dev and ws_dev must be 16-byte aligned");
    require_huff_descs(descs, n, coef_bytes);
    const HuffLayout l = huff_layout(descs, n);
    SSD_REQUIRE(ws_bytes >= l.total, "jpeg: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    const size_t need = jpeg_huff_out_bytes(descs, n);
    SSD_REQUIRE(out_bytes >= need, "jpeg: the output buffer holds %zu bytes, the batch needs %zu", out_bytes, need);
    // (the staging block outlives the call: the copy below reads it)
    static thread_local std::vector<unsigned char> staging;
    staging.assign(l.upload, 0);                                         // (the status words start at 0)
    unsigned* T = reinterpret_cast<unsigned*>(staging.data() + l.tab_off);
    jpeg_huff_code_tables(reinterpret_cast<unsigned(*)[16]>(T), reinterpret_cast<unsigned(*)[256]>(T + 32));
    HuffImage* imgs = reinterpret_cast<HuffImage*>(staging.data() + l.img_off);
    int* wg = reinterpret_cast<int*>(staging.data() + l.wg_off);
    int* ck = reinterpret_cast<int*>(staging.data() + l.ck_off);
    long long nwg = 0, nck = 0;
    size_t stream = l.stream_off;
    double blocks = 0;
    for (int i = 0; i < n; ++i) {
        const ssd_jpeg_desc& d = descs[i];
        HuffImage& D = imgs[i];
        D.hs = d.hs; D.vs = d.vs; D.mcus_x = d.mcus_x;
        D.nblocks = (int)huff_blocks(d);
        D.nluma = d.hs * d.vs;
        D.bpm = D.nluma + 2;
        D.bw0 = d.mcus_x * d.hs;
        for (int c = 0; c < 3; ++c) D.coef_off[c] = d.coef_off[c];
        D.stream_off = stream;
        D.stream_cap = huff_stream_cap(d);
        stream += D.stream_cap;
        jpeg_file_header(d, staging.data() + l.hdr_off + (size_t)i * HEADER_STRIDE);
        wg[i] = (int)nwg;
        ck[i] = (int)nck;
        nwg += (long long)((huff_blocks(d) + HUFF_BLOCKS - 1) / HUFF_BLOCKS);
        nck += (long long)((huff_blocks(d) * BLOCK_MAX_BYTES + STUFF_CHUNK - 1) / STUFF_CHUNK);
        blocks += D.nblocks;
    }
    wg[n] = (int)nwg;
    ck[n] = (int)nck;
    unsigned char* base = static_cast<unsigned char*>(ws);
    HIP_OK(hipMemcpyAsync(base, staging.data(), l.upload, hipMemcpyHostToDevice, s));
    HuffArgs A;
    A.tabs = reinterpret_cast<const unsigned*>(base + l.tab_off);
    A.imgs = reinterpret_cast<const HuffImage*>(base + l.img_off);
    A.wg_start = reinterpret_cast<const int*>(base + l.wg_off);
    A.ck_start = reinterpret_cast<const int*>(base + l.ck_off);
    A.headers = base + l.hdr_off;
    A.status = reinterpret_cast<int*>(base + l.status_off);
    A.total_bits = reinterpret_cast<unsigned long long*>(base + l.bits_off);
    A.sizes = reinterpret_cast<unsigned long long*>(base + l.size_off);
    A.wg_bits = reinterpret_cast<unsigned*>(base + l.wgbits_off);
    A.wg_pos = reinterpret_cast<unsigned long long*>(base + l.wgpos_off);
    A.ck_ff = reinterpret_cast<unsigned*>(base + l.ckff_off);
    A.ck_pos = reinterpret_cast<unsigned*>(base + l.ckpos_off);
    A.ws = base;
    A.n = n;
    {
        ProfScope prof("jpeg_huff_count", 0.0, blocks * 128, s);
        hipLaunchKernelGGL(jpeg_huff_count_kernel, dim3((unsigned)nwg), dim3(256), 0, s, coef_dev, A);
    }
    {
        ProfScope prof("jpeg_huff_scan", 0.0, (double)nwg * 12, s);
        hipLaunchKernelGGL(jpeg_huff_scan_kernel, dim3((unsigned)n), dim3(256), 0, s, A);
    }
    {
        ProfScope prof("jpeg_huff_emit", 0.0, blocks * 128, s);
        hipLaunchKernelGGL(jpeg_huff_emit_kernel, dim3((unsigned)nwg), dim3(256), 0, s, coef_dev, A);
    }
    {
        ProfScope prof("jpeg_huff_stuff", 0.0, 0.0, s);
        hipLaunchKernelGGL(jpeg_huff_ffcount_kernel, dim3((unsigned)nck), dim3(256), 0, s, A);
        hipLaunchKernelGGL(jpeg_huff_ffscan_kernel, dim3((unsigned)n), dim3(256), 0, s, A);
        hipLaunchKernelGGL(jpeg_huff_offsets_kernel, dim3(1), dim3(256), 0, s, A, files_dev);
    }
    {
        ProfScope prof("jpeg_huff_write", 0.0, 0.0, s);
        hipLaunchKernelGGL(jpeg_huff_write_kernel, dim3((unsigned)nck), dim3(256), 0, s, A, (const ssd_jpeg_file_rec*)files_dev, out_dev);
    }
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
