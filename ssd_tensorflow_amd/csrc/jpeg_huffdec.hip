// Baseline JPEG Huffman decoding on the GPU: the inverse of jpeg_huff.hip, and the last serial stage of the decoder
// (jpeg.hip's entropy_decode) moved off the CPU.  A code's position depends on every code before it, but JPEG Huffman streams
// self-synchronise: a decoder started at a wrong bit falls into step with the true decode after a few codes.  So every segment
// (the bytes between two restart markers) is cut into subsequences of SUBSEQ stream bytes, one lane each:
//
//   state       (bit position, zigzag index k with 0 = "at DC", block index inside the MCU)
//   e_i, x_i    entry and exit state of subsequence i; x_i = decode(e_i) run until the position passes the subsequence's end;
//               e_0 is the segment's true start, every other e_i starts as a guess (the subsequence's first bit, at DC, block 0)
//   round       e_i <- x_(i-1), re-decode what changed, count the blocks each subsequence completes.  The GROUP subsequences of a
//               workgroup iterate among themselves behind a barrier until nothing changes; between workgroups the exit states
//               travel through global memory from one launch to the next (double-buffered: a launch reads what the last wrote)
//   write pass  after a prefix sum of the block counts: decode once more from e_i, store the nonzero coefficients, and RE-CHECK THE
//               CHAIN: every x_i it computes must equal e_(i+1), and the segment must complete exactly its MCUs' blocks inside
//               its last byte.  A chain that is consistent from a true start IS the serial decode, by induction over i; how the
//               rounds were scheduled does not matter.  Any failed link -> the image's record says SSD_JPEG_TO_HOST.
//
// Then the DC differences are summed per component in scan order (segmented at the restart intervals, 64-bit), checked against
// 16 bits, and max_l1 is taken.  Whatever entropy_decode calls an error, and whatever this stage is not sure of, is
// SSD_JPEG_TO_HOST: the stage may hand any file to the host stage, it never accepts one with another outcome.
//
// The only synchronisation is the workgroup barrier and the kernel boundary.  The number of launches is fixed by the host before
// the first one (5 + rounds), every loop is bounded by a count the host checked, every read is guarded by the segment's end and
// every write by the image's block count: no input bytes make the stage read past a file or write outside the image's slot.
#include "jpeg_huffdec.h"

namespace ssd {

namespace {
constexpr int SUBSEQ = 64;               // stream bytes per subsequence (stuffed bytes counted)
constexpr int GROUP = 256;               // subsequences per workgroup
constexpr int DEFAULT_ROUNDS = 4;        // twice the most any file of the test set needs
constexpr int MAX_ROUNDS = 64;
constexpr unsigned long long INVALID = ~0ull;
enum { RUN_OK = 0, RUN_SHORT = 1, RUN_BAD = 2 };

struct DecImage {
    unsigned long long file_off;
    unsigned long long coef_off[3];      // int16 elements
    unsigned long long slot_elems;
    long long sub_base;                  // first subsequence of the image in the state arrays
    long long mcus;
    int file_bytes;
    int comps, hs, vs, mcus_x;
    int bpm;                             // blocks per MCU
    int interval;                        // MCUs per segment
    int nseg, seg_base;                  // into the segment table
    int nsub;
    int dc_sel[3], ac_sel[3];
    unsigned short qt[3][64];
};
struct DecSeg {
    unsigned begin, end;                 // inside the file
    int sub0;                            // first subsequence, counted inside the image
};

__device__ __constant__ unsigned char d_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the image a workgroup belongs to: the last i with start[i] <= wg (wave-uniform)
__device__ __forceinline__ int find_image(const int* __restrict__ start, int n, int wg) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= wg) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ int find_seg(const DecSeg* __restrict__ segs, int n, int t) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].sub0 <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ int seg_subs(const DecSeg& s) {
    const unsigned len = s.end - s.begin;
    return len ? (int)((len + SUBSEQ - 1) / SUBSEQ) : 1;
}

__device__ __forceinline__ short* block_ptr(const DecImage& D, short* coef, long long mcu, int b) {
    const int hsvs = D.hs * D.vs;
    const int comp = b < hsvs ? 0 : b - hsvs + 1;
    const int h = comp == 0 ? D.hs : 1, v = comp == 0 ? D.vs : 1;
    const int bi = comp == 0 ? b : 0, by = bi / h, bx = bi - by * h;
    const long long y = mcu / D.mcus_x, x = mcu - y * D.mcus_x;
    return coef + D.coef_off[comp] + (((y * v + by) * ((long long)D.mcus_x * h)) + x * h + bx) * 64;
}

// Decode from `state` until the position reaches byte `stop` of the file (or, WRITE, until block g_end is complete).  A position is
// (byte that holds the next bit, bits of it already used); it never rests on a stuffed 00.  Every byte read lies below seg_end;
// bits behind it do not exist: a code that needs one ends the run with RUN_SHORT and the state in front of that code.
template <bool WRITE>
__device__ int decode_run(const unsigned char* __restrict__ f, unsigned seg_end, unsigned stop, const ssd_jpeg_huff_table* tabs,
                          const unsigned char* dct, const unsigned char* act, int bpm, unsigned long long& state, int& nblocks,
                          const DecImage& D, short* coef, long long g, long long g_end) {
    unsigned pos = (unsigned)(state >> 32);
    unsigned bit = (unsigned)state & 7, k = ((unsigned)state >> 3) & 63, blk = ((unsigned)state >> 9) & 7;
    nblocks = 0;
    if ((int)blk >= bpm) return RUN_BAD;
    int nb = 0, rc = RUN_OK;
    long long mcu = 0;
    short* bp = nullptr;
    if (WRITE) {
        mcu = g / bpm;
        if ((int)(g - mcu * bpm) != (int)blk) return RUN_BAD;
        if (g < g_end) bp = block_ptr(D, coef, mcu, (int)blk);
    }
    while (pos < stop) {
        if (WRITE && g + nb >= g_end) break;
        // the next 5 data bytes and where each of them starts
        unsigned nx[5];
        unsigned long long w = 0;
        unsigned q = pos;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            nx[j] = q;
            const unsigned c = q < seg_end ? f[q] : 0u;
            w = (w << 8) | c;
            q += c == 0xFF ? 2 : 1;
        }
        const unsigned long long acc = w << (24 + bit);
        const ssd_jpeg_huff_table& T = tabs[k == 0 ? dct[blk] : 2 + act[blk]];
        const unsigned idx = (unsigned)(acc >> 55);
        int l = T.fast_len[idx], sym = T.fast_val[idx];
        if (l == 0) {
            const int code16 = (int)(acc >> 48);
            for (int len = 10; len <= 16; ++len) {
                const int c = code16 >> (16 - len);
                if (c <= T.maxcode[len]) {
                    sym = T.vals[(T.valptr[len] + c - T.mincode[len]) & 255];
                    l = len;
                    break;
                }
            }
            if (l == 0) { rc = RUN_BAD; break; }                       // bad Huffman code
        }
        const int s = k == 0 ? sym : (sym & 15), r = sym >> 4;
        if (k == 0 && sym > 15) { rc = RUN_BAD; break; }               // DC size category
        const unsigned t = bit + (unsigned)l + (unsigned)s;            // <= 7 + 16 + 15 bits of the 40 in the window
        unsigned lastb = nx[0], np = nx[0];
#pragma unroll
        for (int j = 1; j < 5; ++j) {
            if (((t - 1) >> 3) >= (unsigned)j) lastb = nx[j];
            if ((t >> 3) >= (unsigned)j) np = nx[j];
        }
        if ((t >> 3) >= 5u) np = q;
        if (lastb >= seg_end) { rc = RUN_SHORT; break; }
        int val = 0;
        if (s) {
            const int v = (int)((acc << l) >> (64 - s));
            val = v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
        }
        bool end_block = false;
        if (k == 0) {
            if (WRITE) bp[0] = (short)val;                             // the difference: the DC pass sums them
            k = 1;
        } else if (s == 0) {
            if (r == 15) { k += 16; end_block = k >= 64; }
            else end_block = true;
        } else {
            k += (unsigned)r;
            if (k > 63) { rc = RUN_BAD; break; }                       // coefficient index past 63
            if (WRITE) bp[d_zigzag[k]] = (short)val;
            ++k;
            end_block = k == 64;
        }
        pos = np;
        bit = t & 7;
        if (end_block) {
            k = 0;
            ++nb;
            if ((int)++blk == bpm) { blk = 0; ++mcu; }
            if (WRITE && g + nb < g_end) bp = block_ptr(D, coef, mcu, (int)blk);
        }
    }
    state = ((unsigned long long)pos << 32) | bit | (k << 3) | (blk << 9);
    nblocks = nb;
    return rc;
}

// what every lane of the two decoding kernels knows about itself
struct LaneInfo {
    bool active, first, last;
    int t, sidx;
    unsigned seg_begin, seg_end, obeg, stop;
    int seg_sub0;
};
__device__ __forceinline__ LaneInfo lane_info(const DecImage& D, const DecSeg* __restrict__ segs, int t) {
    LaneInfo L;
    L.t = t;
    L.active = t < D.nsub;
    L.first = L.last = false;
    L.sidx = 0; L.seg_begin = L.seg_end = L.obeg = L.stop = 0; L.seg_sub0 = 0;
    if (L.active) {
        L.sidx = find_seg(segs + D.seg_base, D.nseg, t);
        const DecSeg sg = segs[D.seg_base + L.sidx];
        L.seg_begin = sg.begin; L.seg_end = sg.end; L.seg_sub0 = sg.sub0;
        const int j = t - sg.sub0;
        L.first = j == 0;
        L.last = j + 1 >= seg_subs(sg);
        L.obeg = sg.begin + (unsigned)j * SUBSEQ;
        const unsigned e = L.obeg + SUBSEQ;
        L.stop = (L.last || e > sg.end) ? sg.end : e;
    }
    return L;
}

__device__ __forceinline__ void load_tables(const DecImage& D, const ssd_jpeg_huff_table* __restrict__ tabs_g, int img,
                                            ssd_jpeg_huff_table* s_tab, unsigned char* s_dct, unsigned char* s_act) {
    const int* src = reinterpret_cast<const int*>(tabs_g + 4 * (size_t)img);
    int* dst = reinterpret_cast<int*>(s_tab);
    for (int i = threadIdx.x; i < (int)(4 * sizeof(ssd_jpeg_huff_table) / sizeof(int)); i += blockDim.x) dst[i] = src[i];
    if (threadIdx.x < 8) {
        const int b = threadIdx.x, hsvs = D.hs * D.vs;
        int comp = b < hsvs ? 0 : b - hsvs + 1;
        if (comp > 2) comp = 2;
        s_dct[b] = (unsigned char)(D.dc_sel[comp] & 1);
        s_act[b] = (unsigned char)(D.ac_sel[comp] & 1);
    }
    __syncthreads();
}
}  // namespace

// 16 KiB of an image's coefficient slot per workgroup
__global__ __launch_bounds__(256) void jpeg_huffdec_zero_kernel(const DecImage* __restrict__ imgs, const int* __restrict__ wg_start, int n,
                                                                short* __restrict__ coef) {
    const int img = find_image(wg_start, n, blockIdx.x);
    const DecImage& D = imgs[img];
    const unsigned long long vecs = D.slot_elems / 8;
    uint4* dst = reinterpret_cast<uint4*>(coef + D.coef_off[0]);
    const unsigned long long base = (unsigned long long)(blockIdx.x - wg_start[img]) * 1024;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long v = base + j * 256 + threadIdx.x;
        if (v < vecs) dst[v] = make_uint4(0, 0, 0, 0);
    }
}

// One round: e_i <- x_(i-1), re-decode what changed.  Inside the workgroup until nothing changes (at most GROUP + 1 turns: turn j
// settles lane j given lane 0's entry); lane 0's left neighbour is what the previous launch left in x_prev.
__global__ __launch_bounds__(256) void jpeg_huffdec_sync_kernel(const unsigned char* __restrict__ files, const DecImage* __restrict__ imgs,
                                                                const DecSeg* __restrict__ segs, const ssd_jpeg_huff_table* __restrict__ tabs_g,
                                                                const int* __restrict__ wg_start, int n, int round,
                                                                unsigned long long* __restrict__ E, const unsigned long long* __restrict__ x_prev,
                                                                unsigned long long* __restrict__ x_cur, int* __restrict__ N) {
    __shared__ ssd_jpeg_huff_table s_tab[4];
    __shared__ unsigned long long sx[GROUP];
    __shared__ unsigned char s_dct[8], s_act[8];
    const int img = find_image(wg_start, n, blockIdx.x);
    const DecImage& D = imgs[img];
    load_tables(D, tabs_g, img, s_tab, s_dct, s_act);
    const int tid = threadIdx.x;
    const LaneInfo L = lane_info(D, segs, (blockIdx.x - wg_start[img]) * GROUP + tid);
    const unsigned char* f = files + D.file_off;
    const long long gi = D.sub_base + L.t;
    unsigned long long e = INVALID, x = INVALID, left0 = INVALID;
    int nb = 0;
    bool need = false;
    if (L.active) {
        if (L.first) e = (unsigned long long)L.seg_begin << 32;
        else if (round == 0) {
            unsigned p = L.obeg;                                        // (a lane that is not its segment's first has obeg < seg_end)
            if (f[p] == 0 && f[p - 1] == 0xFF) ++p;                     // 00 after FF is stuffing
            e = (unsigned long long)p << 32;
        } else e = E[gi];
        if (round == 0) need = true;
        else {
            x = x_prev[gi];
            nb = N[gi];
            if (tid == 0 && !L.first) left0 = x_prev[gi - 1];
        }
    }
    for (int it = 0; it <= GROUP; ++it) {
        sx[tid] = x;
        __syncthreads();
        if (L.active && !L.first) {
            const unsigned long long left = tid ? sx[tid - 1] : left0;
            if (left != INVALID && left != e) { e = left; need = true; }
        }
        int did = 0;
        if (need) {
            unsigned long long st = e;
            const int rc = decode_run<false>(f, L.seg_end, L.stop, s_tab, s_dct, s_act, D.bpm, st, nb, D, nullptr, 0, 0);
            x = rc == RUN_OK ? st : INVALID;
            need = false;
            did = 1;
        }
        if (!__syncthreads_or(did)) break;
    }
    if (L.active) {
        E[gi] = e;
        x_cur[gi] = x;
        N[gi] = nb;
    }
}

// exclusive prefix of the block counts over an image's subsequences: one workgroup per image
__global__ __launch_bounds__(256) void jpeg_huffdec_prefix_kernel(const DecImage* __restrict__ imgs, const int* __restrict__ N, int* __restrict__ P) {
    __shared__ int s[256];
    const DecImage& D = imgs[blockIdx.x];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < D.nsub; base += 256) {
        const int t = base + tid;
        const int v = t < D.nsub ? N[D.sub_base + t] : 0;
        s[tid] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int a = tid >= o ? s[tid - o] : 0;
            __syncthreads();
            s[tid] += a;
            __syncthreads();
        }
        if (t < D.nsub) P[D.sub_base + t] = carry + s[tid] - v;
        carry += s[255];
        __syncthreads();
    }
}

// The write pass and the certificate: decode from e_i at the block the prefix sum names, store, and compare the exit with e_(i+1).
__global__ __launch_bounds__(256) void jpeg_huffdec_write_kernel(const unsigned char* __restrict__ files, const DecImage* __restrict__ imgs,
                                                                 const DecSeg* __restrict__ segs, const ssd_jpeg_huff_table* __restrict__ tabs_g,
                                                                 const int* __restrict__ wg_start, int n, const unsigned long long* __restrict__ E,
                                                                 const int* __restrict__ N, const int* __restrict__ P, short* __restrict__ coef,
                                                                 ssd_jpeg_huffdec_rec* __restrict__ recs) {
    __shared__ ssd_jpeg_huff_table s_tab[4];
    __shared__ unsigned char s_dct[8], s_act[8];
    const int img = find_image(wg_start, n, blockIdx.x);
    const DecImage& D = imgs[img];
    load_tables(D, tabs_g, img, s_tab, s_dct, s_act);
    const LaneInfo L = lane_info(D, segs, (blockIdx.x - wg_start[img]) * GROUP + threadIdx.x);
    if (!L.active) return;
    const unsigned char* f = files + D.file_off;
    const long long gi = D.sub_base + L.t;
    const long long base = (long long)P[gi] - (long long)P[D.sub_base + L.seg_sub0];
    const long long m_end = ((long long)L.sidx + 1) * D.interval;
    const long long g0 = (long long)L.sidx * D.interval * D.bpm + base;
    const long long g_end = (m_end < D.mcus ? m_end : D.mcus) * D.bpm;
    bool ok = base >= 0 && g0 <= g_end;
    if (ok) {
        unsigned long long st = E[gi];
        ok = st != INVALID && (unsigned)(st >> 32) >= L.seg_begin;
        int nb = 0;
        if (ok) ok = decode_run<true>(f, L.seg_end, L.stop, s_tab, s_dct, s_act, D.bpm, st, nb, D, coef, g0, g_end) == RUN_OK;
        if (ok) {
            const unsigned pos = (unsigned)(st >> 32), bit = (unsigned)st & 7;
            if (!L.last) ok = pos >= L.stop && nb == N[gi] && st == E[gi + 1];
            else {
                // all the segment's blocks and nothing behind them but the rest of the last byte; at DC, at the MCU's first block
                ok = g0 + nb == g_end && ((unsigned)st & 0xFF8u) == 0;
                if (bit == 0) ok = ok && pos == L.seg_end;
                else ok = ok && pos < L.seg_end && pos + (f[pos] == 0xFF ? 2u : 1u) == L.seg_end;
            }
        }
    }
    if (!ok) atomicMax(&recs[img].status, SSD_JPEG_TO_HOST);
}

// DC differences -> values: a segmented inclusive scan per component in scan order, restarting where a segment starts; 64-bit sums.
// One workgroup per (image, component).
__global__ __launch_bounds__(256) void jpeg_huffdec_dc_kernel(const DecImage* __restrict__ imgs, short* __restrict__ coef,
                                                              ssd_jpeg_huffdec_rec* __restrict__ recs) {
    __shared__ long long sv[256];
    __shared__ int sf[256];
    const int img = blockIdx.x / 3, comp = blockIdx.x % 3;
    const DecImage& D = imgs[img];
    if (comp >= D.comps) return;
    const int tid = threadIdx.x;
    const int bpc = comp == 0 ? D.hs * D.vs : 1, b0 = comp == 0 ? 0 : D.hs * D.vs + comp - 1;
    const long long total = D.mcus * bpc;
    long long carry = 0;
    bool bad = false;
    for (long long base = 0; base < total; base += 256) {
        const long long j = base + tid;
        const bool on = j < total;
        short* p = nullptr;
        long long v = 0;
        int flag = 0;
        if (on) {
            const long long mcu = j / bpc;
            const int b = (int)(j - mcu * bpc);
            p = block_ptr(D, coef, mcu, b0 + b);
            v = p[0];
            flag = b == 0 && mcu % D.interval == 0;
        }
        sv[tid] = v;
        sf[tid] = flag;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            long long a = 0;
            int fa = 0;
            if (tid >= o) { a = sv[tid - o]; fa = sf[tid - o]; }
            __syncthreads();
            if (tid >= o && !sf[tid]) { sv[tid] += a; sf[tid] = fa; }
            __syncthreads();
        }
        const long long r = sf[tid] ? sv[tid] : carry + sv[tid];
        if (on) {
            if (r < -32768 || r > 32767) bad = true;
            p[0] = (short)r;
        }
        carry = sf[255] ? sv[255] : carry + sv[255];
        __syncthreads();
    }
    if (bad) atomicMax(&recs[img].status, SSD_JPEG_TO_HOST);
}

// max over blocks of sum |coef * q|, one lane per block
__global__ __launch_bounds__(256) void jpeg_huffdec_l1_kernel(const DecImage* __restrict__ imgs, const int* __restrict__ wg_start, int n,
                                                              const short* __restrict__ coef, ssd_jpeg_huffdec_rec* __restrict__ recs) {
    const int img = find_image(wg_start, n, blockIdx.x);
    const DecImage& D = imgs[img];
    const long long lb = (long long)(blockIdx.x - wg_start[img]) * 256 + threadIdx.x;
    const long long n0 = D.mcus * D.hs * D.vs, nall = n0 + (D.comps == 3 ? 2 * D.mcus : 0);
    long long l1 = 0;
    if (lb < nall) {
        const int comp = lb < n0 ? 0 : (lb < n0 + D.mcus ? 1 : 2);
        const long long bi = comp == 0 ? lb : lb - n0 - (comp - 1) * D.mcus;
        const uint4* src = reinterpret_cast<const uint4*>(coef + D.coef_off[comp] + bi * 64);
        const unsigned short* q = D.qt[comp];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint4 v = src[j];
            const unsigned wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int lo = (short)(wds[u] & 0xFFFF), hi = (short)(wds[u] >> 16);
                l1 += (long long)(lo < 0 ? -lo : lo) * q[j * 8 + u * 2] + (long long)(hi < 0 ? -hi : hi) * q[j * 8 + u * 2 + 1];
            }
        }
    }
    int m = l1 > 0x7fffffffll ? 0x7fffffff : (int)l1;
    for (int o = 32; o; o >>= 1) {
        const int other = __shfl_xor(m, o);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&recs[img].max_l1, m);
}

namespace {
size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct Layout {
    size_t img_off, seg_off, tab_off, wga_off, wgz_off, wgl_off, head;       // head: what the host fills and copies
    size_t e_off, xa_off, xb_off, n_off, p_off, total;
    long long subs, segs;
};

bool sampling_ok(const ssd_jpeg_desc& d) {
    if (d.components == 1) return d.hs == 1 && d.vs == 1;
    return d.components == 3 && ((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2));
}

size_t coef_elems(const ssd_jpeg_desc& d) {
    return (size_t)d.mcus_x * d.mcus_y * ((size_t)d.hs * d.vs + (d.components == 3 ? 2 : 0)) * 64;
}

long long plan_subs(const ssd_jpeg_plan& p) {
    long long subs = 0;
    for (int s = 0; s < p.segments; ++s) {
        const long long len = (long long)p.seg[s].end - (long long)p.seg[s].begin;
        subs += len > 0 ? (len + SUBSEQ - 1) / SUBSEQ : 1;
    }
    return subs;
}

// everything that does not depend on the buffers' sizes
void require_plan(const ssd_jpeg_plan& p, const ssd_jpeg_desc& d, int i) {
    SSD_REQUIRE(d.width >= 1 && d.height >= 1 && d.width <= 16384 && d.height <= 16384, "jpeg: image %d: size %d x %d", i, d.width, d.height);
    SSD_REQUIRE(sampling_ok(d), "jpeg: image %d: %d components with luma sampling %dx%d", i, d.components, d.hs, d.vs);
    SSD_REQUIRE(d.mcus_x == (d.width + 8 * d.hs - 1) / (8 * d.hs) && d.mcus_y == (d.height + 8 * d.vs - 1) / (8 * d.vs),
                "jpeg: image %d: %d x %d MCUs do not match its %d x %d pixels", i, d.mcus_x, d.mcus_y, d.width, d.height);
    const long long mcus = (long long)d.mcus_x * d.mcus_y;
    SSD_REQUIRE(p.restart_interval >= 0 && p.restart_interval <= 65535, "jpeg: image %d: restart interval %d", i, p.restart_interval);
    const long long expect = p.restart_interval ? (mcus + p.restart_interval - 1) / p.restart_interval : 1;
    SSD_REQUIRE(p.segments == expect, "jpeg: image %d: the plan has %d segments, %lld MCUs at an interval of %d make %lld", i, p.segments, mcus,
                p.restart_interval, expect);
    SSD_REQUIRE(p.seg != nullptr && p.seg_cap >= p.segments, "jpeg: image %d: the plan's segment array holds %d of %d entries", i, p.seg_cap, p.segments);
    SSD_REQUIRE(p.file_bytes >= 4 && p.file_bytes < (1ull << 30), "jpeg: image %d: a file of %llu bytes", i, p.file_bytes);
    for (int s = 0; s < p.segments; ++s)
        SSD_REQUIRE(p.seg[s].begin <= p.seg[s].end && p.seg[s].end <= p.file_bytes, "jpeg: image %d: segment %d (bytes %u .. %u) outside the file of %llu bytes",
                    i, s, p.seg[s].begin, p.seg[s].end, p.file_bytes);
    for (int c = 0; c < 3; ++c)
        SSD_REQUIRE(p.dc_sel[c] >= 0 && p.dc_sel[c] <= 1 && p.ac_sel[c] >= 0 && p.ac_sel[c] <= 1, "jpeg: image %d: table selector of component %d", i, c);
    for (int k = 0; k < 4; ++k) {                                    // (a fast code length beyond 9 would let a code consume no bit)
        const ssd_jpeg_huff_table& t = k < 2 ? p.dc[k] : p.ac[k - 2];
        for (int j = 0; j < 512; ++j) SSD_REQUIRE(t.fast_len[j] <= 9, "jpeg: image %d: Huffman table %d is not in lookup form", i, k);
    }
    size_t off = d.coef_off[0];
    for (int c = 0; c < d.components; ++c) {
        SSD_REQUIRE(d.coef_off[c] == off, "jpeg: image %d: coefficient plane %d does not follow the plane before it", i, c);
        off += (size_t)mcus * (c == 0 ? d.hs * d.vs : 1) * 64;
    }
    SSD_REQUIRE(d.coef_off[0] % 8 == 0, "jpeg: image %d: coefficient offset %llu is not a multiple of 8", i, d.coef_off[0]);
}

Layout ws_layout(const ssd_jpeg_plan* plans, const ssd_jpeg_desc* descs, int n) {
    SSD_REQUIRE(n >= 1 && plans && descs, "jpeg: empty batch");
    Layout l;
    l.subs = l.segs = 0;
    for (int i = 0; i < n; ++i) {
        require_plan(plans[i], descs[i], i);
        l.subs += plan_subs(plans[i]);
        l.segs += plans[i].segments;
    }
    SSD_REQUIRE(l.subs < (1ll << 30) && l.segs < (1ll << 30), "jpeg: batch too large for one launch");
    l.img_off = 0;
    l.seg_off = up256((size_t)n * sizeof(DecImage));
    l.tab_off = l.seg_off + up256((size_t)l.segs * sizeof(DecSeg));
    l.wga_off = l.tab_off + up256((size_t)n * 4 * sizeof(ssd_jpeg_huff_table));
    l.wgz_off = l.wga_off + up256((size_t)(n + 1) * sizeof(int));
    l.wgl_off = l.wgz_off + up256((size_t)(n + 1) * sizeof(int));
    l.head = l.wgl_off + up256((size_t)(n + 1) * sizeof(int));
    l.e_off = l.head;
    l.xa_off = l.e_off + up256((size_t)(l.subs + 1) * 8);            // (+1: the write pass's last lane never reads e of the next image, but keep the slot)
    l.xb_off = l.xa_off + up256((size_t)l.subs * 8);
    l.n_off = l.xb_off + up256((size_t)l.subs * 8);
    l.p_off = l.n_off + up256((size_t)l.subs * 4);
    l.total = l.p_off + up256((size_t)l.subs * 4);
    return l;
}
}  // namespace

size_t jpeg_huffdec_ws_bytes(const ssd_jpeg_plan* plans, const ssd_jpeg_desc* descs, int n) { return ws_layout(plans, descs, n).total; }

void jpeg_huffdec_batch(const unsigned char* files_dev, size_t files_bytes, const ssd_jpeg_plan* plans, const ssd_jpeg_desc* descs,
                        int n, short* coef_dev, size_t coef_bytes, ssd_jpeg_huffdec_rec* recs_dev, void* ws, size_t ws_bytes,
                        int max_rounds, hipStream_t s) {
    SSD_REQUIRE(n >= 1 && plans && descs, "jpeg: empty batch");
    SSD_REQUIRE(files_dev && coef_dev && recs_dev && ws, "jpeg: null argument");
    SSD_REQUIRE(((uintptr_t)files_dev | (uintptr_t)coef_dev | (uintptr_t)recs_dev | (uintptr_t)ws) % 16 == 0,
                "jpeg: files_dev, coef_dev, recs_dev and ws_dev must be 16-byte aligned");
    SSD_REQUIRE(max_rounds >= 0 && max_rounds <= MAX_ROUNDS, "jpeg: max_rounds must be in 0..%d (got %d)", MAX_ROUNDS, max_rounds);
    const int rounds = max_rounds ? max_rounds : DEFAULT_ROUNDS;
    const Layout l = ws_layout(plans, descs, n);
    SSD_REQUIRE(ws_bytes >= l.total, "jpeg: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    static thread_local std::vector<unsigned char> staging;           // (outlives the call: the copy below reads it)
    staging.assign(l.head, 0);
    DecImage* imgs = reinterpret_cast<DecImage*>(staging.data() + l.img_off);
    DecSeg* segs = reinterpret_cast<DecSeg*>(staging.data() + l.seg_off);
    ssd_jpeg_huff_table* tabs = reinterpret_cast<ssd_jpeg_huff_table*>(staging.data() + l.tab_off);
    int* wga = reinterpret_cast<int*>(staging.data() + l.wga_off);
    int* wgz = reinterpret_cast<int*>(staging.data() + l.wgz_off);
    int* wgl = reinterpret_cast<int*>(staging.data() + l.wgl_off);
    long long na = 0, nz = 0, nl = 0, sub = 0, seg = 0;
    double bytes = 0, blocks = 0;
    for (int i = 0; i < n; ++i) {
        const ssd_jpeg_plan& p = plans[i];
        const ssd_jpeg_desc& d = descs[i];
        SSD_REQUIRE(p.file_off % 16 == 0 && p.file_off <= files_bytes && p.file_bytes <= files_bytes - p.file_off,
                    "jpeg: image %d: a file of %llu bytes at offset %llu outside the %zu-byte buffer", i, p.file_bytes, p.file_off, files_bytes);
        const size_t elems = coef_elems(d);
        SSD_REQUIRE(d.coef_off[0] <= coef_bytes / 2 && elems <= coef_bytes / 2 - d.coef_off[0],
                    "jpeg: image %d: %zu coefficients at offset %llu outside the %zu-byte buffer", i, elems, d.coef_off[0], coef_bytes);
        DecImage& D = imgs[i];
        D.file_off = p.file_off;
        D.file_bytes = (int)p.file_bytes;
        D.slot_elems = elems;
        D.sub_base = sub;
        D.mcus = (long long)d.mcus_x * d.mcus_y;
        D.comps = d.components; D.hs = d.hs; D.vs = d.vs; D.mcus_x = d.mcus_x;
        D.bpm = d.hs * d.vs + (d.components == 3 ? 2 : 0);
        D.interval = p.restart_interval ? p.restart_interval : (int)std::min<long long>(D.mcus, 0x7fffffff);
        D.nseg = p.segments;
        D.seg_base = (int)seg;
        for (int c = 0; c < 3; ++c) {
            D.coef_off[c] = c < d.components ? d.coef_off[c] : d.coef_off[0];
            D.dc_sel[c] = p.dc_sel[c];
            D.ac_sel[c] = p.ac_sel[c];
            memcpy(D.qt[c], d.qt[c], sizeof D.qt[c]);
        }
        int t = 0;
        for (int k = 0; k < p.segments; ++k) {
            DecSeg& S = segs[seg + k];
            S.begin = p.seg[k].begin; S.end = p.seg[k].end; S.sub0 = t;
            const unsigned len = S.end - S.begin;
            t += len ? (int)((len + SUBSEQ - 1) / SUBSEQ) : 1;
            bytes += len;
        }
        D.nsub = t;
        tabs[4 * i + 0] = p.dc[0]; tabs[4 * i + 1] = p.dc[1]; tabs[4 * i + 2] = p.ac[0]; tabs[4 * i + 3] = p.ac[1];
        wga[i] = (int)na; wgz[i] = (int)nz; wgl[i] = (int)nl;
        na += cdiv(t, GROUP);
        nz += cdiv((long long)(elems / 8), 1024);
        nl += cdiv((long long)(elems / 64), 256);
        sub += t;
        seg += p.segments;
        blocks += (double)(elems / 64);
    }
    SSD_REQUIRE(na < (1ll << 30) && nz < (1ll << 30) && nl < (1ll << 30), "jpeg: batch too large for one launch");
    wga[n] = (int)na; wgz[n] = (int)nz; wgl[n] = (int)nl;
    char* base = static_cast<char*>(ws);
    HIP_OK(hipMemcpyAsync(base, staging.data(), l.head, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemsetAsync(recs_dev, 0, (size_t)n * sizeof(ssd_jpeg_huffdec_rec), s));
    const DecImage* imgs_dev = reinterpret_cast<const DecImage*>(base + l.img_off);
    const DecSeg* segs_dev = reinterpret_cast<const DecSeg*>(base + l.seg_off);
    const ssd_jpeg_huff_table* tabs_dev = reinterpret_cast<const ssd_jpeg_huff_table*>(base + l.tab_off);
    const int* wga_dev = reinterpret_cast<const int*>(base + l.wga_off);
    unsigned long long* E = reinterpret_cast<unsigned long long*>(base + l.e_off);
    unsigned long long* X[2] = {reinterpret_cast<unsigned long long*>(base + l.xa_off), reinterpret_cast<unsigned long long*>(base + l.xb_off)};
    int* N = reinterpret_cast<int*>(base + l.n_off);
    int* P = reinterpret_cast<int*>(base + l.p_off);
    {
        ProfScope prof("jpeg_huffdec_zero", 0.0, blocks * 128, s);
        hipLaunchKernelGGL(jpeg_huffdec_zero_kernel, dim3((unsigned)nz), dim3(256), 0, s, imgs_dev, reinterpret_cast<const int*>(base + l.wgz_off), n, coef_dev);
    }
    {
        ProfScope prof("jpeg_huffdec_sync", 0.0, bytes * rounds, s);
        for (int r = 0; r < rounds; ++r)
            hipLaunchKernelGGL(jpeg_huffdec_sync_kernel, dim3((unsigned)na), dim3(GROUP), 0, s, files_dev, imgs_dev, segs_dev, tabs_dev, wga_dev, n, r, E,
                               X[(r + 1) & 1], X[r & 1], N);
    }
    {
        ProfScope prof("jpeg_huffdec_write", 0.0, bytes + blocks * 128, s);
        hipLaunchKernelGGL(jpeg_huffdec_prefix_kernel, dim3((unsigned)n), dim3(256), 0, s, imgs_dev, N, P);
        hipLaunchKernelGGL(jpeg_huffdec_write_kernel, dim3((unsigned)na), dim3(GROUP), 0, s, files_dev, imgs_dev, segs_dev, tabs_dev, wga_dev, n, E, N, P,
                           coef_dev, recs_dev);
    }
    {
        ProfScope prof("jpeg_huffdec_dc_l1", 0.0, blocks * 128, s);
        hipLaunchKernelGGL(jpeg_huffdec_dc_kernel, dim3((unsigned)n * 3), dim3(256), 0, s, imgs_dev, coef_dev, recs_dev);
        hipLaunchKernelGGL(jpeg_huffdec_l1_kernel, dim3((unsigned)nl), dim3(256), 0, s, imgs_dev, reinterpret_cast<const int*>(base + l.wgl_off), n, coef_dev,
                           recs_dev);
    }
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
