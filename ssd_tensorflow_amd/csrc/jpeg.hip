// Baseline JPEG decode, bit-exact with libjpeg-turbo's default path: cv2.imread of the reference's
// detect.py:101, infer.py:44-54 and transforms.py:38-43.
//
// Host half: marker parser + Huffman decoder.  It is serial per restart interval, so it stays on the CPU, but native, batched
// and multi-threaded; it sees files from the outside world, so every read is bounds-checked and every table index validated.
// It leaves int16 coefficients in natural order, one [64] block after the other, per component plane padded to whole MCUs.
//
// Device half: two launches per batch.
//   jpeg_idct_kernel     dequantise + libjpeg's "islow" 8 x 8 inverse DCT in int32 -> planar uint8 component planes
//   jpeg_pack_kernel     "fancy" (triangle) chroma upsampling + 16-bit fixed-point YCbCr -> packed [h][w][3] uint8 BGR
// Both walk all images of the batch through a per-image prefix table of workgroups; nothing synchronises per image.
#include "jpeg.h"
#include <atomic>
#include <mutex>
#include <thread>

namespace ssd {

// ------------------------------------------------------------------------------------------------------------------------
// host: parser
// ------------------------------------------------------------------------------------------------------------------------
namespace {

const unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int FAST_BITS = 9;

struct HuffTable {
    bool present = false;
    unsigned char fast_len[1 << FAST_BITS];      // 0: the code is longer than FAST_BITS
    unsigned char fast_val[1 << FAST_BITS];
    int maxcode[17];                             // per code length 1..16; -1: no code of that length
    int mincode[17];
    int valptr[17];
    unsigned char vals[256];
};

struct Parsed {
    ssd_jpeg_desc d;
    unsigned short qtab[4][64];      // natural order
    bool qt_present[4] = {false, false, false, false};
    HuffTable dc[4], ac[4];
    int dri = 0;
    bool frame = false, jfif = false, adobe = false;
    int adobe_transform = 0;
    int comp_id[3], comp_tq[3], comp_td[3], comp_ta[3];
    size_t scan_pos = 0;
};

void build_huffman(HuffTable& h, const unsigned char* counts, const unsigned char* vals, int total) {
    memset(h.fast_len, 0, sizeof h.fast_len);
    memset(h.fast_val, 0, sizeof h.fast_val);
    memcpy(h.vals, vals, (size_t)total);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = counts[l - 1];
        SSD_REQUIRE(code + cnt <= (1 << l), "jpeg: Huffman table has more codes of length %d than fit", l);
        h.valptr[l] = k;
        h.mincode[l] = code;
        h.maxcode[l] = cnt ? code + cnt - 1 : -1;
        if (l <= FAST_BITS)
            for (int i = 0; i < cnt; ++i) {
                const int first = (code + i) << (FAST_BITS - l);
                for (int j = 0; j < (1 << (FAST_BITS - l)); ++j) {
                    h.fast_len[first + j] = (unsigned char)l;
                    h.fast_val[first + j] = vals[k + i];
                }
            }
        code = (code + cnt) << 1;
        k += cnt;
    }
    h.present = true;
}

inline int be16(const unsigned char* p) { return (p[0] << 8) | p[1]; }

// SSD_JPEG_OK with p.scan_pos at the first entropy-coded byte, or SSD_JPEG_UNSUPPORTED; corrupt input throws.
int parse(const unsigned char* b, size_t n, Parsed& P) {
    SSD_REQUIRE(b != nullptr && n >= 4 && b[0] == 0xFF && b[1] == 0xD8, "jpeg: no SOI marker");
    memset(&P.d, 0, sizeof P.d);
    size_t p = 2;
    for (;;) {
        SSD_REQUIRE(p < n, "jpeg: truncated before the scan (no SOS marker)");
        SSD_REQUIRE(b[p] == 0xFF, "jpeg: marker expected at byte %zu", p);
        while (p < n && b[p] == 0xFF) ++p;                    // fill bytes
        SSD_REQUIRE(p < n, "jpeg: truncated inside a marker");
        const int m = b[p++];
        SSD_REQUIRE(m != 0, "jpeg: stuffed byte where a marker is expected (byte %zu)", p - 1);
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;      // no length
        SSD_REQUIRE(m != 0xD9, "jpeg: EOI before any scan");
        SSD_REQUIRE(p + 2 <= n, "jpeg: truncated inside a segment header");
        const int L = be16(b + p);
        SSD_REQUIRE(L >= 2 && p + (size_t)L <= n, "jpeg: segment 0x%02X at byte %zu has length %d, past the end of the data", m, p - 2, L);
        const unsigned char* seg = b + p + 2;
        const int sl = L - 2;
        p += (size_t)L;
        if (m == 0xDB) {                                      // DQT
            int s = 0;
            while (s < sl) {
                const int pq = seg[s] >> 4, tq = seg[s] & 15;
                ++s;
                SSD_REQUIRE(pq <= 1 && tq <= 3, "jpeg: bad quantisation table header");
                const int bytes = pq ? 128 : 64;
                SSD_REQUIRE(s + bytes <= sl, "jpeg: quantisation table runs past its segment");
                for (int k = 0; k < 64; ++k) P.qtab[tq][ZIGZAG[k]] = (unsigned short)(pq ? be16(seg + s + 2 * k) : seg[s + k]);
                P.qt_present[tq] = true;
                s += bytes;
            }
        } else if (m == 0xC4) {                               // DHT
            int s = 0;
            while (s < sl) {
                const int tc = seg[s] >> 4, th = seg[s] & 15;
                ++s;
                SSD_REQUIRE(tc <= 1 && th <= 3, "jpeg: bad Huffman table header");
                SSD_REQUIRE(s + 16 <= sl, "jpeg: Huffman table runs past its segment");
                int total = 0;
                for (int i = 0; i < 16; ++i) total += seg[s + i];
                SSD_REQUIRE(total <= 256, "jpeg: Huffman table counts sum to %d (> 256)", total);
                SSD_REQUIRE(s + 16 + total <= sl, "jpeg: Huffman table runs past its segment");
                build_huffman(tc ? P.ac[th] : P.dc[th], seg + s, seg + s + 16, total);
                s += 16 + total;
            }
        } else if (m == 0xC0 || m == 0xC1) {                  // SOF0 / SOF1
            SSD_REQUIRE(!P.frame, "jpeg: two frame headers");
            SSD_REQUIRE(sl >= 6, "jpeg: short frame header");
            const int prec = seg[0], H = be16(seg + 1), W = be16(seg + 3), nc = seg[5];
            SSD_REQUIRE(sl == 6 + 3 * nc, "jpeg: frame header length does not match its %d components", nc);
            if (prec != 8 || (nc != 1 && nc != 3) || W < 1 || H < 1 || W > 16384 || H > 16384) return SSD_JPEG_UNSUPPORTED;
            int hs[3], vs[3];
            for (int i = 0; i < nc; ++i) {
                P.comp_id[i] = seg[6 + 3 * i];
                hs[i] = seg[7 + 3 * i] >> 4;
                vs[i] = seg[7 + 3 * i] & 15;
                P.comp_tq[i] = seg[8 + 3 * i];
                SSD_REQUIRE(hs[i] >= 1 && hs[i] <= 4 && vs[i] >= 1 && vs[i] <= 4 && P.comp_tq[i] <= 3, "jpeg: bad component %d in the frame header", i);
            }
            const bool luma_ok = (hs[0] == 1 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 2);
            if (nc == 1 && !(hs[0] == 1 && vs[0] == 1)) return SSD_JPEG_UNSUPPORTED;
            if (nc == 3 && !(luma_ok && hs[1] == 1 && vs[1] == 1 && hs[2] == 1 && vs[2] == 1)) return SSD_JPEG_UNSUPPORTED;
            P.d.width = W; P.d.height = H; P.d.components = nc; P.d.hs = hs[0]; P.d.vs = vs[0];
            P.d.mcus_x = (W + 8 * hs[0] - 1) / (8 * hs[0]);
            P.d.mcus_y = (H + 8 * vs[0] - 1) / (8 * vs[0]);
            P.frame = true;
        } else if (m >= 0xC2 && m <= 0xCF) {                  // progressive, lossless, differential, arithmetic (SOFn, JPG, DAC)
            return SSD_JPEG_UNSUPPORTED;
        } else if (m == 0xDD) {                               // DRI
            SSD_REQUIRE(sl == 2, "jpeg: bad restart interval segment");
            P.dri = be16(seg);
        } else if (m == 0xE0) {
            if (sl >= 5 && memcmp(seg, "JFIF\0", 5) == 0) P.jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) { P.adobe = true; P.adobe_transform = seg[11]; }
        } else if (m == 0xDA) {                               // SOS
            SSD_REQUIRE(P.frame, "jpeg: SOS before the frame header");
            SSD_REQUIRE(sl >= 1, "jpeg: short scan header");
            const int ns = seg[0], nc = P.d.components;
            SSD_REQUIRE(ns >= 1 && ns <= 4 && sl == 4 + 2 * ns, "jpeg: scan header length does not match its %d components", ns);
            if (ns != nc) return SSD_JPEG_UNSUPPORTED;       // one of several scans
            for (int i = 0; i < ns; ++i) {
                if (seg[1 + 2 * i] != P.comp_id[i]) return SSD_JPEG_UNSUPPORTED;
                P.comp_td[i] = seg[2 + 2 * i] >> 4;
                P.comp_ta[i] = seg[2 + 2 * i] & 15;
                SSD_REQUIRE(P.comp_td[i] <= 3 && P.comp_ta[i] <= 3, "jpeg: bad table selector in the scan header");
            }
            if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0) return SSD_JPEG_UNSUPPORTED;
            if (nc == 3) {        // libjpeg's colour-space guess (jdapimin.c default_decompress_parms) must say YCbCr
                bool ycc;
                if (P.jfif) ycc = true;
                else if (P.adobe) ycc = P.adobe_transform == 1;
                else ycc = P.comp_id[0] == 1 && P.comp_id[1] == 2 && P.comp_id[2] == 3;
                if (!ycc) return SSD_JPEG_UNSUPPORTED;
            }
            for (int i = 0; i < nc; ++i) {
                SSD_REQUIRE(P.qt_present[P.comp_tq[i]], "jpeg: quantisation table %d is missing", P.comp_tq[i]);
                SSD_REQUIRE(P.dc[P.comp_td[i]].present, "jpeg: DC Huffman table %d is missing", P.comp_td[i]);
                SSD_REQUIRE(P.ac[P.comp_ta[i]].present, "jpeg: AC Huffman table %d is missing", P.comp_ta[i]);
                memcpy(P.d.qt[i], P.qtab[P.comp_tq[i]], sizeof P.d.qt[i]);
            }
            size_t off = 0;
            for (int i = 0; i < nc; ++i) {
                P.d.coef_off[i] = off;
                const int h = i == 0 ? P.d.hs : 1, v = i == 0 ? P.d.vs : 1;
                off += (size_t)P.d.mcus_x * h * P.d.mcus_y * v * 64;
            }
            P.scan_pos = p;
            return SSD_JPEG_OK;
        }
        // other APPn, COM, DNL, ...: skipped
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// host: entropy decoder
// ------------------------------------------------------------------------------------------------------------------------
struct Bits {
    const unsigned char* b;
    size_t n, p;
    uint64_t acc = 0;        // the next bits, left-aligned
    int cnt = 0;             // bits in acc
    int fake = 0;            // ... of which zero bits pushed behind the end of the data (a marker or the end of the file)
    bool marker = false;

    void fill() {
        while (cnt <= 56) {
            unsigned c = 0;
            if (!marker && p < n) {
                c = b[p];
                if (c == 0xFF) {
                    if (p + 1 < n && b[p + 1] == 0) p += 2;
                    else { marker = true; c = 0; fake += 8; }
                } else ++p;
            } else {
                marker = true;
                fake += 8;
            }
            acc |= (uint64_t)c << (56 - cnt);
            cnt += 8;
        }
    }
    void consume(int k) {
        acc <<= k;
        cnt -= k;
        if (cnt < fake) {
            if (p + 1 < n) fail("jpeg: marker 0xFF%02X at byte %zu where entropy-coded data is expected", b[p + 1], p);
            fail("jpeg: entropy-coded data ends early (truncated file)");
        }
    }
    int symbol(const HuffTable& h) {
        fill();
        const unsigned idx = (unsigned)(acc >> (64 - FAST_BITS));
        const int l = h.fast_len[idx];
        if (l) { consume(l); return h.fast_val[idx]; }
        const int code16 = (int)(acc >> 48);
        for (int len = FAST_BITS + 1; len <= 16; ++len) {
            const int c = code16 >> (16 - len);
            if (c <= h.maxcode[len]) {
                const int v = h.vals[h.valptr[len] + c - h.mincode[len]];
                consume(len);
                return v;
            }
        }
        fail("jpeg: bad Huffman code at byte %zu", p);
        return 0;
    }
    int receive_extend(int t) {          // t in 1..15
        fill();
        const int v = (int)(acc >> (64 - t));
        consume(t);
        return v >= (1 << (t - 1)) ? v : v - (1 << t) + 1;
    }
    void restart(int expect) {
        acc = 0; cnt = 0; fake = 0;
        SSD_REQUIRE(p + 1 < n && b[p] == 0xFF, "jpeg: restart marker RST%d missing at byte %zu", expect, p);
        while (p + 2 < n && b[p + 1] == 0xFF) ++p;
        SSD_REQUIRE(b[p + 1] == 0xD0 + expect, "jpeg: marker 0xFF%02X at byte %zu where RST%d is expected", b[p + 1], p, expect);
        p += 2;
        marker = false;
    }
};

int entropy_decode(const unsigned char* bytes, size_t n, short* coef, size_t cap_bytes, ssd_jpeg_desc* desc) {
    std::vector<Parsed> holder(1);           // (8 Huffman tables: off the stack)
    Parsed& P = holder[0];
    const int st = parse(bytes, n, P);
    if (st != SSD_JPEG_OK) { memset(desc, 0, sizeof *desc); return st; }
    const ssd_jpeg_desc& d = P.d;
    const size_t need = jpeg_coef_bytes(d);
    SSD_REQUIRE(coef != nullptr && need <= cap_bytes, "jpeg: the coefficient buffer holds %zu bytes, the image needs %zu", cap_bytes, need);
    memset(coef, 0, need);
    Bits br{bytes, n, P.scan_pos};
    const int nc = d.components;
    int pred[3] = {0, 0, 0};
    long long max_l1 = 0;
    int rst = 0;
    long long done = 0;
    for (int y = 0; y < d.mcus_y; ++y)
        for (int x = 0; x < d.mcus_x; ++x) {
            if (P.dri && done && done % P.dri == 0) {
                br.restart(rst);
                rst = (rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
            }
            ++done;
            for (int ci = 0; ci < nc; ++ci) {
                const int h = ci == 0 ? d.hs : 1, v = ci == 0 ? d.vs : 1;
                const size_t bw = (size_t)d.mcus_x * h;
                const HuffTable& hd = P.dc[P.comp_td[ci]];
                const HuffTable& ha = P.ac[P.comp_ta[ci]];
                const unsigned short* q = d.qt[ci];
                for (int by = 0; by < v; ++by)
                    for (int bx = 0; bx < h; ++bx) {
                        short* blk = coef + d.coef_off[ci] + (((size_t)y * v + by) * bw + (size_t)x * h + bx) * 64;
                        const int t = br.symbol(hd);
                        SSD_REQUIRE(t <= 15, "jpeg: DC size category %d", t);
                        if (t) pred[ci] += br.receive_extend(t);
                        SSD_REQUIRE(pred[ci] >= -32768 && pred[ci] <= 32767, "jpeg: DC value %d outside 16 bits", pred[ci]);
                        blk[0] = (short)pred[ci];
                        long long l1 = (long long)(pred[ci] < 0 ? -pred[ci] : pred[ci]) * q[0];
                        int k = 1;
                        while (k < 64) {
                            const int rs = br.symbol(ha), r = rs >> 4, s = rs & 15;
                            if (s == 0) {
                                if (r == 15) { k += 16; continue; }
                                break;
                            }
                            k += r;
                            SSD_REQUIRE(k <= 63, "jpeg: coefficient index %d past 63", k);
                            const int c = br.receive_extend(s);
                            const int z = ZIGZAG[k];
                            blk[z] = (short)c;
                            l1 += (long long)(c < 0 ? -c : c) * q[z];
                            ++k;
                        }
                        if (l1 > max_l1) max_l1 = l1;
                    }
            }
        }
    *desc = d;
    if (max_l1 > SSD_JPEG_MAX_L1) {          // the int32 kernels are not proven exact for it: the caller's fallback decodes it
        desc->max_l1 = max_l1 > 0x7fffffff ? 0x7fffffff : (int)max_l1;
        return SSD_JPEG_UNSUPPORTED;
    }
    desc->max_l1 = (int)max_l1;
    return SSD_JPEG_OK;
}

void export_table(const HuffTable& h, ssd_jpeg_huff_table& t) {
    memcpy(t.fast_len, h.fast_len, sizeof t.fast_len);
    memcpy(t.fast_val, h.fast_val, sizeof t.fast_val);
    memcpy(t.maxcode, h.maxcode, sizeof t.maxcode);
    memcpy(t.mincode, h.mincode, sizeof t.mincode);
    memcpy(t.valptr, h.valptr, sizeof t.valptr);
    memcpy(t.vals, h.vals, sizeof t.vals);
    t.maxcode[0] = -1; t.mincode[0] = 0; t.valptr[0] = 0;      // (length 0 is never used)
}

// the selectors of one table class -> at most two slots; false: the scan selects three different tables
bool assign_tables(const Parsed& P, const int* sel, const HuffTable* src, int* slot_out, ssd_jpeg_huff_table* dst) {
    int used[2], nu = 0;
    for (int c = 0; c < P.d.components; ++c) {
        int s = -1;
        for (int u = 0; u < nu; ++u)
            if (used[u] == sel[c]) s = u;
        if (s < 0) {
            if (nu == 2) return false;
            used[nu] = sel[c];
            export_table(src[sel[c]], dst[nu]);
            s = nu++;
        }
        slot_out[c] = s;
    }
    for (int c = P.d.components; c < 3; ++c) slot_out[c] = 0;
    return true;
}

}  // namespace

size_t jpeg_scan_segments(const unsigned char* bytes, size_t n) {
    std::vector<Parsed> holder(1);
    Parsed& P = holder[0];
    if (parse(bytes, n, P) != SSD_JPEG_OK) return 0;
    const long long mcus = (long long)P.d.mcus_x * P.d.mcus_y;
    return (size_t)(P.dri ? (mcus + P.dri - 1) / P.dri : 1);
}

// The markers as entropy_decode sees them, then the segments by a byte search alone: a segment runs up to the first FF that no
// 00 follows (Bits::fill's rule), and between two segments stands FF .. FF Dn with the index Bits::restart expects.
int jpeg_scan_plan(const unsigned char* bytes, size_t n, ssd_jpeg_desc* desc, ssd_jpeg_plan* plan) {
    SSD_REQUIRE(desc && plan, "jpeg: null argument");
    std::vector<Parsed> holder(1);
    Parsed& P = holder[0];
    const int st = parse(bytes, n, P);
    if (st != SSD_JPEG_OK) { memset(desc, 0, sizeof *desc); return st; }
    *desc = P.d;
    const long long mcus = (long long)P.d.mcus_x * P.d.mcus_y;
    const long long expect = P.dri ? (mcus + P.dri - 1) / P.dri : 1;
    SSD_REQUIRE(plan->seg != nullptr && plan->seg_cap >= expect, "jpeg: the segment array holds %d entries, the scan has %lld", plan->seg_cap, expect);
    plan->file_bytes = n;
    plan->scan_pos = P.scan_pos;
    plan->restart_interval = P.dri;
    plan->segments = (int)expect;
    if (n >= ((size_t)1 << 30)) return SSD_JPEG_TO_HOST;
    if (!assign_tables(P, P.comp_td, P.dc, plan->dc_sel, plan->dc) || !assign_tables(P, P.comp_ta, P.ac, plan->ac_sel, plan->ac))
        return SSD_JPEG_TO_HOST;
    size_t p = P.scan_pos;
    for (long long s = 0; s < expect; ++s) {
        const size_t begin = p;
        size_t end = n;
        while (p < n) {
            const unsigned char* q = static_cast<const unsigned char*>(memchr(bytes + p, 0xFF, n - p));
            if (!q) break;
            const size_t at = (size_t)(q - bytes);
            if (at + 1 < n && bytes[at + 1] == 0) { p = at + 2; continue; }
            end = at;
            break;
        }
        plan->seg[s].begin = (unsigned)begin;
        plan->seg[s].end = (unsigned)end;
        if (s + 1 == expect) break;
        p = end;
        if (!(p + 1 < n)) return SSD_JPEG_TO_HOST;                     // no marker where a restart is due
        while (p + 2 < n && bytes[p + 1] == 0xFF) ++p;
        if (bytes[p + 1] != 0xD0 + (int)(s & 7)) return SSD_JPEG_TO_HOST;
        p += 2;
    }
    return SSD_JPEG_OK;
}

int jpeg_parse_header(const unsigned char* bytes, size_t n, ssd_jpeg_desc* desc) {
    std::vector<Parsed> holder(1);
    const int st = parse(bytes, n, holder[0]);
    if (st == SSD_JPEG_OK) *desc = holder[0].d;
    else memset(desc, 0, sizeof *desc);
    return st;
}

size_t jpeg_coef_bytes(const ssd_jpeg_desc& d) {
    const size_t mcus = (size_t)d.mcus_x * d.mcus_y;
    return mcus * ((size_t)d.hs * d.vs + (d.components == 3 ? 2 : 0)) * 64 * sizeof(short);
}

int jpeg_entropy_decode(const unsigned char* bytes, size_t n, short* coef_out, size_t cap_bytes, ssd_jpeg_desc* desc) {
    return entropy_decode(bytes, n, coef_out, cap_bytes, desc);
}

void jpeg_entropy_decode_batch(const unsigned char* const* files, const size_t* sizes, int n, int threads, short* coef_out,
                               const unsigned long long* offsets, ssd_jpeg_desc* descs, int* status_out) {
    SSD_REQUIRE(n >= 0 && files && sizes && offsets && descs && status_out, "jpeg: null argument");
    SSD_REQUIRE(threads >= 1 && threads <= 64, "jpeg: threads must be in 1..64 (got %d)", threads);
    for (int i = 0; i < n; ++i)
        SSD_REQUIRE(offsets[i] % 16 == 0 && offsets[i] <= offsets[i + 1], "jpeg: offsets must ascend in multiples of 16 bytes (file %d)", i);
    std::atomic<int> next{0};
    std::mutex mu;
    int first_bad = n;
    std::string first_msg;
    auto work = [&]() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n) return;
            try {
                status_out[i] = entropy_decode(files[i], sizes[i], coef_out + offsets[i] / 2, (size_t)(offsets[i + 1] - offsets[i]), &descs[i]);
                if (status_out[i] == SSD_JPEG_OK)
                    for (int c = 0; c < descs[i].components; ++c) descs[i].coef_off[c] += offsets[i] / 2;
            } catch (const std::exception& e) {
                status_out[i] = SSD_JPEG_ERROR;
                memset(&descs[i], 0, sizeof descs[i]);
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
    if (first_bad < n) set_error("file %d: %s", first_bad, first_msg.c_str());
}

// ------------------------------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------------------------------
struct JpegImage {
    int w, h, comps, hs, vs;
    int bw[3], bh[3];                    // component planes in 8 x 8 blocks (whole MCUs)
    int blk_pre[4];                      // prefix of the planes' block counts
    unsigned long long coef_off[3];      // int16 elements
    unsigned long long plane_off[3];     // bytes inside the plane scratch; pitch = 8 * bw
    unsigned long long dst_off;
    unsigned short qt[3][64];
};

constexpr int IDCT_BLOCKS = 32;          // 8 x 8 blocks per workgroup of 256 (8 lanes per block)
constexpr int PACK_PIXELS = 16;          // pixels per lane = 48 bytes = three 16-byte stores

// jidctint.c (libjpeg's "islow" transform), one dimension.  int32 is exact for the accepted range (SSD_JPEG_MAX_L1).
__device__ __forceinline__ void idct_1d(const int* in, int* out, int shift) {
    int z1 = (in[2] + in[6]) * 4433;
    const int t2 = z1 - in[6] * 15137, t3 = z1 + in[2] * 6270;
    const int t0 = (in[0] + in[4]) * 8192, t1 = (in[0] - in[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = in[7], a1 = in[5], a2 = in[3], a3 = in[1];
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 = a0 + z1 + z3; a1 = a1 + z2 + z4; a2 = a2 + z2 + z3; a3 = a3 + z1 + z4;      // (this order of sums is the one DESIGN.md 13 bounds)
    const int r = 1 << (shift - 1);
    out[0] = (t10 + a3 + r) >> shift; out[7] = (t10 - a3 + r) >> shift;
    out[1] = (t11 + a2 + r) >> shift; out[6] = (t11 - a2 + r) >> shift;
    out[2] = (t12 + a1 + r) >> shift; out[5] = (t12 - a1 + r) >> shift;
    out[3] = (t13 + a0 + r) >> shift; out[4] = (t13 - a0 + r) >> shift;
}

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

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// 8 lanes per block.  Lane (block, i) loads coefficient row i as one 16-byte vector (a wave covers 1 KiB of contiguous
// coefficients), transforms COLUMN i after a trip through LDS, then ROW i after a second one, and stores the 8 pixels of row i.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const short* __restrict__ coef, const JpegImage* __restrict__ imgs,
                                                        const int* __restrict__ wg_start, int n, unsigned char* __restrict__ planes) {
    __shared__ __attribute__((aligned(16))) short sc[IDCT_BLOCKS * 64];
    __shared__ __attribute__((aligned(16))) int sw[IDCT_BLOCKS * 72];      // 72: the column pass's 64 lanes hit 64 different banks
    const int img = find_image(wg_start, n, blockIdx.x);
    const JpegImage& D = imgs[img];
    const int tid = threadIdx.x, slot = tid >> 3, i = tid & 7;
    const int lb = (blockIdx.x - wg_start[img]) * IDCT_BLOCKS + slot;
    const bool valid = lb < D.blk_pre[3];
    const int comp = valid ? (lb >= D.blk_pre[1]) + (lb >= D.blk_pre[2]) : 0;
    const int b = lb - D.blk_pre[comp];
    if (valid) {
        const uint4 v = *reinterpret_cast<const uint4*>(coef + D.coef_off[comp] + (size_t)b * 64 + i * 8);
        *reinterpret_cast<uint4*>(sc + slot * 64 + i * 8) = v;
    }
    __syncthreads();
    if (valid) {
        int x[8], o[8];
        for (int r = 0; r < 8; ++r) x[r] = (int)sc[slot * 64 + r * 8 + i] * (int)D.qt[comp][r * 8 + i];
        idct_1d(x, o, 11);
        for (int r = 0; r < 8; ++r) sw[slot * 72 + r * 8 + i] = o[r];
    }
    __syncthreads();
    if (valid) {
        int x[8], o[8];
        const int4 lo = *reinterpret_cast<const int4*>(sw + slot * 72 + i * 8), hi = *reinterpret_cast<const int4*>(sw + slot * 72 + i * 8 + 4);
        x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w; x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
        idct_1d(x, o, 18);
        unsigned p[8];
        for (int c = 0; c < 8; ++c) p[c] = (unsigned)clamp255(o[c] + 128);
        uint2 px;
        px.x = p[0] | (p[1] << 8) | (p[2] << 16) | (p[3] << 24);
        px.y = p[4] | (p[5] << 8) | (p[6] << 16) | (p[7] << 24);
        const int bw = D.bw[comp], by = b / bw, bx = b - by * bw;
        *reinterpret_cast<uint2*>(planes + D.plane_off[comp] + ((size_t)by * 8 + i) * ((size_t)bw * 8) + (size_t)bx * 8) = px;
    }
}

// jdsample.c's h2v1 / h2v2 "fancy" upsampling of one chroma plane at output pixel (x, y); cw x ch = the REAL chroma size
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ p, int pitch, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(size_t)y * pitch + x];
    const int cx = x >> 1, odd = x & 1;
    int nb = odd ? cx + 1 : cx - 1;
    nb = nb < 0 ? 0 : (nb > cw - 1 ? cw - 1 : nb);
    if (vs == 1) {
        const unsigned char* row = p + (size_t)y * pitch;
        return (3 * row[cx] + row[nb] + (odd ? 2 : 1)) >> 2;
    }
    const int cy = y >> 1;
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : (fy > ch - 1 ? ch - 1 : fy);
    const unsigned char* near = p + (size_t)cy * pitch;
    const unsigned char* far = p + (size_t)fy * pitch;
    const int s = 3 * near[cx] + far[cx], sn = 3 * near[nb] + far[nb];
    return (3 * s + sn + (odd ? 7 : 8)) >> 4;
}

// One lane = 16 consecutive pixels of the image's flat [h*w] order (48 bytes); the workgroup's 12 KiB go through LDS so that
// every store instruction writes 256 consecutive 16-byte vectors.
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const unsigned char* __restrict__ planes, const JpegImage* __restrict__ imgs,
                                                        const int* __restrict__ wg_start, int n, unsigned char* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) unsigned so[256 * 12];
    const int img = find_image(wg_start, n, blockIdx.x);
    const JpegImage& D = imgs[img];
    const int tid = threadIdx.x;
    const int wg = blockIdx.x - wg_start[img];
    const int w = D.w, h = D.h, npix = w * h;
    const int p0 = (wg * 256 + tid) * PACK_PIXELS;
    const unsigned char* py = planes + D.plane_off[0];
    const int pitch_y = D.bw[0] * 8;
    const bool color = D.comps == 3;
    const unsigned char* pcb = planes + D.plane_off[color ? 1 : 0];
    const unsigned char* pcr = planes + D.plane_off[color ? 2 : 0];
    const int pitch_c = D.bw[color ? 1 : 0] * 8;
    const int cw = (w + D.hs - 1) / D.hs, ch = (h + D.vs - 1) / D.vs;
    int y = p0 / w, x = p0 - y * w;
    unsigned char px[48];
#pragma unroll
    for (int k = 0; k < PACK_PIXELS; ++k) {
        int B = 0, G = 0, R = 0;
        if (p0 + k < npix) {
            const int Y = py[(size_t)y * pitch_y + x];
            if (color) {
                const int cb = chroma_at(pcb, pitch_c, cw, ch, D.hs, D.vs, x, y) - 128;
                const int cr = chroma_at(pcr, pitch_c, cw, ch, D.hs, D.vs, x, y) - 128;
                R = clamp255(Y + ((91881 * cr + 32768) >> 16));
                B = clamp255(Y + ((116130 * cb + 32768) >> 16));
                G = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
            } else {
                B = G = R = Y;
            }
        }
        px[3 * k] = (unsigned char)B; px[3 * k + 1] = (unsigned char)G; px[3 * k + 2] = (unsigned char)R;
        if (++x == w) { x = 0; ++y; }
    }
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        uint4 q;
        unsigned t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = v * 16 + j * 4;
            t[j] = (unsigned)px[o] | ((unsigned)px[o + 1] << 8) | ((unsigned)px[o + 2] << 16) | ((unsigned)px[o + 3] << 24);
        }
        q.x = t[0]; q.y = t[1]; q.z = t[2]; q.w = t[3];
        *reinterpret_cast<uint4*>(so + tid * 12 + v * 4) = q;
    }
    __syncthreads();
    const size_t bytes = ((size_t)npix * 3 + 15) / 16 * 16;      // the last vector may reach into the alignment padding behind the image
    const size_t base = (size_t)wg * 256 * 48;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const int c = v * 256 + tid;
        const size_t off = base + (size_t)c * 16;
        if (off < bytes) *reinterpret_cast<uint4*>(dst + D.dst_off + off) = *reinterpret_cast<const uint4*>(so + c * 4);
    }
}

namespace {
struct Layout {
    size_t img_off, wg1_off, wg2_off, plane_off, total;
};
Layout ws_layout(int n) {
    Layout l;
    l.img_off = 0;
    l.wg1_off = ((size_t)n * sizeof(JpegImage) + 255) / 256 * 256;
    l.wg2_off = l.wg1_off + ((size_t)(n + 1) * sizeof(int) + 255) / 256 * 256;
    l.plane_off = l.wg2_off + ((size_t)(n + 1) * sizeof(int) + 255) / 256 * 256;
    l.total = l.plane_off;
    return l;
}
bool sampling_ok(const ssd_jpeg_desc& d) {
    if (d.components == 1) return d.hs == 1 && d.vs == 1;
    return d.components == 3 && ((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2));
}
void require_desc(const ssd_jpeg_desc& d, int i) {
    SSD_REQUIRE(d.width >= 1 && d.height >= 1 && d.width <= 16384 && d.height <= 16384, "jpeg: image %d: size %d x %d", i, d.width, d.height);
    SSD_REQUIRE(sampling_ok(d), "jpeg: image %d: %d components with luma sampling %dx%d", i, d.components, d.hs, d.vs);
    SSD_REQUIRE(d.mcus_x == (d.width + 8 * d.hs - 1) / (8 * d.hs) && d.mcus_y == (d.height + 8 * d.vs - 1) / (8 * d.vs),
                "jpeg: image %d: %d x %d MCUs do not match its %d x %d pixels", i, d.mcus_x, d.mcus_y, d.width, d.height);
}
size_t plane_bytes(const ssd_jpeg_desc& d) { return jpeg_coef_bytes(d) / sizeof(short); }      // one byte per coefficient
}  // namespace

size_t jpeg_ws_bytes(const ssd_jpeg_desc* descs, int n) {
    SSD_REQUIRE(n >= 1 && descs, "jpeg: empty batch");
    size_t total = ws_layout(n).total;
    for (int i = 0; i < n; ++i) {
        require_desc(descs[i], i);
        total += (plane_bytes(descs[i]) + 255) / 256 * 256;
    }
    return total;
}

void jpeg_decode_batch(const short* coef_dev, size_t coef_bytes, const ssd_jpeg_desc* descs, int n, unsigned char* dst_dev,
                       size_t dst_bytes, void* ws, size_t ws_bytes, hipStream_t s) {
    SSD_REQUIRE(n >= 1 && descs, "jpeg: empty batch");
    SSD_REQUIRE(coef_dev && dst_dev && ws, "jpeg: null argument");
    SSD_REQUIRE(((uintptr_t)coef_dev | (uintptr_t)dst_dev | (uintptr_t)ws) % 16 == 0, "jpeg: coef_dev, dst_dev and ws_dev must be 16-byte aligned");
    SSD_REQUIRE(ws_bytes >= jpeg_ws_bytes(descs, n), "jpeg: workspace of %zu bytes, %zu needed", ws_bytes, jpeg_ws_bytes(descs, n));
    const Layout l = ws_layout(n);
    // (the staging block outlives the call: the copy below reads it)
    static thread_local std::vector<unsigned char> staging;
    staging.assign(l.plane_off, 0);
    JpegImage* imgs = reinterpret_cast<JpegImage*>(staging.data() + l.img_off);
    int* wg1 = reinterpret_cast<int*>(staging.data() + l.wg1_off);
    int* wg2 = reinterpret_cast<int*>(staging.data() + l.wg2_off);
    size_t plane = l.plane_off;
    long long n1 = 0, n2 = 0;
    double blocks = 0, pixels = 0;
    for (int i = 0; i < n; ++i) {
        const ssd_jpeg_desc& d = descs[i];
        require_desc(d, i);
        SSD_REQUIRE(d.max_l1 >= 0 && d.max_l1 <= SSD_JPEG_MAX_L1, "jpeg: image %d: block L1 norm %d beyond the 32-bit range guard %d", i, d.max_l1, SSD_JPEG_MAX_L1);
        JpegImage& D = imgs[i];
        D.w = d.width; D.h = d.height; D.comps = d.components; D.hs = d.hs; D.vs = d.vs;
        D.blk_pre[0] = 0;
        for (int c = 0; c < 3; ++c) {
            const bool on = c < d.components;
            D.bw[c] = on ? d.mcus_x * (c == 0 ? d.hs : 1) : 0;
            D.bh[c] = on ? d.mcus_y * (c == 0 ? d.vs : 1) : 0;
            const size_t nb = (size_t)D.bw[c] * D.bh[c];
            D.blk_pre[c + 1] = D.blk_pre[c] + (int)nb;
            D.coef_off[c] = on ? d.coef_off[c] : 0;
            D.plane_off[c] = plane - l.plane_off;
            if (on) {
                SSD_REQUIRE(d.coef_off[c] % 8 == 0 && d.coef_off[c] <= coef_bytes / 2 && nb * 64 <= coef_bytes / 2 - d.coef_off[c],
                            "jpeg: image %d: coefficient plane %d (offset %llu, %zu blocks) outside the %zu-byte buffer", i, c, d.coef_off[c], nb, coef_bytes);
                plane += nb * 64;
            }
            memcpy(D.qt[c], d.qt[c], sizeof D.qt[c]);
        }
        plane = (plane + 255) / 256 * 256;
        D.dst_off = d.dst_off;
        const size_t out = ((size_t)d.width * d.height * 3 + 15) / 16 * 16;
        SSD_REQUIRE(d.dst_off % 16 == 0 && d.dst_off <= dst_bytes && out <= dst_bytes - d.dst_off,
                    "jpeg: image %d: %zu bytes at offset %llu outside the %zu-byte destination", i, out, d.dst_off, dst_bytes);
        wg1[i] = (int)n1; wg2[i] = (int)n2;
        n1 += cdiv(D.blk_pre[3], IDCT_BLOCKS);
        n2 += cdiv((long long)d.width * d.height, 256 * PACK_PIXELS);
        blocks += D.blk_pre[3];
        pixels += (double)d.width * d.height;
    }
    SSD_REQUIRE(n1 < (1ll << 30) && n2 < (1ll << 30), "jpeg: batch too large for one launch");
    wg1[n] = (int)n1; wg2[n] = (int)n2;
    char* base = static_cast<char*>(ws);
    HIP_OK(hipMemcpyAsync(base, staging.data(), l.plane_off, hipMemcpyHostToDevice, s));
    const JpegImage* imgs_dev = reinterpret_cast<const JpegImage*>(base + l.img_off);
    unsigned char* planes = reinterpret_cast<unsigned char*>(base + l.plane_off);
    {
        ProfScope prof("jpeg_idct", 0.0, blocks * (128 + 64), s);
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)n1), dim3(256), 0, s, coef_dev, imgs_dev, reinterpret_cast<const int*>(base + l.wg1_off), n, planes);
    }
    {
        ProfScope prof("jpeg_pack", 0.0, blocks * 64 + pixels * 3, s);
        hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)n2), dim3(256), 0, s, planes, imgs_dev, reinterpret_cast<const int*>(base + l.wg2_off), n, dst_dev);
    }
    HIP_OK(hipGetLastError());
}

}  // namespace ssd
