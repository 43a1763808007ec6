"""Test oracle: the front half of a baseline JPEG encode (BGR -> YCbCr, edge replication, chroma downsampling, libjpeg's "islow"
forward DCT, quantisation, the dummy-block rule) from pixels to coefficient planes, in numpy int64.  It restates libjpeg-turbo's
default encoder path rule by rule; the product never imports it.  `fdct_bounds` derives the 32-bit bound of
DESIGN.md 14 from the same transform."""
import numpy as np

STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                       47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
SAMPLING = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}


class Desc:
    """the fields of ssd_jpeg_desc the tests compare"""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def quant_tables(quality):
    """jcparam.c: jpeg_quality_scaling + jpeg_add_quant_table with force_baseline"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((t * scale + 50) // 100, 1, 255) for t in (STD_LUMA, STD_CHROMA)]


def ycc_planes(bgr):
    """jccolor.c, 16-bit fixed point: three [h, w] int64 planes"""
    B, G, R = [bgr[:, :, k].astype(np.int64) for k in range(3)]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    return Y, Cb, Cr


def _pad(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode='edge')


def downsample(p, hs, vs, mcus_x, mcus_y):
    """jcprepct.c + jcsample.c: full-size samples replicated to the right up to whole MCUs and downwards up to a whole row group,
    h2v1 / h2v2 box filter with the alternating bias restarting in every output row, then the DOWNSAMPLED rows replicated
    downwards up to whole MCUs"""
    h, w = p.shape
    ch = -(-h // vs)
    p = _pad(p, ch * vs, mcus_x * 8 * hs)
    cols = np.arange(mcus_x * 8)
    if (hs, vs) == (1, 1):
        out = p
    elif (hs, vs) == (2, 1):
        out = (p[:, 0::2] + p[:, 1::2] + (cols & 1)) >> 1
    else:
        out = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + (cols & 1)) >> 2
    return _pad(out, mcus_y * 8, mcus_x * 8)


def _fdct_1d(d):
    """d [..., 8]: the eight outputs of jfdctint.c's pass before the descale; [0] and [4] are the plain sums"""
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., k] for k in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    o[0], o[4] = t10 + t11, t10 - t11
    z1 = (t12 + t13) * 4433
    o[2] = z1 + t13 * 6270
    o[6] = z1 - t12 * 15137
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    z3 = -z3 * 16069 + z5
    z4 = -z4 * 3196 + z5
    z1, z2 = -z1 * 7373, -z2 * 20995
    o[7] = t4 * 2446 + z1 + z3
    o[5] = t5 * 16819 + z2 + z4
    o[3] = t6 * 25172 + z2 + z3
    o[1] = t7 * 12299 + z1 + z4
    return o


def fdct_blocks(s):
    """s [..., 8, 8] int64 samples - 128 (row, column) -> coefficients scaled by 8, as jfdctint.c leaves them"""
    o = _fdct_1d(s)                                                                   # rows
    w = np.stack([o[k] << 2 if k in (0, 4) else (o[k] + 1024) >> 11 for k in range(8)], -1)
    o = _fdct_1d(np.swapaxes(w, -1, -2))                                              # columns
    return np.stack([(o[k] + 2) >> 2 if k in (0, 4) else (o[k] + 16384) >> 15 for k in range(8)], -2)


def quantise(c, q):
    """jcdctmgr.c: divisor 8 q, half of it added to the magnitude, truncating division, sign restored"""
    d = np.asarray(q, np.int64).reshape(8, 8) << 3
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def plane_coefs(p, q):
    """[bh*8, bw*8] samples -> [bh, bw, 64] quantised coefficients, natural order"""
    bh, bw = p.shape[0] // 8, p.shape[1] // 8
    blocks = (p - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    return quantise(fdct_blocks(blocks), q).reshape(bh, bw, 64)


def encode_planes(bgr, quality=95, subsampling='4:2:0'):
    """uint8 [h, w, 3] BGR -> (Desc, int16 coefficient array) laid out as ssd_jpeg_entropy_decode leaves them for libjpeg's file"""
    hs, vs = SAMPLING[subsampling]
    h, w = bgr.shape[:2]
    mcus_x, mcus_y = -(-w // (8 * hs)), -(-h // (8 * vs))
    ql, qc = quant_tables(quality)
    Y, Cb, Cr = ycc_planes(bgr)
    luma = plane_coefs(_pad(Y, mcus_y * vs * 8, mcus_x * hs * 8), ql)
    # jccoefct.c: only ceil(w/8) x ceil(h/8) luma blocks are transformed; a dummy block has AC 0 and the DC of the block before it
    # in the MCU's order (left neighbour; for a dummy row: the right block of the row above)
    rbw, rbh = -(-w // 8), -(-h // 8)
    if rbw < mcus_x * hs:
        luma[:, rbw, 1:] = 0
        luma[:, rbw, 0] = luma[:, rbw - 1, 0]
    if rbh < mcus_y * vs:
        luma[rbh, :, 1:] = 0
        luma[rbh, 0::2, 0] = luma[rbh - 1, 1::2, 0]
        luma[rbh, 1::2, 0] = luma[rbh - 1, 1::2, 0]
    planes = [luma] + [plane_coefs(downsample(c, hs, vs, mcus_x, mcus_y), qc) for c in (Cb, Cr)]
    coef = np.concatenate([p.reshape(-1) for p in planes]).astype(np.int16)
    off = np.cumsum([0] + [p.size for p in planes])
    d = Desc(width=w, height=h, components=3, hs=hs, vs=vs, mcus_x=mcus_x, mcus_y=mcus_y, coef_off=[int(o) for o in off[:3]],
             qt=[[int(v) for v in t] for t in (ql, qc, qc)])
    return d, coef


def fdct_bounds():
    """The largest magnitude any int32 value of the kernel's two passes can take for samples in -128 .. 127, derived as DESIGN.md
    14 does: every sub-expression of `_fdct_1d` is an integer linear form of its eight inputs, so its magnitude is at most the
    L1 norm of its coefficients (read off unit impulses) times the largest input magnitude.  Returns (row pass, column pass)."""
    forms = []

    class V:                                        # a linear form that records every intermediate it takes part in
        def __init__(self, c):
            self.c = np.asarray(c, np.int64)
            forms.append(self.c)

        def __add__(self, o):
            return V(self.c + o.c)

        def __sub__(self, o):
            return V(self.c - o.c)

        def __mul__(self, k):
            return V(self.c * k)

        def __neg__(self):
            return V(-self.c)

    class Row:
        def __getitem__(self, key):
            return V(np.eye(8, dtype=np.int64)[key[-1]])

    outs = _fdct_1d(Row())
    l1 = max(int(np.abs(f).sum()) for f in forms)                           # any intermediate
    out_l1 = [int(np.abs(o.c).sum()) for o in outs]
    rows = 128 * l1 + 1024                                                   # + the rounding term of the descale
    # a column holds row-pass outputs of ONE frequency k: |w_k| <= 4 * 128 * L1 (k = 0, 4) or (128 * L1 + 1024) >> 11
    w = [128 * out_l1[k] * 4 if k in (0, 4) else (128 * out_l1[k] + 1024) >> 11 for k in range(8)]
    cols = max(w) * l1 + 16384
    return rows, cols
