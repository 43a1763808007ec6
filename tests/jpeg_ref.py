"""Test oracle: the back half of a baseline JPEG decode (dequantise, libjpeg's "islow" inverse DCT, "fancy" chroma upsampling,
YCbCr -> BGR) from coefficient planes, in numpy int64.  It restates libjpeg-turbo's default decode path rule by rule
(DESIGN.md 13); the product never imports it."""
import numpy as np

C = dict(a=2446, b=3196, c=4433, d=6270, e=7373, f=9633, g=12299, h=15137, i=16069, j=16819, k=20995, l=25172)


def _idct_1d(x, shift):
    """x [..., 8 (frequency), n] int64 -> the transform along axis -2, descaled by `shift` bits with round-half-up"""
    i0, i1, i2, i3, i4, i5, i6, i7 = [x[..., k, :] for k in range(8)]
    z1 = (i2 + i6) * C['c']
    t2 = z1 - i6 * C['h']
    t3 = z1 + i2 * C['d']
    t0 = (i0 + i4) * 8192
    t1 = (i0 - i4) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1 = a0 + a3
    z2 = a1 + a2
    z3 = a0 + a2
    z4 = a1 + a3
    z5 = (z3 + z4) * C['f']
    a0 = a0 * C['a']
    a1 = a1 * C['j']
    a2 = a2 * C['l']
    a3 = a3 * C['g']
    z1 = -z1 * C['e']
    z2 = -z2 * C['k']
    z3 = -z3 * C['i'] + z5
    z4 = -z4 * C['b'] + z5
    a0 = a0 + z1 + z3
    a1 = a1 + z2 + z4
    a2 = a2 + z2 + z3
    a3 = a3 + z1 + z4
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    r = 1 << (shift - 1)
    return np.stack([(v + r) >> shift for v in out], axis=-2)


def idct_blocks(deq):
    """deq [..., 8, 8] int64 dequantised coefficients (row, column) -> pixels 0..255"""
    w = _idct_1d(deq, 11)                                  # columns first, 11 bits
    w = _idct_1d(np.swapaxes(w, -1, -2), 18)               # then rows, 18 bits
    return np.clip(np.swapaxes(w, -1, -2) + 128, 0, 255)


def plane_pixels(coef, bh, bw, q):
    """coef [bh*bw*64] int16 in natural order, q [64] -> the [bh*8, bw*8] component plane"""
    c = coef.astype(np.int64).reshape(bh, bw, 8, 8) * np.asarray(q, np.int64).reshape(8, 8)
    return idct_blocks(c).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample(s, hs, vs, W, H):
    """the real ceil(W/hs) x ceil(H/vs) chroma samples -> [H, W] by the triangle filters; a missing neighbour is the sample itself"""
    if hs == 1 and vs == 1:
        return s[:H, :W]
    if vs == 2:
        up = np.concatenate([s[:1], s[:-1]])
        dn = np.concatenate([s[1:], s[-1:]])
        rows = np.empty((2 * s.shape[0], s.shape[1]), np.int64)
        rows[0::2] = 3 * s + up
        rows[1::2] = 3 * s + dn
        b0, b1, sh = 8, 7, 4
    else:
        rows, b0, b1, sh = s, 1, 2, 2
    left = np.concatenate([rows[:, :1], rows[:, :-1]], 1)
    right = np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    o = np.empty((rows.shape[0], 2 * rows.shape[1]), np.int64)
    o[:, 0::2] = (3 * rows + left + b0) >> sh
    o[:, 1::2] = (3 * rows + right + b1) >> sh
    return o[:H, :W]


def decode_planes(coef, desc):
    """coef: int16 array the entropy stage wrote; desc: an object with width, height, components, hs, vs, mcus_x, mcus_y,
    coef_off[3], qt[3][64] (ssd_jpeg_desc).  Returns uint8 [H, W, 3] BGR."""
    W, H, nc, hs, vs = desc.width, desc.height, desc.components, desc.hs, desc.vs
    planes = []
    for c in range(nc):
        bw = desc.mcus_x * (hs if c == 0 else 1)
        bh = desc.mcus_y * (vs if c == 0 else 1)
        off = int(desc.coef_off[c])
        planes.append(plane_pixels(np.asarray(coef[off:off + bw * bh * 64]), bh, bw, list(desc.qt[c])))
    Y = planes[0][:H, :W]
    if nc == 1:
        return np.repeat(Y[:, :, None], 3, 2).astype(np.uint8)
    cw, ch = -(-W // hs), -(-H // vs)
    cb = upsample(planes[1][:ch, :cw], hs, vs, W, H) - 128
    cr = upsample(planes[2][:ch, :cw], hs, vs, W, H) - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([B, G, R], -1), 0, 255).astype(np.uint8)
