"""numpy / torch-CPU oracle of the mxfp6 inference format: OCP MX FP6 E2M3 codes (1 sign, 2 exponent bits of bias 1,
3 mantissa bits, no Inf / NaN; magnitudes 0, 0.125 ... 0.875, 1 ... 1.875, 2 ... 3.75, 4 ... 7.5) with one E8M0 scale byte per 32
consecutive channels (byte e = 2^(e - 127)).

Scale rule on the bit pattern of the block's fp32 absmax a (E = biased exponent - 127, m = the 23 mantissa bits):
x = clamp(E - 2 + (m > 0x700000), -127, 127), byte x + 127 (an all-zero block: byte 0); codes = RNE(clamp(ldexp(v, -x), -7.5, 7.5)).
x is the smallest power of two with a / 2^x <= 7.5 = 1.875 * 2^2 (scale_exponent_by_definition says so without looking at bits).

Packing: code j of a block sits in bits 6 j ... 6 j + 5 of a little-endian 24-byte string.  Activations: codes uint8
[..., C / 32, 24] + scales uint8 [..., C / 32].  Filters: blocks along Ci, w6 [tap][Co][Ci / 32][24] + wscales [tap][Co][Ci / 32],
no per-channel scale.  Everything the GPU tests compare against is computed here, in float64, from the bytes the kernels read."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ssdvgg_ref as ref

BLOCK = 32
BYTES = 24                                   # 32 codes of 6 bits
E2M3_MAX = 7.5
OUT_BF16, OUT_F32, OUT_MX, OUT_BF16_MX = 0, 1, 4, 5


def _decode_table():
    t = np.zeros(64, np.float64)
    for c in range(64):
        s, e, m = c >> 5, (c >> 3) & 3, c & 7
        v = m / 8.0 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 1)
        t[c] = -v if s else v
    return t


DECODE = _decode_table()
_POS = DECODE[:32]                           # the 32 non-negative values, ascending: 0 ... 7.5
_MID = (_POS[1:] + _POS[:-1]) / 2            # midpoints between neighbours (exact)


def decode(codes):
    """unpacked codes (0 ... 63) -> float64 values"""
    return DECODE[np.asarray(codes, np.uint8)]


def encode(v):
    """float values -> unpacked uint8 codes: clamp to +-7.5, then round to nearest, ties to the even code; the sign bit follows the
    input's (-0 and negative values that round to zero give code 32)"""
    v = np.asarray(v, np.float64)
    a = np.minimum(np.abs(v), E2M3_MAX)
    lo = np.searchsorted(_MID, a, side='left')        # first midpoint >= a: a lies in (mid[lo-1], mid[lo]]
    tie = (lo < len(_MID)) & (a == _MID[np.minimum(lo, len(_MID) - 1)])
    code = np.where(tie & (lo % 2 == 1), lo + 1, lo)   # at a midpoint between codes lo and lo + 1 take the even one
    return (code.astype(np.uint8) | (np.signbit(v).astype(np.uint8) << 5)).astype(np.uint8)


def pack(codes):
    """unpacked codes [..., C] -> bytes [..., C / 32, 24]: code j of a block in bits 6 j ... 6 j + 5, little-endian"""
    c = np.asarray(codes, np.uint8)
    assert c.shape[-1] % BLOCK == 0 and c.max(initial=0) < 64
    c = c.reshape(c.shape[:-1] + (c.shape[-1] // BLOCK, BLOCK // 4, 4)).astype(np.uint32)
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)      # four codes = three bytes
    out = np.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF], -1).astype(np.uint8)
    return out.reshape(out.shape[:-2] + (BYTES,))


def unpack(packed):
    """bytes [..., C / 32, 24] -> unpacked codes [..., C]"""
    p = np.asarray(packed, np.uint8)
    assert p.shape[-1] == BYTES
    b = p.reshape(p.shape[:-1] + (BLOCK // 4, 3)).astype(np.uint32)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    c = np.stack([w & 63, (w >> 6) & 63, (w >> 12) & 63, (w >> 18) & 63], -1).astype(np.uint8)
    return c.reshape(p.shape[:-2] + (p.shape[-2] * BLOCK,))


def scale_exponent(amax):
    """the rule on bits: fp32 absmax (>= 0) -> int x in -127 ... 127"""
    u = np.ascontiguousarray(amax, np.float32).view(np.uint32).astype(np.int64)
    x = ((u >> 23) & 0xFF) - 127 - 2 + ((u & 0x7FFFFF) > 0x700000)
    return np.clip(x, -127, 127)


def scale_exponent_by_definition(amax):
    """the smallest x in -127 ... 127 with a / 2^x <= 7.5, by exact arithmetic on fractions"""
    from fractions import Fraction
    out = []
    for a in np.asarray(amax, np.float32).ravel().tolist():
        a = Fraction(a)
        x = -127
        while x < 127 and a / Fraction(2) ** x > Fraction(15, 2):
            x += 1
        out.append(x)
    return np.array(out, np.int64).reshape(np.shape(amax))


def scale_bytes(v):
    """v [..., C] -> uint8 [..., C / 32]"""
    v = np.asarray(v, np.float32)
    assert v.shape[-1] % BLOCK == 0
    am = np.abs(v.reshape(v.shape[:-1] + (v.shape[-1] // BLOCK, BLOCK))).max(-1)
    return (scale_exponent(am) + 127).astype(np.uint8)


def quantize_codes(v):
    """fp32 [..., C] -> (unpacked codes [..., C], scales [..., C / 32]); the scaling is an exact ldexp in fp32"""
    v = np.asarray(v, np.float32)
    s = scale_bytes(v)
    x = np.repeat(s.astype(np.int32) - 127, BLOCK, axis=-1)
    return encode(np.ldexp(v, -x).astype(np.float64)), s


def quantize(v):
    """fp32 [..., C] -> (bytes [..., C / 32, 24], scales [..., C / 32])"""
    c, s = quantize_codes(v)
    return pack(c), s


def scale_values(scales):
    """scale bytes -> float64 2^(e - 127)"""
    return np.ldexp(1.0, np.asarray(scales, np.uint8).astype(np.int32) - 127)


def dequantize(packed, scales):
    """-> float64 [..., C]: code value times 2^(e - 127) (exact)"""
    return decode(unpack(packed)) * np.repeat(scale_values(scales), BLOCK, axis=-1)


def quantize_filter(w_hwio):
    """fp32 [kh][kw][Ci][Co] -> (w6 [tap][Co][Ci / 32][24], wscales [tap][Co][Ci / 32]): blocks along Ci"""
    w = np.asarray(w_hwio, np.float32)
    kh, kw, ci, co = w.shape
    return quantize(np.ascontiguousarray(np.transpose(w.reshape(kh * kw, ci, co), (0, 2, 1))))


def dequantize_filter(w6, wscales, kh, kw):
    """-> float64 HWIO [kh][kw][Ci][Co]"""
    v = dequantize(w6, wscales)                       # [tap][Co][Ci]
    taps, co, ci = v.shape
    return np.ascontiguousarray(np.transpose(v, (0, 2, 1))).reshape(kh, kw, ci, co)


def conv_values(xv, wv, stride, dil, padding):
    """float64 convolution of dequantised activations xv [B,H,W,Ci] with the dequantised filter wv (HWIO).
    -> (acc [B,Ho,Wo,Co], absacc: the same sum over |x * w|)"""
    x = torch.from_numpy(np.asarray(xv, np.float64)).permute(0, 3, 1, 2)
    w = torch.from_numpy(np.asarray(wv, np.float64))
    if padding == 'BR1':
        x = F.pad(x, (0, 1, 0, 1))
        padding = 'VALID'
    acc = ref.conv2d_tf(x, w, stride, padding, dil).permute(0, 2, 3, 1).numpy()
    absacc = ref.conv2d_tf(x.abs(), w.abs(), stride, padding, dil).permute(0, 2, 3, 1).numpy()
    return acc, absacc


def conv_values_rows(xv, wv, dil, r0, r1):
    """conv_values for the output rows [r0, r1) of a stride-1 SAME layer (odd square kernel)"""
    x = torch.from_numpy(np.asarray(xv, np.float64)).permute(0, 3, 1, 2)
    w = torch.from_numpy(np.asarray(wv, np.float64)).permute(3, 2, 0, 1)
    k = w.shape[2]
    p = dil * (k - 1) // 2
    x = F.pad(x, (p, p, p, p))[:, :, r0:r1 + 2 * p, :]
    acc = F.conv2d(x, w, None, 1, 0, dil).permute(0, 2, 3, 1).numpy()
    absacc = F.conv2d(x.abs(), w.abs(), None, 1, 0, dil).permute(0, 2, 3, 1).numpy()
    return acc, absacc


def epilogue(acc, bias, relu):
    """float64 y_ref = relu?(acc + bias[co]): every scale went through the operands"""
    y = acc + (0.0 if bias is None else np.asarray(bias, np.float64))
    return np.maximum(y, 0.0) if relu else y


def accumulation_bound(absacc, K):
    """B = K * 2^-23 * sum |x * w| over the dequantised operands: K fp32 additions at one ulp each"""
    return K * 2.0 ** -23 * absacc


def e2m3_step(a):
    """spacing of the e2m3 grid at magnitude a (float64 array): 1/8 below 2, 1/4 below 4, 1/2 up to 7.5"""
    a = np.minimum(np.abs(a), E2M3_MAX)
    return np.where(a < 2, 0.125, np.where(a < 4, 0.25, 0.5))


def maxpool(packed, scales, k, stride):
    """TF SAME max-pool of the dequantised tensor (cells outside the image never win), quantised again.  -> (bytes, scales)"""
    x = torch.from_numpy(dequantize(packed, scales)).permute(0, 3, 1, 2)
    y = ref.maxpool_tf(x, k, stride).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    return quantize(y.astype(np.float32))
