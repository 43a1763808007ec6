"""numpy / torch-CPU oracle of the mxfp8 inference format: OCP e4m3fn codes [..., C] with one E8M0 scale byte per 32
consecutive channels [..., C / 32] (byte e = 2^(e - 127)).

Scale rule on the bit pattern of the block's fp32 absmax a (E = biased exponent - 127, m = the 23 mantissa bits):
x = clamp(E - 8 + (m > 0x600000), -127, 127), byte x + 127; codes = RNE(clamp(ldexp(v, -x), -448, 448)).  x is the smallest power of
two with a / 2^x <= 448 = 1.75 * 2^8 (scale_exponent_by_definition says so without looking at bits).  Everything the GPU tests
compare against is computed here, in float64, from the same codes and scales the kernels read."""
import numpy as np
import torch
import torch.nn.functional as F

import fp8_ref as f8
from oracle import ssdvgg_ref as ref

BLOCK = 32
OUT_BF16, OUT_F32, OUT_MX, OUT_BF16_MX = 0, 1, 4, 5


def scale_exponent(amax):
    """the rule on bits: fp32 absmax (>= 0) -> int x in -127 ... 127"""
    u = np.ascontiguousarray(amax, np.float32).view(np.uint32).astype(np.int64)
    x = ((u >> 23) & 0xFF) - 127 - 8 + ((u & 0x7FFFFF) > 0x600000)
    return np.clip(x, -127, 127)


def scale_exponent_by_definition(amax):
    """the smallest x in -127 ... 127 with a / 2^x <= 448, by exact arithmetic on Python integers / fractions"""
    from fractions import Fraction
    out = []
    for a in np.asarray(amax, np.float32).ravel().tolist():
        a = Fraction(a)
        x = -127
        while x < 127 and a / Fraction(2) ** x > 448:
            x += 1
        out.append(x)
    return np.array(out, np.int64).reshape(np.shape(amax))


def scale_bytes(v):
    """v [..., C] -> uint8 [..., C / 32]"""
    v = np.asarray(v, np.float32)
    assert v.shape[-1] % BLOCK == 0
    am = np.abs(v.reshape(v.shape[:-1] + (v.shape[-1] // BLOCK, BLOCK))).max(-1)
    return (scale_exponent(am) + 127).astype(np.uint8)


def quantize(v):
    """fp32 [..., C] -> (codes uint8 [..., C], scales uint8 [..., C / 32]); the scaling is an exact ldexp in fp32"""
    v = np.asarray(v, np.float32)
    s = scale_bytes(v)
    x = np.repeat(s.astype(np.int32) - 127, BLOCK, axis=-1)
    return f8.encode(np.ldexp(v, -x).astype(np.float64)), s


def scale_values(scales):
    """scale bytes -> float64 2^(e - 127)"""
    return np.ldexp(1.0, np.asarray(scales, np.uint8).astype(np.int32) - 127)


def dequantize(codes, scales):
    """-> float64 [..., C]: code value times 2^(e - 127) (exact; also exact in fp32 for fp32-normal results)"""
    return f8.decode(codes) * np.repeat(scale_values(scales), BLOCK, axis=-1)


def _filter_hwio(w8, kh, kw):
    taps, co, ci = w8.shape
    return torch.from_numpy(f8.decode(w8)).permute(0, 2, 1).reshape(kh, kw, ci, co)


def conv_values(xv, w8, kh, kw, stride, dil, padding):
    """float64 convolution of dequantised activations xv [B,H,W,Ci] with the filter codes w8 [tap][Co][Ci] at unit filter scale.
    -> (acc [B,Ho,Wo,Co], absacc: the same sum over |x * w_code|)"""
    x = torch.from_numpy(np.asarray(xv, np.float64)).permute(0, 3, 1, 2)
    w = _filter_hwio(w8, kh, kw)
    if padding == 'BR1':
        x = F.pad(x, (0, 1, 0, 1))
        padding = 'VALID'
    acc = ref.conv2d_tf(x, w, stride, padding, dil).permute(0, 2, 3, 1).numpy()
    absacc = ref.conv2d_tf(x.abs(), w.abs(), stride, padding, dil).permute(0, 2, 3, 1).numpy()
    return acc, absacc


def conv_values_rows(xv, w8, k, dil, r0, r1):
    """conv_values for the output rows [r0, r1) of a stride-1 SAME layer (odd k)"""
    x = torch.from_numpy(np.asarray(xv, np.float64)).permute(0, 3, 1, 2)
    w = _filter_hwio(w8, k, k).permute(3, 2, 0, 1)
    p = dil * (k - 1) // 2
    x = F.pad(x, (p, p, p, p))[:, :, r0:r1 + 2 * p, :]
    acc = F.conv2d(x, w, None, 1, 0, dil).permute(0, 2, 3, 1).numpy()
    absacc = F.conv2d(x.abs(), w.abs(), None, 1, 0, dil).permute(0, 2, 3, 1).numpy()
    return acc, absacc


def epilogue(acc, s_w, bias, relu):
    """float64 y_ref = relu?(acc * s_w[co] + bias[co]): there is no input scale"""
    y = acc * np.asarray(s_w, np.float32).astype(np.float64) + (0.0 if bias is None else np.asarray(bias, np.float64))
    return np.maximum(y, 0.0) if relu else y


def accumulation_bound(absacc, K, s_w):
    """B = K * 2^-23 * s_w[co] * sum |x * w_code|: K fp32 additions at one ulp each (x = the dequantised activation)"""
    return K * 2.0 ** -23 * np.asarray(s_w, np.float32).astype(np.float64) * absacc


def maxpool(codes, scales, k, stride):
    """TF SAME max-pool of the dequantised tensor (cells outside the image never win), quantised again.  -> (codes, scales)"""
    x = torch.from_numpy(dequantize(codes, scales)).permute(0, 3, 1, 2)
    y = ref.maxpool_tf(x, k, stride).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    return quantize(y.astype(np.float32))
