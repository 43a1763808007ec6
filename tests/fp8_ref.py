"""numpy / torch-CPU oracle of the fp8 inference format: OCP e4m3fn codes, saturating round-to-nearest-even
quantisation at one scale per activation tensor and one per filter output channel, exact products, and the fp32 epilogue
y = relu?(acc * (s_in * s_w[co]) + bias[co]).  Everything the GPU tests compare against is computed here in float64 from the
same codes the kernels read."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ssdvgg_ref as ref

E4M3_MAX = 448.0
OUT_BF16, OUT_F32, OUT_E4M3, OUT_BF16_E4M3 = 0, 1, 2, 3


def _decode_table():
    t = np.zeros(256, np.float64)
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -v if s else v
    return t


DECODE = _decode_table()
_POS = DECODE[:0x7F]                       # the 127 non-negative finite values, ascending: 0 .. 448
_MID = (_POS[1:] + _POS[:-1]) / 2          # midpoints between neighbours (exact in float64)


def decode(codes):
    """uint8 codes -> float64 values (NaN for 0x7F / 0xFF)"""
    return DECODE[np.asarray(codes, np.uint8)]


def encode(v):
    """float values -> uint8 codes: clamp to +-448, then round to nearest, ties to the even code.  NaN -> 0x7F | sign."""
    v = np.asarray(v, np.float64)
    a = np.minimum(np.abs(v), E4M3_MAX)
    a0 = np.where(np.isnan(a), 0.0, a)
    lo = np.searchsorted(_MID, a0, side='left')       # first midpoint >= a: a lies in (mid[lo-1], mid[lo]]
    tie = (lo < len(_MID)) & (a0 == _MID[np.minimum(lo, len(_MID) - 1)])
    code = np.where(tie & (lo % 2 == 1), lo + 1, lo)   # at a midpoint between codes lo and lo + 1 take the even one
    code = np.where(np.isnan(a), 0x7F, code).astype(np.uint8)
    return (code | (np.signbit(v).astype(np.uint8) << 7)).astype(np.uint8)


def quantize(v, scale):
    """the contract's code = RNE(clamp(v / s, -448, 448)) with the division in fp32, as the kernels do it"""
    q = np.asarray(v, np.float32) / np.float32(scale)
    return encode(q)


def filter_scales(w_hwio):
    """fp32 s_w[co] = absmax_co / 448 (IEEE fp32 division), 1 for an all-zero channel"""
    w = np.asarray(w_hwio, np.float32)
    am = np.abs(w.reshape(-1, w.shape[-1])).max(0).astype(np.float32)
    return np.where(am > 0, am / np.float32(448.0), np.float32(1.0)).astype(np.float32)


def quantize_filter(w_hwio):
    """fp32 [kh][kw][Ci][Co] -> (codes [tap][Co][Ci] uint8, s_w [Co] fp32)"""
    w = np.asarray(w_hwio, np.float32)
    kh, kw, ci, co = w.shape
    s = filter_scales(w)
    codes = encode(w / s)                                     # fp32 division, per output channel
    return np.ascontiguousarray(np.transpose(codes.reshape(kh * kw, ci, co), (0, 2, 1))), s


def conv_codes(x8, w8, kh, kw, stride, dil, padding):
    """float64 convolution of the dequantised codes at unit scales.  x8 [B,H,W,Ci] uint8, w8 [tap][Co][Ci] uint8.
    -> (acc [B,Ho,Wo,Co] float64, absacc: the same sum over |x_code * w_code|)"""
    x = torch.from_numpy(decode(x8)).permute(0, 3, 1, 2)
    taps, co, ci = w8.shape
    w = torch.from_numpy(decode(w8)).permute(0, 2, 1).reshape(kh, kw, ci, co)      # HWIO
    if padding == 'BR1':
        x = F.pad(x, (0, 1, 0, 1))
        padding = 'VALID'
    acc = ref.conv2d_tf(x, w, stride, padding, dil).permute(0, 2, 3, 1).numpy()
    absacc = ref.conv2d_tf(x.abs(), w.abs(), stride, padding, dil).permute(0, 2, 3, 1).numpy()
    return acc, absacc


def epilogue(acc, s_in, s_w, bias, relu):
    """float64 y_ref = relu?(acc * (s_in * s_w[co]) + bias[co]); the product of the two scales is the kernel's fp32 one"""
    sc = (np.float32(s_in) * np.asarray(s_w, np.float32)).astype(np.float64)
    y = acc * sc + (0.0 if bias is None else np.asarray(bias, np.float64))
    return np.maximum(y, 0.0) if relu else y


def accumulation_bound(absacc, K, s_in, s_w):
    """B = K * 2^-23 * (s_in * s_w[co]) * sum |x_code * w_code|: K fp32 additions at one ulp each"""
    sc = (np.float32(s_in) * np.asarray(s_w, np.float32)).astype(np.float64)
    return K * 2.0 ** -23 * sc * absacc


def e4m3_step(a):
    """spacing of the e4m3 grid at magnitude a (float64 array): 2^-9 in the subnormal range, 2^(e-3) in binade e"""
    a = np.minimum(np.abs(a), E4M3_MAX)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -6)))
    return 2.0 ** (e - 3)


def maxpool_codes(x8, k, stride):
    """TF SAME max-pool of the decoded values, encoded again (exact: a maximum is one of its inputs).  x8 [B,H,W,C] uint8
    without NaN codes and without -0 (whose order against +0 the float maximum does not define)."""
    x = torch.from_numpy(decode(x8)).permute(0, 3, 1, 2)
    return encode(ref.maxpool_tf(x, k, stride).permute(0, 2, 3, 1).numpy())


def conv_codes_rows(x8, w8, k, dil, r0, r1):
    """conv_codes for the output rows [r0, r1) of a stride-1 SAME layer (odd k): the large maps of a whole model are checked
    on bands of rows, at the cost of those bands"""
    x = torch.from_numpy(decode(x8)).permute(0, 3, 1, 2)
    taps, co, ci = w8.shape
    w = torch.from_numpy(decode(w8)).permute(0, 2, 1).reshape(k, k, ci, co).permute(3, 2, 0, 1)
    p = dil * (k - 1) // 2
    x = F.pad(x, (p, p, p, p))[:, :, r0:r1 + 2 * p, :]
    acc = F.conv2d(x, w, None, 1, 0, dil).permute(0, 2, 3, 1).numpy()
    absacc = F.conv2d(x.abs(), w.abs(), None, 1, 0, dil).permute(0, 2, 3, 1).numpy()
    return acc, absacc
