"""-m gpu: the mxfp6 inference kernels and handle through the C ABI against tests/mxfp6_ref.py.

The quantisers and the pool are compared byte for byte, codes and scales.  The convolution is compared on data whose sums are exact in
fp32 in any order (a misplaced scale byte on either operand, a permuted 6-bit field or a misplaced tap shows as a wrong number), and on
real-valued layers against the float64 convolution of the dequantised operands with the bound B = K * 2^-23 * sum |x * w| (+ 2^-8 |y|
for a bf16 output); an MX6 output is compared byte for byte with the oracle's quantiser applied to the kernel's own fp32 output."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import mxfp6_ref as m6
from gpu_util import lib, check, dev, ptr, host, conv_geom, same_pad, rel_err
from ssd_tensorflow_amd._lib import last_error
from test_gpu_fp8 import layout_operands, layout_reference_input, REAL_CASES, FOUR_MODES_CASE, FP8_LAYERS, FP8_SCALED, FP8_POOLS, bf16_round, u8
from test_gpu_mxfp8 import LAYOUT_CASES, POOL_CASES, NO_SCALES, build

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ quantise
def gpu_quantize(v, x_f32):
    """v [rows, C] fp32 (bf16-representable where x_f32 is False) -> (bytes [rows, C/32, 24], scales [rows, C/32]) with 16 guard bytes
    behind each checked"""
    rows, cc = v.shape
    nb = v.size // 32
    x_ = dev(v) if x_f32 else dev(v).bfloat16()
    y_, s_ = u8((nb * 24 + 16,)), u8((nb + 16,))
    check(lib.ssd_op_quantize_mxfp6(ptr(x_), int(x_f32), rows, cc, ptr(y_), ptr(s_), None))
    y, s = host(y_), host(s_)
    assert np.all(y[nb * 24:] == 0xAB) and np.all(s[nb:] == 0xAB)
    return y[:nb * 24].reshape(rows, cc // 32, 24), s[:nb].reshape(rows, cc // 32)


@pytest.mark.parametrize('x_f32', [False, True], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('c', [32, 64, 96])
def test_quantize_bit_exact(x_f32, c):
    rng = np.random.default_rng(61 + c)
    rows = 300
    v = (rng.normal(0, 1, (rows, c)) * np.exp2(rng.integers(-100, 101, (rows, c // 32)).repeat(32, 1))).astype(np.float32)
    v[0] = 0                                                        # zero blocks
    v[1, :32] = rng.normal(0, 0.3, 32).clip(-1, 1); v[1, 3] = 7.5   # a maximum of exactly 7.5 * 2^k, k = 0, 5, -9
    v[2, :32] = rng.normal(0, 9, 32).clip(-200, 200); v[2, 31] = -7.5 * 32      # ... as a negative value
    v[3, :32] = rng.normal(0, 1e-4, 32); v[3, 0] = 7.5 / 512
    v[4, :32] = rng.normal(0, 0.5, 32).clip(-1.8, 1.8); v[4, 7] = 1.875                                     # mantissa 1.875 ...
    v[5, :32] = v[4, :32]; v[5, 7] = np.float32(1.8828125) if not x_f32 else np.nextafter(np.float32(1.875), np.float32(2))      # ... and the next value up
    v[6, :32] = -np.abs(rng.normal(0, 3, 32))                       # an all-negative block
    v[7, :32] = np.ldexp(rng.normal(0, 1, 32), 100); v[8, :32] = np.ldexp(rng.normal(0, 1, 32), -100)
    v[9, :32] = np.array([0.0625, 0.1875, 1.0625, 1.1875, 7.25, -0.0625, -7.25, 6.75] * 4); v[9, 0] = 7.5   # ties at scale 2^0
    if not x_f32:
        v = bf16_round(v)
    got6, gots = gpu_quantize(v, x_f32)
    want6, wants = m6.quantize(v)
    assert np.array_equal(gots, wants), np.argwhere(gots != wants)[:8]
    assert np.array_equal(got6, want6), np.argwhere(got6 != want6)[:8]
    assert gots[0, 0] == 0 and gots[1, 0] == 127 and gots[2, 0] == 132 and gots[3, 0] == 118 and gots[4, 0] == 125 and gots[5, 0] == 126
    codes = m6.unpack(got6)
    assert codes[1, 3] == 31 and codes[2, 31] == 63 and gots.max() < 255 and not got6[0].any()
    assert m6.decode(codes[9, 1:8]).tolist() == [0.25, 1.0, 1.25, 7.0, -0.0, -7.0, 7.0]
    assert np.abs(m6.decode(codes)).reshape(rows, c // 32, 32)[1:].max(-1).min() >= 3.75      # every block uses its range


def test_quantize_bit_exact_second_sweep():
    """the grid is capped at 8192 workgroups of 256 threads: n8 = 2 097 280 is 128 threads' work past one sweep of the grid-stride
    loop, where a block's four lanes must still loop together for the 24-byte store.  The last 1024 rows straddle the end of the
    first sweep at row 262 144."""
    rng = np.random.default_rng(98)
    rows, c = 262160, 64
    assert rows * c // 8 == 8192 * 256 + 128
    v = rng.standard_normal((rows, c), np.float32) * np.exp2(rng.integers(-20, 21, (rows, c // 32))).astype(np.float32).repeat(32, 1)
    got6, gots = gpu_quantize(v, True)
    for sl in (slice(0, 1024), slice(rows - 1024, rows)):
        want6, wants = m6.quantize(v[sl])
        assert np.array_equal(gots[sl], wants), np.argwhere(gots[sl] != wants)[:8]
        assert np.array_equal(got6[sl], want6), np.argwhere(got6[sl] != want6)[:8]


def test_quantize_refuses_c24():
    x_ = dev(np.ones((4, 24), np.float32))
    y_, s_ = u8((96,)), u8((8,))
    assert lib.ssd_op_quantize_mxfp6(ptr(x_), 1, 4, 24, ptr(y_), ptr(s_), None) != 0
    assert 'multiple of 32' in last_error()
    assert np.all(host(y_) == 0xAB) and np.all(host(s_) == 0xAB)


def gpu_quantize_filter(w):
    """fp32 HWIO -> (w6 [tap][Co][Ci/32][24], wscales [tap][Co][Ci/32]) device tensors, 16 guard bytes behind each"""
    kh, kw, ci, co = w.shape
    nb = kh * kw * co * (ci // 32)
    w6_, ws_ = u8((nb * 24 + 16,)), u8((nb + 16,))
    check(lib.ssd_op_quantize_filter_mxfp6(ptr(dev(w)), ptr(w6_), ptr(ws_), kh * kw, ci, co, None))
    assert np.all(host(w6_)[nb * 24:] == 0xAB) and np.all(host(ws_)[nb:] == 0xAB)
    return w6_[:nb * 24].view(kh * kw, co, ci // 32, 24), ws_[:nb].view(kh * kw, co, ci // 32)


@pytest.mark.parametrize('shape', [(3, 3, 64, 40), (1, 1, 128, 8)], ids=['3x3x64x40', '1x1x128x8'])
def test_quantize_filter_bit_exact(shape):
    rng = np.random.default_rng(11 + shape[3])
    w = (rng.normal(0, 1, shape) / 24).astype(np.float32)
    w[:, :, :32, 5] = 0                               # all-zero blocks: byte 0, codes 0
    w[0, 0, 33, 7] = -3.0                             # a block whose absmax is a negative value
    w6_, ws_ = gpu_quantize_filter(w)
    want6, wants = m6.quantize_filter(w)
    assert np.array_equal(host(ws_), wants), np.argwhere(host(ws_) != wants)[:4]
    assert np.array_equal(host(w6_), want6), np.argwhere(host(w6_) != want6)[:4]
    assert np.all(host(ws_)[:, 5, 0] == 0) and host(ws_)[0, 7, 1] == 126 and m6.unpack(host(w6_))[0, 7, 33] == 32 + 28      # -3 = -6 * 2^-1


# ------------------------------------------------------------------------------------------------------------ convolution
def run_conv(x6, xs, w6, ws, bias, geom, mode, relu):
    """-> (y: fp32 numpy of the bf16 / fp32 output or None, y6, ys: uint8 numpy or None)"""
    b, hi, wi, ci, ho, wo, co = geom[:7]
    x_, xs_, w_, ws_ = (t if torch.is_tensor(t) else dev(t) for t in (x6, xs, w6, ws))
    wants6 = mode in (m6.OUT_MX, m6.OUT_BF16_MX)
    y_ = None if mode == m6.OUT_MX else torch.full((b, ho, wo, co), 9.0, dtype=torch.float32 if mode == m6.OUT_F32 else torch.bfloat16, device='cuda')
    y6_ = u8((b, ho, wo, co // 32, 24)) if wants6 else None
    ys_ = u8((b, ho, wo, co // 32)) if wants6 else None
    check(lib.ssd_op_conv2d_fwd_mxfp6(ptr(x_), ptr(xs_), ptr(w_), ptr(ws_), ptr(dev(bias)), ptr(y_), ptr(y6_), ptr(ys_), mode, *geom, int(relu), None))
    torch.cuda.synchronize()
    return (None if y_ is None else y_.float().cpu().numpy()), (y6_.cpu().numpy() if wants6 else None), (ys_.cpu().numpy() if wants6 else None)


@pytest.mark.parametrize('tile', ['0', '1'], ids=['128x128', '64x64'])
@pytest.mark.parametrize('case', LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_conv_layout_exact(case, tile, monkeypatch):
    """activations i * 2^s with i in 0 ... 7 and s in -2 ... 2 varying with pixel and block, filter values j * 2^t with j in -3 ... 3 and
    t in -2 ... 1 varying with tap, output channel and input block, asymmetric in pixel, channel, tap and output channel: every product is
    a multiple of 2^-4 and every sum of magnitudes stays below 2^20, exact in fp32 in any order"""
    monkeypatch.setenv('SSD_TILE_FP8', tile)
    name, b, hi, wi, ci, co, kh, kw, stride, dil, padding = case
    iv, _, bias, geom = layout_operands(case)
    B, H, W, Cc = np.meshgrid(np.arange(b), np.arange(hi), np.arange(wi), np.arange(ci), indexing='ij')
    sv = (2 * B + 3 * H + W + 2 * (Cc // 32) + (H * (Cc // 32)) % 3) % 5 - 2
    xv = np.ldexp(iv.astype(np.float32), sv).astype(np.float32)
    KH, KW, CI, CO = np.meshgrid(np.arange(kh), np.arange(kw), np.arange(ci), np.arange(co), indexing='ij')
    jv = (2 * KH + 3 * KW + CI + 7 * CO + (CI * CO) % 3 + (KH * CI) % 2 + (CI // 32)) % 7 - 3
    tv = (KH * kw + KW + 2 * CO + 3 * (CI // 32) + (CO * (CI // 32)) % 3) % 4 - 2
    wv = np.ldexp(jv.astype(np.float32), tv).astype(np.float32)
    x6, xs = m6.quantize(xv)
    w6, ws = m6.quantize_filter(wv)
    assert np.array_equal(m6.dequantize(x6, xs), xv.astype(np.float64)) and len(np.unique(xs)) >= 5      # lossless; scales vary
    assert np.array_equal(m6.dequantize_filter(w6, ws, kh, kw), wv.astype(np.float64)) and len(np.unique(ws)) >= 4
    xv_ref, padding_ref = layout_reference_input(xv, case)
    acc, absacc = m6.conv_values(xv_ref, wv, stride, dil, padding_ref)
    want = acc + bias
    assert want.shape == (geom[0], geom[4], geom[5], co)
    assert absacc.max() + 8 < 2 ** 20 and np.array_equal(want * 16, np.round(want * 16)) and len(np.unique(want)) > 50
    y, _, _ = run_conv(x6, xs, w6, ws, bias, geom, m6.OUT_F32, False)
    assert np.array_equal(y, want.astype(np.float32)), f'{name}: {np.argwhere(y != want)[:4]}'
    pos = np.maximum(want, 0).astype(np.float32)
    if co % 32:
        y, _, _ = run_conv(x6, xs, w6, ws, bias, geom, m6.OUT_BF16, True)
        assert np.array_equal(y, bf16_round(pos))
        return
    y, y6, ys = run_conv(x6, xs, w6, ws, bias, geom, m6.OUT_BF16_MX, True)
    assert np.array_equal(y, bf16_round(pos))
    want6, wants = m6.quantize(pos)
    assert np.array_equal(ys, wants) and np.array_equal(y6, want6)


def check_real_layer(name, xv, x6, xs, w6, ws, bias, geom, k, stride, dil, padding, relu, mx_out):
    """one layer from given MX6 operands: fp32 and bf16 out within the bound; -> largest fp32-out error / B"""
    K = k * k * geom[3]
    acc, absacc = m6.conv_values(xv, m6.dequantize_filter(host(w6), host(ws), k, k), stride, dil, padding)
    y_ref = m6.epilogue(acc, bias, relu)
    Bd = m6.accumulation_bound(absacc, K)
    y32, _, _ = run_conv(x6, xs, w6, ws, bias, geom, m6.OUT_F32, relu)
    err = np.abs(y32 - y_ref)
    worst = float((err / np.maximum(Bd, 1e-300))[Bd > 0].max())
    print(f'\n[mxfp6 conv] {name}: largest fp32-out error / B = {worst:.4f}')
    assert np.all(err <= Bd), f'{name} fp32 out: max (err - bound) {float((err - Bd).max()):.3e}'
    y16, _, _ = run_conv(x6, xs, w6, ws, bias, geom, m6.OUT_BF16, relu)
    lim = Bd + np.abs(y_ref) * 2.0 ** -8
    assert np.all(np.abs(y16 - y_ref) <= lim), f'{name} bf16 out: max (err - bound) {float((np.abs(y16 - y_ref) - lim).max()):.3e}'
    if mx_out:
        # the epilogue is deterministic: the MX6 bytes are the oracle's quantiser applied to the kernel's OWN fp32 output, byte for byte
        want6, wants = m6.quantize(y32)
        _, y6, ys = run_conv(x6, xs, w6, ws, bias, geom, m6.OUT_MX, relu)
        assert np.array_equal(ys, wants), np.argwhere(ys != wants)[:4]
        assert np.array_equal(y6, want6), np.argwhere(y6 != want6)[:4]
        y16b, y6, ys = run_conv(x6, xs, w6, ws, bias, geom, m6.OUT_BF16_MX, relu)
        assert np.array_equal(ys, wants) and np.array_equal(y6, want6) and np.array_equal(y16b, y16)
    return worst


REAL6 = [c for c in REAL_CASES if c[6] * c[6] <= 9 and c[4] % 64 == 0]


@pytest.mark.parametrize('case', REAL6, ids=[c[0] for c in REAL6])
def test_conv_real_valued(case, capsys):
    name, b, hi, wi, ci, co, k, stride, dil, padding, relu, _ = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ph, pw, ho, wo = conv_geom(hi, wi, k, stride, dil, padding)
    x = (rng.normal(0, 1, (b, hi, wi, ci)) * np.exp2(rng.integers(-3, 4, (b, hi, wi, ci // 32)).repeat(32, -1))).astype(np.float32)
    w = (rng.normal(0, 1, (k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.normal(0, 0.1, (co,)).astype(np.float32)
    x6, xs = gpu_quantize(x.reshape(-1, ci), True)                # (bytes pinned by test_quantize_bit_exact)
    x6, xs = x6.reshape(b, hi, wi, ci // 32, 24), xs.reshape(b, hi, wi, ci // 32)
    w6_, ws_ = gpu_quantize_filter(w)                             # (... by test_quantize_filter_bit_exact)
    geom = (b, hi, wi, ci, ho, wo, co, k, k, stride, dil, ph, pw)
    with capsys.disabled():
        check_real_layer(name, m6.dequantize(x6, xs), x6, xs, w6_, ws_, bias, geom, k, stride, dil, padding, relu, name == FOUR_MODES_CASE)


@pytest.mark.parametrize('what', ['Ci=96', '25 taps', 'Co=20', 'MX out Co=40'])
def test_conv_refused_shapes_write_nothing(what):
    ci, co, k = (96, 64, 3) if what == 'Ci=96' else (64, 64, 5) if what == '25 taps' else (64, 20, 3) if what == 'Co=20' else (64, 40, 3)
    mode = m6.OUT_BF16_MX if what == 'MX out Co=40' else m6.OUT_F32
    b, hi, wi = 1, 6, 6
    ph, pw, ho, wo = conv_geom(hi, wi, k, 1, 1, 'SAME')
    x6_, xs_ = u8((b, hi, wi, ci // 32, 24), 0x38), u8((b, hi, wi, ci // 32), 0x7F)
    w6_, ws_ = u8((k * k, co, ci // 32, 24), 0x38), u8((k * k, co, ci // 32), 0x7F)
    y_ = torch.full((b, ho, wo, co), 9.0, dtype=torch.float32, device='cuda')
    y6_, ys_ = u8((b, ho, wo, co // 32 + 1, 24)), u8((b, ho, wo, co // 32 + 1))
    rc = lib.ssd_op_conv2d_fwd_mxfp6(ptr(x6_), ptr(xs_), ptr(w6_), ptr(ws_), None, ptr(y_), ptr(y6_), ptr(ys_), mode,
                                     b, hi, wi, ci, ho, wo, co, k, k, 1, 1, ph, pw, 1, None)
    assert rc != 0 and 'mxfp6 conv' in last_error()
    assert np.all(host(y_) == 9.0) and np.all(host(y6_) == 0xAB) and np.all(host(ys_) == 0xAB)


# ------------------------------------------------------------------------------------------------------------ pooling
def gpu_pool(x6, xs, k, stride):
    b, hi, wi, cb = xs.shape
    ph, ho = same_pad(hi, k, stride)
    pw, wo = same_pad(wi, k, stride)
    x6_, xs_, y6_, ys_ = dev(x6), dev(xs), u8((b, ho, wo, cb, 24)), u8((b, ho, wo, cb))
    check(lib.ssd_op_maxpool_fwd_mxfp6(ptr(x6_), ptr(xs_), ptr(y6_), ptr(ys_), b, hi, wi, cb * 32, ho, wo, k, stride, ph, pw, None))
    return host(y6_), host(ys_)


@pytest.mark.parametrize('c', [32, 64])
@pytest.mark.parametrize('case', POOL_CASES, ids=[p[0] for p in POOL_CASES])
def test_maxpool_bytes(case, c):
    name, b, hi, wi, k, stride = case
    rng = np.random.default_rng(zlib.crc32(name.encode()) + c)
    ok = np.array([v for v in range(64) if v != 32], np.uint8)                            # (-0 against +0 has no defined maximum)
    codes = rng.choice(ok, size=(b, hi, wi, c))
    xs = rng.integers(121, 134, (b, hi, wi, c // 32)).astype(np.uint8)                    # 2^-6 ... 2^6
    codes[0, :3, :3, :] = rng.choice(np.arange(33, 64, dtype=np.uint8), size=(3, 3, c))   # windows that are all negative
    # a window (2x2: rows 2..3, columns 2..3 = output (1, 1); 3x3 s1: around (4, 4)) whose maximum comes from the cell with the smallest scale
    r = 2 if k == 2 else 3
    codes[0, r:r + k, r:r + k, :] = 1; xs[0, r:r + k, r:r + k, :] = 123                   # 0.125 * 2^-4 each
    codes[0, r + 1, r + 1, :] = 30; codes[0, r + 1, r + 1, 0] = 31; xs[0, r + 1, r + 1, :] = 121      # 7 (channel 0: 7.5) * 2^-6, the smallest scale
    x6 = m6.pack(codes)
    y6, ys = gpu_pool(x6, xs, k, stride)
    want6, wants = m6.maxpool(x6, xs, k, stride)
    assert want6.shape == y6.shape and wants.shape == ys.shape
    assert np.array_equal(ys, wants), np.argwhere(ys != wants)[:4]
    assert np.array_equal(y6, want6), np.argwhere(y6 != want6)[:4]
    o = (r + 1) // stride
    got = m6.dequantize(y6, ys)
    assert got[0, o, o, 0] == 7.5 / 64 and np.all(got[0, o, o, 1:] == 7.0 / 64) and np.all(got[0, 0, 0] < 0)
    if c == 32:
        ph, ho = same_pad(hi, k, stride)
        pw, wo = same_pad(wi, k, stride)
        bad_, xs_, y6_, ys_ = u8((b, hi, wi, 12), 0x38), dev(xs), u8((b, ho, wo, 24)), u8((b, ho, wo, 1))
        assert lib.ssd_op_maxpool_fwd_mxfp6(ptr(bad_), ptr(xs_), ptr(y6_), ptr(ys_), b, hi, wi, 16, ho, wo, k, stride, ph, pw, None) != 0
        assert 'multiple of 32' in last_error() and np.all(host(y6_) == 0xAB) and np.all(host(ys_) == 0xAB)


# ------------------------------------------------------------------------------------------------------------ whole model
MX_TENSORS = FP8_SCALED + FP8_POOLS      # the tensors kept as codes + scales: conv3_1 (quantised behind the bf16 layer) ... mod_conv6, the pools


@pytest.fixture(scope='module')
def model():
    from oracle import boxes as ob, ssdvgg_ref as ref
    from ssd_tensorflow_amd.ssdvgg import Session
    preset = ob.get_preset('vgg300')
    w = ref.init_params(preset, 20, seed=42, alive=True)
    b = 2
    x = ref.synth_images(np.random.default_rng(99), b, preset)
    sess = Session(0)
    nets = {dt: build(sess, 'vgg300', w, b, dt) for dt in ('mxfp6', 'mxfp8', 'bf16', 'f32')}
    assert nets['mxfp6'].dtype == 'mxfp6'
    res = {dt: nets[dt].infer(x) for dt in ('mxfp6', 'mxfp8', 'bf16', 'f32')}      # (mxfp6 straight after creation: nothing to calibrate)
    yield dict(preset=preset, w=w, b=b, x=x, nets=nets, res=res, ref=ref, sess=sess)
    sess.close()


def mx_codes(net, name, b):
    """(dequantised fp32, unpacked codes, scale bytes) of an MX6 tensor of the handle"""
    a, s = net.activation(name, b), net.activation('scale:' + name, b)
    m, e = np.frexp(s)
    assert np.all(m == 0.5) and s.shape == a.shape[:-1] + (a.shape[-1] // 32,), f'{name}: a block scale is no power of two'
    sb = (e - 1 + 127).astype(np.uint8)
    codes = m6.encode(a.astype(np.float64) / np.repeat(s.astype(np.float64), 32, -1))
    assert np.array_equal(m6.decode(codes) * np.repeat(m6.scale_values(sb), 32, -1), a.astype(np.float64))
    return a, codes, sb


def check_scales_follow_rule(name, a, codes, sb):
    """the scale is the rule applied to the dequantised block's absmax, except where that absmax was rounded down to 3.75 of its scale
    (= 7.5 * 2^(x - 1), for which the rule gives x - 1)"""
    blk = np.abs(a).reshape(a.shape[:-1] + (a.shape[-1] // 32, 32)).max(-1)
    again = (m6.scale_exponent(blk) + 127).astype(np.uint8)
    top = np.abs(m6.decode(codes)).reshape(blk.shape + (32,)).max(-1)
    assert np.all((again == sb) | ((top == 3.75) & (again == sb - 1)) | ((blk == 0) & (sb == 0))), f'{name}: {np.argwhere(again != sb)[:4]}'
    assert np.all(top[blk > 0] >= 3.75) and sb.max() < 255


def test_model_mx6_layers_local(model, capsys):
    """every MX6 layer's output against the oracle applied to the kernel's OWN dequantised input, with the bound of the op test.  Maps
    higher than 40 rows are checked on three bands of rows (top border, middle, bottom border, every column and channel)."""
    ref, b, w, net = model['ref'], model['b'], model['w'], model['nets']['mxfp6']
    ops = {op[1]: op for op in ref.graph(model['preset']) if op[0] in ('conv', 'pool')}
    lines = []
    for name in FP8_LAYERS:
        _, _, src, k, stride, padding, dil = ops[name]
        assert stride == 1 and padding == 'SAME'
        xv, _, _ = mx_codes(net, src, b)
        wv = m6.dequantize_filter(*m6.quantize_filter(w[name + '/filter']), k, k)
        bias = w[name + '/biases']
        H = xv.shape[1]
        bands = [(0, 5), (H // 2, H // 2 + 3), (H - 5, H)] if H > 40 else [(0, H)]
        got6 = mx_codes(net, name, b) if name != 'mod_conv7' else None
        got16 = net.activation(('bf16:' if got6 is not None else '') + name, b) if name in ('conv4_3', 'mod_conv7') else None
        if got6 is not None:
            check_scales_follow_rule(name, *got6)
        worst6 = worst16 = 0.0
        for r0, r1 in bands:
            acc, absacc = m6.conv_values_rows(xv, wv, dil, r0, r1)
            y_ref = m6.epilogue(acc, bias, True)
            Bd = m6.accumulation_bound(absacc, k * k * xv.shape[3])
            assert np.count_nonzero(y_ref) > 0.2 * y_ref.size, f'{name} is (nearly) dead: the test would prove nothing'
            if got6 is not None:
                a, codes, sb = (t[:, r0:r1] for t in got6)
                sv = np.repeat(m6.scale_values(sb), 32, -1)
                err = np.abs(a - y_ref)
                lim = Bd + sv * m6.e2m3_step(y_ref / sv) / 2          # one e2m3 rounding at the block's scale
                assert np.all(err <= lim), f'{name} rows {r0}:{r1}: MX6 output off by {float((err - lim).max()):.3e}'
                worst6 = max(worst6, float((err / np.maximum(lim, 1e-300)).max()))
            if got16 is not None:
                err = np.abs(got16[:, r0:r1] - y_ref)
                lim = Bd + np.abs(y_ref) * 2.0 ** -8
                assert np.all(err <= lim), f'{name} rows {r0}:{r1}: bf16 output off by {float((err - lim).max()):.3e}'
                worst16 = max(worst16, float((err / np.maximum(lim, 1e-300)).max()))
        lines.append(f'{name}: worst error / bound: MX6 out {worst6:.3f}, bf16 out {worst16:.3f} (0: no such output)')
    with capsys.disabled():
        print('\n[mxfp6 model] ' + '\n[mxfp6 model] '.join(lines))


def test_model_mx6_boundaries_and_pools(model):
    ref, b, nets = model['ref'], model['b'], model['nets']
    net = nets['mxfp6']
    # conv3_1: the bf16 handle's kernels up to here, then the one stand-alone quantise pass
    c31 = net.activation('bf16:conv3_1', b)
    assert np.array_equal(c31, nets['bf16'].activation('conv3_1', b))
    a, codes, sb = mx_codes(net, 'conv3_1', b)
    wantc, wants = m6.quantize_codes(c31)
    assert np.array_equal(sb, wants) and np.array_equal(codes & 31, wantc & 31)      # (a zero's sign is not visible in the dequantised tensor)
    assert np.array_equal(m6.decode(codes), m6.decode(wantc))
    # the pools: the maximum of the dequantised cells, quantised again
    ops = {op[1]: op for op in ref.graph(model['preset']) if op[0] == 'pool'}
    for name in FP8_POOLS:
        _, _, src, k, s = ops[name]
        _, c_in, s_in = mx_codes(net, src, b)
        _, c_out, s_out = mx_codes(net, name, b)
        want6, wants = m6.maxpool(m6.pack(c_in), s_in, k, s)
        assert np.array_equal(s_out, wants) and np.array_equal(m6.decode(c_out), m6.decode(m6.unpack(want6))), name
    with pytest.raises(RuntimeError, match='no bf16 form'):
        net.activation('bf16:conv3_2', b)
    with pytest.raises(RuntimeError, match='no block scales'):
        net.activation('scale:mod_conv7', b)


def test_model_mx6_untouched_layers_and_result(model, capsys):
    """conv8_1 onwards, the l2 norm and the heads are the bf16 handle's code: each against the bf16 oracle applied to the tensor it
    actually read; then the result, and its distance to fp32 against the mxfp8 handle's in the same run"""
    from test_gpu_bf16 import layer_local_forward_check, TOL_BF
    ref, b, nets, res = model['ref'], model['b'], model['nets'], model['res']
    net = nets['mxfp6']

    class Bf16View:
        def activation(self, name, n):
            return net.activation(('bf16:' if name in MX_TENSORS else '') + name, n)

    m = ref.RefModel('vgg300', params=model['w'])
    only = [op[1] for op in ref.graph(model['preset']) if op[0] == 'conv' and op[1] not in FP8_LAYERS + ['conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1']]
    only += ['l2_norm_conv4_3'] + ['heads/map%d' % i for i in range(6)]
    assert 'conv8_1' in only and 'conv11_2' in only
    assert layer_local_forward_check(Bf16View(), m, model['preset'], b, model['x'], only=only) < TOL_BF
    rm = res['mxfp6']
    assert np.isfinite(rm).all() and np.abs(rm[..., :21].sum(-1) - 1).max() < 1e-4
    d = {dt: rel_err(res[dt], res['f32']) for dt in ('mxfp6', 'mxfp8', 'bf16')}
    with capsys.disabled():
        print(f"\n[mxfp6 model] rel_err(result, result fp32): mxfp6 {d['mxfp6']:.4e}, mxfp8 {d['mxfp8']:.4e}, bf16 {d['bf16']:.4e}")
    # a CPU emulation of both formats on this fixture gives a ratio of 1.02; a layout or scale bug gives O(1): the factor 2 is a cap
    assert d['mxfp6'] <= 2 * d['mxfp8']


def test_model_no_state(model):
    nets, x, b = model['nets'], model['x'], model['b']
    net = nets['mxfp6']
    dark = np.floor(x / 8).astype(np.float32)
    # the result for x does not depend on what was inferred before, nor on the rest of the batch
    r0 = net.infer(x)
    assert np.array_equal(r0, model['res']['mxfp6'])
    net.infer(dark)
    assert np.array_equal(net.infer(x), r0)
    other = np.stack([dark[1], x[1]])
    assert np.array_equal(net.infer(other)[1], r0[1])
    assert not np.array_equal(net.infer(other)[0], r0[0])


def test_lifecycle(model):
    net, x, b, w = model['nets']['mxfp6'], model['x'], model['b'], model['w']
    # nothing to calibrate, and the calls say so
    n = C.c_int(-1)
    buf = C.create_string_buffer(64)
    one = np.ones(16, np.float32)
    xd = torch.from_numpy(x).cuda()
    for call in (lambda: lib.ssd_fp8_num_scales(net._h, C.byref(n)), lambda: lib.ssd_fp8_scale_name(net._h, 0, buf, 64),
                 lambda: lib.ssd_fp8_get_scales(net._h, one.ctypes.data, 16), lambda: lib.ssd_fp8_set_scales(net._h, one.ctypes.data, 16),
                 lambda: lib.ssd_fp8_calibrate_dev(net._h, xd.data_ptr(), b, 0)):
        assert call() != 0 and NO_SCALES in last_error()
    with pytest.raises(RuntimeError, match=NO_SCALES):
        net.calibrate_fp8(x)
    with pytest.raises(RuntimeError, match=NO_SCALES):
        net.fp8_scales
    with pytest.raises(RuntimeError, match=NO_SCALES):
        net.fp8_scales = {'conv3_1': 1.0}
    d = C.c_int(-1)
    check(lib.ssd_get_dtype(net._h, C.byref(d)))
    assert d.value == 4
    # the e2m3 filters follow the fp32 masters: mod_conv7's filter and bias times 4 -> its (relu) output times 4, exactly up to the bf16
    # output's range (a power of two moves the block scales alone; a stale filter would leave a distance of 3/4)
    r0 = net.infer(x)
    y0 = net.activation('mod_conv7', b)
    net.load_variables({'mod_conv7/filter': w['mod_conv7/filter'] * 4, 'mod_conv7/biases': w['mod_conv7/biases'] * 4})
    net.infer(x)
    y1 = net.activation('mod_conv7', b)
    assert np.count_nonzero(y0) > 0.2 * y0.size and rel_err(y1, 4 * y0) < 2.0 ** -6
    net.load_variables({'mod_conv7/filter': w['mod_conv7/filter'], 'mod_conv7/biases': w['mod_conv7/biases']})
    assert np.array_equal(net.infer(x), r0)


def test_vgg512_batch1(model, capsys):
    from oracle import boxes as ob
    ref = model['ref']
    preset = ob.get_preset('vgg512')
    w = ref.init_params(preset, 20, seed=42, alive=True)
    x = ref.synth_images(np.random.default_rng(5), 1, preset)
    r = {dt: build(model['sess'], 'vgg512', w, 1, dt).infer(x) for dt in ('mxfp6', 'bf16')}
    assert np.isfinite(r['mxfp6']).all() and np.abs(r['mxfp6'][..., :21].sum(-1) - 1).max() < 1e-4
    with capsys.disabled():
        print(f"\n[mxfp6 model] vgg512 batch 1: rel_err(result mxfp6, result bf16) = {rel_err(r['mxfp6'], r['bf16']):.4e}")


def test_fc_graph_batch1(model, capsys):
    """the fc graph: fc6 (7x7) stays on the bf16 kernel with the quantise pass behind it; fc7 (1x1, 4096 -> 4096) runs on MX6 operands"""
    import fc_ref
    from test_gpu_fp8_bigk import CHECKED
    ref = model['ref']
    w = fc_ref.init_params(model['preset'], 20, seed=42)
    x = ref.synth_images(np.random.default_rng(99), 1, model['preset'])
    net = build(model['sess'], 'vgg300', w, 1, 'mxfp6', a_trous=False)
    r = net.infer(x)
    assert np.isfinite(r).all() and np.abs(r[..., :21].sum(-1) - 1).max() < 1e-4
    # fc6 on bf16: its bf16 form exists, conv5_3 / mod_pool5 in front of it are bf16 only, and its MX6 form is the quantiser's
    a16 = net.activation('bf16:mod_conv6', 1)
    with pytest.raises(RuntimeError, match='no block scales'):
        net.activation('scale:mod_pool5', 1)
    xv, codes, sb = mx_codes(net, 'mod_conv6', 1)
    wantc, wants = m6.quantize_codes(a16)
    assert np.array_equal(sb, wants) and np.array_equal(m6.decode(codes), m6.decode(wantc))
    # fc7 locally, on the output channels CHECKED (the filter's blocks run along Ci: a subset of output channels is exact)
    wv = m6.dequantize_filter(*m6.quantize_filter(w['fc7/weights'][..., CHECKED]), 1, 1)
    acc, absacc = m6.conv_values(xv, wv, 1, 1, 'SAME')
    y_ref = m6.epilogue(acc, w['fc7/biases'][CHECKED], True)
    Bd = m6.accumulation_bound(absacc, xv.shape[3])
    assert np.count_nonzero(y_ref) > 0.2 * y_ref.size
    err = np.abs(net.activation('mod_conv7', 1)[..., CHECKED] - y_ref)
    lim = Bd + np.abs(y_ref) * 2.0 ** -8
    assert np.all(err <= lim), f'mod_conv7: bf16 output off by {float((err - lim).max()):.3e}'
    with capsys.disabled():
        print(f'\n[mxfp6 fc model] mod_conv7: worst error / bound {float((err / np.maximum(lim, 1e-300)).max()):.3f}')


def test_detect_tool_mxfp6_child_process(tmp_path):
    """detect.py --dtype mxfp6 on three small images, twice with the files in opposite order: the same detections per image, with
    nothing calibrated and nothing stored; --fp8-calibration is an argument error"""
    import os, subprocess, sys
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model_file = str(tmp_path / 'model.npz')
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 3, max_batch=2)
        net.build_optimizer()
        net.save_checkpoint(model_file, class_names=['class_%d' % i for i in range(3)])
    rng = np.random.default_rng(9)
    files = []
    for k, (h, w_) in enumerate([(300, 300), (240, 352), (100, 90)]):
        files.append(str(tmp_path / ('img%d.npy' % k)))
        np.save(files[-1], rng.integers(0, 256, (h, w_, 3)).astype(np.uint8))
    cmd = [sys.executable, '-m', 'ssd_tensorflow_amd.detect', '--model', model_file, '--batch-size', '2', '--dtype', 'mxfp6']
    outs = []
    for run, order in enumerate((files, files[::-1])):
        odir = str(tmp_path / ('out%d' % run))
        r = subprocess.run(cmd + ['--output-dir', odir] + order, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert 'fp8 scales' not in r.stdout
        outs.append([open(os.path.join(odir, os.path.basename(f) + '.txt')).read() for f in files])
    assert outs[0] == outs[1] and any(len(t) for t in outs[0])
    r = subprocess.run(cmd + ['--output-dir', str(tmp_path / 'out2'), '--fp8-calibration', str(tmp_path / 's.npz')] + files, cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and NO_SCALES in r.stderr and not os.path.exists(str(tmp_path / 's.npz'))
