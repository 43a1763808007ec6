"""-m gpu: the mxfp8 inference kernels and handle through the C ABI against tests/mxfp8_ref.py.

The quantiser and the pool are compared byte for byte, codes and scales.  The convolution is compared on data whose sums are exact in
fp32 in any order (a misplaced scale byte, a permuted k or a misplaced tap shows as a wrong number), and on real-valued layers against
the float64 convolution of the dequantised activations with the bound B = K * 2^-23 * s_w[co] * sum |x * w_code| (+ 2^-8 |y| for a
bf16 output); an MX output is compared byte for byte with the oracle's quantiser applied to the kernel's own fp32 output."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import fp8_ref as f8
import mxfp8_ref as mx
from gpu_util import lib, check, dev, ptr, host, conv_geom, same_pad, rel_err
from ssd_tensorflow_amd._lib import last_error
from test_gpu_fp8 import LAYOUT_CASES as FP8_LAYOUT_CASES, layout_operands, layout_reference_input, REAL_CASES, FOUR_MODES_CASE, FP8_LAYERS, FP8_SCALED, FP8_POOLS, bf16_round, u8, gpu_quantize_filter

pytestmark = pytest.mark.gpu

NO_SCALES = 'no calibration scales'


# ------------------------------------------------------------------------------------------------------------ quantise
def gpu_quantize(v, x_f32, c=None):
    """v [rows, C] fp32 (bf16-representable where x_f32 is False) -> (codes, scales) with 16 guard bytes behind each checked"""
    rows, cc = v.shape
    x_ = dev(v) if x_f32 else dev(v).bfloat16()
    y_, s_ = u8((v.size + 16,)), u8((v.size // 32 + 16,))
    check(lib.ssd_op_quantize_mxfp8(ptr(x_), int(x_f32), rows, cc, ptr(y_), ptr(s_), None))
    y, s = host(y_), host(s_)
    assert np.all(y[v.size:] == 0xAB) and np.all(s[v.size // 32:] == 0xAB)
    return y[:v.size].reshape(rows, cc), s[:v.size // 32].reshape(rows, cc // 32)


@pytest.mark.parametrize('x_f32', [False, True], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('c', [32, 64, 96])
def test_quantize_bit_exact(x_f32, c):
    rng = np.random.default_rng(31 + c)
    rows = 300
    v = (rng.normal(0, 1, (rows, c)) * np.exp2(rng.integers(-100, 101, (rows, c // 32)).repeat(32, 1))).astype(np.float32)
    v[0] = 0                                                        # zero blocks
    v[1, :32] = rng.normal(0, 0.3, 32); v[1, 3] = 448.0             # a maximum of exactly 448 * 2^k, k = 0, 5, -9
    v[2, :32] = rng.normal(0, 9, 32); v[2, 31] = -448.0 * 32        # ... as a negative value
    v[3, :32] = rng.normal(0, 1e-4, 32); v[3, 0] = 448.0 / 512
    v[4, :32] = rng.normal(0, 0.5, 32).clip(-1.7, 1.7); v[4, 7] = 1.75                                      # mantissa 1.75 ...
    v[5, :32] = v[4, :32]; v[5, 7] = np.float32(1.7578125) if not x_f32 else np.nextafter(np.float32(1.75), np.float32(2))      # ... and the next value up
    v[6, :32] = -np.abs(rng.normal(0, 3, 32))                       # an all-negative block
    v[7, :32] = np.ldexp(rng.normal(0, 1, 32), 100); v[8, :32] = np.ldexp(rng.normal(0, 1, 32), -100)
    if not x_f32:
        v = bf16_round(v)
    got8, gots = gpu_quantize(v, x_f32)
    want8, wants = mx.quantize(v)
    assert np.array_equal(gots, wants), np.argwhere(gots != wants)[:8]
    assert np.array_equal(got8, want8), np.argwhere(got8 != want8)[:8]
    assert gots[0, 0] == 0 and gots[1, 0] == 127 and gots[2, 0] == 132 and gots[3, 0] == 118 and gots[4, 0] == 119 and gots[5, 0] == 120
    assert got8[1, 3] == 0x7E and got8[2, 31] == 0xFE and gots.max() < 255
    assert f8.decode(got8).reshape(rows, c // 32, 32)[1:].__abs__().max(-1).min() >= 224.0      # every block uses its range


def test_quantize_bit_exact_second_sweep():
    """the grid is capped at 8192 workgroups of 256 threads: n8 = 2 097 280 is 128 threads' work past one sweep of the grid-stride
    loop.  The last 1024 rows straddle the end of the first sweep at row 262 144."""
    rng = np.random.default_rng(97)
    rows, c = 262160, 64
    assert rows * c // 8 == 8192 * 256 + 128
    v = rng.standard_normal((rows, c), np.float32) * np.exp2(rng.integers(-20, 21, (rows, c // 32))).astype(np.float32).repeat(32, 1)
    got8, gots = gpu_quantize(v, True)
    for sl in (slice(0, 1024), slice(rows - 1024, rows)):
        want8, wants = mx.quantize(v[sl])
        assert np.array_equal(gots[sl], wants), np.argwhere(gots[sl] != wants)[:8]
        assert np.array_equal(got8[sl], want8), np.argwhere(got8[sl] != want8)[:8]


def test_quantize_refuses_c24():
    x_ = dev(np.ones((4, 24), np.float32))
    y_, s_ = u8((96,)), u8((8,))
    assert lib.ssd_op_quantize_mxfp8(ptr(x_), 1, 4, 24, ptr(y_), ptr(s_), None) != 0
    assert 'multiple of 32' in last_error()
    assert np.all(host(y_) == 0xAB) and np.all(host(s_) == 0xAB)


# ------------------------------------------------------------------------------------------------------------ convolution
def run_conv(x8, xs, w8, s_w, bias, geom, mode, relu):
    """-> (y: fp32 numpy of the bf16 / fp32 output or None, y8, ys: uint8 numpy or None)"""
    b, hi, wi, ci, ho, wo, co = geom[:7]
    x_, xs_, w_, s_ = dev(x8), dev(xs), (w8 if torch.is_tensor(w8) else dev(w8)), (s_w if torch.is_tensor(s_w) else dev(np.asarray(s_w, np.float32)))
    wants8 = mode in (mx.OUT_MX, mx.OUT_BF16_MX)
    y_ = None if mode == mx.OUT_MX else torch.full((b, ho, wo, co), 9.0, dtype=torch.float32 if mode == mx.OUT_F32 else torch.bfloat16, device='cuda')
    y8_ = u8((b, ho, wo, co)) if wants8 else None
    ys_ = u8((b, ho, wo, co // 32)) if wants8 else None
    check(lib.ssd_op_conv2d_fwd_mxfp8(ptr(x_), ptr(xs_), ptr(w_), ptr(s_), ptr(dev(bias)), ptr(y_), ptr(y8_), ptr(ys_), mode, *geom, int(relu), None))
    torch.cuda.synchronize()
    return (None if y_ is None else y_.float().cpu().numpy()), (y8_.cpu().numpy() if wants8 else None), (ys_.cpu().numpy() if wants8 else None)


# test_gpu_fp8's cases.  An MX output needs Co % 32 == 0: a case with another Co checks the fp32 and the bf16 output, and the stride-2
# case is there once more with Co = 96 (across the 64-wide tile, inside the 128-wide one) for the MX output
STRIDE2 = next(c for c in FP8_LAYOUT_CASES if c[0] == '3x3 stride2 SAME 64->72 1x10x9')
LAYOUT_CASES = FP8_LAYOUT_CASES + [('3x3 stride2 SAME 64->96 1x10x9',) + STRIDE2[1:5] + (96,) + STRIDE2[6:]]


@pytest.mark.parametrize('tile', ['0', '1'], ids=['128x128', '64x64'])
@pytest.mark.parametrize('case', LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_conv_layout_exact(case, tile, monkeypatch):
    """activations i * 2^s with i in 0 ... 7 and s in -2 ... 2 varying with pixel and block, filter codes in -2 ... 2, asymmetric in
    pixel, channel, tap and output channel: every sum is a multiple of 1/4 below 2^22, exact in any order"""
    monkeypatch.setenv('SSD_TILE_FP8', tile)
    name, b, hi, wi, ci, co, kh, kw, stride, dil, padding = case
    iv, w8, bias, geom = layout_operands(case)
    B, H, W, Cc = np.meshgrid(np.arange(b), np.arange(hi), np.arange(wi), np.arange(ci), indexing='ij')
    sv = (2 * B + 3 * H + W + 2 * (Cc // 32) + (H * (Cc // 32)) % 3) % 5 - 2
    xv = np.ldexp(iv.astype(np.float32), sv).astype(np.float32)
    x8, xs = mx.quantize(xv)
    assert np.array_equal(mx.dequantize(x8, xs), xv.astype(np.float64)) and len(np.unique(xs)) >= 5      # lossless; scales vary
    xv_ref, padding_ref = layout_reference_input(xv, case)
    acc, absacc = mx.conv_values(xv_ref, w8, kh, kw, stride, dil, padding_ref)
    want = acc + bias
    assert want.shape == (geom[0], geom[4], geom[5], co)
    assert absacc.max() + 8 < 2 ** 22 and np.array_equal(want * 4, np.round(want * 4)) and len(np.unique(want)) > 50
    y, _, _ = run_conv(x8, xs, w8, np.ones(co), bias, geom, mx.OUT_F32, False)
    assert np.array_equal(y, want.astype(np.float32)), f'{name}: {np.argwhere(y != want)[:4]}'
    pos = np.maximum(want, 0).astype(np.float32)
    if co % 32:
        y, _, _ = run_conv(x8, xs, w8, np.ones(co), bias, geom, mx.OUT_BF16, True)
        assert np.array_equal(y, bf16_round(pos))
        return
    y, y8, ys = run_conv(x8, xs, w8, np.ones(co), bias, geom, mx.OUT_BF16_MX, True)
    assert np.array_equal(y, bf16_round(pos))
    want8, wants = mx.quantize(pos)
    assert np.array_equal(ys, wants) and np.array_equal(y8, want8)


def check_real_layer(name, xv, x8, xs, w8, s_w, bias, geom, k, stride, dil, padding, relu, mx_out):
    """one layer from given MX activations: fp32 and bf16 out within the bound; -> largest fp32-out error / B"""
    K = k * k * geom[3]
    acc, absacc = mx.conv_values(xv, w8, k, k, stride, dil, padding)
    y_ref = mx.epilogue(acc, s_w, bias, relu)
    Bd = mx.accumulation_bound(absacc, K, s_w)
    y32, _, _ = run_conv(x8, xs, w8, s_w, bias, geom, mx.OUT_F32, relu)
    err = np.abs(y32 - y_ref)
    worst = float((err / np.maximum(Bd, 1e-300))[Bd > 0].max())
    print(f'\n[mxfp8 conv] {name}: largest fp32-out error / B = {worst:.4f}')
    assert np.all(err <= Bd), f'{name} fp32 out: max (err - bound) {float((err - Bd).max()):.3e}'
    y16, _, _ = run_conv(x8, xs, w8, s_w, bias, geom, mx.OUT_BF16, relu)
    lim = Bd + np.abs(y_ref) * 2.0 ** -8
    assert np.all(np.abs(y16 - y_ref) <= lim), f'{name} bf16 out: max (err - bound) {float((np.abs(y16 - y_ref) - lim).max()):.3e}'
    if mx_out:
        # the epilogue is deterministic: the MX bytes are the oracle's quantiser applied to the kernel's OWN fp32 output, byte for byte
        want8, wants = mx.quantize(y32)
        _, y8, ys = run_conv(x8, xs, w8, s_w, bias, geom, mx.OUT_MX, relu)
        assert np.array_equal(ys, wants), np.argwhere(ys != wants)[:4]
        assert np.array_equal(y8, want8), np.argwhere(y8 != want8)[:4]
        y16b, y8, ys = run_conv(x8, xs, w8, s_w, bias, geom, mx.OUT_BF16_MX, relu)
        assert np.array_equal(ys, wants) and np.array_equal(y8, want8) and np.array_equal(y16b, y16)
    return worst


@pytest.mark.parametrize('case', REAL_CASES, ids=[c[0] for c in REAL_CASES])
def test_conv_real_valued(case, capsys):
    name, b, hi, wi, ci, co, k, stride, dil, padding, relu, _ = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ph, pw, ho, wo = conv_geom(hi, wi, k, stride, dil, padding)
    x = (rng.normal(0, 1, (b, hi, wi, ci)) * np.exp2(rng.integers(-3, 4, (b, hi, wi, ci // 32)).repeat(32, -1))).astype(np.float32)
    w = (rng.normal(0, 1, (k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.normal(0, 0.1, (co,)).astype(np.float32)
    x8, xs = gpu_quantize(x.reshape(-1, ci), True)                # (bytes pinned by test_quantize_bit_exact)
    x8, xs = x8.reshape(b, hi, wi, ci), xs.reshape(b, hi, wi, ci // 32)
    w8_, s_ = gpu_quantize_filter(w)
    geom = (b, hi, wi, ci, ho, wo, co, k, k, stride, dil, ph, pw)
    with capsys.disabled():
        check_real_layer(name, mx.dequantize(x8, xs), x8, xs, host(w8_), host(s_), bias, geom, k, stride, dil, padding, relu, name == FOUR_MODES_CASE)


@pytest.mark.parametrize('what', ['Ci=96', '25 taps', 'Co=20', 'MX out Co=40'])
def test_conv_refused_shapes_write_nothing(what):
    ci, co, k = (96, 64, 3) if what == 'Ci=96' else (64, 64, 5) if what == '25 taps' else (64, 20, 3) if what == 'Co=20' else (64, 40, 3)
    mode = mx.OUT_BF16_MX if what == 'MX out Co=40' else mx.OUT_F32
    b, hi, wi = 1, 6, 6
    ph, pw, ho, wo = conv_geom(hi, wi, k, 1, 1, 'SAME')
    x8_, xs_, w8_ = u8((b, hi, wi, ci), 0x38), u8((b, hi, wi, ci // 32), 0x7F), u8((k * k, co, ci), 0x38)
    y_ = torch.full((b, ho, wo, co), 9.0, dtype=torch.float32, device='cuda')
    y8_, ys_ = u8((b, ho, wo, co)), u8((b, ho, wo, co // 32 + 1))
    rc = lib.ssd_op_conv2d_fwd_mxfp8(ptr(x8_), ptr(xs_), ptr(w8_), ptr(dev(np.ones(co, np.float32))), None, ptr(y_), ptr(y8_), ptr(ys_), mode,
                                     b, hi, wi, ci, ho, wo, co, k, k, 1, 1, ph, pw, 1, None)
    assert rc != 0 and 'mxfp8 conv' in last_error()
    assert np.all(host(y_) == 9.0) and np.all(host(y8_) == 0xAB) and np.all(host(ys_) == 0xAB)


# ------------------------------------------------------------------------------------------------------------ pooling
POOL_CASES = [('5->3 ceil 2x2 s2', 2, 5, 5, 2, 2), ('7x9 3x3 s1', 1, 7, 9, 3, 1)]


def gpu_pool(x8, xs, k, stride):
    b, hi, wi, c = x8.shape
    ph, ho = same_pad(hi, k, stride)
    pw, wo = same_pad(wi, k, stride)
    x8_, xs_, y8_, ys_ = dev(x8), dev(xs), u8((b, ho, wo, c)), u8((b, ho, wo, c // 32))      # (named: both inputs stay allocated)
    check(lib.ssd_op_maxpool_fwd_mxfp8(ptr(x8_), ptr(xs_), ptr(y8_), ptr(ys_), b, hi, wi, c, ho, wo, k, stride, ph, pw, None))
    return host(y8_), host(ys_)


@pytest.mark.parametrize('c', [32, 64])
@pytest.mark.parametrize('case', POOL_CASES, ids=[p[0] for p in POOL_CASES])
def test_maxpool_bytes(case, c):
    name, b, hi, wi, k, stride = case
    rng = np.random.default_rng(zlib.crc32(name.encode()) + c)
    ok = np.array([v for v in range(256) if v not in (0x7F, 0xFF, 0x80)], np.uint8)      # (no NaN; -0 against +0 has no defined maximum)
    x8 = rng.choice(ok, size=(b, hi, wi, c))
    xs = rng.integers(121, 134, (b, hi, wi, c // 32)).astype(np.uint8)                   # 2^-6 ... 2^6
    x8[0, :3, :3, :] = rng.choice(np.arange(0x81, 0xFF, dtype=np.uint8), size=(3, 3, c))  # windows that are all negative
    # a window (2x2: rows 2..3, columns 2..3 = output (1, 1); 3x3 s1: around (4, 4)) whose maximum comes from the cell with the smallest scale
    r = 2 if k == 2 else 3
    x8[0, r:r + k, r:r + k, :] = f8.encode(np.array([2.0 ** -6]))[0]; xs[0, r:r + k, r:r + k, :] = 133      # 1.0 each
    x8[0, r + 1, r + 1, :] = 0x7E; xs[0, r + 1, r + 1, :] = 121                                             # 448 * 2^-6 = 7
    y8, ys = gpu_pool(x8, xs, k, stride)
    want8, wants = mx.maxpool(x8, xs, k, stride)
    assert want8.shape == y8.shape and wants.shape == ys.shape
    assert np.array_equal(ys, wants), np.argwhere(ys != wants)[:4]
    assert np.array_equal(y8, want8), np.argwhere(y8 != want8)[:4]
    o = (r + 1) // stride
    assert np.all(mx.dequantize(y8, ys)[0, o, o] == 7.0) and np.all(mx.dequantize(y8, ys)[0, 0, 0] < 0)
    if c == 32:
        bad = rng.choice(ok, size=(b, hi, wi, 16))
        ph, ho = same_pad(hi, k, stride)
        pw, wo = same_pad(wi, k, stride)
        bad_, xs_, y8_, ys_ = dev(bad), dev(xs), u8((b, ho, wo, 16)), u8((b, ho, wo, 1))
        assert lib.ssd_op_maxpool_fwd_mxfp8(ptr(bad_), ptr(xs_), ptr(y8_), ptr(ys_), b, hi, wi, 16, ho, wo, k, stride, ph, pw, None) != 0
        assert 'multiple of 32' in last_error() and np.all(host(y8_) == 0xAB) and np.all(host(ys_) == 0xAB)


# ------------------------------------------------------------------------------------------------------------ whole model
MX_TENSORS = FP8_SCALED + FP8_POOLS      # the tensors kept as codes + scales: conv3_1 (quantised behind the bf16 layer) ... mod_conv6, the pools


def build(sess, preset_name, w, b, dtype, a_trous=True):
    from ssd_tensorflow_amd.ssdvgg import SSDVGG
    net = SSDVGG(sess, preset_name)
    net.build_from_vgg(None, 20, a_trous=a_trous, max_batch=b, training=False, weights=w, dtype=dtype)
    return net


@pytest.fixture(scope='module')
def model():
    from oracle import boxes as ob, ssdvgg_ref as ref
    from ssd_tensorflow_amd.ssdvgg import Session
    preset = ob.get_preset('vgg300')
    w = ref.init_params(preset, 20, seed=42, alive=True)
    b = 2
    x = ref.synth_images(np.random.default_rng(99), b, preset)
    sess = Session(0)
    nets = {dt: build(sess, 'vgg300', w, b, dt) for dt in ('mxfp8', 'fp8', 'bf16', 'f32')}
    assert nets['mxfp8'].dtype == 'mxfp8'
    res = {'mxfp8': nets['mxfp8'].infer(x)}                  # straight after creation: nothing to calibrate
    nets['fp8'].calibrate_fp8(x)
    res.update({dt: nets[dt].infer(x) for dt in ('fp8', 'bf16', 'f32')})
    yield dict(preset=preset, w=w, b=b, x=x, nets=nets, res=res, ref=ref, sess=sess)
    sess.close()


def mx_codes(net, name, b):
    """(dequantised fp32, codes, scale bytes) of an MX tensor of the handle"""
    a, s = net.activation(name, b), net.activation('scale:' + name, b)
    m, e = np.frexp(s)
    assert np.all(m == 0.5) and s.shape == a.shape[:-1] + (a.shape[-1] // 32,), f'{name}: a block scale is no power of two'
    sb = (e - 1 + 127).astype(np.uint8)
    codes = f8.encode(a.astype(np.float64) / np.repeat(s.astype(np.float64), 32, -1))
    assert np.array_equal(mx.dequantize(codes, sb), a.astype(np.float64))
    return a, codes, sb


def check_scales_follow_rule(name, a, codes, sb):
    """the scale is the rule applied to the dequantised block's absmax, except where that absmax was rounded down to 1.75 * 2^7 of its
    scale (= 448 * 2^(x - 1), for which the rule gives x - 1)"""
    blk = np.abs(a).reshape(a.shape[:-1] + (a.shape[-1] // 32, 32)).max(-1)
    again = (mx.scale_exponent(blk) + 127).astype(np.uint8)
    top = np.abs(f8.decode(codes)).reshape(blk.shape + (32,)).max(-1)
    assert np.all((again == sb) | ((top == 224.0) & (again == sb - 1))), f'{name}: {np.argwhere(again != sb)[:4]}'
    assert np.all(top[blk > 0] >= 224.0) and sb.max() < 255


def test_model_mx_layers_local(model, capsys):
    """every MX layer's output against the oracle applied to the kernel's OWN dequantised input, with the bound of the op test.  Maps
    higher than 40 rows are checked on three bands of rows (top border, middle, bottom border, every column and channel)."""
    ref, b, w, net = model['ref'], model['b'], model['w'], model['nets']['mxfp8']
    ops = {op[1]: op for op in ref.graph(model['preset']) if op[0] in ('conv', 'pool')}
    lines = []
    for name in FP8_LAYERS:
        _, _, src, k, stride, padding, dil = ops[name]
        assert stride == 1 and padding == 'SAME'
        xv, _, _ = mx_codes(net, src, b)
        w8, s_w = f8.quantize_filter(w[name + '/filter'])
        bias = w[name + '/biases']
        H = xv.shape[1]
        bands = [(0, 5), (H // 2, H // 2 + 3), (H - 5, H)] if H > 40 else [(0, H)]
        got8 = mx_codes(net, name, b) if name != 'mod_conv7' else None
        got16 = net.activation(('bf16:' if got8 is not None else '') + name, b) if name in ('conv4_3', 'mod_conv7') else None
        if got8 is not None:
            check_scales_follow_rule(name, *got8)
        worst8 = worst16 = 0.0
        for r0, r1 in bands:
            acc, absacc = mx.conv_values_rows(xv, w8, k, dil, r0, r1)
            y_ref = mx.epilogue(acc, s_w, bias, True)
            Bd = mx.accumulation_bound(absacc, k * k * xv.shape[3], s_w)
            assert np.count_nonzero(y_ref) > 0.2 * y_ref.size, f'{name} is (nearly) dead: the test would prove nothing'
            if got8 is not None:
                a, codes, sb = (t[:, r0:r1] for t in got8)
                sv = np.repeat(mx.scale_values(sb), 32, -1)
                err = np.abs(a - y_ref)
                lim = Bd + sv * f8.e4m3_step(y_ref / sv) / 2          # one e4m3 rounding at the block's scale
                assert np.all(err <= lim), f'{name} rows {r0}:{r1}: MX output off by {float((err - lim).max()):.3e}'
                worst8 = max(worst8, float((err / np.maximum(lim, 1e-300)).max()))
            if got16 is not None:
                err = np.abs(got16[:, r0:r1] - y_ref)
                lim = Bd + np.abs(y_ref) * 2.0 ** -8
                assert np.all(err <= lim), f'{name} rows {r0}:{r1}: bf16 output off by {float((err - lim).max()):.3e}'
                worst16 = max(worst16, float((err / np.maximum(lim, 1e-300)).max()))
        lines.append(f'{name}: worst error / bound: MX out {worst8:.3f}, bf16 out {worst16:.3f} (0: no such output)')
    with capsys.disabled():
        print('\n[mxfp8 model] ' + '\n[mxfp8 model] '.join(lines))


def test_model_mx_boundaries_and_pools(model):
    ref, b, nets = model['ref'], model['b'], model['nets']
    net = nets['mxfp8']
    # conv3_1: the bf16 handle's kernels up to here, then the one stand-alone quantise pass
    c31 = net.activation('bf16:conv3_1', b)
    assert np.array_equal(c31, nets['bf16'].activation('conv3_1', b))
    a, codes, sb = mx_codes(net, 'conv3_1', b)
    want8, wants = mx.quantize(c31)
    assert np.array_equal(sb, wants) and np.array_equal(codes, want8)
    # the pools: the maximum of the dequantised cells, quantised again
    ops = {op[1]: op for op in ref.graph(model['preset']) if op[0] == 'pool'}
    for name in FP8_POOLS:
        _, _, src, k, s = ops[name]
        _, c_in, s_in = mx_codes(net, src, b)
        _, c_out, s_out = mx_codes(net, name, b)
        want8, wants = mx.maxpool(c_in, s_in, k, s)
        assert np.array_equal(s_out, wants) and np.array_equal(c_out, want8), name
    with pytest.raises(RuntimeError, match='no bf16 form'):
        net.activation('bf16:conv3_2', b)
    with pytest.raises(RuntimeError, match='no block scales'):
        net.activation('scale:mod_conv7', b)


def test_model_mx_untouched_layers_and_result(model, capsys):
    """conv8_1 onwards, the l2 norm and the heads are the bf16 handle's code: each against the bf16 oracle applied to the tensor it
    actually read; then the result, and its distance to fp32 against the calibrated fp8 handle's in the same run"""
    from test_gpu_bf16 import layer_local_forward_check, TOL_BF
    ref, b, nets, res = model['ref'], model['b'], model['nets'], model['res']
    net = nets['mxfp8']

    class Bf16View:
        def activation(self, name, n):
            return net.activation(('bf16:' if name in MX_TENSORS else '') + name, n)

    m = ref.RefModel('vgg300', params=model['w'])
    only = [op[1] for op in ref.graph(model['preset']) if op[0] == 'conv' and op[1] not in FP8_LAYERS + ['conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1']]
    only += ['l2_norm_conv4_3'] + ['heads/map%d' % i for i in range(6)]
    assert 'conv8_1' in only and 'conv11_2' in only
    assert layer_local_forward_check(Bf16View(), m, model['preset'], b, model['x'], only=only) < TOL_BF
    rm = res['mxfp8']
    assert np.isfinite(rm).all() and np.abs(rm[..., :21].sum(-1) - 1).max() < 1e-4
    d = {dt: rel_err(res[dt], res['f32']) for dt in ('mxfp8', 'fp8', 'bf16')}
    with capsys.disabled():
        print(f"\n[mxfp8 model] rel_err(result, result fp32): mxfp8 {d['mxfp8']:.4e}, fp8 {d['fp8']:.4e}, bf16 {d['bf16']:.4e}")
    # both are ten layers of the same 2^-4 element rounding; a layout or scale bug gives O(1): the factor 2 is a cap to catch a bug
    assert d['mxfp8'] <= 2 * d['fp8']


def test_model_no_state(model):
    nets, x, b = model['nets'], model['x'], model['b']
    net, n8 = nets['mxfp8'], nets['fp8']
    dark = np.floor(x / 8).astype(np.float32)
    # the calibrated handle: scales from dark images saturate on the bright ones
    n8.calibrate_fp8(dark)
    n8.infer(x)
    s = np.float32(n8.fp8_scales['conv3_1'])
    assert np.abs(n8.activation('conv3_1', b) / s).max() == 448.0 and np.abs(n8.activation('bf16:conv3_1', b)).max() > 448.0 * s
    n8.calibrate_fp8(x)
    # the mxfp8 handle: the result for x does not depend on what was inferred before, nor on the rest of the batch
    r0 = net.infer(x)
    assert np.array_equal(r0, model['res']['mxfp8'])
    net.infer(dark)
    assert np.array_equal(net.infer(x), r0)
    other = np.stack([dark[1], x[1]])
    assert np.array_equal(net.infer(other)[1], r0[1])
    assert not np.array_equal(net.infer(other)[0], r0[0])


def test_lifecycle(model):
    net, x, b, w = model['nets']['mxfp8'], model['x'], model['b'], model['w']
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
    # the e4m3 filters follow the fp32 masters: mod_conv7's filter and bias times 3 -> its (relu) output times 3, up to a second
    # rounding of the codes and of the bf16 output (far below 2^-6 in the L2 norm; a stale filter would leave a distance of 2/3)
    r0 = net.infer(x)
    y0 = net.activation('mod_conv7', b)
    net.load_variables({'mod_conv7/filter': w['mod_conv7/filter'] * 3, 'mod_conv7/biases': w['mod_conv7/biases'] * 3})
    net.infer(x)
    y1 = net.activation('mod_conv7', b)
    assert np.count_nonzero(y0) > 0.2 * y0.size and rel_err(y1, 3 * y0) < 2.0 ** -6
    net.load_variables({'mod_conv7/filter': w['mod_conv7/filter'], 'mod_conv7/biases': w['mod_conv7/biases']})
    assert np.array_equal(net.infer(x), r0)


def test_vgg512_batch1(model, capsys):
    from oracle import boxes as ob
    ref = model['ref']
    preset = ob.get_preset('vgg512')
    w = ref.init_params(preset, 20, seed=42, alive=True)
    x = ref.synth_images(np.random.default_rng(5), 1, preset)
    r = {dt: build(model['sess'], 'vgg512', w, 1, dt).infer(x) for dt in ('mxfp8', 'bf16')}
    assert np.isfinite(r['mxfp8']).all() and np.abs(r['mxfp8'][..., :21].sum(-1) - 1).max() < 1e-4
    with capsys.disabled():
        print(f"\n[mxfp8 model] vgg512 batch 1: rel_err(result mxfp8, result bf16) = {rel_err(r['mxfp8'], r['bf16']):.4e}")


def test_fc_graph_batch1(model, capsys):
    """the fc graph: fc6 (7x7) stays on the bf16 kernel with the quantise pass behind it; fc7 (1x1, 4096 -> 4096) runs on MX operands"""
    import fc_ref
    from test_gpu_fp8_bigk import CHECKED
    ref = model['ref']
    w = fc_ref.init_params(model['preset'], 20, seed=42)
    x = ref.synth_images(np.random.default_rng(99), 1, model['preset'])
    net = build(model['sess'], 'vgg300', w, 1, 'mxfp8', a_trous=False)
    r = net.infer(x)
    assert np.isfinite(r).all() and np.abs(r[..., :21].sum(-1) - 1).max() < 1e-4
    # fc6 on bf16: its bf16 form exists, conv5_3 / mod_pool5 in front of it are bf16 only, and its MX form is the quantiser's
    a16 = net.activation('bf16:mod_conv6', 1)
    with pytest.raises(RuntimeError, match='no block scales'):
        net.activation('scale:mod_pool5', 1)
    xv, codes, sb = mx_codes(net, 'mod_conv6', 1)
    want8, wants = mx.quantize(a16)
    assert np.array_equal(sb, wants) and np.array_equal(codes, want8)
    # fc7 locally, on the output channels CHECKED (a per-channel filter scale makes a channel subset exact)
    w8, s_w = f8.quantize_filter(w['fc7/weights'][..., CHECKED])
    acc, absacc = mx.conv_values(xv, w8, 1, 1, 1, 1, 'SAME')
    y_ref = mx.epilogue(acc, s_w, w['fc7/biases'][CHECKED], True)
    Bd = mx.accumulation_bound(absacc, xv.shape[3], s_w)
    assert np.count_nonzero(y_ref) > 0.2 * y_ref.size
    err = np.abs(net.activation('mod_conv7', 1)[..., CHECKED] - y_ref)
    lim = Bd + np.abs(y_ref) * 2.0 ** -8
    assert np.all(err <= lim), f'mod_conv7: bf16 output off by {float((err - lim).max()):.3e}'
    with capsys.disabled():
        print(f'\n[mxfp8 fc model] mod_conv7: worst error / bound {float((err / np.maximum(lim, 1e-300)).max()):.3f}')


def test_detect_tool_mxfp8_child_process(tmp_path):
    """detect.py --dtype mxfp8 on three small images, twice with the files in opposite order: the same detections per image, with
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
    cmd = [sys.executable, '-m', 'ssd_tensorflow_amd.detect', '--model', model_file, '--batch-size', '2', '--dtype', 'mxfp8']
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
