"""-m gpu: the fp8 (e4m3) inference kernels through the C ABI against tests/fp8_ref.py.

Quantisation and pooling are compared byte for byte.  The convolution is compared twice: on small-integer data whose sums are
exact in fp32 (any permuted k, swapped row / column or misplaced tap shows as a wrong integer), and on real-valued layers against
the float64 convolution of the SAME codes with the bound B = K * 2^-23 * (s_in * s_w[co]) * sum |x_code * w_code| (K fp32
additions at one ulp each) -- plus one bf16 rounding (2^-8 |y|) or half an e4m3 step where the output is stored that way."""
import zlib

import numpy as np
import pytest
import torch

import fp8_ref as f8
from gpu_util import lib, check, dev, ptr, host, conv_geom, same_pad
from ssd_tensorflow_amd._lib import last_error
from test_gpu_bf16 import CONV_CASES

pytestmark = pytest.mark.gpu


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def u8(shape, fill=0xAB):
    return torch.full(shape, fill, dtype=torch.uint8, device='cuda')


# ------------------------------------------------------------------------------------------------------------ quantise
def edge_values():
    """every finite code's value, every tie between two codes, every half step of the subnormal range, the values at and above
    448, both zeros"""
    pos = f8.decode(np.arange(0x7F, dtype=np.uint8))
    mids = (pos[1:] + pos[:-1]) / 2
    sub = np.arange(0, 34) * 2.0 ** -10
    big = np.array([440.0, 448.0, 450.0, 463.0, 464.0, 466.0, 480.0, 512.0, 1e6, 3e38])
    v = np.concatenate([pos, mids, sub, big])
    return np.concatenate([v, -v]).astype(np.float32)


@pytest.mark.parametrize('x_f32', [False, True], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('scale', [1.0, 0.25, 0.0371], ids=['s1', 's0.25', 's0.0371'])
def test_quantize_bit_exact(x_f32, scale):
    rng = np.random.default_rng(7)
    edge = edge_values() * np.float32(scale if scale != 0.0371 else 1.0)      # (exact ties need a power-of-two scale)
    v = np.concatenate([edge, rng.normal(0, 150 * scale, 4096 - edge.size).astype(np.float32)])
    assert v.size == 4096
    if not x_f32:
        v = bf16_round(v)
    x_ = dev(v) if x_f32 else dev(v).bfloat16()
    y_ = u8((4096 + 16,))
    check(lib.ssd_op_quantize_fp8(ptr(x_), int(x_f32), 4096, scale, ptr(y_), None))
    got = host(y_)
    want = f8.quantize(v, scale)
    assert np.array_equal(got[:4096], want), np.flatnonzero(got[:4096] != want)[:8]
    assert np.all(got[4096:] == 0xAB)
    assert got[np.flatnonzero(np.signbit(v) & (v == 0))[0]] == 0x80          # -0 keeps its sign
    # a length that is no multiple of the vector width
    check(lib.ssd_op_quantize_fp8(ptr(x_), int(x_f32), 4093, scale, ptr(y_), None))
    assert np.array_equal(host(y_)[:4093], want[:4093])


def test_absmax_bf16():
    rng = np.random.default_rng(3)
    v = bf16_round(rng.normal(0, 1, 70001))
    v[12345] = -37.5
    v[7] = np.inf                      # skipped: calibration must not be poisoned by one overflow
    out_ = dev(np.array([1e9], np.float32))
    check(lib.ssd_op_absmax_bf16(ptr(dev(v).bfloat16()), v.size, ptr(out_), 0, None))
    assert host(out_)[0] == 37.5
    check(lib.ssd_op_absmax_bf16(ptr(dev(v[:100] * 0).bfloat16()), 100, ptr(out_), 1, None))
    assert host(out_)[0] == 37.5       # accumulate keeps the larger
    check(lib.ssd_op_absmax_bf16(ptr(dev(v[:100] * 0 + 64).bfloat16()), 100, ptr(out_), 1, None))
    assert host(out_)[0] == 64.0


def gpu_quantize_filter(w):
    kh, kw, ci, co = w.shape
    w8_ = u8((kh * kw, co, ci))
    s_ = torch.full((co,), -1.0, dtype=torch.float32, device='cuda')
    check(lib.ssd_op_quantize_filter_fp8(ptr(dev(w)), ptr(w8_), ptr(s_), kh * kw, ci, co, None))
    return w8_, s_


def test_quantize_filter_bit_exact():
    rng = np.random.default_rng(11)
    w = (rng.normal(0, 1, (3, 3, 64, 72)) / 24).astype(np.float32)
    w[..., 5] = 0                                     # an all-zero output channel: scale 1, codes 0
    w[1, 2, 33, 9] = -3.0                             # a channel whose absmax is a negative value
    w8_, s_ = gpu_quantize_filter(w)
    codes, s = f8.quantize_filter(w)
    assert np.array_equal(host(s_).view(np.uint32), s.view(np.uint32))
    assert host(s_)[5] == 1.0 and host(s_)[9] == np.float32(3.0) / np.float32(448.0)
    assert np.array_equal(host(w8_), codes)
    assert host(w8_)[1 * 3 + 2, 9, 33] == 0xFE


# ------------------------------------------------------------------------------------------------------------ convolution
def run_conv(x8, w8, s_in, s_w, bias, geom, mode, s_out, relu):
    """-> (y: fp32 numpy of the bf16 / fp32 output or None, y8: uint8 numpy or None)"""
    b, hi, wi, ci, ho, wo, co = geom[:7]
    x_ = x8 if torch.is_tensor(x8) else dev(x8)
    w_ = w8 if torch.is_tensor(w8) else dev(w8)
    s_ = s_w if torch.is_tensor(s_w) else dev(np.asarray(s_w, np.float32))
    y_ = None if mode == f8.OUT_E4M3 else torch.full((b, ho, wo, co), 9.0, dtype=torch.float32 if mode == f8.OUT_F32 else torch.bfloat16, device='cuda')
    y8_ = u8((b, ho, wo, co)) if mode in (f8.OUT_E4M3, f8.OUT_BF16_E4M3) else None
    check(lib.ssd_op_conv2d_fwd_fp8(ptr(x_), ptr(w_), s_in, ptr(s_), ptr(dev(bias)), ptr(y_), ptr(y8_), mode, s_out, *geom, int(relu), None))
    torch.cuda.synchronize()
    return (None if y_ is None else y_.float().cpu().numpy()), (None if y8_ is None else y8_.cpu().numpy())


def geom2(hi, wi, kh, kw, stride, dil, padding):
    """gpu_util.conv_geom with kh and kw apart: (pad_h, pad_w, ho, wo)"""
    if padding == 'SAME':
        ph, ho = same_pad(hi, kh, stride, dil)
        pw, wo = same_pad(wi, kw, stride, dil)
        return ph, pw, ho, wo
    return 0, 0, (hi - ((kh - 1) * dil + 1)) // stride + 1, (wi - ((kw - 1) * dil + 1)) // stride + 1


# The last three are what the tap walk (counters over kernel rows and columns, a separable row / column validity mask) can get wrong
# at few taps: a stride with SAME on an even and an odd side (leading pad 0 and 1), Co across the 64-wide tile and inside the 128-wide
# one, M = 25; kh != kw with two channel chunks and the smallest Co; nine taps in one kernel row, wider than any 3x3.
#               name                                  b  hi  wi  ci   co  kh kw stride dil padding
LAYOUT_CASES = [('3x3 SAME 64->64 2x9x7',             2,  9,  7, 64,  64, 3, 3, 1, 1, 'SAME'),
                ('1x1 128->64 1x5x5',                 1,  5,  5, 128, 64, 1, 1, 1, 1, 'SAME'),
                ('3x3 dil6 128->64 1x19x19',          1, 19, 19, 128, 64, 3, 3, 1, 6, 'SAME'),
                ('3x3 stride2 SAME 64->72 1x10x9',    1, 10,  9, 64,  72, 3, 3, 2, 1, 'SAME'),
                ('2x3 VALID 128->8 1x6x7',            1,  6,  7, 128, 8,  2, 3, 1, 1, 'VALID'),
                ('1x9 SAME 64->64 1x3x11',            1,  3, 11, 64,  64, 1, 9, 1, 1, 'SAME')]


def layout_reference_input(a, case):
    """The oracle pads SAME by the kernel's rows, for rows and columns alike.  For kh != kw: (a [B,H,W,C] with the zeros SAME adds,
    'VALID'), the same sums; otherwise (a, padding).  The pads come from same_pad, like the pad_h / pad_w that geom2 hands to the
    kernel: for these cases the sums and the output shape are the oracle's, the split of the padding is not checked against it (the
    stride-2 SAME case, a square kernel, goes through the oracle's own SAME)."""
    hi, wi, kh, kw, stride, dil, padding = case[2], case[3], *case[6:]
    if padding != 'SAME' or kh == kw:
        return a, padding
    pads = []
    for n, k in ((hi, kh), (wi, kw)):
        lead, out = same_pad(n, k, stride, dil)
        pads.append((lead, max((out - 1) * stride + (k - 1) * dil + 1 - n, 0) - lead))
    return np.pad(a, ((0, 0), pads[0], pads[1], (0, 0))), 'VALID'


def layout_operands(case):
    """(x integers [B,H,W,Ci] in 0 ... 7, filter codes [tap][Co][Ci] of integers in -2 ... 2, bias, geom) of a layout case:
    asymmetric in pixel, channel, tap and output channel"""
    name, b, hi, wi, ci, co, kh, kw, stride, dil, padding = case
    ph, pw, ho, wo = geom2(hi, wi, kh, kw, stride, dil, padding)
    B, H, W, Cc = np.meshgrid(np.arange(b), np.arange(hi), np.arange(wi), np.arange(ci), indexing='ij')
    iv = (3 * B + 5 * H + 7 * W + 11 * Cc + (H * W) % 3 + (Cc * W) % 5 + (Cc // 16)) % 8
    KH, KW, CI, CO = np.meshgrid(np.arange(kh), np.arange(kw), np.arange(ci), np.arange(co), indexing='ij')
    wv = (2 * KH + 3 * KW + CI + 7 * CO + (CI * CO) % 3 + (KH * CI) % 2 + (CI // 32)) % 5 - 2
    w8 = np.ascontiguousarray(np.transpose(f8.encode(wv.astype(np.float64)).reshape(kh * kw, ci, co), (0, 2, 1)))
    bias = ((np.arange(co) * 5) % 17 - 8).astype(np.float32)
    return iv, w8, bias, (b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, ph, pw)


@pytest.mark.parametrize('tile', ['0', '1'], ids=['128x128', '64x64'])
@pytest.mark.parametrize('case', LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_conv_layout_exact(case, tile, monkeypatch):
    """small integers, asymmetric in pixel, channel, tap and output channel; all scales 1: every sum is an integer < 2^24"""
    monkeypatch.setenv('SSD_TILE_FP8', tile)
    name, co, (kh, kw, stride, dil, padding) = case[0], case[5], case[6:]
    xv, w8, bias, geom = layout_operands(case)
    x8 = f8.encode(xv.astype(np.float64))
    x8_ref, padding_ref = layout_reference_input(x8, case)
    acc, _ = f8.conv_codes(x8_ref, w8, kh, kw, stride, dil, padding_ref)
    want = acc + bias
    assert want.shape == (geom[0], geom[4], geom[5], co)
    assert np.abs(want).max() < 2 ** 24 and len(np.unique(want)) > 50
    y, _ = run_conv(x8, w8, 1.0, np.ones(co), bias, geom, f8.OUT_F32, 0.0, False)
    assert np.array_equal(y, want.astype(np.float32)), f'{name}: {np.argwhere(y != want)[:4]}'
    y, y8 = run_conv(x8, w8, 1.0, np.ones(co), bias, geom, f8.OUT_BF16_E4M3, 1.0, True)
    assert np.array_equal(y, bf16_round(np.maximum(want, 0)))
    assert np.array_equal(y8, f8.encode(np.maximum(want, 0)))          # one rounding of an exact value, saturating at 448


REAL_CASES = [c for c in CONV_CASES if c[4] % 64 == 0 and 'head' not in c[0]]
FOUR_MODES_CASE = 'ragged M, 1 image'


def check_real_layer(name, x8, w8, s_in, s_w, bias, geom, k, stride, dil, padding, relu, modes, tag=''):
    """One layer from given codes: every requested output mode within the bound; returns the float64 reference"""
    K = k * k * geom[3]
    acc, absacc = f8.conv_codes(x8, w8, k, k, stride, dil, padding)
    y_ref = f8.epilogue(acc, s_in, s_w, bias, relu)
    Bd = f8.accumulation_bound(absacc, K, s_in, s_w)
    s_out = float(np.float32(max(np.abs(y_ref).max(), 1e-30) / 448.0 * 0.9))      # 0.9: a few values saturate
    worst = 0.0
    for mode in modes:
        y, y8 = run_conv(x8, w8, s_in, s_w, bias, geom, mode, s_out, relu)
        if y is not None:
            err = np.abs(y - y_ref)
            worst = max(worst, float((err / np.maximum(Bd, 1e-300))[Bd > 0].max()) if mode == f8.OUT_F32 else 0.0)
            lim = Bd + (0 if mode == f8.OUT_F32 else np.abs(y_ref) * 2.0 ** -8)
            assert np.all(err <= lim), f'{name} mode {mode}: max (err - bound) {float((err - lim).max()):.3e}'
        if y8 is not None:
            t = np.clip(y_ref / np.float64(np.float32(s_out)), -448.0, 448.0)
            err8 = np.abs(f8.decode(y8) - t)
            lim8 = f8.e4m3_step(t) / 2 + Bd / s_out
            assert not np.isnan(err8).any() and np.all(err8 <= lim8), f'{name} mode {mode}: e4m3 out off by {float((err8 - lim8).max()):.3e}'
            assert f8.decode(y8).max() == 448.0 or np.abs(t).max() < 448.0
    return y_ref, worst


@pytest.mark.parametrize('case', REAL_CASES, ids=[c[0] for c in REAL_CASES])
def test_conv_real_valued(case, capsys):
    name, b, hi, wi, ci, co, k, stride, dil, padding, relu, _ = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ph, pw, ho, wo = conv_geom(hi, wi, k, stride, dil, padding)
    x = rng.normal(0, 1, (b, hi, wi, ci)).astype(np.float32)
    w = (rng.normal(0, 1, (k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.normal(0, 0.1, (co,)).astype(np.float32)
    s_in = float(np.float32(np.abs(x).max()) / np.float32(448.0))
    x8_ = u8(x.shape)
    check(lib.ssd_op_quantize_fp8(ptr(dev(x)), 1, x.size, s_in, ptr(x8_), None))
    w8_, s_ = gpu_quantize_filter(w)
    x8, w8, s_w = host(x8_), host(w8_), host(s_)
    assert np.array_equal(x8, f8.quantize(x, s_in))
    geom = (b, hi, wi, ci, ho, wo, co, k, k, stride, dil, ph, pw)
    modes = (f8.OUT_F32, f8.OUT_BF16, f8.OUT_E4M3, f8.OUT_BF16_E4M3) if name == FOUR_MODES_CASE else (f8.OUT_F32, f8.OUT_BF16)
    _, worst = check_real_layer(name, x8, w8, s_in, s_w, bias, geom, k, stride, dil, padding, relu, modes)
    with capsys.disabled():
        print(f'\n[fp8 conv] {name}: largest fp32-out error / B = {worst:.4f}')


@pytest.mark.parametrize('what', ['Ci=96', '25 taps', 'Co=20'])
def test_conv_refused_shapes_write_nothing(what):
    ci, co, k = (96, 64, 3) if what == 'Ci=96' else (64, 64, 5) if what == '25 taps' else (64, 20, 3)
    b, hi, wi = 1, 6, 6
    ph, pw, ho, wo = conv_geom(hi, wi, k, 1, 1, 'SAME')
    x8_, w8_ = u8((b, hi, wi, ci), 0x38), u8((k * k, co, ci), 0x38)
    y_ = torch.full((b, ho, wo, co), 9.0, dtype=torch.float32, device='cuda')
    y8_ = u8((b, ho, wo, co))
    rc = lib.ssd_op_conv2d_fwd_fp8(ptr(x8_), ptr(w8_), 1.0, ptr(dev(np.ones(co, np.float32))), None, ptr(y_), ptr(y8_), f8.OUT_F32, 1.0,
                                   b, hi, wi, ci, ho, wo, co, k, k, 1, 1, ph, pw, 1, None)
    assert rc != 0 and 'fp8 conv' in last_error()
    assert np.all(host(y_) == 9.0) and np.all(host(y8_) == 0xAB)


# ------------------------------------------------------------------------------------------------------------ pooling
POOL_CASES = [('pool3 75->38 ceil', 2, 75, 75, 64, 2, 2, False), ('mod_pool5 3x3 s1', 2, 19, 19, 128, 3, 1, False),
              ('negative codes 2x2', 1, 11, 13, 32, 2, 2, True), ('negative codes 3x3 s1', 1, 7, 9, 16, 3, 1, True)]


@pytest.mark.parametrize('case', POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_maxpool_fp8_bytes(case):
    name, b, hi, wi, c, k, stride, signed = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ok = [v for v in range(256) if v not in (0x7F, 0xFF, 0x80) and (signed or v < 0x80)]
    x8 = rng.choice(np.array(ok, np.uint8), size=(b, hi, wi, c))
    if signed:
        x8[0, :3, :3, :] = rng.choice(np.arange(0x81, 0xFF, dtype=np.uint8), size=(3, 3, c))      # windows that are all negative
    ph, ho = same_pad(hi, k, stride)
    pw, wo = same_pad(wi, k, stride)
    y8_ = u8((b, ho, wo, c))
    check(lib.ssd_op_maxpool_fwd_fp8(ptr(dev(x8)), ptr(y8_), b, hi, wi, c, ho, wo, k, stride, ph, pw, None))
    want = f8.maxpool_codes(x8, k, stride)
    assert want.shape == (b, ho, wo, c)
    assert np.array_equal(host(y8_), want)
    assert lib.ssd_op_maxpool_fwd_fp8(ptr(dev(x8)), ptr(y8_), b, hi, wi, 24, ho, wo, k, stride, ph, pw, None) != 0


# ------------------------------------------------------------------------------------------------------------ whole model
# the layers with at least 256 input channels (conv1_2 ... conv3_1 measured no faster than bf16 and stay there: DESIGN 18)
FP8_LAYERS = ['conv3_2', 'conv3_3', 'conv4_1', 'conv4_2', 'conv4_3', 'conv5_1', 'conv5_2', 'conv5_3', 'mod_conv6', 'mod_conv7']
FP8_SCALED = ['conv3_1'] + FP8_LAYERS[:-1]      # tensors that own a scale: conv3_1's output (quantised behind the bf16 layer) and the
                                                # e4m3 outputs of the fp8 layers (mod_conv7's output is bf16 only)
FP8_POOLS = ['pool3', 'pool4', 'mod_pool5']     # run on e4m3 bytes


@pytest.fixture(scope='module')
def model():
    from oracle import boxes as ob, ssdvgg_ref as ref
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    preset = ob.get_preset('vgg300')
    w = ref.init_params(preset, 20, seed=42, alive=True)
    b = 2
    x = ref.synth_images(np.random.default_rng(99), b, preset)
    sess = Session(0)
    nets = {}
    for dt in ('fp8', 'bf16', 'f32'):
        nets[dt] = SSDVGG(sess, 'vgg300')
        nets[dt].build_from_vgg(None, 20, max_batch=b, training=False, weights=w, dtype=dt)
    n8 = nets['fp8']
    assert n8.dtype == 'fp8' and list(n8.fp8_scales) == FP8_SCALED and all(v == 0.0 for v in n8.fp8_scales.values())
    with pytest.raises(RuntimeError, match='no activation scales'):
        n8.infer(x)                                       # an uncalibrated handle refuses
    n8.calibrate_fp8(x)
    res = {dt: nets[dt].infer(x) for dt in nets}
    yield dict(preset=preset, w=w, b=b, x=x, nets=nets, res=res, ref=ref)
    sess.close()


def codes_of(a, scale):
    """the e4m3 codes behind a dequantised activation (code * scale in fp32: the division gives the code's value back to 2 ulp)"""
    return f8.encode(np.asarray(a, np.float32) / np.float32(scale))


def test_model_fp8_layers_local(model, capsys):
    """every fp8 layer's output against the oracle applied to the kernel's OWN input codes, with the bounds of the op tests.  Maps
    higher than 40 rows are checked on three bands of rows (top border, middle, bottom border, every column and channel)."""
    ref, b, w, net = model['ref'], model['b'], model['w'], model['nets']['fp8']
    scales = net.fp8_scales
    assert all(v > 0 for v in scales.values())
    ops = {op[1]: op for op in ref.graph(model['preset']) if op[0] in ('conv', 'pool')}

    def scale_of(t):
        return scales[t] if t in scales else scale_of(ops[t][2])       # a pool's output shares its input's scale

    lines = []
    for name in FP8_LAYERS:
        _, _, src, k, stride, padding, dil = ops[name]
        assert stride == 1 and padding == 'SAME'
        s_in = scale_of(src)
        x8 = codes_of(net.activation(src, b), s_in)
        w8, s_w = f8.quantize_filter(w[name + '/filter'])
        bias = w[name + '/biases']
        H = x8.shape[1]
        bands = [(0, 5), (H // 2, H // 2 + 3), (H - 5, H)] if H > 40 else [(0, H)]
        got8 = net.activation(name, b) if name in scales else None
        got16 = net.activation(('bf16:' if name in scales else '') + name, b) if name in ('conv4_3', 'mod_conv7') else None
        worst8 = worst16 = 0.0
        for r0, r1 in bands:
            acc, absacc = f8.conv_codes_rows(x8, w8, k, dil, r0, r1)
            y_ref = f8.epilogue(acc, s_in, s_w, bias, True)
            Bd = f8.accumulation_bound(absacc, k * k * x8.shape[3], s_in, s_w)
            assert np.count_nonzero(y_ref) > 0.2 * y_ref.size, f'{name} is (nearly) dead: the test would prove nothing'
            if got8 is not None:
                s_out = np.float32(scales[name])
                t = np.clip(y_ref / np.float64(s_out), -448.0, 448.0)
                err = np.abs(f8.decode(codes_of(got8[:, r0:r1], s_out)) - t)
                lim = f8.e4m3_step(t) / 2 + Bd / np.float64(s_out)
                assert np.all(err <= lim), f'{name} rows {r0}:{r1}: e4m3 output off by {float((err - lim).max()):.3e} steps of scale'
                worst8 = max(worst8, float((err / lim).max()))
            if got16 is not None:
                err = np.abs(got16[:, r0:r1] - y_ref)
                lim = Bd + np.abs(y_ref) * 2.0 ** -8
                assert np.all(err <= lim), f'{name} rows {r0}:{r1}: bf16 output off by {float((err - lim).max()):.3e}'
                worst16 = max(worst16, float((err / np.maximum(lim, 1e-300)).max()))
        lines.append(f'{name}: worst error / bound: e4m3 out {worst8:.3f}, bf16 out {worst16:.3f} (0: no such output)')
    with capsys.disabled():
        print('\n[fp8 model] ' + '\n[fp8 model] '.join(lines))


def test_model_fp8_boundaries_and_pools(model):
    ref, b, nets = model['ref'], model['b'], model['nets']
    net, scales = nets['fp8'], nets['fp8'].fp8_scales
    # conv3_1: the bf16 handle's kernels up to here (pools fused as there), then the one stand-alone quantise pass
    c31 = net.activation('bf16:conv3_1', b)
    assert np.array_equal(c31, nets['bf16'].activation('conv3_1', b))
    want = (f8.decode(f8.quantize(c31, scales['conv3_1'])) * np.float64(np.float32(scales['conv3_1']))).astype(np.float32)
    assert np.array_equal(net.activation('conv3_1', b), want)
    # pools on e4m3 bytes: the maximum of the dequantised inputs, exactly
    ops = {op[1]: op for op in ref.graph(model['preset']) if op[0] == 'pool'}
    for name in FP8_POOLS:
        _, _, src, k, s = ops[name]
        a = torch.from_numpy(net.activation(src, b)).permute(0, 3, 1, 2)
        assert np.array_equal(net.activation(name, b), ref.maxpool_tf(a, k, s).permute(0, 2, 3, 1).numpy()), name
    with pytest.raises(RuntimeError, match='no bf16 form'):
        net.activation('bf16:conv3_2', b)


def test_model_fp8_untouched_layers_and_result(model, capsys):
    """conv8_1 onwards, the l2 norm and the heads are the bf16 handle's code: each against the bf16 oracle applied to the tensor it
    actually read (the bf16 form of conv4_3 and of mod_conv7's output), with test_gpu_bf16.py's tolerances"""
    from test_gpu_bf16 import layer_local_forward_check, TOL_BF
    from gpu_util import rel_err
    ref, b, nets, res = model['ref'], model['b'], model['nets'], model['res']
    net = nets['fp8']

    class Bf16View:
        def activation(self, name, n):
            return net.activation(('bf16:' if name in net.fp8_scales else '') + name, n)

    m = ref.RefModel('vgg300', params=model['w'])
    only = [op[1] for op in ref.graph(model['preset']) if op[0] == 'conv' and op[1] not in FP8_LAYERS + ['conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1']]
    only += ['l2_norm_conv4_3'] + ['heads/map%d' % i for i in range(6)]
    assert 'conv8_1' in only and 'conv11_2' in only
    assert layer_local_forward_check(Bf16View(), m, model['preset'], b, model['x'], only=only) < TOL_BF
    r8 = res['fp8']
    assert np.isfinite(r8).all() and np.abs(r8[..., :21].sum(-1) - 1).max() < 1e-4
    with capsys.disabled():
        print(f"\n[fp8 model] rel_err(result fp8, result bf16) = {rel_err(r8, res['bf16']):.4e}, "
              f"rel_err(result fp8, result fp32) = {rel_err(r8, res['f32']):.4e}, "
              f"rel_err(result bf16, result fp32) = {rel_err(res['bf16'], res['f32']):.4e}")


def test_fp8_lifecycle(model):
    from gpu_util import rel_err
    net, x, b = model['nets']['fp8'], model['x'], model['b']
    s0 = net.fp8_scales
    r0 = net.infer(x)
    # set / get round trip, and the scales are what inference uses
    doubled = {k: np.float32(v) * np.float32(2) for k, v in s0.items()}
    net.fp8_scales = doubled
    assert net.fp8_scales == {k: float(v) for k, v in doubled.items()}
    assert not np.array_equal(net.infer(x), r0)
    with pytest.raises(ValueError):
        net.fp8_scales = {k: v for k, v in list(s0.items())[1:]}
    with pytest.raises(RuntimeError, match='positive'):
        net.fp8_scales = dict(s0, conv3_1=0.0)
    net.fp8_scales = s0
    assert np.array_equal(net.infer(x), r0)                          # deterministic
    # accumulate only grows
    net.calibrate_fp8(x * 0.25, accumulate=True)
    s1 = net.fp8_scales
    assert all(s1[k] >= s0[k] for k in s0) and s1['conv3_1'] == s0['conv3_1']
    net.calibrate_fp8(x * 2, accumulate=True)
    s2 = net.fp8_scales
    assert all(s2[k] >= s1[k] for k in s0) and s2['conv3_1'] > s0['conv3_1']
    net.calibrate_fp8(x * 0.25)                                       # without accumulate the scales follow the batch down
    assert net.fp8_scales['conv3_1'] < s0['conv3_1']
    net.calibrate_fp8(x)
    assert net.fp8_scales == s0
    # the e4m3 filters follow the fp32 masters: mod_conv7's filter and bias times 3 -> its (relu) output times 3.  Not exactly:
    # 3 w / (3 s) is rounded again, so a code at a rounding boundary may move by one step and the bf16 output is rounded again
    # (2^-8); both are far below 2^-6 in the L2 norm, a stale filter would leave the output unchanged (distance 2/3)
    net.infer(x)                                                      # (the last pass was a calibration pass, on the bf16 kernels)
    y0 = net.activation('mod_conv7', b)
    w = model['w']
    net.load_variables({'mod_conv7/filter': w['mod_conv7/filter'] * 3, 'mod_conv7/biases': w['mod_conv7/biases'] * 3})
    net.infer(x)
    y1 = net.activation('mod_conv7', b)
    assert np.count_nonzero(y0) > 0.2 * y0.size and rel_err(y1, 3 * y0) < 2.0 ** -6
    net.load_variables({'mod_conv7/filter': w['mod_conv7/filter'], 'mod_conv7/biases': w['mod_conv7/biases']})
    assert np.array_equal(net.infer(x), r0)


def test_detect_tool_fp8_child_process(tmp_path):
    """detect.py --dtype fp8 on three small images: calibrates on them, writes the detections and the scales; a second run loads
    the scales and writes the same detections"""
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
    cal = str(tmp_path / 'scales.npz')
    outs = []
    for run in range(2):
        odir = str(tmp_path / ('out%d' % run))
        r = subprocess.run([sys.executable, '-m', 'ssd_tensorflow_amd.detect', '--model', model_file, '--output-dir', odir, '--batch-size', '2',
                            '--dtype', 'fp8', '--fp8-calibration', cal] + files, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ('calibrated on the first 3 inputs' if run == 0 else 'loaded from') in r.stdout
        assert os.path.exists(cal)
        outs.append([open(os.path.join(odir, os.path.basename(f) + '.txt')).read() for f in files])
    with np.load(cal) as f:
        assert sorted(f.files) == sorted(FP8_SCALED) and all(float(f[k]) > 0 for k in f.files)
    assert outs[0] == outs[1]
