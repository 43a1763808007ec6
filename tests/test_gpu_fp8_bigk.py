"""-m gpu: fp8 (e4m3) convolutions with more than 9 taps (ssd_op_conv2d_fwd_fp8_bigk) and the fc graph's fp8 handle
with its 7x7 fc6 on e4m3 (SSD_FP8_BIGK=1), against tests/fp8_ref.py with the rules and bounds of test_gpu_fp8.py.

The layout cases are the smallest shapes at which each mechanism of the kernel can fail: the computed tap offsets (dilation,
stride, kh != kw), the separable validity mask (every pixel with taps outside the image, a map smaller than the kernel, the
121-tap limit), the chunk / tap loop order (two channel chunks) and the tile edges (Co = 136 and 8, M = 361)."""
import numpy as np
import pytest
import torch

import fc_ref
import fp8_ref as f8
import test_gpu_fp8 as t8
from gpu_util import lib, check, dev, ptr, host, rel_err
from ssd_tensorflow_amd._lib import last_error

pytestmark = pytest.mark.gpu


geom2 = t8.geom2      # gpu_util.conv_geom with kh and kw apart: (pad_h, pad_w, ho, wo)


def run_conv_bigk(x8, w8, s_in, s_w, bias, geom, mode, s_out, relu):
    """test_gpu_fp8.run_conv on the entry point for more than 9 taps"""
    b, hi, wi, ci, ho, wo, co = geom[:7]
    x_ = x8 if torch.is_tensor(x8) else dev(x8)
    w_ = w8 if torch.is_tensor(w8) else dev(w8)
    s_ = s_w if torch.is_tensor(s_w) else dev(np.asarray(s_w, np.float32))
    y_ = None if mode == f8.OUT_E4M3 else torch.full((b, ho, wo, co), 9.0, dtype=torch.float32 if mode == f8.OUT_F32 else torch.bfloat16, device='cuda')
    y8_ = t8.u8((b, ho, wo, co)) if mode in (f8.OUT_E4M3, f8.OUT_BF16_E4M3) else None
    check(lib.ssd_op_conv2d_fwd_fp8_bigk(ptr(x_), ptr(w_), s_in, ptr(s_), ptr(dev(bias)), ptr(y_), ptr(y8_), mode, s_out, *geom, int(relu), None))
    torch.cuda.synchronize()
    return (None if y_ is None else y_.float().cpu().numpy()), (None if y8_ is None else y8_.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------ layout, exact
#               name                                    b  hi  wi  ci   co  kh  kw  stride dil padding
LAYOUT_CASES = [('7x7 SAME 64->64 2x9x8',               2,  9,  8, 64,  64,  7,  7, 1, 1, 'SAME'),
                ('7x7 SAME 128->136 1x5x5',             1,  5,  5, 128, 136, 7,  7, 1, 1, 'SAME'),
                ('5x5 dil2 SAME 64->8 1x11x7',          1, 11,  7, 64,  8,   5,  5, 1, 2, 'SAME'),
                ('3x5 VALID stride2 64->64 1x9x12',     1,  9, 12, 64,  64,  3,  5, 2, 1, 'VALID'),
                ('11x11 SAME 64->64 1x6x6',             1,  6,  6, 64,  64, 11, 11, 1, 1, 'SAME'),
                ('7x7 SAME 64->64 1x19x19',             1, 19, 19, 64,  64,  7,  7, 1, 1, 'SAME')]
_LAYOUT = {}


def layout_data(case):
    """(x8, w8, bias, want, geom) of a layout case: small integers, asymmetric in pixel, channel, kernel row, kernel column and
    output channel; all scales 1.  x in 0 ... 7, w in -2 ... 2: every sum is an integer below 121 * 128 * 14 < 2^24.  Computed once."""
    if case[0] not in _LAYOUT:
        name, b, hi, wi, ci, co, kh, kw, stride, dil, padding = case
        ph, pw, ho, wo = geom2(hi, wi, kh, kw, stride, dil, padding)
        B, H, W, Cc = np.meshgrid(np.arange(b), np.arange(hi), np.arange(wi), np.arange(ci), indexing='ij')
        xv = (3 * B + 5 * H + 7 * W + 11 * Cc + (H * W) % 3 + (Cc * W) % 5 + (Cc // 16)) % 8
        KH, KW, CI, CO = np.meshgrid(np.arange(kh), np.arange(kw), np.arange(ci), np.arange(co), indexing='ij')
        wv = (2 * KH + 3 * KW + CI + 7 * CO + (CI * CO) % 3 + (KH * CI) % 2 + (KH * KW) % 3 + (KW * CO) % 2 + (CI // 32)) % 5 - 2
        x8 = f8.encode(xv.astype(np.float64))
        w8 = np.ascontiguousarray(np.transpose(f8.encode(wv.astype(np.float64)).reshape(kh * kw, ci, co), (0, 2, 1)))
        bias = ((np.arange(co) * 5) % 17 - 8).astype(np.float32)
        acc, _ = f8.conv_codes(x8, w8, kh, kw, stride, dil, padding)
        want = acc + bias
        assert want.shape == (b, ho, wo, co)
        assert np.abs(want).max() < 2 ** 24 and len(np.unique(want)) > 50
        _LAYOUT[case[0]] = (x8, w8, bias, want, (b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, ph, pw))
    return _LAYOUT[case[0]]


@pytest.mark.parametrize('tile', ['0', '1'], ids=['128x128', '64x64'])
@pytest.mark.parametrize('case', LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_bigk_layout_exact(case, tile, monkeypatch):
    monkeypatch.setenv('SSD_TILE_FP8', tile)
    x8, w8, bias, want, geom = layout_data(case)
    co = geom[6]
    y, _ = run_conv_bigk(x8, w8, 1.0, np.ones(co), bias, geom, f8.OUT_F32, 0.0, False)
    assert np.array_equal(y, want.astype(np.float32)), f'{case[0]}: {np.argwhere(y != want)[:4]}'
    y, y8 = run_conv_bigk(x8, w8, 1.0, np.ones(co), bias, geom, f8.OUT_BF16_E4M3, 1.0, True)
    assert np.array_equal(y, t8.bf16_round(np.maximum(want, 0)))
    assert np.array_equal(y8, f8.encode(np.maximum(want, 0)))          # one rounding of an exact value, saturating at 448


# ------------------------------------------------------------------------------------------------------------ real-valued
def test_bigk_real_valued(monkeypatch, capsys):
    """7x7 SAME 512->256 on 1x19x19 (K = 25 088), x and w through the GPU quantisers: all four output modes within
    B = K * 2^-23 * (s_in * s_w[co]) * sum |x_code * w_code| by test_gpu_fp8.check_real_layer's rules"""
    name, b, hi, wi, ci, co, k = '7x7 SAME 512->256 1x19x19', 1, 19, 19, 512, 256, 7
    rng = np.random.default_rng(1907)
    ph, pw, ho, wo = geom2(hi, wi, k, k, 1, 1, 'SAME')
    x = rng.normal(0, 1, (b, hi, wi, ci)).astype(np.float32)
    w = (rng.normal(0, 1, (k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.normal(0, 0.1, (co,)).astype(np.float32)
    s_in = float(np.float32(np.abs(x).max()) / np.float32(448.0))
    x8_ = t8.u8(x.shape)
    check(lib.ssd_op_quantize_fp8(ptr(dev(x)), 1, x.size, s_in, ptr(x8_), None))
    w8_, s_ = t8.gpu_quantize_filter(w)
    x8, w8, s_w = host(x8_), host(w8_), host(s_)
    assert np.array_equal(x8, f8.quantize(x, s_in))
    geom = (b, hi, wi, ci, ho, wo, co, k, k, 1, 1, ph, pw)
    monkeypatch.setattr(t8, 'run_conv', run_conv_bigk)      # check_real_layer's rules, on this entry point
    modes = (f8.OUT_F32, f8.OUT_BF16, f8.OUT_E4M3, f8.OUT_BF16_E4M3)
    _, worst = t8.check_real_layer(name, x8, w8, s_in, s_w, bias, geom, k, 1, 1, 'SAME', True, modes)
    with capsys.disabled():
        print(f'\n[fp8 bigk conv] {name}: largest fp32-out error / B = {worst:.4f}')


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('what', ['9 taps', '13x13', 'Ci=96', 'Co=20'])
def test_bigk_refused_shapes_write_nothing(what):
    ci, co, k = {'9 taps': (64, 64, 3), '13x13': (64, 64, 13), 'Ci=96': (96, 64, 7), 'Co=20': (64, 20, 7)}[what]
    b, hi, wi = 1, 6, 6
    ph, pw, ho, wo = geom2(hi, wi, k, k, 1, 1, 'SAME')
    x8_, w8_ = t8.u8((b, hi, wi, ci), 0x38), t8.u8((k * k, co, ci), 0x38)
    y_ = torch.full((b, ho, wo, co), 9.0, dtype=torch.float32, device='cuda')
    y8_ = t8.u8((b, ho, wo, co))
    rc = lib.ssd_op_conv2d_fwd_fp8_bigk(ptr(x8_), ptr(w8_), 1.0, ptr(dev(np.ones(co, np.float32))), None, ptr(y_), ptr(y8_), f8.OUT_F32, 1.0,
                                        b, hi, wi, ci, ho, wo, co, k, k, 1, 1, ph, pw, 1, None)
    assert rc != 0 and 'fp8 conv' in last_error()
    if what == '9 taps':
        assert 'ssd_op_conv2d_fwd_fp8' in last_error()      # names the entry point that runs it
    assert np.all(host(y_) == 9.0) and np.all(host(y8_) == 0xAB)


# ------------------------------------------------------------------------------------------------------------ filter quantiser
QUANT_CASES = [('49 taps 64->40', 7, 7, 64, 40),            # the issue's case: one ragged 64 x 64 tile of the row-split quantiser
               ('25 taps 128->136', 5, 5, 128, 136),        # two ci tiles, three co tiles with an 8-wide remainder
               ('49 taps 64->42', 7, 7, 64, 42),            # Co no multiple of 4: the table-driven kernel at 49 taps
               ('77 taps 64->8', 7, 11, 64, 8)]             # 4928 rows: more than one row per lane of an absmax slice


@pytest.mark.parametrize('case', QUANT_CASES, ids=[c[0] for c in QUANT_CASES])
def test_quantize_filter_many_taps_bit_exact(case):
    name, kh, kw, ci, co = case
    rng = np.random.default_rng(49)
    w = (rng.normal(0, 1, (kh, kw, ci, co)) / 56).astype(np.float32)
    w[..., 3] = 0                                     # an all-zero output channel: scale 1, codes 0
    w[kh - 1, kw - 1, ci - 1, co - 1] = -2.5          # the last tap, input and output channel carries its channel's absmax
    w8_, s_ = t8.gpu_quantize_filter(w)
    codes, s = f8.quantize_filter(w)
    assert codes.shape == (kh * kw, co, ci)
    assert np.array_equal(host(s_).view(np.uint32), s.view(np.uint32))
    assert host(s_)[3] == 1.0 and host(s_)[co - 1] == np.float32(2.5) / np.float32(448.0)
    assert np.array_equal(host(w8_), codes)
    assert host(w8_)[kh * kw - 1, co - 1, ci - 1] == 0xFE


# ------------------------------------------------------------------------------------------------------------ whole fc model
CHECKED = np.r_[0:32, 2032:2064, 4064:4096]      # fc6 / fc7 output channels under the float64 oracle: both ends and a tile boundary
A_TROUS_SCALED = t8.FP8_SCALED                   # the a-trous handle's list: conv3_1 ... mod_conv6


def build_fc(sess, w, dtype, bigk, b=1):
    """an fc-graph inference handle created under SSD_FP8_BIGK = bigk (read when the handle is created)"""
    from ssd_tensorflow_amd.ssdvgg import SSDVGG
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('SSD_FP8_BIGK', bigk)
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 20, a_trous=False, max_batch=b, training=False, weights=w, dtype=dtype)
    return net


@pytest.fixture(scope='module')
def fc_model():
    from oracle import boxes as ob, ssdvgg_ref as ref
    from ssd_tensorflow_amd.ssdvgg import Session
    preset = ob.get_preset('vgg300')
    w = fc_ref.init_params(preset, 20, seed=42)
    x = ref.synth_images(np.random.default_rng(99), 1, preset)
    sess = Session(0)
    nets = {'fp8': build_fc(sess, w, 'fp8', '1'), 'bf16': build_fc(sess, w, 'bf16', '1')}
    nets['fp8'].calibrate_fp8(x)
    res = {dt: nets[dt].infer(x) for dt in nets}
    yield dict(preset=preset, w=w, x=x, nets=nets, res=res, ref=ref, sess=sess)
    sess.close()


def test_fc_model_plan(fc_model):
    """fc6 on e4m3: conv5_3's output and fc6's own own a scale, mod_pool5 runs on bytes, no bf16 form of fc6's output is left"""
    net, ref = fc_model['nets']['fp8'], fc_model['ref']
    scales = net.fp8_scales
    assert list(scales) == A_TROUS_SCALED and 'conv5_3' in scales and 'mod_conv6' in scales
    assert all(v > 0 for v in scales.values())
    a = torch.from_numpy(net.activation('conv5_3', 1)).permute(0, 3, 1, 2)
    assert np.array_equal(net.activation('mod_pool5', 1), ref.maxpool_tf(a, 3, 1).permute(0, 2, 3, 1).numpy())
    with pytest.raises(RuntimeError, match='no bf16 form'):
        net.activation('bf16:mod_conv6', 1)           # the quantise pass behind fc6 is gone: the epilogue writes e4m3 only
    with pytest.raises(RuntimeError, match='no bf16 form'):
        net.activation('bf16:mod_pool5', 1)


def test_fc_model_fc6_fc7_local(fc_model, capsys):
    """mod_conv6 (7x7, e4m3 out at fc7's input scale) and mod_conv7 (1x1, bf16 out) against the oracle applied to the kernels' OWN
    input codes: every pixel, the output channels CHECKED (a per-channel filter scale makes a channel subset exact)"""
    net, w = fc_model['nets']['fp8'], fc_model['w']
    scales = net.fp8_scales
    lines = []
    for name, var, src, s_in, k in (('mod_conv6', 'fc6', 'mod_pool5', scales['conv5_3'], 7), ('mod_conv7', 'fc7', 'mod_conv6', scales['mod_conv6'], 1)):
        x8 = t8.codes_of(net.activation(src, 1), s_in)
        w8, s_w = f8.quantize_filter(w[var + '/weights'][..., CHECKED])
        bias = w[var + '/biases'][CHECKED]
        acc, absacc = f8.conv_codes(x8, w8, k, k, 1, 1, 'SAME')
        y_ref = f8.epilogue(acc, s_in, s_w, bias, True)
        Bd = f8.accumulation_bound(absacc, k * k * x8.shape[3], s_in, s_w)
        for blk in range(3):
            part = y_ref[..., 32 * blk:32 * blk + 32]
            assert np.count_nonzero(part) > 0.2 * part.size, f'{name} channels {CHECKED[32 * blk]}.. are (nearly) dead: the test would prove nothing'
        if name == 'mod_conv6':
            s_out = np.float32(scales[name])
            t = np.clip(y_ref / np.float64(s_out), -448.0, 448.0)
            err = np.abs(f8.decode(t8.codes_of(net.activation(name, 1)[..., CHECKED], s_out)) - t)
            lim = f8.e4m3_step(t) / 2 + Bd / np.float64(s_out)
            assert np.all(err <= lim), f'{name}: e4m3 output off by {float((err - lim).max()):.3e} steps of scale'
        else:
            assert name not in scales                  # bf16 only: conv8_1 and the 4096-wide head of map 1 read it
            err = np.abs(net.activation(name, 1)[..., CHECKED] - y_ref)
            lim = Bd + np.abs(y_ref) * 2.0 ** -8
            assert np.all(err <= lim), f'{name}: bf16 output off by {float((err - lim).max()):.3e}'
        lines.append(f'{name}: worst error / bound {float((err / np.maximum(lim, 1e-300)).max()):.3f}')
    with capsys.disabled():
        print('\n[fp8 fc model] ' + '\n[fp8 fc model] '.join(lines))


def test_fc_model_result(fc_model, capsys):
    r8, r16 = fc_model['res']['fp8'], fc_model['res']['bf16']
    assert np.isfinite(r8).all() and np.abs(r8[..., :21].sum(-1) - 1).max() < 1e-4
    with capsys.disabled():
        print(f'\n[fp8 fc model] rel_err(result fp8, result bf16) = {rel_err(r8, r16):.4e}')


def test_fc_model_parents_plan(fc_model):
    """SSD_FP8_BIGK=0: fc6 stays on the bf16 kernel, conv5_3's output is bf16 only and a quantise pass behind fc6 feeds fc7"""
    net = build_fc(fc_model['sess'], fc_model['w'], 'fp8', '0')
    names = list(net.fp8_scales)
    assert 'conv5_3' not in names and 'mod_conv6' in names and 'conv5_2' in names
    net.calibrate_fp8(fc_model['x'])
    r = net.infer(fc_model['x'])
    assert np.isfinite(r).all()
    a16 = net.activation('bf16:mod_conv6', 1)
    s = net.fp8_scales['mod_conv6']
    want = (f8.decode(f8.quantize(a16, s)) * np.float64(np.float32(s))).astype(np.float32)
    assert np.array_equal(net.activation('mod_conv6', 1), want)
    with pytest.raises(ValueError, match='conv5_3'):      # scales of the other plan are refused, and the message names what is expected
        net.fp8_scales = fc_model['nets']['fp8'].fp8_scales
