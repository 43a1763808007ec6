"""-m gpu: mxfp8 convolutions with more than 9 taps (ssd_op_conv2d_fwd_mxfp8_bigk) and the fc graph's mxfp8 handle with
its 7x7 fc6 on MX operands (SSD_MXFP8_BIGK=1), against tests/mxfp8_ref.py with the rules and bounds of test_gpu_mxfp8.py.

The layout cases are test_gpu_fp8_bigk.py's (computed tap offsets, the separable validity mask, the chunk / tap loop order, the tile
edges) with block scales that vary with pixel and 32-channel block, plus the shapes at which the scale dword's byte selection can go
wrong: an image whose scales start between two dwords, 6 scale bytes per pixel, two channel chunks, a scale buffer handed over 2 bytes
past a dword boundary."""
import numpy as np
import pytest
import torch

import fc_ref
import fp8_ref as f8
import mxfp8_ref as mx
import test_gpu_mxfp8 as tmx
from gpu_util import lib, check, dev, ptr, host, rel_err
from ssd_tensorflow_amd._lib import last_error
from test_gpu_fp8 import bf16_round, u8, gpu_quantize_filter
from test_gpu_fp8_bigk import LAYOUT_CASES as FP8_BIGK_CASES, CHECKED, geom2

pytestmark = pytest.mark.gpu


def run_conv_bigk(x8, xs, w8, s_w, bias, geom, mode, relu, xs_dev=None):
    """test_gpu_mxfp8.run_conv on the entry point for more than 9 taps; xs_dev: a device pointer to the scales instead of xs"""
    b, hi, wi, ci, ho, wo, co = geom[:7]
    x_, w_, s_ = dev(x8), (w8 if torch.is_tensor(w8) else dev(w8)), (s_w if torch.is_tensor(s_w) else dev(np.asarray(s_w, np.float32)))
    xs_ = None if xs_dev is not None else dev(xs)
    wants8 = mode in (mx.OUT_MX, mx.OUT_BF16_MX)
    y_ = None if mode == mx.OUT_MX else torch.full((b, ho, wo, co), 9.0, dtype=torch.float32 if mode == mx.OUT_F32 else torch.bfloat16, device='cuda')
    y8_ = u8((b, ho, wo, co)) if wants8 else None
    ys_ = u8((b, ho, wo, co // 32)) if wants8 else None
    check(lib.ssd_op_conv2d_fwd_mxfp8_bigk(ptr(x_), xs_dev if xs_dev is not None else ptr(xs_), ptr(w_), ptr(s_), ptr(dev(bias)), ptr(y_), ptr(y8_),
                                           ptr(ys_), mode, *geom, int(relu), None))
    torch.cuda.synchronize()
    return (None if y_ is None else y_.float().cpu().numpy()), (y8_.cpu().numpy() if wants8 else None), (ys_.cpu().numpy() if wants8 else None)


# ------------------------------------------------------------------------------------------------------------ layout, exact
#               name                                    b  hi  wi  ci   co  kh  kw  stride dil padding
LAYOUT_CASES = [FP8_BIGK_CASES[0],                                                                           # 7x7 SAME 64->64 2x9x8
                ('7x7 SAME 64->64 2x5x5',               2,  5,  5, 64,  64,  7,  7, 1, 1, 'SAME'),           # 50 scale bytes per image: image 1's start between two dwords
                FP8_BIGK_CASES[1],                                                                           # 7x7 SAME 128->136 1x5x5: two chunks (2 cc), ragged Co, no MX output
                ('7x7 SAME 192->32 2x5x3',              2,  5,  3, 192, 32,  7,  7, 1, 1, 'SAME'),           # 6 scale bytes per pixel; the smallest MX output
                FP8_BIGK_CASES[2], FP8_BIGK_CASES[3], FP8_BIGK_CASES[4], FP8_BIGK_CASES[5]]
assert [c[0] for c in LAYOUT_CASES[4:]] == ['5x5 dil2 SAME 64->8 1x11x7', '3x5 VALID stride2 64->64 1x9x12', '11x11 SAME 64->64 1x6x6', '7x7 SAME 64->64 1x19x19']
_LAYOUT = {}


def layout_data(case):
    """(x8, xs, w8, bias, want, geom) of a layout case.  Activations i * 2^s, i in 0 ... 7 and s in -2 ... 2 varying with pixel and
    32-channel block (test_gpu_mxfp8.test_conv_layout_exact's), filter codes in -2 ... 2 by test_gpu_fp8_bigk.layout_data's formula
    (asymmetric in kernel row and column), integer bias: every sum is a multiple of 1/4 far below 2^22, exact in any order.  Once."""
    if case[0] not in _LAYOUT:
        name, b, hi, wi, ci, co, kh, kw, stride, dil, padding = case
        ph, pw, ho, wo = geom2(hi, wi, kh, kw, stride, dil, padding)
        B, H, W, Cc = np.meshgrid(np.arange(b), np.arange(hi), np.arange(wi), np.arange(ci), indexing='ij')
        iv = (3 * B + 5 * H + 7 * W + 11 * Cc + (H * W) % 3 + (Cc * W) % 5 + (Cc // 16)) % 8
        sv = (2 * B + 3 * H + W + 2 * (Cc // 32) + (H * (Cc // 32)) % 3) % 5 - 2
        xv = np.ldexp(iv.astype(np.float32), sv).astype(np.float32)
        x8, xs = mx.quantize(xv)
        assert np.array_equal(mx.dequantize(x8, xs), xv.astype(np.float64)) and len(np.unique(xs)) >= 5      # lossless; scales vary
        KH, KW, CI, CO = np.meshgrid(np.arange(kh), np.arange(kw), np.arange(ci), np.arange(co), indexing='ij')
        wv = (2 * KH + 3 * KW + CI + 7 * CO + (CI * CO) % 3 + (KH * CI) % 2 + (KH * KW) % 3 + (KW * CO) % 2 + (CI // 32)) % 5 - 2
        w8 = np.ascontiguousarray(np.transpose(f8.encode(wv.astype(np.float64)).reshape(kh * kw, ci, co), (0, 2, 1)))
        bias = ((np.arange(co) * 5) % 17 - 8).astype(np.float32)
        acc, absacc = mx.conv_values(xv, w8, kh, kw, stride, dil, padding)
        want = acc + bias
        assert want.shape == (b, ho, wo, co)
        assert absacc.max() + 8 < 2 ** 22 and np.array_equal(want * 4, np.round(want * 4)) and len(np.unique(want)) > 50
        _LAYOUT[case[0]] = (x8, xs, w8, bias, want, (b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, ph, pw))
    return _LAYOUT[case[0]]


def check_layout(case, xs_dev_of=None):
    x8, xs, w8, bias, want, geom = layout_data(case)
    co = geom[6]
    kw = {} if xs_dev_of is None else {'xs_dev': xs_dev_of(xs)}
    y, _, _ = run_conv_bigk(x8, xs, w8, np.ones(co), bias, geom, mx.OUT_F32, False, **kw)
    assert np.array_equal(y, want.astype(np.float32)), f'{case[0]}: {np.argwhere(y != want)[:4]}'
    pos = np.maximum(want, 0).astype(np.float32)
    if co % 32:                                  # no MX output for this Co: the bf16 form alone
        y, _, _ = run_conv_bigk(x8, xs, w8, np.ones(co), bias, geom, mx.OUT_BF16, True, **kw)
        assert np.array_equal(y, bf16_round(pos))
        return
    y, y8, ys = run_conv_bigk(x8, xs, w8, np.ones(co), bias, geom, mx.OUT_BF16_MX, True, **kw)
    assert np.array_equal(y, bf16_round(pos))
    want8, wants = mx.quantize(pos)
    assert np.array_equal(ys, wants) and np.array_equal(y8, want8)


@pytest.mark.parametrize('tile', ['0', '1'], ids=['128x128', '64x64'])
@pytest.mark.parametrize('case', LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_bigk_layout_exact(case, tile, monkeypatch):
    monkeypatch.setenv('SSD_TILE_FP8', tile)
    check_layout(case)


@pytest.mark.parametrize('tile', ['0', '1'], ids=['128x128', '64x64'])
def test_bigk_layout_exact_scales_between_dwords(tile, monkeypatch):
    """the first case with the scale buffer handed over 2 bytes past a dword boundary (sc_delta = 2), inside an allocation with 2
    bytes in front of it and 8 behind: the same bytes"""
    monkeypatch.setenv('SSD_TILE_FP8', tile)
    keep = []

    def shifted(xs):
        buf = u8((2 + xs.size + 8,), 0x7F)
        buf[2:2 + xs.size] = dev(xs.reshape(-1))
        assert buf.data_ptr() % 4 == 0
        keep.append(buf)
        return buf.data_ptr() + 2

    check_layout(LAYOUT_CASES[0], shifted)


# ------------------------------------------------------------------------------------------------------------ real-valued
def test_bigk_real_valued(monkeypatch, capsys):
    """7x7 SAME 512->256 on 1x19x19 (K = 25 088; six pixel tiles x four filter columns at 64 x 64), x = normal * 2^integers(-3, 4) per
    block through ssd_op_quantize_mxfp8 and the GPU filter quantiser: all four output modes by test_gpu_mxfp8.check_real_layer's rules"""
    name, b, hi, wi, ci, co, k = '7x7 SAME 512->256 1x19x19', 1, 19, 19, 512, 256, 7
    rng = np.random.default_rng(1907)
    ph, pw, ho, wo = geom2(hi, wi, k, k, 1, 1, 'SAME')
    x = (rng.normal(0, 1, (b, hi, wi, ci)) * np.exp2(rng.integers(-3, 4, (b, hi, wi, ci // 32)).repeat(32, -1))).astype(np.float32)
    w = (rng.normal(0, 1, (k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.normal(0, 0.1, (co,)).astype(np.float32)
    x8, xs = tmx.gpu_quantize(x.reshape(-1, ci), True)                # (bytes pinned by test_gpu_mxfp8.test_quantize_bit_exact)
    x8, xs = x8.reshape(b, hi, wi, ci), xs.reshape(b, hi, wi, ci // 32)
    w8_, s_ = gpu_quantize_filter(w)
    geom = (b, hi, wi, ci, ho, wo, co, k, k, 1, 1, ph, pw)
    monkeypatch.setattr(tmx, 'run_conv', run_conv_bigk)               # check_real_layer's rules, on this entry point
    with capsys.disabled():
        worst = tmx.check_real_layer(name, mx.dequantize(x8, xs), x8, xs, host(w8_), host(s_), bias, geom, k, 1, 1, 'SAME', True, True)
        print(f'\n[mxfp8 bigk conv] {name}: largest fp32-out error / B = {worst:.4f}')


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('what', ['9 taps', '13x13', 'Ci=96', 'Co=20', 'MX out Co=40', 'null scales'])
def test_bigk_refused_shapes_write_nothing(what):
    ci, co, k = {'9 taps': (64, 64, 3), '13x13': (64, 64, 13), 'Ci=96': (96, 64, 7), 'Co=20': (64, 20, 7), 'MX out Co=40': (64, 40, 7),
                 'null scales': (64, 64, 7)}[what]
    mode = mx.OUT_BF16_MX if what == 'MX out Co=40' else mx.OUT_F32
    b, hi, wi = 1, 6, 6
    ph, pw, ho, wo = geom2(hi, wi, k, k, 1, 1, 'SAME')
    x8_, xs_, w8_ = u8((b, hi, wi, ci), 0x38), u8((b, hi, wi, ci // 32 + 2), 0x7F), u8((k * k, co, ci), 0x38)
    y_ = torch.full((b, ho, wo, co), 9.0, dtype=torch.float32, device='cuda')
    y8_, ys_ = u8((b, ho, wo, co)), u8((b, ho, wo, co // 32 + 1))
    rc = lib.ssd_op_conv2d_fwd_mxfp8_bigk(ptr(x8_), None if what == 'null scales' else ptr(xs_), ptr(w8_), ptr(dev(np.ones(co, np.float32))), None,
                                          ptr(y_), ptr(y8_), ptr(ys_), mode, b, hi, wi, ci, ho, wo, co, k, k, 1, 1, ph, pw, 1, None)
    assert rc != 0 and 'mxfp8 conv' in last_error()
    if what == '9 taps':
        assert 'ssd_op_conv2d_fwd_mxfp8' in last_error()      # names the entry point that runs it
    assert np.all(host(y_) == 9.0) and np.all(host(y8_) == 0xAB) and np.all(host(ys_) == 0xAB)


# ------------------------------------------------------------------------------------------------------------ whole fc model
def build_net(sess, preset_name, w, dtype, a_trous, switch, fp8_bigk='1', b=1):
    """an inference handle created under SSD_MXFP8_BIGK = switch (None: unset) and SSD_FP8_BIGK = fp8_bigk: both are read when the
    handle is created"""
    from ssd_tensorflow_amd.ssdvgg import SSDVGG
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('SSD_FP8_BIGK', fp8_bigk)
        if switch is None:
            mp.delenv('SSD_MXFP8_BIGK', raising=False)
        else:
            mp.setenv('SSD_MXFP8_BIGK', switch)
        net = SSDVGG(sess, preset_name)
        net.build_from_vgg(None, 20, a_trous=a_trous, max_batch=b, training=False, weights=w, dtype=dtype)
    return net


@pytest.fixture(scope='module')
def fc_model():
    from oracle import boxes as ob, ssdvgg_ref as ref
    from ssd_tensorflow_amd.ssdvgg import Session
    preset = ob.get_preset('vgg300')
    w = fc_ref.init_params(preset, 20, seed=42)
    x = ref.synth_images(np.random.default_rng(99), 1, preset)
    sess = Session(0)
    nets = {'bf16': build_net(sess, 'vgg300', w, 'bf16', False, None), 'fp8': build_net(sess, 'vgg300', w, 'fp8', False, None),
            'mx0': build_net(sess, 'vgg300', w, 'mxfp8', False, '0'), 'mx1': build_net(sess, 'vgg300', w, 'mxfp8', False, '1')}
    nets['fp8'].calibrate_fp8(x)
    res = {k: nets[k].infer(x) for k in nets}
    yield dict(preset=preset, w=w, x=x, nets=nets, res=res, ref=ref, sess=sess)
    sess.close()


def test_fc_model_plan(fc_model):
    """fc6 on MX operands: conv5_3, mod_pool5 and fc6 itself are MX only, mod_conv7 is bf16 only, the pool is the MX pool"""
    net = fc_model['nets']['mx1']
    got = {n: tmx.mx_codes(net, n, 1) for n in ('conv5_3', 'mod_pool5', 'mod_conv6')}      # 'scale:<name>' exists for each
    for n in got:
        with pytest.raises(RuntimeError, match='no bf16 form'):
            net.activation('bf16:' + n, 1)
    with pytest.raises(RuntimeError, match='no block scales'):
        net.activation('scale:mod_conv7', 1)
    want8, wants = mx.maxpool(got['conv5_3'][1], got['conv5_3'][2], 3, 1)
    assert np.array_equal(got['mod_pool5'][2], wants) and np.array_equal(got['mod_pool5'][1], want8)


def test_fc_model_fc6_fc7_local(fc_model, capsys):
    """mod_conv6 (7x7, MX out) and mod_conv7 (1x1, bf16 out) against the oracle applied to the kernels' OWN input (codes and scales):
    every pixel, the output channels CHECKED, with test_gpu_mxfp8.test_model_mx_layers_local's limits"""
    net, w = fc_model['nets']['mx1'], fc_model['w']
    lines = []
    for name, var, src, k in (('mod_conv6', 'fc6', 'mod_pool5', 7), ('mod_conv7', 'fc7', 'mod_conv6', 1)):
        xv, _, _ = tmx.mx_codes(net, src, 1)
        w8, s_w = f8.quantize_filter(w[var + '/weights'][..., CHECKED])
        acc, absacc = mx.conv_values(xv, w8, k, k, 1, 1, 'SAME')
        y_ref = mx.epilogue(acc, s_w, w[var + '/biases'][CHECKED], True)
        Bd = mx.accumulation_bound(absacc, k * k * xv.shape[3], s_w)
        for blk in range(3):
            part = y_ref[..., 32 * blk:32 * blk + 32]
            assert np.count_nonzero(part) > 0.2 * part.size, f'{name} channels {CHECKED[32 * blk]}.. are (nearly) dead: the test would prove nothing'
        if name == 'mod_conv6':
            a, codes, sb = tmx.mx_codes(net, name, 1)
            tmx.check_scales_follow_rule(name, a, codes, sb)
            sv = np.repeat(mx.scale_values(sb), 32, -1)[..., CHECKED]
            err = np.abs(a[..., CHECKED] - y_ref)
            lim = Bd + sv * f8.e4m3_step(y_ref / sv) / 2          # one e4m3 rounding at the block's scale
            assert np.all(err <= lim), f'{name}: MX output off by {float((err - lim).max()):.3e}'
        else:
            err = np.abs(net.activation(name, 1)[..., CHECKED] - y_ref)
            lim = Bd + np.abs(y_ref) * 2.0 ** -8
            assert np.all(err <= lim), f'{name}: bf16 output off by {float((err - lim).max()):.3e}'
        lines.append(f'{name}: worst error / bound {float((err / np.maximum(lim, 1e-300)).max()):.3f}')
    with capsys.disabled():
        print('\n[mxfp8 bigk fc model] ' + '\n[mxfp8 bigk fc model] '.join(lines))


def test_fc_model_result(fc_model, capsys):
    res = fc_model['res']
    r = res['mx1']
    assert np.isfinite(r).all() and np.abs(r[..., :21].sum(-1) - 1).max() < 1e-4
    d = {k: rel_err(res[k], res['bf16']) for k in ('mx1', 'mx0', 'fp8')}
    with capsys.disabled():
        print(f"\n[mxfp8 bigk fc model] rel_err(result, result bf16): SSD_MXFP8_BIGK=1 {d['mx1']:.4e}, =0 {d['mx0']:.4e}, fp8 {d['fp8']:.4e}")
    # both quantise the same tensors with the same 2^-4 element rounding; a layout or scale bug gives O(1): the factor 2 is the cap
    # of test_gpu_mxfp8.test_model_mx_untouched_layers_and_result
    assert d['mx1'] <= 2 * d['fp8']


def test_fc_model_no_state(fc_model):
    """max_batch 2: image A alone (M = 361) and as row 0 of [A, B] (M = 722; both on the 64 x 64 tile) give the same bytes, and so
    does A again after something else was inferred"""
    ref, preset = fc_model['ref'], fc_model['preset']
    net = build_net(fc_model['sess'], 'vgg300', fc_model['w'], 'mxfp8', False, '1', b=2)
    a = fc_model['x']
    bb = ref.synth_images(np.random.default_rng(7), 1, preset)
    alone = net.infer(a)
    pair = net.infer(np.concatenate([a, bb]))
    assert np.array_equal(pair[0], alone[0]) and not np.array_equal(pair[1], alone[0])
    net.infer(np.floor(bb / 8).astype(np.float32))
    assert np.array_equal(net.infer(a), alone)


def test_switch_off_and_a_trous(fc_model):
    """the switch changes nothing but the fc graph's plan under SSD_MXFP8_BIGK=1"""
    ref, preset, sess = fc_model['ref'], fc_model['preset'], fc_model['sess']
    w = ref.init_params(preset, 20, seed=42, alive=True)
    x = fc_model['x']
    r = [build_net(sess, 'vgg300', w, 'mxfp8', True, sw).infer(x) for sw in ('1', None)]
    assert np.isfinite(r[0]).all() and np.array_equal(r[0], r[1])
    net0 = fc_model['nets']['mx0']
    net0.activation('bf16:mod_conv6', 1)
    with pytest.raises(RuntimeError, match='no block scales'):
        net0.activation('scale:mod_pool5', 1)


def test_lifecycle(fc_model):
    net, x = fc_model['nets']['mx1'], fc_model['x']
    with pytest.raises(RuntimeError, match=tmx.NO_SCALES):
        net.calibrate_fp8(x)
    with pytest.raises(RuntimeError, match=tmx.NO_SCALES):
        net.fp8_scales


def test_vgg512_fc_batch1(fc_model, capsys):
    from oracle import boxes as ob
    ref = fc_model['ref']
    preset = ob.get_preset('vgg512')
    w = fc_ref.init_params(preset, 20, seed=42)
    x = ref.synth_images(np.random.default_rng(5), 1, preset)
    r = {k: build_net(fc_model['sess'], 'vgg512', w, dt, False, '1').infer(x) for k, dt in (('mx1', 'mxfp8'), ('bf16', 'bf16'))}
    assert np.isfinite(r['mx1']).all() and np.abs(r['mx1'][..., :21].sum(-1) - 1).max() < 1e-4
    with capsys.disabled():
        print(f"\n[mxfp8 bigk fc model] vgg512 batch 1: rel_err(result SSD_MXFP8_BIGK=1, result bf16) = {rel_err(r['mx1'], r['bf16']):.4e}")
