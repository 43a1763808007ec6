"""-m gpu: the fc graph (SSDVGG.build_from_vgg(a_trous=False), ssdvgg.py:210-228) and the convolutions with more than 9 taps
behind its 7x7 fc6 (csrc/conv_bigk.hip).

Op level: fp32 passes against a float64 reference (im2col + double GEMMs on the CPU) with max-rel <= 1e-3 AND rel-L2 <= 1e-4,
every fp32 case run twice (bit-identical); bf16 passes through test_gpu_bf16's checks.  Step level: the fc graph against the CPU
restatement tests/fc_ref.py; the default graph is untouched; checkpoints and drivers carry the graph."""
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import boxes as ob
from oracle import ssdvgg_ref as ref
from gpu_util import lib, check, dev, ptr, host, rel_err, max_rel, conv_geom
from test_gpu_bf16 import conv_case_check, TOL as TOL_B, TOL_BF
import fc_ref
from ssd_tensorflow_amd import ssdvgg as ssdvgg_mod
from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session

pytestmark = pytest.mark.gpu
TOL = 1e-3          # max-rel
TOL_L2 = 1e-4       # rel-L2 (fc6's data gradient sums 200,704 products per output; measured rel-L2 is printed)
WD = 0.0005

# (name, b, h, w, ci, co, k, relu)
F32_CASES = [
    ('fc6 vgg300 7x7 512->4096', 2, 19, 19, 512, 4096, 7, True),
    ('fc6 vgg512 7x7 512->4096', 1, 32, 32, 512, 4096, 7, True),
    ('ragged 7x7, image 5x7, 40->72', 1, 5, 7, 40, 72, 7, True),
    ('ragged 5x5, 6x9, 24->136', 2, 6, 9, 24, 136, 5, True),
    ('fc7 1x1 4096->4096', 2, 19, 19, 4096, 4096, 1, True),
    ('conv8_1 1x1 4096->256', 2, 19, 19, 4096, 256, 1, True),
    ('head1 3x3 4096->152', 2, 19, 19, 4096, 152, 3, False),
]


def im2col64(x, k, ph, pw):
    """x NHWC float64 torch -> (cols [B, Ci*k*k, H*W], padded size); SAME stride 1"""
    xp = F.pad(x.permute(0, 3, 1, 2), (pw, k - 1 - pw, ph, k - 1 - ph))
    return F.unfold(xp, k), xp.shape[2:]


def conv64(x, w, bias, dy, ph, pw):
    """float64 forward (pre-activation), data gradient and weight / bias gradient of a stride-1 SAME conv; x / dy NHWC, w HWIO"""
    x = torch.from_numpy(x).double(); w = torch.from_numpy(w).double(); dy = torch.from_numpy(dy).double()
    b, h, wd, ci = x.shape
    k, co = w.shape[0], w.shape[3]
    cols, psize = im2col64(x, k, ph, pw)
    wm = w.permute(3, 2, 0, 1).reshape(co, ci * k * k)
    y = (wm @ cols).reshape(b, co, h, wd).permute(0, 2, 3, 1) + torch.from_numpy(bias).double()
    dyf = dy.permute(0, 3, 1, 2).reshape(b, co, h * wd)
    dx = F.fold(wm.t() @ dyf, psize, k)[:, :, ph:ph + h, pw:pw + wd].permute(0, 2, 3, 1)
    dwm = sum(dyf[i] @ cols[i].t() for i in range(b))
    dw = dwm.reshape(co, ci, k, k).permute(2, 3, 1, 0)
    return y.numpy(), dx.numpy(), dw.numpy(), dy.sum((0, 1, 2)).numpy()


def both(tag, got, want):
    e, l2 = max_rel(got, want), rel_err(got, want)
    print(f'    {tag:<48s} max-rel {e:.2e}  rel-L2 {l2:.2e}')
    assert e <= TOL and l2 <= TOL_L2, (tag, e, l2)


@pytest.mark.parametrize('case', F32_CASES, ids=[c[0] for c in F32_CASES])
def test_conv_f32_against_float64(case):
    name, b, h, w_, ci, co, k, relu = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ph, pw, ho, wo = conv_geom(h, w_, k, 1, 1, 'SAME')
    x = rng.normal(0, 1, (b, h, w_, ci)).astype(np.float32)
    w = (rng.normal(0, 1, (k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.normal(0, 0.1, (co,)).astype(np.float32)
    dy = rng.normal(0, 1, (b, h, w_, co)).astype(np.float32)
    pre, dx_ref, dw_ref, db_ref = conv64(x, w, bias, dy, ph, pw)
    y_ref = np.maximum(pre, 0) if relu else pre
    geom = (b, h, w_, ci, ho, wo, co, k, k, 1, 1, ph, pw)
    x_, w_d, b_, dy_ = dev(x), dev(w), dev(bias), dev(dy)
    prev = rng.normal(0, 1, x.shape).astype(np.float32)
    mask = rng.normal(0, 1, x.shape).astype(np.float32)
    nws = lib.ssd_op_conv2d_wgrad_ws_floats(*geom)
    if k * k > 9:
        assert nws == 0      # the >9-tap weight gradient takes no workspace
    ws_ = torch.empty((max(nws, 1),), device='cuda')
    runs = []
    for rep in range(2):
        y_ = torch.full((b, ho, wo, co), 9.0, device='cuda')
        check(lib.ssd_op_conv2d_fwd(ptr(x_), ptr(w_d), ptr(b_), ptr(y_), *geom, int(relu), None))
        gx_ = torch.full((b, h, w_, ci), 3.0, device='cuda')
        check(lib.ssd_op_conv2d_dgrad(ptr(dy_), ptr(w_d), ptr(gx_), None, 0, *geom, None))
        ga_ = dev(prev)
        check(lib.ssd_op_conv2d_dgrad(ptr(dy_), ptr(w_d), ptr(ga_), ptr(dev(mask)), 1, *geom, None))
        gw_ = torch.full((k, k, ci, co), 7.0, device='cuda'); gb_ = torch.full((co,), 7.0, device='cuda')
        check(lib.ssd_op_conv2d_wgrad(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_d), WD, ptr(ws_), *geom, None))
        runs.append([host(t) for t in (y_, gx_, ga_, gw_, gb_)])
    for a, c in zip(runs[0], runs[1]):
        assert np.array_equal(a, c), f'{name}: two runs differ'
    y, gx, ga, gw, gb = runs[0]
    both(f'{name} forward', y, y_ref)
    both(f'{name} data gradient', gx, dx_ref)
    both(f'{name} data gradient accumulate+mask', ga, (dx_ref + prev) * (mask > 0))
    both(f'{name} weight gradient', gw, dw_ref + WD * w.astype(np.float64))
    both(f'{name} bias gradient', gb, db_ref)


# (name, b, hi, wi, ci, co, k, stride, dil, padding, relu, y_f32): test_gpu_bf16.conv_case_check
BF16_CASES = [
    ('bf16 fc6 vgg300', 2, 19, 19, 512, 4096, 7, 1, 1, 'SAME', True, False),
    ('bf16 fc6 vgg512', 1, 32, 32, 512, 4096, 7, 1, 1, 'SAME', True, False),
    ('bf16 ragged 7x7 5x7 40->72', 1, 5, 7, 40, 72, 7, 1, 1, 'SAME', True, False),
    ('bf16 ragged 5x5 6x9 24->136', 2, 6, 9, 24, 136, 5, 1, 1, 'SAME', True, False),
    ('bf16 fc7 1x1 4096->4096', 2, 19, 19, 4096, 4096, 1, 1, 1, 'SAME', True, False),
    ('bf16 conv8_1 1x1 4096->256', 2, 19, 19, 4096, 256, 1, 1, 1, 'SAME', True, False),
    ('bf16 head1 3x3 4096->152 f32 out', 2, 19, 19, 4096, 152, 3, 1, 1, 'SAME', False, True),
]


@pytest.mark.parametrize('case', BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_conv_bf16(case):
    conv_case_check(case, chain=False)


def test_head1_winograd_form():
    """fp32 head 3x3 4096 -> 152 through the Winograd entry points (the step keeps this layer on the direct kernels)"""
    b, h, ci, co = 2, 19, 4096, 152
    rng = np.random.default_rng(5)
    geom = (b, h, h, ci, h, h, co, 3, 3, 1, 1, 1, 1)
    nws = lib.ssd_op_conv2d_wino_ws_floats(*geom)
    assert nws > 0
    x = rng.normal(0, 1, (b, h, h, ci)).astype(np.float32)
    w = (rng.normal(0, 1, (3, 3, ci, co)) / np.sqrt(9 * ci)).astype(np.float32)
    bias = rng.normal(0, 0.1, (co,)).astype(np.float32)
    dy = rng.normal(0, 1, (b, h, h, co)).astype(np.float32)
    pre, dx_ref, dw_ref, db_ref = conv64(x, w, bias, dy, 1, 1)
    x_, w_, b_, dy_ = dev(x), dev(w), dev(bias), dev(dy)
    wws = torch.empty((nws,), device='cuda')
    y_ = torch.empty((b, h, h, co), device='cuda'); gx_ = torch.empty_like(x_)
    gw_ = torch.empty_like(w_); gb_ = torch.empty_like(b_)
    check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), ptr(b_), ptr(y_), None, None, None, ptr(wws), 0, *geom, 0, None))
    check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(gx_), None, None, 0, None, 0, 0, ptr(wws), 0, *geom, None))
    check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), ptr(b_), ptr(y_), None, None, None, ptr(wws), 0, *geom, 0, None))
    check(lib.ssd_op_conv2d_wino_wgrad(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_), WD, ptr(wws), 2, *geom, None))
    for tag, got, want in (('forward', host(y_), pre), ('data gradient', host(gx_), dx_ref),
                           ('weight gradient', host(gw_), dw_ref + WD * w), ('bias gradient', host(gb_), db_ref)):
        e = max_rel(got, want)
        print(f'    winograd head1 {tag:<20s} max-rel {e:.2e}  rel-L2 {rel_err(got, want):.2e}')
        assert e < TOL


# ------------------------------------------------------------------------------------------------ step level
_REF = {}


def fc_reference(pname, b):
    """(weights, x, y, result, losses, gradients) of the CPU restatement, computed once per (preset, batch)"""
    key = (pname, b)
    if key not in _REF:
        preset = ob.get_preset(pname)
        w = fc_ref.init_params(preset, 20, seed=11)
        rng = np.random.default_rng(77)
        x, y, _ = ref.synth_batch(rng, b, preset)
        m = fc_ref.RefModelFC(pname, w)
        r, L, g = m.grads(x, y)
        _REF[key] = (w, x, y, r, L, g)
    return _REF[key]


@pytest.mark.parametrize('pname,b,dtype', [('vgg300', 2, 'f32'), ('vgg512', 1, 'f32'), ('vgg300', 2, 'bf16'), ('vgg512', 1, 'bf16')])
def test_fc_step(pname, b, dtype):
    w, x, y, r_ref, L_ref, g_ref = fc_reference(pname, b)
    with Session(0) as sess:
        net = SSDVGG(sess, pname)
        net.build_from_vgg(None, 20, a_trous=False, max_batch=b, weights=w, dtype=dtype)
        assert net.a_trous is False
        gr = C_int()
        check(lib.ssd_graph(net._h, gr)); assert gr.value == 1
        names = dict(net.variables())
        assert names['fc6/weights'] == (7, 7, 512, 4096) and names['fc7/weights'] == (1, 1, 4096, 4096)
        assert 'mod_conv6/filter' not in names and set(names) == set(g_ref)
        assert net.arena_floats == lib.ssd_arena_floats_graph(pname.encode(), 20, 1)
        net.build_optimizer(learning_rate=0.001, weight_decay=WD, momentum=0.9)
        r, L = sess.run([net.result, net.losses], feed_dict={net.image_input: x, net.labels: y})
        er = max_rel(r, r_ref)
        print(f'    {pname} b{b} {dtype}: result max-rel {er:.2e}; losses', {k: (round(L[k], 5), round(L_ref[k], 5)) for k in L})
        assert abs(L['l2'] - L_ref['l2']) < TOL * L_ref['l2']      # fp32 masters, fc filters included
        xt = torch.from_numpy(x).cuda(); yt = torch.from_numpy(y).cuda()
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        g = net.save_gradients()
        errs = {k: rel_err(g[k], g_ref[k]) for k in g_ref}
        for k in ('fc6/weights', 'fc6/biases', 'fc7/weights', 'fc7/biases', 'conv8_1/filter', 'classifiers/classifier1_0/filter'):
            print(f'    gradient {k:<36s} rel-L2 {errs[k]:.2e}')
        upper = [k for k in g_ref if k.startswith(('classifiers', 'conv8', 'conv9', 'conv10', 'conv11', 'conv12', 'fc6', 'fc7'))]
        if dtype == 'f32':
            assert er < TOL
            for k in ('total', 'localization', 'confidence'):
                assert abs(L[k] - L_ref[k]) < TOL * abs(L_ref[k]), (k, L[k], L_ref[k])
            assert max(errs[k] for k in upper) < TOL      # nothing chaotic above mod_pool5 (test_gpu_model.py)
            assert max(errs.values()) < 3e-2
        else:
            # bf16 activations: the distance to the fp32 restatement, with test_gpu_bf16.py's bound on the total loss.  End to end,
            # a bf16 gradient moves by ~2^-9 per layer it passes (conv8_1's measured 7e-2); the fc layers' own gradients are held
            # to 5 %, the op-level tests above hold every pass of these layers to TOL / TOL_BF
            assert abs(L['total'] - L_ref['total']) < 0.05 * abs(L_ref['total'])
            assert er < 0.05
            assert max(errs[k] for k in ('fc6/weights', 'fc6/biases', 'fc7/weights', 'fc7/biases')) < 0.05
        # two momentum updates from the same gradient arena
        w0 = net.save_variables()
        net.apply_gradients_dev(1.0)
        w1 = net.save_variables(); mom = net.save_momentum()
        for k in ('fc6/weights', 'fc7/biases', 'conv8_1/filter', 'conv4_2/filter'):
            assert np.allclose(mom[k], g[k], rtol=1e-6, atol=1e-12)
            assert np.allclose(w1[k], w0[k] - np.float32(0.001) * g[k], rtol=1e-6, atol=1e-9)
        net.apply_gradients_dev(1.0)
        w2 = net.save_variables()
        for k in ('fc6/weights', 'fc7/weights', 'classifiers/classifier1_3/biases'):
            assert np.allclose(w2[k], w1[k] - np.float32(0.001) * (np.float32(0.9) * g[k] + g[k]), rtol=1e-5, atol=1e-9)
        assert net.global_step == 2


def C_int():
    import ctypes
    return ctypes.c_int()


class _DtypeLib:
    """the library with ssd_create_graph answered by the pre-existing ssd_create_dtype (graph argument dropped)"""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, n):
        return getattr(self._real, n)

    def ssd_create_graph(self, *a):
        assert a[10] == 0
        return self._real.ssd_create_dtype(*a[:10], a[11])


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_default_graph_untouched(dtype, monkeypatch):
    preset = ob.get_preset('vgg300')
    rng = np.random.default_rng(3)
    x, y, _ = ref.synth_batch(rng, 2, preset)
    xt = torch.from_numpy(x).cuda(); yt = torch.from_numpy(y).cuda()
    out = []
    with Session(0) as sess:
        for via_dtype in (False, True):
            if via_dtype:
                monkeypatch.setattr(ssdvgg_mod, 'lib', _DtypeLib(ssdvgg_mod.lib))
            net = SSDVGG(sess, 'vgg300')
            net.build_from_vgg(None, 20, max_batch=2, seed=5, dtype=dtype)      # the library's own initial weights
            gr = C_int()
            check(lib.ssd_graph(net._h, gr)); assert gr.value == 0
            net.build_optimizer(learning_rate=0.001, weight_decay=WD, momentum=0.9)
            p = net.save_variables()
            net.forward_backward_dev(xt, yt)
            torch.cuda.synchronize()
            r = sess.run(net.result, feed_dict={net.image_input: x, net.keep_prob: 1})
            out.append((p, net.save_gradients(), r))
            net.close()
    (p0, g0, r0), (p1, g1, r1) = out
    assert set(p0) == set(p1) and 'mod_conv6/filter' in p0
    for k in p0:
        assert np.array_equal(p0[k], p1[k]), k
        assert np.array_equal(g0[k], g1[k]), k
    assert np.array_equal(r0, r1)


def test_fc_checkpoint_roundtrip(tmp_path):
    w, x, y, _, _, _ = fc_reference('vgg300', 2)
    path = str(tmp_path / 'fc.npz')
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 20, a_trous=False, max_batch=2, training=False, weights=w)
        r0 = sess.run(net.result, feed_dict={net.image_input: x, net.keep_prob: 1})
        net.save_checkpoint(path)
        net.close()
        ck = np.load(path)
        assert int(ck['__a_trous__']) == 0 and ck['__a_trous__'].dtype.kind == 'i' and ck['fc6/weights'].shape == (7, 7, 512, 4096)
        net2 = SSDVGG(sess, 'vgg300')
        net2.build_from_metagraph(None, path, max_batch=2)
        assert net2.a_trous is False
        r1 = sess.run(net2.result, feed_dict={net2.image_input: x, net2.keep_prob: 1})
        assert np.array_equal(r0, r1)


def test_train_resume_infer_fc(tmp_path, capsys):
    from ssd_tensorflow_amd import train, infer
    common = ['--batch-size', '2', '--synthetic-train', '4', '--synthetic-valid', '2', '--lr-values', '0.0001;0.00001',
              '--lr-boundaries', '4', '--a-trous', 'false']
    run = str(tmp_path / 'run'); tb = str(tmp_path / 'tb')
    assert train.main(['--name', run, '--tensorboard-dir', tb, '--epochs', '1', '--checkpoint-interval', '1'] + common) == 0
    ck = np.load(run + '/e1.npz')
    assert int(ck['__a_trous__']) == 0 and 'fc7/weights' in ck.files and '__momentum__/fc6/weights' in ck.files
    del ck
    os.remove(run + '/final.npz')
    # resume for a second epoch (the checkpoint decides the graph even when the flag says otherwise) vs. two epochs straight
    resume = [a if a != 'false' else 'true' for a in common]
    assert train.main(['--name', run, '--tensorboard-dir', tb, '--epochs', '2', '--checkpoint-interval', '5',
                       '--continue-training', 'true'] + resume) == 0
    os.remove(run + '/e1.npz')
    straight = str(tmp_path / 'straight')
    assert train.main(['--name', straight, '--tensorboard-dir', tb, '--epochs', '2', '--checkpoint-interval', '5'] + common) == 0
    a, b = np.load(run + '/final.npz'), np.load(straight + '/final.npz')
    assert int(a['__a_trous__']) == 0 and int(a['__global_step__']) == int(b['__global_step__']) == 4
    for k in b.files:
        assert np.array_equal(a[k], b[k]), k
    del a, b
    capsys.readouterr()
    odir = str(tmp_path / 'out')
    assert infer.main(['--name', run, '--synthetic', '2', '--batch-size', '2', '--threshold', '0.0', '--dump-predictions', 'true',
                       '--output-dir', odir]) == 0
    out = capsys.readouterr().out
    assert '[i] Processed 2 images' in out
    dumps = sorted(f for f in os.listdir(odir) if f.endswith('.npy'))
    assert len(dumps) == 2 and np.load(os.path.join(odir, dumps[0])).shape == (8732, 25)
