"""-m gpu: the GIoU localization loss through the handle (ssd_set_loc_loss) at vgg300, batch 2, labels from the
oracle's synth_batch, under mining and under focal.  Layer-local, as test_gpu_focal_model.py checks the focal loss: the loss
gradient is recomputed in float64 (tests/giou_ref.py with loss_ref.py / focal_ref.py) from the GPU's OWN head outputs and compared
at 1e-3 (fp32 handle) or TOL_BF = 4e-3 (bf16 handle: bf16 gradient buffers), the bounds of that file; the losses at 1e-3.  Then
the switch itself: smooth_l1 after giou is bitwise a fresh handle, the staged backward is bitwise the plain one, a checkpoint
keeps kind and weight, and the driver trains and continues."""
import numpy as np
import pytest
import torch

import focal_ref as fr
import giou_ref as gr
import loss_ref as lr
from oracle import boxes as ob
from oracle import ssdvgg_ref as ref
from gpu_util import max_rel
from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session

pytestmark = pytest.mark.gpu
TOL = 1e-3
TOL_BF = 4e-3
WD = 0.0005
B = 2
GAMMA, ALPHA = 2.0, 0.25


@pytest.fixture(scope='module')
def batch():
    """(preset, weights, x, y): computed once, never modified"""
    preset = ob.get_preset('vgg300')
    w = ref.init_params(preset, 20, seed=42, alive=True)
    x, y, _ = ref.synth_batch(np.random.default_rng(1234), B, preset)
    assert ((y[:, :, 20] == 0).sum(1) > 0).all()          # every sample has positives
    for a in (x, y):
        a.setflags(write=False)
    return preset, w, x, y


def make_net(sess, w, dtype='f32', **opt):
    net = SSDVGG(sess, 'vgg300')
    net.build_from_vgg(None, 20, max_batch=B, weights=w, dtype=dtype)
    net.build_optimizer(learning_rate=0.001, weight_decay=WD, momentum=0.9, **opt)
    return net


def head_out_from_buffers(net, preset, b, prefix=''):
    """[b, A, 25] in anchor order from the fused head buffers 'head<i>' ([b,H,W,ld], columns j*25..), and the pad columns"""
    parts, pads = [], []
    for i, (fk, s, ars) in enumerate(preset['maps']):
        buf = net.activation(prefix + f'head{i}', b)
        nj = 2 + len(ars)
        for j in range(nj):
            parts.append(buf[..., j * 25:(j + 1) * 25].reshape(b, fk * fk, 25))
        pads.append(buf[..., nj * 25:])
    return np.concatenate(parts, 1), pads


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_against_chain(net, preset, y, tol_grad, conf, weight, tag=''):
    out_gpu, _ = head_out_from_buffers(net, preset, B)
    a = lr.stage_a(out_gpu, y, 20)
    sl1 = gr.terms(out_gpu, y, 20, weight)
    if conf == 'focal':
        s = fr.stage_f(a['ce'], a['pos'], sl1, GAMMA, ALPHA)
        d = fr.grad(a['result'], y, a['ce'], a['pos'], s['sample'][:, 2], 20, GAMMA, ALPHA)
    else:
        s = lr.stage_b(a['ce'], a['pos'], sl1)
        d = lr.grad(a['result'], y, s['sel'], a['pos'], s['sample'][:, 2], 20)
    d_out = gr.with_loc_grad(d, out_gpu, y, 20, weight, s['sample'][:, 2])
    got, pads = head_out_from_buffers(net, preset, B, 'grad:')
    e_g = max_rel(got, d_out)
    e_loc = max_rel(got[:, :, 21:], d_out[:, :, 21:])
    L = net.get_losses()
    e_c = abs(L['confidence'] - s['losses'][2]) / s['losses'][2]
    e_l = abs(L['localization'] - s['losses'][1]) / s['losses'][1]
    print(f'    {tag} d(loss)/d(head outputs) {e_g:.3e} (loc columns alone {e_loc:.3e})  confidence {e_c:.3e}  localization {e_l:.3e}  '
          f'losses {L}')
    assert np.isfinite(got).all() and e_g < tol_grad and e_loc < tol_grad
    assert all(not p.any() for p in pads)
    assert e_c < TOL and e_l < TOL
    assert abs(L['total'] - (L['confidence'] + L['localization'] + L['l2'])) <= 1e-6 * L['total']
    pos = y[:, :, 20] == 0
    assert np.abs(got[:, :, 21:][pos]).max() > 0 and not got[:, :, 21:][~pos].any()
    return L


@pytest.mark.parametrize('conf', ['mining', 'focal'])
def test_giou_step_fp32_and_back_to_smooth_l1(batch, conf):
    preset, w, x, y = batch
    xt = torch.tensor(x).cuda(); yt = torch.tensor(y).cuda()
    opt = dict(loss=conf, focal_gamma=GAMMA, focal_alpha=ALPHA)
    with Session(0) as sess:
        fresh = make_net(sess, w, **opt)
        assert fresh.get_loc_loss() == ('smooth_l1', 1.0)
        fresh.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        L_s, g_s = fresh.get_losses(), fresh.save_gradients()

        net = make_net(sess, w, loc_loss='giou', loc_weight=2.0, **opt)
        assert net.get_loc_loss() == ('giou', 2.0) and net.get_loss()[0] == conf
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        L_g = check_against_chain(net, preset, y, TOL, conf, 2.0, tag=f'fp32 {conf} + giou')
        g_g = net.save_gradients()
        # the confidence half is the smooth-L1 handle's, bit for bit; the localization half is not
        assert L_g['confidence'] == L_s['confidence'] and L_g['l2'] == L_s['l2']
        assert L_g['localization'] != L_s['localization']

        # the staged backward under GIoU: bitwise the plain one
        net.forward_dev(xt, yt)
        ranges = list(net.backward_staged(yt, B, 1 << 20))
        torch.cuda.synchronize()
        assert len(ranges) > 1
        g_st = net.save_gradients()
        for k in g_g:
            assert np.array_equal(bits(g_g[k]), bits(g_st[k])), f'staged backward differs at {k}'

        # eval_step reports the GIoU loss (the same forward: bitwise); another weight holds from the next step on
        _, L_e = net.eval_step(x, y, want_result=False)
        assert L_e == L_g
        net.set_loc_loss('giou', 1.0)
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        L_1 = check_against_chain(net, preset, y, TOL, conf, 1.0, tag=f'fp32 {conf} + giou weight 1')
        assert abs(L_1['localization'] * 2 - L_g['localization']) <= 1e-6 * L_g['localization']

        # ... and smooth-L1 again: losses and every gradient are a fresh handle's, bit for bit
        net.set_loc_loss('smooth_l1')
        assert net.get_loc_loss() == ('smooth_l1', 1.0)
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        assert net.get_losses() == L_s
        g_b = net.save_gradients()
        for k in g_s:
            assert np.array_equal(bits(g_s[k]), bits(g_b[k])), f'smooth_l1 after giou differs from a fresh handle at {k}'
        with pytest.raises(ValueError, match='localization loss'):
            net.set_loc_loss('giou', 0.0)
        assert net.get_loc_loss() == ('smooth_l1', 1.0)


@pytest.mark.parametrize('conf', ['mining', 'focal'])
def test_giou_step_bf16(batch, conf):
    preset, w, x, y = batch
    xt = torch.tensor(x).cuda(); yt = torch.tensor(y).cuda()
    with Session(0) as sess:
        net = make_net(sess, w, dtype='bf16', loss=conf, focal_gamma=GAMMA, focal_alpha=ALPHA, loc_loss='giou', loc_weight=2.0)
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        check_against_chain(net, preset, y, TOL_BF, conf, 2.0, tag=f'bf16 {conf} + giou')


def test_giou_checkpoint_round_trip(batch, tmp_path):
    preset, w, x, y = batch
    path = str(tmp_path / 'giou.npz')
    with Session(0) as sess:
        net = make_net(sess, w, loss='focal', focal_gamma=1.5, focal_alpha=0.75, loc_loss='giou', loc_weight=2.5)
        net.save_checkpoint(path)
        old = make_net(sess, w)
        old.save_checkpoint(str(tmp_path / 'plain.npz'))
    with np.load(path, allow_pickle=False) as ck:
        assert str(ck['__loc_loss__']) == 'giou' and float(ck['__loc_weight__']) == 2.5 and str(ck['__loss__']) == 'focal'
    with np.load(str(tmp_path / 'plain.npz'), allow_pickle=False) as ck:
        assert str(ck['__loc_loss__']) == 'smooth_l1' and float(ck['__loc_weight__']) == 1.0
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_metagraph(None, path, max_batch=B, training=True)
        net.build_optimizer_from_metagraph()
        assert net.get_loc_loss() == ('giou', 2.5) and net.get_loss() == ('focal', 1.5, 0.75)


def test_giou_drivers(tmp_path, capsys):
    """train.py --loc-loss giou --loc-weight 2 for 2 steps, then --continue-training with the default (continues as giou and says
    so) for 2 more: the checkpoint keys and the banner agree"""
    from ssd_tensorflow_amd import train
    common = ['--batch-size', '4', '--synthetic-train', '8', '--synthetic-valid', '4', '--lr-values', '0.0001;0.00001',
              '--lr-boundaries', '4', '--tensorboard-dir', str(tmp_path / 'tb'), '--checkpoint-interval', '1']
    run = str(tmp_path / 'run')
    assert train.main(['--name', run, '--epochs', '1', '--loc-loss', 'giou', '--loc-weight', '2'] + common) == 0
    out = capsys.readouterr().out
    assert 'giou (weight 2)' in out.split('[i] Localization loss:')[1].splitlines()[0]
    assert 'mining' in out.split('[i] Loss:')[1].splitlines()[0]
    assert 'loss is NaN' not in out
    with np.load(run + '/e1.npz', allow_pickle=False) as ck:
        assert str(ck['__loc_loss__']) == 'giou' and float(ck['__loc_weight__']) == 2.0 and str(ck['__loss__']) == 'mining'
        assert int(ck['__global_step__']) == 2
        assert np.isfinite(ck['classifiers/classifier0_0/biases']).all()
    assert train.checkpoint_loc_loss(run + '/e1.npz') == ('giou', 2.0)
    assert train.main(['--name', run, '--epochs', '2', '--continue-training', 'true'] + common) == 0
    out = capsys.readouterr().out
    assert '--loc-loss smooth_l1 disagrees with the checkpoint' in out and "'giou'" in out
    assert 'giou (weight 2)' in out.split('[i] Localization loss:')[1].splitlines()[0]
    with np.load(run + '/e2.npz', allow_pickle=False) as ck:
        assert str(ck['__loc_loss__']) == 'giou' and float(ck['__loc_weight__']) == 2.0 and int(ck['__global_step__']) == 4
    assert train.main(['--name', str(tmp_path / 'bad'), '--epochs', '1', '--loc-loss', 'giou', '--loc-weight', '-1'] + common) == 1
    assert '[!] Bad loss:' in capsys.readouterr().out
