"""-m gpu: the focal loss through the handle (ssd_set_loss) at vgg300, batch 2, labels from the oracle's synth_batch.
Layer-local, as test_gpu_model.py checks the mining loss: the loss gradient is recomputed in float64 (tests/focal_ref.py) from the
GPU's OWN head outputs and compared at 1e-3 (fp32 handle) or TOL_BF = 4e-3 (bf16 handle: bf16 gradient buffers), the bounds of
test_gpu_model.py / test_gpu_bf16.py; the losses at 1e-3.  Then the switch itself: mining after focal is bitwise a fresh handle,
the staged backward is bitwise the plain one, eval_step reports the focal loss, a checkpoint keeps kind, gamma and alpha, and
the drivers train, continue and infer."""
import numpy as np
import pytest
import torch

import focal_ref as fr
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


def check_against_chain(net, preset, y, tol_grad, gamma=GAMMA, alpha=ALPHA, tag=''):
    out_gpu, _ = head_out_from_buffers(net, preset, B)
    a, f, d_out = fr.full_chain(out_gpu, y, 20, gamma, alpha)
    got, pads = head_out_from_buffers(net, preset, B, 'grad:')
    e_g = max_rel(got, d_out)
    L = net.get_losses()
    e_c = abs(L['confidence'] - f['losses'][2]) / f['losses'][2]
    e_l = abs(L['localization'] - f['losses'][1]) / f['losses'][1]
    print(f'    {tag} d(loss)/d(head outputs) {e_g:.3e}  confidence {e_c:.3e}  localization {e_l:.3e}  losses {L}')
    assert np.isfinite(got).all() and e_g < tol_grad
    assert all(not p.any() for p in pads)
    assert e_c < TOL and e_l < TOL
    assert abs(L['total'] - (L['confidence'] + L['localization'] + L['l2'])) <= 1e-6 * L['total']
    dense = np.count_nonzero(got[:, :, :21].any(-1)) / (B * got.shape[1])
    assert dense > 0.99, f'the focal gradient reaches only {dense:.3f} of the anchors'
    return L


def test_focal_step_fp32_and_back_to_mining(batch):
    preset, w, x, y = batch
    xt = torch.tensor(x).cuda(); yt = torch.tensor(y).cuda()
    with Session(0) as sess:
        fresh = make_net(sess, w)
        assert fresh.get_loss() == ('mining', 2.0, 0.25)
        fresh.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        L_m, g_m = fresh.get_losses(), fresh.save_gradients()
        sel_frac = np.count_nonzero(head_out_from_buffers(fresh, preset, B, 'grad:')[0][:, :, :21].any(-1)) / (B * 8732)
        assert sel_frac < 0.5          # mining's gradient is sparse: the two losses are told apart below

        net = make_net(sess, w, loss='focal', focal_gamma=GAMMA, focal_alpha=ALPHA)
        assert net.get_loss() == ('focal', GAMMA, ALPHA)
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        L_f = check_against_chain(net, preset, y, TOL, tag='fp32')
        g_f = net.save_gradients()
        # every sample has positives: the localization loss is the mining handle's, bit for bit; the confidence loss is not
        assert L_f['localization'] == L_m['localization'] and L_f['l2'] == L_m['l2']
        assert L_f['confidence'] != L_m['confidence']

        # the staged backward under focal: bitwise the plain one
        net.forward_dev(xt, yt)
        ranges = list(net.backward_staged(yt, B, 1 << 20))
        torch.cuda.synchronize()
        assert len(ranges) > 1
        g_s = net.save_gradients()
        for k in g_f:
            assert np.array_equal(bits(g_f[k]), bits(g_s[k])), f'staged backward differs at {k}'

        # eval_step reports the focal loss (the same forward: bitwise), and other parameters hold from the next step on
        _, L_e = net.eval_step(x, y, want_result=False)
        assert L_e == L_f
        net.set_loss('focal', 0.5, 0.75)
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        L_h = check_against_chain(net, preset, y, TOL, 0.5, 0.75, tag='fp32 gamma 0.5 alpha 0.75')
        assert L_h['confidence'] != L_f['confidence']

        # ... and mining again: losses and every gradient are a fresh handle's, bit for bit
        net.set_loss('mining')
        assert net.get_loss() == ('mining', 2.0, 0.25)
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        assert net.get_losses() == L_m
        g_b = net.save_gradients()
        for k in g_m:
            assert np.array_equal(bits(g_m[k]), bits(g_b[k])), f'mining after focal differs from a fresh handle at {k}'
        with pytest.raises(ValueError, match='loss'):
            net.set_loss('focal', 7.0, 0.25)
        assert net.get_loss() == ('mining', 2.0, 0.25)


def test_focal_step_bf16(batch):
    preset, w, x, y = batch
    xt = torch.tensor(x).cuda(); yt = torch.tensor(y).cuda()
    with Session(0) as sess:
        net = make_net(sess, w, dtype='bf16', loss='focal', focal_gamma=GAMMA, focal_alpha=ALPHA)
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        check_against_chain(net, preset, y, TOL_BF, tag='bf16')


def test_focal_checkpoint_round_trip_and_prior(batch, tmp_path):
    preset, w, x, y = batch
    path = str(tmp_path / 'focal.npz')
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 20, max_batch=B, weights=w, background_prior=0.01)
        net.build_optimizer(learning_rate=0.001, weight_decay=WD, momentum=0.9, loss='focal', focal_gamma=1.5, focal_alpha=0.75)
        # the prior: background entry log(C (1 - P) / P), class entries 0, offsets as they were
        v = net.save_variables()
        names = [k for k in v if k.startswith('classifiers/') and k.endswith('/biases')]
        assert len(names) == 4 + 6 + 6 + 6 + 4 + 4
        for k in names:
            assert not v[k][:20].any() and v[k][20] == np.float32(np.log(20 * 0.99 / 0.01))
            assert np.array_equal(v[k][21:], np.asarray(w[k], np.float32)[21:])
        r = net.infer(x)
        assert r.shape == (B, 8732, 25)
        net.save_checkpoint(path)
    with np.load(path, allow_pickle=False) as ck:
        assert str(ck['__loss__']) == 'focal' and float(ck['__focal_gamma__']) == 1.5 and float(ck['__focal_alpha__']) == 0.75
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_metagraph(None, path, max_batch=B, training=True)
        net.build_optimizer_from_metagraph()
        assert net.get_loss() == ('focal', 1.5, 0.75)


def test_focal_drivers(tmp_path, capsys):
    """train.py --loss focal, then --continue-training with --loss mining (continues as focal and says so), then infer.py"""
    from ssd_tensorflow_amd import train, infer
    common = ['--batch-size', '4', '--synthetic-train', '8', '--synthetic-valid', '4', '--lr-values', '0.0001;0.00001',
              '--lr-boundaries', '4', '--tensorboard-dir', str(tmp_path / 'tb'), '--checkpoint-interval', '1']
    run = str(tmp_path / 'run')
    assert train.main(['--name', run, '--epochs', '1', '--loss', 'focal'] + common) == 0
    out = capsys.readouterr().out
    assert 'focal (gamma 2, alpha 0.25)' in out.split('[i] Loss:')[1].splitlines()[0]
    assert 'Confidence loss is NaN' not in out
    with np.load(run + '/e1.npz', allow_pickle=False) as ck:
        assert str(ck['__loss__']) == 'focal' and float(ck['__focal_gamma__']) == 2.0 and float(ck['__focal_alpha__']) == 0.25
        assert int(ck['__global_step__']) == 2
        assert np.isfinite(ck['classifiers/classifier0_0/biases']).all()
    assert train.checkpoint_loss(run + '/e1.npz') == ('focal', 2.0, 0.25)
    assert train.main(['--name', run, '--epochs', '2', '--continue-training', 'true', '--loss', 'mining'] + common) == 0
    out = capsys.readouterr().out
    assert '--loss mining disagrees with the checkpoint' in out and "'focal'" in out
    assert 'focal' in out.split('[i] Loss:')[1].splitlines()[0]
    with np.load(run + '/e2.npz', allow_pickle=False) as ck:
        assert str(ck['__loss__']) == 'focal' and int(ck['__global_step__']) == 4
    odir = str(tmp_path / 'out')
    assert infer.main(['--name', run, '--synthetic', '3', '--batch-size', '2', '--threshold', '0.01', '--output-dir', odir]) == 0
    capsys.readouterr()
    assert train.main(['--name', str(tmp_path / 'bad'), '--epochs', '1', '--loss', 'focal', '--focal-gamma', '9'] + common) == 1
    assert '[!] Bad loss:' in capsys.readouterr().out
