"""-m gpu: gradient clipping through the handle (ssd_set_grad_clip) at vgg300, batch 2, fp32 and bf16.  Measuring alone
(clip_norm = inf) is bitwise the step without clipping; the reported norm is the float64 oracle's (tests/clip_ref.py) on a host copy of
the gradient arena, to 1 ulp (the bound of test_gpu_grad_clip.py); a clipped update is bitwise the unclipped update of a twin handle
under grad_scale = the reported factor; a NaN in the arena skips the update and still counts the step; the data-parallel step over
a single-rank RCCL group equals the plain clipped step; the checkpoint keeps the value and the driver trains, reports and continues."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

import clip_ref as cr
from oracle import boxes as ob
from oracle import ssdvgg_ref as ref
from ssd_tensorflow_amd import parallel
from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session

pytestmark = pytest.mark.gpu
WD = 0.0005
B = 2
INF = float('inf')
CLIP = 0.01          # below the weight-decay term's own norm at these weights (0.0005 x |filters|): every update here is clipped


@pytest.fixture(scope='module')
def batch():
    """(weights, x, y device tensors): computed once, never modified"""
    preset = ob.get_preset('vgg300')
    w = ref.init_params(preset, 20, seed=42, alive=True)
    x, y, _ = ref.synth_batch(np.random.default_rng(1234), B, preset)
    return w, torch.tensor(x).cuda(), torch.tensor(y).cuda()


def make_net(sess, w, dtype='f32', **opt):
    net = SSDVGG(sess, 'vgg300')
    net.build_from_vgg(None, 20, max_batch=B, weights=w, dtype=dtype)
    net.build_optimizer(learning_rate=0.001, weight_decay=WD, momentum=0.9, **opt)
    return net


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_measuring_alone_is_bitwise_the_step_without_clipping(batch, dtype):
    w, xt, yt = batch
    with Session(0) as sess:
        off, inf = make_net(sess, w, dtype), make_net(sess, w, dtype, clip_norm=INF)
        assert off.get_grad_clip() == 0.0 and inf.get_grad_clip() == INF
        with pytest.raises(RuntimeError, match='no clipped update'):
            inf.get_grad_norm_step()
        for _ in range(2):
            off.train_step_dev(xt, yt)
            inf.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        assert same_bits(off.params_flat, inf.params_flat) and same_bits(off.momentum_flat, inf.momentum_flat)
        assert off.global_step == inf.global_step == 2
        (n1, f1), (n0, f0) = inf.get_grad_norm_step(0), inf.get_grad_norm_step(1)
        assert f0 == f1 == 1.0 and np.isfinite([n0, n1]).all() and n0 > 0 and n1 > 0 and n0 != n1
        with pytest.raises(RuntimeError, match='gradient clipping is off'):
            off.get_grad_norm_step()
        with pytest.raises(RuntimeError, match='steps_back'):
            inf.get_grad_norm_step(3)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_norm_factor_and_the_unclipped_twin(batch, dtype):
    w, xt, yt = batch
    with Session(0) as sess:
        inf = make_net(sess, w, dtype, clip_norm=INF)
        inf.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        g = inf.grads_flat.cpu().numpy()
        inf.apply_gradients_dev()
        norm, f = inf.get_grad_norm_step()
        want = cr.norm(g, 1.0)
        print(f'{dtype}: reported norm {norm!r}, oracle {want!r}')
        assert f == 1.0 and cr.ulps(norm, np.float32(want)) <= 1
        half = float(np.float32(0.5 * want))
        clip, twin = make_net(sess, w, dtype, clip_norm=half), make_net(sess, w, dtype)
        clip.forward_backward_dev(xt, yt)
        twin.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        assert same_bits(clip.grads_flat, inf.grads_flat) and same_bits(twin.grads_flat, inf.grads_flat)
        clip.apply_gradients_dev()
        norm_c, f_c = clip.get_grad_norm_step()
        want_f = cr.factor(g, 1.0, half)
        print(f'{dtype}: clip_norm {half!r}: reported factor {f_c!r}, oracle {want_f!r}')
        assert norm_c == norm and 0.0 < f_c < 1.0 and cr.ulps(f_c, want_f) <= 1
        twin.apply_gradients_dev(f_c)
        torch.cuda.synchronize()
        assert same_bits(clip.params_flat, twin.params_flat) and same_bits(clip.momentum_flat, twin.momentum_flat)
        assert not same_bits(clip.params_flat, inf.params_flat)
        assert clip.global_step == twin.global_step == 1


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_a_nan_in_the_arena_skips_the_update_and_counts_the_step(batch, dtype):
    w, xt, yt = batch
    with Session(0) as sess:
        net = make_net(sess, w, dtype, clip_norm=CLIP)
        net.train_step_dev(xt, yt)                      # momentum != 0 from here on
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        net.grads_flat[net.grads_flat.numel() // 2] = float('nan')
        p0, m0, step0 = net.params_flat.clone(), net.momentum_flat.clone(), net.global_step
        torch.cuda.synchronize()
        assert m0.abs().max() > 0
        net.apply_gradients_dev()
        torch.cuda.synchronize()
        assert same_bits(net.params_flat, p0) and same_bits(net.momentum_flat, m0)
        assert net.global_step == step0 + 1 == 2
        norm, f = net.get_grad_norm_step()
        assert f == 0.0 and not np.isfinite(norm)
        (n1, f1) = net.get_grad_norm_step(1)            # the update before it was clipped, not skipped
        assert 0.0 < f1 < 1.0 and np.isfinite(n1)
        net.train_step_dev(xt, yt)                      # and the next one updates again
        torch.cuda.synchronize()
        assert not same_bits(net.params_flat, p0) and net.get_grad_norm_step()[1] > 0.0


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.fixture(scope='module')
def nccl_group():
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()))
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    yield
    dist.destroy_process_group()


@pytest.mark.parametrize('bucket', [4_000_000, 0], ids=['bucketed', 'unbucketed'])
def test_data_parallel_step_equals_the_plain_clipped_step(batch, nccl_group, bucket):
    w, xt, yt = batch
    with Session(0) as sess:
        plain, dp = make_net(sess, w, clip_norm=CLIP), make_net(sess, w, clip_norm=CLIP)
        for net in (plain, dp):
            net.set_stream(torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            plain.train_step_dev(xt, yt)
            parallel.train_step_dp(dp, xt, yt, 1, bucket_floats=bucket, force_collectives=True)
        torch.cuda.synchronize()
        assert same_bits(plain.params_flat, dp.params_flat) and same_bits(plain.momentum_flat, dp.momentum_flat)
        assert plain.get_grad_norm_step() == dp.get_grad_norm_step() and plain.get_grad_norm_step(1) == dp.get_grad_norm_step(1)
        assert 0.0 < dp.get_grad_norm_step()[1] < 1.0 and dp.global_step == 2


def test_checkpoint_round_trip(batch, tmp_path):
    w = batch[0]
    with Session(0) as sess:
        for name, v in (('clip', 3.5), ('inf', INF), ('plain', 0.0)):
            make_net(sess, w, clip_norm=v).save_checkpoint(str(tmp_path / (name + '.npz')))
    for name, v in (('clip', 3.5), ('inf', INF), ('plain', 0.0)):
        with np.load(str(tmp_path / (name + '.npz')), allow_pickle=False) as ck:
            assert float(ck['__clip_norm__']) == v
        with Session(0) as sess:
            net = SSDVGG(sess, 'vgg300')
            net.build_from_metagraph(None, str(tmp_path / (name + '.npz')), max_batch=B, training=True)
            net.build_optimizer_from_metagraph()
            assert net.get_grad_clip() == v


def test_drivers(tmp_path, capsys):
    """train.py --clip-norm 0.01 (below the weight-decay term's own norm: every update is clipped) for 2 steps, then --continue-training
    without the flag (continues with 0.01) for 2 more: the checkpoint key, the banner and the epoch line with its counts"""
    import re
    from ssd_tensorflow_amd import train
    common = ['--batch-size', '4', '--synthetic-train', '8', '--synthetic-valid', '4', '--lr-values', '0.0001;0.00001',
              '--lr-boundaries', '4', '--tensorboard-dir', str(tmp_path / 'tb'), '--checkpoint-interval', '1']
    run = str(tmp_path / 'run')
    line = r'\[i\] Grad +1/1  norm median \S+  max \S+  clipped (\d+)  skipped (\d+)  of 2 updates'
    assert train.main(['--name', run, '--epochs', '1', '--clip-norm', str(CLIP)] + common) == 0
    out = capsys.readouterr().out
    assert 'global norm <= 0.01' in out.split('[i] Gradient clipping:')[1].splitlines()[0]
    m = re.search(line, out)
    assert m, out
    assert int(m.group(1)) == 2 and int(m.group(2)) == 0          # the driver books factors below 1
    with np.load(run + '/e1.npz', allow_pickle=False) as ck:
        assert float(ck['__clip_norm__']) == float(np.float32(CLIP)) and int(ck['__global_step__']) == 2
    assert train.checkpoint_clip_norm(run + '/e1.npz') == float(np.float32(CLIP))
    assert train.main(['--name', run, '--epochs', '2', '--continue-training', 'true'] + common) == 0
    out = capsys.readouterr().out
    assert 'global norm <= 0.01' in out.split('[i] Gradient clipping:')[1].splitlines()[0]
    assert re.search(line.replace('1/1', '2/2'), out), out
    with np.load(run + '/e2.npz', allow_pickle=False) as ck:
        assert float(ck['__clip_norm__']) == float(np.float32(CLIP)) and int(ck['__global_step__']) == 4
    rows = open(os.path.join(str(tmp_path / 'tb'), 'run', 'scalars.jsonl')).read()
    assert rows.count('"grad_norm"') == 4 and '"grad_clipped"' in rows
    # measuring only; and off prints no line
    assert train.main(['--name', str(tmp_path / 'inf'), '--epochs', '1', '--clip-norm', 'inf'] + common) == 0
    out = capsys.readouterr().out
    assert 'never clipped' in out and re.search(line.replace(r'(\d+)  skipped', r'0  skipped'), out)
    assert train.main(['--name', str(tmp_path / 'off'), '--epochs', '1'] + common) == 0
    out = capsys.readouterr().out
    assert '[i] Grad ' not in out and 'off' in out.split('[i] Gradient clipping:')[1].splitlines()[0]
    assert train.main(['--name', str(tmp_path / 'bad'), '--epochs', '1', '--clip-norm', '-1'] + common) == 1
    assert 'gradient clipping' in capsys.readouterr().out
