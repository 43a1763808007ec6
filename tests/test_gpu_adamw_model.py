"""-m gpu: AdamW through the handle (ssd_set_update_rule) at vgg300, batch 2, fp32 and bf16.  After a backward pass the
float32 oracle of tests/adamw_ref.py on host copies of parameters, first moment, second moment and gradient gives, bit for bit, what
ssd_apply_gradients_dev leaves -- for two consecutive updates (t = 1, 2), with and without clipping at half the measured norm.  The
copies go by variable (ssd_save_variable / _momentum / _second_moment / _gradient): the update is element-wise, a variable under
'/filter' lies in front of filter_floats and decays, every other one does not.  Then: a NaN in the arena skips the update while t and
global_step advance; changing the rule zeroes the state and setting it again keeps it; the default rule launches what it launched;
the data-parallel step over a single-rank RCCL group equals the plain step; checkpoints resume bit-identically; the driver trains
and continues."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

import adamw_ref as ar
import clip_ref as cr
from oracle import boxes as ob
from oracle import ssdvgg_ref as ref
from ssd_tensorflow_amd import parallel
from ssd_tensorflow_amd._lib import lib, check
from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session

pytestmark = pytest.mark.gpu
WD = 0.0005
B = 2
HP = ar.hyper(lr=0.001)          # the defaults: beta 0.9 / 0.999, eps 1e-8, decay 0.01


@pytest.fixture(scope='module')
def batch():
    """(weights, x, y device tensors): computed once, never modified"""
    preset = ob.get_preset('vgg300')
    w = ref.init_params(preset, 20, seed=42, alive=True)
    x, y, _ = ref.synth_batch(np.random.default_rng(1234), B, preset)
    return w, torch.tensor(x).cuda(), torch.tensor(y).cuda()


def make_net(sess, w, dtype='f32', optimizer='adamw', **opt):
    net = SSDVGG(sess, 'vgg300')
    net.build_from_vgg(None, 20, max_batch=B, weights=w, dtype=dtype)
    net.build_optimizer(learning_rate=0.001, weight_decay=WD, momentum=0.9, optimizer=optimizer, **opt)
    return net


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def state(net):
    """host copies by variable: (w, m, v)"""
    return net.save_variables(), net.save_momentum(), net.save_second_moment()


def same_state(a, b):
    return all(x.keys() == y.keys() and all(x[k].tobytes() == y[k].tobytes() for k in x) for x, y in zip(a, b))


def oracle(st, grads, t, gscale):
    """the contract on every variable: the decoupled decay on the filters alone"""
    out = ({}, {}, {})
    for k in st[0]:
        shape = st[0][k].shape
        n = st[0][k].size
        res = ar.adamw(st[0][k].ravel(), st[1][k].ravel(), st[2][k].ravel(), grads[k].ravel(), n if k.endswith('/filter') else 0, HP, t, gscale)
        for d, a in zip(out, res):
            d[k] = a.reshape(shape)
    return out


@pytest.mark.parametrize('clip', [False, True], ids=['plain', 'clipped'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_two_updates_have_the_bits_of_the_oracle(batch, dtype, clip):
    w, xt, yt = batch
    with Session(0) as sess:
        net = make_net(sess, w, dtype)
        assert net.get_update_rule() == ('adamw',) + tuple(float(x) for x in HP[1:]) and net.adam_step == 0
        assert any(k.endswith('/filter') for k, _ in net.variables()) and not any(k.endswith('/weights') for k, _ in net.variables())
        for t in (1, 2):
            net.forward_backward_dev(xt, yt)
            torch.cuda.synchronize()
            before, grads = state(net), net.save_gradients()
            gscale = np.float32(1.0)
            if clip:
                flat = np.concatenate([g.ravel() for g in grads.values()])      # (what the arena holds besides is padding: zeros)
                half = float(np.float32(0.5 * cr.norm(flat, 1.0)))
                net.set_grad_clip(half)
            net.apply_gradients_dev()
            torch.cuda.synchronize()
            if clip:
                norm, f = net.get_grad_norm_step()
                print(f'{dtype} t {t}: clip_norm {half!r}: norm {norm!r}, factor {f!r}')
                assert 0.0 < f < 1.0 and cr.ulps(f, cr.factor(flat, 1.0, half)) <= 1      # (the bound of test_gpu_grad_clip.py)
                gscale = np.float32(1.0) * np.float32(f)
            want = oracle(before, grads, t, gscale)
            got = state(net)
            for name, a, b in zip(('w', 'm', 'v'), got, want):
                bad = [k for k in a if a[k].tobytes() != b[k].tobytes()]
                print(f'{dtype} t {t} {name}: {len(bad)} of {len(a)} variables differ {bad[:3]}')
            assert same_state(got, want)
            assert not same_state(got[:1], before[:1])
            assert net.adam_step == t == net.global_step


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_a_nan_in_the_arena_skips_the_update_and_counts_the_step(batch, dtype):
    w, xt, yt = batch
    with Session(0) as sess:
        net = make_net(sess, w, dtype, clip_norm=0.01)
        net.train_step_dev(xt, yt)
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        net.grads_flat[net.grads_flat.numel() // 2] = float('nan')
        torch.cuda.synchronize()
        before = state(net)
        assert max(np.abs(a).max() for a in before[2].values()) > 0
        net.apply_gradients_dev()
        torch.cuda.synchronize()
        assert same_state(state(net), before)
        assert net.adam_step == 2 == net.global_step
        norm, f = net.get_grad_norm_step()
        assert f == 0.0 and not np.isfinite(norm)
        net.train_step_dev(xt, yt)                      # the next one updates again, as t = 3
        torch.cuda.synchronize()
        assert not same_state(state(net), before) and net.adam_step == 3 and net.get_grad_norm_step()[1] > 0.0


def test_switching_the_rule_zeroes_the_state_and_setting_it_again_keeps_it(batch):
    w, xt, yt = batch
    with Session(0) as sess:
        net = make_net(sess, w, optimizer='momentum')
        assert net.get_update_rule()[0] == 'momentum'
        with pytest.raises(RuntimeError, match='never been under AdamW'):
            net.save_second_moment()
        net.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        assert net.momentum_flat.abs().max() > 0 and net.adam_step == 0
        p0 = net.params_flat.clone()
        net.set_update_rule('adamw')                     # momentum -> adamw: m, v, t zeroed; the parameters stay
        torch.cuda.synchronize()
        assert net.momentum_flat.abs().max() == 0 and net.adam_step == 0 and same_bits(net.params_flat, p0)
        assert all((a == 0).all() for a in net.save_second_moment().values())
        net.train_step_dev(xt, yt)
        net.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        kept = state(net)
        assert net.adam_step == 2 and max(np.abs(a).max() for a in kept[2].values()) > 0
        net.set_update_rule('adamw', adam_beta1=0.8, adam_decay=0.0)      # the same kind, other hyper-parameters: kept
        torch.cuda.synchronize()
        assert same_state(state(net), kept) and net.adam_step == 2
        assert net.get_update_rule() == ('adamw', float(np.float32(0.8)), float(np.float32(0.999)), float(np.float32(1e-8)), 0.0)
        net.set_update_rule('momentum')                  # and back: zeroed again
        torch.cuda.synchronize()
        assert net.momentum_flat.abs().max() == 0 and net.adam_step == 0
        assert all((a == 0).all() for a in net.save_second_moment().values())


def _report(net, xt, yt):
    check(lib.ssd_profile_enable(net._h, 1))
    net.train_step_dev(xt, yt)
    torch.cuda.synchronize()
    buf = C.create_string_buffer(1 << 16)
    check(lib.ssd_profile_report(net._h, buf, len(buf)))
    check(lib.ssd_profile_enable(net._h, 0))
    return [ln.split('\t')[0] for ln in buf.value.decode().strip().split('\n') if ln]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_the_default_rule_launches_the_momentum_update(batch, dtype):
    w, xt, yt = batch
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 20, max_batch=B, weights=w, dtype=dtype)
        net.build_optimizer(learning_rate=0.001, weight_decay=WD, momentum=0.9)
        kernels = _report(net, xt, yt)
        assert sum(k.startswith('momentum_update') for k in kernels) == 1 and not any('adamw' in k for k in kernels), kernels
        assert not any('grad_norm' in k for k in kernels)
        adam = _report(make_net(sess, w, dtype), xt, yt)
        assert sum(k.startswith('adamw_update') for k in adam) == 1 and not any('momentum' in k for k in adam), adam
        both = _report(make_net(sess, w, dtype, clip_norm=0.01), xt, yt)
        assert sum(k.startswith('adamw_update_clipped') for k in both) == 1 and sum(k.startswith('grad_norm') for k in both) == 1
        # but for the update's own line the three steps are the same list
        strip = lambda ks: [k for k in ks if not k.startswith(('momentum_update', 'adamw_update', 'grad_norm'))]
        assert strip(kernels) == strip(adam) == strip(both)


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
def test_data_parallel_step_equals_the_plain_step(batch, nccl_group, bucket):
    w, xt, yt = batch
    with Session(0) as sess:
        plain, dp = make_net(sess, w), make_net(sess, w)
        for net in (plain, dp):
            net.set_stream(torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            plain.train_step_dev(xt, yt)
            parallel.train_step_dp(dp, xt, yt, 1, bucket_floats=bucket, force_collectives=True)
        torch.cuda.synchronize()
        assert same_bits(plain.params_flat, dp.params_flat) and same_bits(plain.momentum_flat, dp.momentum_flat)
        assert same_state(state(plain)[2:], state(dp)[2:])
        assert plain.adam_step == dp.adam_step == 2 == dp.global_step


MOMENTUM_KEYS_ONLY = ('__optimizer__', '__adam_beta1__', '__adam_beta2__', '__adam_eps__', '__adam_decay__', '__adam_step__')


def test_checkpoint_round_trip_is_bit_identical(batch, tmp_path):
    w, xt, yt = batch
    path = str(tmp_path / 'adam.npz')
    with Session(0) as sess:
        a = make_net(sess, w, adam_beta1=0.8, adam_beta2=0.99, adam_eps=1e-6, adam_decay=0.02, clip_norm=0.5)
        for _ in range(3):
            a.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        a.save_checkpoint(path)
        with np.load(path, allow_pickle=False) as ck:
            assert str(ck['__optimizer__']) == 'adamw' and int(ck['__adam_step__']) == 3 and int(ck['__global_step__']) == 3
            assert [np.float32(ck[k]) for k in MOMENTUM_KEYS_ONLY[1:5]] == [np.float32(x) for x in (0.8, 0.99, 1e-6, 0.02)]
            names = [k for k, _ in a.variables()]
            assert sorted(k[len('__adam_v__/'):] for k in ck.files if k.startswith('__adam_v__/')) == sorted(names)
            assert sorted(k[len('__momentum__/'):] for k in ck.files if k.startswith('__momentum__/')) == sorted(names)
        b = SSDVGG(sess, 'vgg300')
        b.build_from_metagraph(None, path, max_batch=B, training=True)
        b.build_optimizer_from_metagraph()
        assert b.get_update_rule() == a.get_update_rule() and b.adam_step == 3 and b.get_grad_clip() == 0.5
        assert same_state(state(a), state(b))
        a.train_step_dev(xt, yt)
        b.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        assert same_state(state(a), state(b)) and a.adam_step == b.adam_step == 4
        assert a.get_grad_norm_step() == b.get_grad_norm_step()


def test_a_momentum_checkpoint_holds_its_old_keys_and_loads_as_before(batch, tmp_path):
    w, xt, yt = batch
    path = str(tmp_path / 'mom.npz')
    with Session(0) as sess:
        a = make_net(sess, w, optimizer='momentum')
        a.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        a.save_checkpoint(path)
        with np.load(path, allow_pickle=False) as ck:
            assert not any(k in ck.files for k in MOMENTUM_KEYS_ONLY) and not any(k.startswith('__adam_v__/') for k in ck.files)
        b = SSDVGG(sess, 'vgg300')
        b.build_from_metagraph(None, path, max_batch=B, training=True)
        b.build_optimizer_from_metagraph()
        assert b.get_update_rule()[0] == 'momentum' and b.adam_step == 0
        with pytest.raises(RuntimeError, match='never been under AdamW'):
            b.save_second_moment()
        assert same_bits(a.params_flat, b.params_flat) and same_bits(a.momentum_flat, b.momentum_flat)
        a.train_step_dev(xt, yt)
        b.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        assert same_bits(a.params_flat, b.params_flat) and same_bits(a.momentum_flat, b.momentum_flat)


def test_drivers(tmp_path, capsys):
    """train.py --optimizer adamw for 2 steps, then --continue-training without the flag (continues under adamw, t = 4 at the end);
    the banner names the rule and both decays; a momentum run's banner and checkpoint as before"""
    from ssd_tensorflow_amd import train
    common = ['--batch-size', '4', '--synthetic-train', '8', '--synthetic-valid', '4', '--lr-values', '0.0001;0.00001',
              '--lr-boundaries', '4', '--tensorboard-dir', str(tmp_path / 'tb'), '--checkpoint-interval', '1']
    run = str(tmp_path / 'run')
    assert train.main(['--name', run, '--epochs', '1', '--optimizer', 'adamw', '--adam-decay', '0.02'] + common) == 0
    out = capsys.readouterr().out
    assert 'adamw (beta1 0.9, beta2 0.999, eps 1e-08)' in out.split('[i] Update rule:')[1].splitlines()[0]
    assert out.split('[i] Weight decay:')[1].split()[0] == '0.0' and out.split('[i] Decoupled decay:')[1].split()[0] == '0.02'
    with np.load(run + '/e1.npz', allow_pickle=False) as ck:
        assert str(ck['__optimizer__']) == 'adamw' and int(ck['__adam_step__']) == 2 == int(ck['__global_step__'])
        assert np.float32(ck['__adam_decay__']) == np.float32(0.02) and float(ck['__weight_decay__']) == 0.0
        assert max(np.abs(ck[k]).max() for k in ck.files if k.startswith('__adam_v__/')) > 0
    assert train.main(['--name', run, '--epochs', '2', '--continue-training', 'true'] + common) == 0
    out = capsys.readouterr().out
    assert '--optimizer' not in out                      # (no flag given: nothing to disagree with)
    assert 'adamw' in out.split('[i] Update rule:')[1].splitlines()[0] and out.split('[i] Decoupled decay:')[1].split()[0] == '0.02'
    assert out.split('[i] Weight decay:')[1].split()[0] == '0.0'
    with np.load(run + '/e2.npz', allow_pickle=False) as ck:
        assert str(ck['__optimizer__']) == 'adamw' and int(ck['__adam_step__']) == 4 == int(ck['__global_step__'])
        assert np.float32(ck['__adam_decay__']) == np.float32(0.02) and float(ck['__weight_decay__']) == 0.0
    assert train.main(['--name', str(tmp_path / 'mom'), '--epochs', '1'] + common) == 0
    out = capsys.readouterr().out
    assert out.split('[i] Update rule:')[1].split()[0] == 'momentum' and out.split('[i] Weight decay:')[1].split()[0] == '0.0005'
    assert out.split('[i] Decoupled decay:')[1].split()[0] == 'none'
    with np.load(str(tmp_path / 'mom') + '/e1.npz', allow_pickle=False) as ck:
        assert '__optimizer__' not in ck.files and float(ck['__weight_decay__']) == 0.0005
    assert train.main(['--name', str(tmp_path / 'bad'), '--epochs', '1', '--optimizer', 'adamw', '--adam-beta2', '1.0'] + common) == 1
    assert 'update rule: beta2' in capsys.readouterr().out
