"""-m gpu: the weight EMA through the handle (ssd_set_ema) at vgg300, batch 2, fp32 and bf16.  After every one of three
consecutive steps the float32 oracle of tests/ema_ref.py on host copies of the previous average and the new weights gives, bit for
bit, what the update's EMA kernel leaves -- under momentum and AdamW, plain and clipped.  The copies go by variable (ssd_save_ema /
ssd_save_variable): the update is element-wise.  Then: a NaN in the gradient arena skips the update under clipping while the average
still moves and counts; enabling copies the weights, off-and-on copies again, the same decay set again keeps the state; inside
averaged_weights() a forward pass has the bits of the same handle's forward after load_variables(save_ema()) -- which is what shows
that no mirror, quantised image or filter transform survives the swap -- and leaving restores everything; the refusals while
swapped; the default handle launches no EMA kernel and the EMA adds exactly one; the data-parallel step over a single-rank RCCL group
leaves the plain step's average; checkpoints resume bit-identically and load either set; the drivers."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

import ema_ref as er
from oracle import boxes as ob
from oracle import ssdvgg_ref as ref
from ssd_tensorflow_amd import parallel
from ssd_tensorflow_amd._lib import lib, check, np_ptr
from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session

pytestmark = pytest.mark.gpu
WD = 0.0005
B = 2
DECAY = 0.9
EMA_KEYS = ('__ema_decay__', '__ema_step__')


@pytest.fixture(scope='module')
def batch():
    """(weights, x, y device tensors): computed once, never modified"""
    preset = ob.get_preset('vgg300')
    w = ref.init_params(preset, 20, seed=42, alive=True)
    x, y, _ = ref.synth_batch(np.random.default_rng(1234), B, preset)
    return w, torch.tensor(x).cuda(), torch.tensor(y).cuda()


def make_net(sess, w, dtype='f32', ema_decay=DECAY, **opt):
    net = SSDVGG(sess, 'vgg300')
    net.build_from_vgg(None, 20, max_batch=B, weights=w, dtype=dtype)
    net.build_optimizer(learning_rate=0.001, weight_decay=WD, momentum=0.9, ema_decay=ema_decay, **opt)
    return net


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def same(a, b):
    """two {variable: array} with the same bits"""
    return a.keys() == b.keys() and all(a[k].tobytes() == b[k].tobytes() for k in a)


def oracle(prev, weights, decay, t):
    return {k: er.ema(prev[k].ravel(), weights[k].ravel(), decay, t).reshape(prev[k].shape) for k in prev}


@pytest.mark.parametrize('clip', [False, True], ids=['plain', 'clipped'])
@pytest.mark.parametrize('optimizer', ['momentum', 'adamw'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_three_steps_have_the_bits_of_the_oracle(batch, dtype, optimizer, clip):
    w, xt, yt = batch
    with Session(0) as sess:
        net = make_net(sess, w, dtype, optimizer=optimizer, clip_norm=0.5 if clip else 0.0)
        assert net.get_ema() == (float(np.float32(DECAY)), 0, False)
        avg = net.save_ema()
        assert same(avg, net.save_variables())               # enabling copied the weights
        for t in range(3):
            net.train_step_dev(xt, yt)
            torch.cuda.synchronize()
            weights = net.save_variables()
            want = oracle(avg, weights, DECAY, t)
            got = net.save_ema()
            bad = [k for k in got if got[k].tobytes() != want[k].tobytes()]
            print(f'{dtype} {optimizer} t {t}: {len(bad)} of {len(got)} variables differ {bad[:3]}')
            assert same(got, want)
            assert not same(got, avg) and not same(got, weights)
            assert net.get_ema() == (float(np.float32(DECAY)), t + 1, False) and net.global_step == t + 1
            if clip:
                assert net.get_grad_norm_step()[1] > 0.0
            avg = got


@pytest.mark.parametrize('optimizer', ['momentum', 'adamw'])
def test_a_skipped_update_still_moves_the_average_and_counts(batch, optimizer):
    w, xt, yt = batch
    with Session(0) as sess:
        net = make_net(sess, w, optimizer=optimizer, clip_norm=0.01)
        net.train_step_dev(xt, yt)
        net.forward_backward_dev(xt, yt)
        torch.cuda.synchronize()
        net.grads_flat[net.grads_flat.numel() // 2] = float('nan')
        torch.cuda.synchronize()
        weights, avg = net.save_variables(), net.save_ema()
        assert not same(weights, avg)
        net.apply_gradients_dev()
        torch.cuda.synchronize()
        norm, f = net.get_grad_norm_step()
        assert f == 0.0 and not np.isfinite(norm)
        assert same(net.save_variables(), weights)                       # the update touched nothing ...
        got = net.save_ema()
        assert same(got, oracle(avg, weights, DECAY, 1)) and not same(got, avg)      # ... and the average followed, as t = 1
        assert net.get_ema()[1] == 2 == net.global_step


def test_enabling_switching_off_and_on(batch):
    w, xt, yt = batch
    with Session(0) as sess:
        net = make_net(sess, w, ema_decay=0.0)
        assert net.get_ema() == (0.0, 0, False)
        with pytest.raises(RuntimeError, match='never been under a weight EMA'):
            net.save_ema()
        with pytest.raises(RuntimeError, match='weight EMA: nothing to swap'):
            net.swap_ema()
        with net.averaged_weights() as on:                   # off: nothing happens, no branch needed
            assert on is False and net.get_ema()[2] is False
        net.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        net.set_ema(DECAY)                                   # enabling copies the weights; t = 0
        torch.cuda.synchronize()
        assert same(net.save_ema(), net.save_variables()) and net.get_ema() == (float(np.float32(DECAY)), 0, False)
        net.train_step_dev(xt, yt)
        net.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        kept = net.save_ema()
        assert net.get_ema()[1] == 2 and not same(kept, net.save_variables())
        net.set_ema(DECAY)                                   # the same decay again: kept
        torch.cuda.synchronize()
        assert same(net.save_ema(), kept) and net.get_ema()[1] == 2
        net.set_ema(0.999)                                   # another decay while on: kept too
        torch.cuda.synchronize()
        assert same(net.save_ema(), kept) and net.get_ema() == (float(np.float32(0.999)), 2, False)
        net.set_ema(0.0)                                     # off: the arena stays, and stays put
        net.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        assert same(net.save_ema(), kept) and net.get_ema()[0] == 0.0
        net.set_ema(DECAY)                                   # on again: copied again, t = 0
        torch.cuda.synchronize()
        assert same(net.save_ema(), net.save_variables()) and not same(net.save_ema(), kept) and net.get_ema()[1] == 0


def _forward(net, xt, yt):
    """(result, detections) of one forward pass through eval_op and detect_last"""
    res, _ = net.eval_step(xt, yt, want_losses=False)
    thr = float(np.quantile(res[:, :, :20].max(-1), 0.999))
    return res, net.detect_last(B, thr, None, 200)


def _same_detections(a, b):
    return all(x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_swap(batch, dtype):
    w, xt, yt = batch
    with Session(0) as sess:
        net = make_net(sess, w, dtype)
        for _ in range(2):
            net.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        raw, avg = net.save_variables(), net.save_ema()
        res_raw, det_raw = _forward(net, xt, yt)
        with net.averaged_weights() as on:
            # first thing behind the swap, nothing synchronised in between: an inference pass on device tensors.  In fp32 at this
            # batch size it is the pass whose side stream does not wait for the main stream on its own: the swap orders it
            inf_in = net.infer(xt)
            assert on is True and net.get_ema() == (float(np.float32(DECAY)), 2, True)
            res_in, det_in = _forward(net, xt, yt)
            assert same(net.save_variables(), avg) and same(net.save_ema(), raw)      # save_variable returns the average
            with net.averaged_weights() as inner:                                     # a block inside the block: still averaged
                assert inner is False and net.get_ema()[2] is True
            assert net.get_ema()[2] is True
            a = np.zeros(raw['conv1_1/biases'].shape, np.float32)
            for call in (lambda: net.apply_gradients_dev(),
                         lambda: net.train_step_dev(xt, yt),
                         lambda: net.forward_backward_dev(xt, yt),
                         lambda: list(net.backward_staged(yt, B, 1 << 20)),
                         lambda: net.null_gradients_dev(),
                         lambda: net.load_variables({'conv1_1/biases': a}),
                         lambda: net.set_ema(0.99),
                         lambda: net.set_ema(0.0),
                         lambda: check(lib.ssd_load_ema(net._h, b'conv1_1/biases', np_ptr(a), a.size)),
                         lambda: check(lib.ssd_set_ema_step(net._h, 5)),
                         lambda: net.save_checkpoint('refused.npz')):
                with pytest.raises(RuntimeError, match='^weight EMA:'):
                    call()
            assert net.get_ema() == (float(np.float32(DECAY)), 2, True) and net.global_step == 2
            assert same(net.save_variables(), avg) and same(net.save_ema(), raw)      # the refused calls touched nothing
        # left: parameters, average and the forward pass as they were, bit for bit
        assert net.get_ema() == (float(np.float32(DECAY)), 2, False)
        assert same(net.save_variables(), raw) and same(net.save_ema(), avg)
        # the last forward pass made its mirrors and filter transforms from the average: no backward behind it
        with pytest.raises(RuntimeError, match='^weight EMA: backward is refused behind a forward pass'):
            list(net.backward_staged(yt, B, 1 << 20))
        with pytest.raises(RuntimeError, match='^weight EMA: backward is refused behind a forward pass'):
            check(lib.ssd_backward_begin_dev(net._h, yt.data_ptr(), B))
        inf_raw = net.infer(xt)
        assert inf_raw.tobytes() != inf_in.tobytes()
        res_back, det_back = _forward(net, xt, yt)
        assert res_back.tobytes() == res_raw.tobytes() and _same_detections(det_back, det_raw)
        # an exception leaves it too
        with pytest.raises(KeyError):
            with net.averaged_weights():
                raise KeyError('inside')
        assert net.get_ema()[2] is False and same(net.save_variables(), raw) and same(net.save_ema(), avg)
        # the same handle with the average LOADED as its weights: every derived copy is made from them by the pass
        net.load_variables(avg)
        inf_loaded = net.infer(xt)
        print(f'{dtype}: inference pass right behind the swap differs from the one on the loaded average in '
              f'{int((inf_in.view(np.uint32) != inf_loaded.view(np.uint32)).sum())} of {inf_in.size} values')
        assert inf_in.tobytes() == inf_loaded.tobytes()
        res_loaded, det_loaded = _forward(net, xt, yt)
        print(f'{dtype}: max |averaged - raw| of the result {np.abs(res_in - res_raw).max():.3e}')
        assert res_in.tobytes() == res_loaded.tobytes() and _same_detections(det_in, det_loaded)
        assert res_in.tobytes() != res_raw.tobytes()
        # ... and training goes on from the raw weights after a swap pair
        net.load_variables(raw)
        assert net.infer(xt).tobytes() == inf_raw.tobytes()
        net.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        assert net.get_ema()[1] == 3 and same(net.save_ema(), oracle(avg, net.save_variables(), DECAY, 2))


def _report(net, xt, yt):
    check(lib.ssd_profile_enable(net._h, 1))
    net.train_step_dev(xt, yt)
    torch.cuda.synchronize()
    buf = C.create_string_buffer(1 << 16)
    check(lib.ssd_profile_report(net._h, buf, len(buf)))
    check(lib.ssd_profile_enable(net._h, 0))
    return [ln.split('\t')[0] for ln in buf.value.decode().strip().split('\n') if ln]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_the_default_handle_launches_no_ema_kernel(batch, dtype):
    w, xt, yt = batch
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 20, max_batch=B, weights=w, dtype=dtype)
        net.build_optimizer(learning_rate=0.001, weight_decay=WD, momentum=0.9)
        kernels = _report(net, xt, yt)
        assert sum(k.startswith('momentum_update') for k in kernels) == 1 and not any('ema_' in k for k in kernels), kernels
        with_ema = _report(make_net(sess, w, dtype), xt, yt)
        assert sum(k == 'ema_update' for k in with_ema) == 1 and sum('ema_' in k for k in with_ema) == 1, with_ema
        # but for that one line the two steps are the same list
        assert [k for k in with_ema if k != 'ema_update'] == kernels


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.fixture(scope='module')
def nccl_group():
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()))
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    yield
    dist.destroy_process_group()


def test_data_parallel_step_leaves_the_plain_steps_average(batch, nccl_group):
    w, xt, yt = batch
    with Session(0) as sess:
        plain, dp = make_net(sess, w), make_net(sess, w)
        for net in (plain, dp):
            net.set_stream(torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            plain.train_step_dev(xt, yt)
            parallel.train_step_dp(dp, xt, yt, 1, bucket_floats=4_000_000, force_collectives=True)
        torch.cuda.synchronize()
        assert same_bits(plain.params_flat, dp.params_flat)
        assert same(plain.save_ema(), dp.save_ema()) and not same(dp.save_ema(), dp.save_variables())
        assert plain.get_ema() == dp.get_ema() == (float(np.float32(DECAY)), 2, False)


def test_checkpoint_round_trip_is_bit_identical(batch, tmp_path):
    w, xt, yt = batch
    path = str(tmp_path / 'ema.npz')
    with Session(0) as sess:
        a = make_net(sess, w, ema_decay=0.75)
        for _ in range(3):
            a.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        a.save_checkpoint(path)
        names = [k for k, _ in a.variables()]
        with np.load(path, allow_pickle=False) as ck:
            assert np.float32(ck['__ema_decay__']) == np.float32(0.75) and ck['__ema_decay__'].dtype == np.float32
            assert int(ck['__ema_step__']) == 3 == int(ck['__global_step__']) and ck['__ema_step__'].dtype == np.int64
            assert sorted(k[len('__ema__/'):] for k in ck.files if k.startswith('__ema__/')) == sorted(names)
            assert all(ck['__ema__/' + k].tobytes() == v.tobytes() for k, v in a.save_ema().items())
        b = SSDVGG(sess, 'vgg300')
        b.build_from_metagraph(None, path, max_batch=B, training=True)       # training: the raw weights are the parameters
        assert b.weights == 'raw'
        b.build_optimizer_from_metagraph()
        assert b.get_ema() == a.get_ema() == (0.75, 3, False)
        assert same(a.save_variables(), b.save_variables()) and same(a.save_momentum(), b.save_momentum()) and same(a.save_ema(), b.save_ema())
        a.train_step_dev(xt, yt)
        b.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        assert same(a.save_variables(), b.save_variables()) and same(a.save_momentum(), b.save_momentum()) and same(a.save_ema(), b.save_ema())
        assert a.get_ema() == b.get_ema() == (0.75, 4, False)
        assert not same(b.save_ema(), b.save_variables())


def test_a_checkpoint_without_the_average_holds_its_old_keys_and_loads_as_before(batch, tmp_path):
    w, xt, yt = batch
    path, path_ema = str(tmp_path / 'plain.npz'), str(tmp_path / 'ema.npz')
    with Session(0) as sess:
        a = make_net(sess, w, ema_decay=0.0)
        e = make_net(sess, w)
        for net in (a, e):
            net.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        a.save_checkpoint(path)
        e.save_checkpoint(path_ema)
        with np.load(path, allow_pickle=False) as ck, np.load(path_ema, allow_pickle=False) as cke:
            assert not any(k in ck.files for k in EMA_KEYS) and not any(k.startswith('__ema__/') for k in ck.files)
            # exactly the keys it wrote before: the other file's without the new ones
            assert sorted(ck.files) == sorted(k for k in cke.files if k not in EMA_KEYS and not k.startswith('__ema__/'))
        b = SSDVGG(sess, 'vgg300')
        b.build_from_metagraph(None, path, max_batch=B, training=True)
        b.build_optimizer_from_metagraph()
        assert b.get_ema() == (0.0, 0, False)
        with pytest.raises(RuntimeError, match='never been under a weight EMA'):
            b.save_ema()
        assert same_bits(a.params_flat, b.params_flat) and same_bits(a.momentum_flat, b.momentum_flat)
        for mode in ('auto', 'raw'):
            c = SSDVGG(sess, 'vgg300')
            c.build_from_metagraph(None, path, max_batch=B, weights=mode)
            assert c.weights == 'raw' and same(c.save_variables(), a.save_variables())
        with pytest.raises(ValueError, match="weights='ema'"):
            SSDVGG(sess, 'vgg300').build_from_metagraph(None, path, max_batch=B, weights='ema')
        with pytest.raises(ValueError, match="weights='ema'"):
            SSDVGG(sess, 'vgg300').build_from_metagraph(None, path, max_batch=B, weights='ema', training=True)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_inference_handles_take_the_average_by_default(batch, tmp_path, dtype):
    w, xt, yt = batch
    path = str(tmp_path / 'ema.npz')
    with Session(0) as sess:
        a = make_net(sess, w)
        for _ in range(2):
            a.train_step_dev(xt, yt)
        torch.cuda.synchronize()
        a.save_checkpoint(path)
        res = {}
        for mode in ('auto', 'ema', 'raw'):
            net = SSDVGG(sess, 'vgg300')
            net.build_from_metagraph(None, path, max_batch=B, dtype=dtype, weights=mode)
            assert net.weights == ('raw' if mode == 'raw' else 'ema')
            assert same(net.save_variables(), a.save_variables() if mode == 'raw' else a.save_ema())
            res[mode] = net.infer(xt)
            net.close()
        assert res['auto'].tobytes() == res['ema'].tobytes() and res['auto'].tobytes() != res['raw'].tobytes()


def test_drivers(tmp_path, capsys):
    """train.py --ema-decay 0.9 on the tiny synthetic set for two epochs, then --continue-training without the flag keeps the decay;
    infer.py on either set and detect.py in bf16 run on the result"""
    from ssd_tensorflow_amd import train, infer, detect
    common = ['--batch-size', '4', '--synthetic-train', '8', '--synthetic-valid', '4', '--lr-values', '0.0001;0.00001',
              '--lr-boundaries', '4', '--tensorboard-dir', str(tmp_path / 'tb'), '--checkpoint-interval', '1']
    run = str(tmp_path / 'run')
    assert train.main(['--name', run, '--epochs', '2', '--ema-decay', '0.9'] + common) == 0
    out = capsys.readouterr().out
    assert 'decay 0.9' in out.split('[i] Weight EMA:')[1].splitlines()[0]
    assert 'validation (averaged)' in out.split('[i] mAP ')[1].splitlines()[0]
    assert os.path.isfile(str(tmp_path / 'tb' / 'run' / 'scalars.jsonl'))
    tags = open(str(tmp_path / 'tb' / 'run' / 'scalars.jsonl')).read()
    assert '"validation (averaged)_total_loss"' in tags and '"validation_total_loss"' not in tags and '"training_total_loss"' in tags
    with np.load(run + '/e2.npz', allow_pickle=False) as ck:
        assert np.float32(ck['__ema_decay__']) == np.float32(0.9) and int(ck['__ema_step__']) == 4 == int(ck['__global_step__'])
        assert any(ck['__ema__/' + k].tobytes() != ck[k].tobytes() for k in ck.files if not k.startswith('__'))
    assert train.main(['--name', run, '--epochs', '3', '--continue-training', 'true'] + common) == 0
    out = capsys.readouterr().out
    assert '--ema-decay' not in out                      # (no flag given: nothing to disagree with)
    assert 'decay 0.9' in out.split('[i] Weight EMA:')[1].splitlines()[0] and 'validation (averaged)' in out
    with np.load(run + '/e3.npz', allow_pickle=False) as ck:
        assert np.float32(ck['__ema_decay__']) == np.float32(0.9) and int(ck['__ema_step__']) == 6 == int(ck['__global_step__'])
    # a run without the flag: the banner says off, the line and the tags are the old ones
    assert train.main(['--name', str(tmp_path / 'off'), '--epochs', '2'] + common) == 0
    out = capsys.readouterr().out
    assert out.split('[i] Weight EMA:')[1].split()[0] == 'off' and 'averaged' not in out and '  validation ' in out.split('[i] mAP ')[1].splitlines()[0]
    with np.load(str(tmp_path / 'off') + '/e2.npz', allow_pickle=False) as ck:
        assert not any(k.startswith('__ema') for k in ck.files)
    assert train.main(['--name', str(tmp_path / 'bad'), '--epochs', '1', '--ema-decay', '1.0'] + common) == 1
    assert 'weight EMA: decay' in capsys.readouterr().out
    # inference on the result: either set, and another dtype
    for weights in ('ema', 'raw'):
        assert infer.main(['--name', run, '--synthetic', '4', '--batch-size', '4', '--weights', weights,
                           '--output-dir', str(tmp_path / ('out_' + weights))]) == 0
        assert out_weights(capsys.readouterr().out) == weights
    assert infer.main(['--name', str(tmp_path / 'off'), '--synthetic', '4', '--batch-size', '4', '--weights', 'ema',
                       '--output-dir', str(tmp_path / 'out_none')]) == 1
    assert "weights='ema'" in capsys.readouterr().out
    np.save(str(tmp_path / 'img.npy'), np.random.default_rng(5).integers(0, 256, (300, 300, 3)).astype(np.float32))
    assert detect.main(['--model', run + '/final.npz', '--dtype', 'bf16', '--batch-size', '4', '--output-dir', str(tmp_path / 'det'),
                        str(tmp_path / 'img')]) == 0
    assert out_weights(capsys.readouterr().out) == 'ema'


def out_weights(out):
    return out.split('[i] Weights:')[1].split()[0]
