"""CPU: gradient clipping in the C ABI (ssd_set_grad_clip / ssd_get_grad_clip / ssd_get_grad_norm_step / ssd_op_grad_norm_ws_bytes /
ssd_op_momentum_update_clipped): declared, exported and given ctypes signatures; the struct; a negative or NaN max_norm is refused on
the host, before any device work (every device pointer here is NULL and no GPU is needed), with an error that names gradient
clipping, while 0 and +inf get as far as the null-handle / null-buffer check; the Python names and defaults, the checkpoint helper
and the driver's flag."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_INT = ('ssd_set_grad_clip', 'ssd_get_grad_clip', 'ssd_get_grad_norm_step', 'ssd_op_momentum_update_clipped')
NEW = NEW_INT + ('ssd_op_grad_norm_ws_bytes',)
INF = float('inf')


def _code():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ssdvgg_hip.h')).read(), flags=re.S)


def test_symbols_declared_exported_and_signed():
    from ssd_tensorflow_amd import _lib
    code = _code()
    for n in NEW:
        assert re.search(r'\b%s\s+%s\s*\(' % ('int' if n in NEW_INT else 'size_t', n), code), f'{n} is not declared in include/ssdvgg_hip.h'
        assert hasattr(_lib.lib, n), f'{n} is not exported'
        assert n in _lib.SIGNATURES, f'{n} has no ctypes signature'
    assert re.search(r'typedef\s+struct\s*\{\s*float\s+max_norm;\s*\}\s*ssd_grad_clip_config;', code)
    assert re.search(r'ssd_set_grad_clip\s*\(\s*ssd_handle\s+h\s*,\s*const\s+ssd_grad_clip_config\s*\*\s*cfg\s*\)', code)
    assert re.search(r'ssd_get_grad_norm_step\s*\(\s*ssd_handle\s+h\s*,\s*int\s+steps_back\s*,\s*float\s+out\[2\]\s*\)', code)
    assert re.search(r'ssd_op_momentum_update_clipped\s*\(\s*float\s*\*\s*w\s*,\s*float\s*\*\s*acc\s*,\s*const\s+float\s*\*\s*g\s*,\s*size_t\s+n\s*,'
                     r'\s*float\s+lr\s*,\s*float\s+momentum\s*,\s*float\s+grad_scale\s*,\s*float\s+max_norm\s*,\s*void\s*\*\s*ws_dev\s*,'
                     r'\s*float\s*\*\s*report_dev\s*,\s*void\s*\*\s*stream\s*\)', code)
    res, args = _lib.SIGNATURES['ssd_op_momentum_update_clipped']
    assert res is C.c_int and len(args) == 11 and args[3] is C.c_size_t and args[4:8] == [C.c_float] * 4
    assert _lib.SIGNATURES['ssd_op_grad_norm_ws_bytes'] == (C.c_size_t, [C.c_size_t])
    # the contract comment names what the tests hold the kernels to
    text = open(os.path.join(ROOT, 'include', 'ssdvgg_hip.h')).read()
    for word in ('gradient clipping', 'fp64', 'max_norm / norm', 'skipped', 'global_step still advances', '+inf'):
        assert word in text, word


def test_struct_and_names():
    from ssd_tensorflow_amd import ssdvgg, train, summaries
    assert C.sizeof(ssdvgg.GradClipConfig) == 4 and [f[0] for f in ssdvgg.GradClipConfig._fields_] == ['max_norm']
    assert ssdvgg.grad_clip_config().max_norm == 0.0
    assert ssdvgg.grad_clip_config(2.5).max_norm == 2.5 and ssdvgg.grad_clip_config(INF).max_norm == INF
    assert [p.default for p in inspect.signature(ssdvgg.grad_clip_config).parameters.values()] == [0.0]
    assert inspect.signature(ssdvgg.SSDVGG.build_optimizer).parameters['clip_norm'].default == 0.0
    assert inspect.signature(ssdvgg.SSDVGG.get_grad_norm_step).parameters['steps_back'].default == 0
    for name in ('set_grad_clip', 'get_grad_clip', 'get_grad_norm_step'):
        assert hasattr(ssdvgg.SSDVGG, name)
    assert callable(train.checkpoint_clip_norm) and callable(ssdvgg.checkpoint_clip_norm)
    assert ssdvgg.LOSS_NAMES == ('total', 'localization', 'confidence', 'l2')          # the four-value loss contract stays
    assert hasattr(summaries, 'GradNormSummary')


def test_python_refuses_a_bad_value_by_name():
    from ssd_tensorflow_amd import ssdvgg
    for bad in (-1.0, -1e-30, float('nan'), -INF):
        with pytest.raises(ValueError, match='gradient clipping'):
            ssdvgg.grad_clip_config(bad)
    net = ssdvgg.SSDVGG(None, 'vgg300')
    with pytest.raises(ValueError, match='gradient clipping'):
        net.set_grad_clip(-2.0)


BAD = [-1.0, float('nan'), -INF]


@pytest.mark.parametrize('bad', BAD, ids=['max_norm %s' % b for b in BAD])
def test_bad_max_norm_is_refused_on_the_host(bad):
    from ssd_tensorflow_amd._lib import lib, last_error
    from ssd_tensorflow_amd.ssdvgg import GradClipConfig
    cfg = GradClipConfig(bad)
    for call in (lambda: lib.ssd_set_grad_clip(None, C.byref(cfg)),
                 lambda: lib.ssd_op_momentum_update_clipped(None, None, None, 1024, 1e-3, 0.9, 1.0, bad, None, None, None)):
        assert call() != 0
        assert 'gradient clipping' in last_error(), last_error()


@pytest.mark.parametrize('good', [0.0, INF, 1.5], ids=['off', 'inf', 'finite'])
def test_good_max_norm_gets_to_the_null_checks(good):
    from ssd_tensorflow_amd._lib import lib, last_error
    from ssd_tensorflow_amd.ssdvgg import GradClipConfig
    cfg = GradClipConfig(good)
    assert lib.ssd_set_grad_clip(None, C.byref(cfg)) != 0 and last_error() == 'null handle'
    assert lib.ssd_get_grad_clip(None, C.byref(cfg)) != 0 and last_error() == 'null handle'
    assert lib.ssd_op_momentum_update_clipped(None, None, None, 1024, 1e-3, 0.9, 1.0, good, None, None, None) != 0
    assert last_error() == 'null buffer'


def test_null_arguments_are_refused():
    from ssd_tensorflow_amd._lib import lib, last_error
    assert lib.ssd_set_grad_clip(None, None) != 0 and 'gradient clipping' in last_error()
    assert lib.ssd_get_grad_clip(None, None) != 0 and 'gradient clipping' in last_error()
    out = (C.c_float * 2)()
    assert lib.ssd_get_grad_norm_step(None, 0, out) != 0 and last_error() == 'null handle'


def test_workspace_size_follows_the_grid():
    """16 bytes of state and one double per block of the norm pass: blocks = ceil(groups / 256), at most 4096"""
    import clip_ref as cr
    from ssd_tensorflow_amd._lib import lib
    def blocks(n):
        return (lib.ssd_op_grad_norm_ws_bytes(n) - 16) // 8
    assert lib.ssd_op_grad_norm_ws_bytes(4) == 24
    assert [blocks(n) for n in (4, 1020, cr.BLOCK_FLOATS, cr.BLOCK_FLOATS + 4)] == [1, 1, 1, 2]
    assert [blocks(n) for n in (cr.GRID_FLOATS - 4, cr.GRID_FLOATS, cr.GRID_FLOATS + 4, 8 * cr.GRID_FLOATS)] == [cr.GRID_CAP] * 4
    assert blocks(cr.GRID_FLOATS - cr.BLOCK_FLOATS) == cr.GRID_CAP - 1


def test_checkpoint_without_the_key_is_off(tmp_path):
    from ssd_tensorflow_amd import ssdvgg, train
    p = str(tmp_path / 'old.npz')
    np.savez(p, __match__=np.array('paper'), __loc_loss__=np.array('giou'), __loc_weight__=np.array(2.5))
    assert train.checkpoint_clip_norm(p) == 0.0
    assert train.checkpoint_loc_loss(p) == ('giou', 2.5)
    np.savez(p, __clip_norm__=np.array(7.5))
    assert train.checkpoint_clip_norm(p) == 7.5
    np.savez(p, __clip_norm__=np.array(INF))
    with np.load(p) as ck:
        assert ssdvgg.checkpoint_clip_norm(ck) == INF


def test_grad_norm_summary(tmp_path):
    from ssd_tensorflow_amd.summaries import GradNormSummary, SummaryWriter
    import json
    w = SummaryWriter(str(tmp_path))
    s = GradNormSummary(w, updates=10)
    for nf in ((2.0, 1.0), (8.0, 0.5), (float('nan'), 0.0), (4.0, 1.0), (6.0, 0.75)):
        s.add(*nf)
    assert s.push(1) == dict(median=5.0, max=8.0, clipped=2, skipped=1, updates=5)
    assert s.push(2) == dict(median=0.0, max=0.0, clipped=0, skipped=0, updates=0)
    w.close()
    rows = [json.loads(line) for line in open(w.path)]
    assert [(r['value'], r['step']) for r in rows if r['tag'] == 'grad_norm'] == [(2.0, 11), (8.0, 12), (4.0, 14), (6.0, 15)]
    assert {r['tag']: r['value'] for r in rows if r['step'] == 1 and r['tag'] != 'grad_norm'} == \
        {'grad_norm_median': 5.0, 'grad_norm_max': 8.0, 'grad_clipped': 2.0, 'grad_skipped': 1.0}


def test_train_help_lists_the_flag(capsys):
    from ssd_tensorflow_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(['--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert '--clip-norm' in out and 'inf' in out
