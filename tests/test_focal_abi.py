"""CPU: the loss selection of the C ABI (ssd_set_loss / ssd_get_loss / ssd_op_multibox_loss_ex / ssd_op_multibox_loss_grad_ex):
declared, exported and given ctypes signatures; the enum values; a bad kind, gamma or alpha is refused on the host, before any
device work (every device pointer here is NULL and no GPU is needed), with an error that names the loss; the Python names."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ssd_set_loss', 'ssd_get_loss', 'ssd_op_multibox_loss_ex', 'ssd_op_multibox_loss_grad_ex')


def _header():
    return open(os.path.join(ROOT, 'include', 'ssdvgg_hip.h')).read()


def test_symbols_declared_exported_and_signed():
    from ssd_tensorflow_amd import _lib
    code = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    for n in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % n, code), f'{n} is not declared in include/ssdvgg_hip.h'
        assert hasattr(_lib.lib, n), f'{n} is not exported'
        assert n in _lib.SIGNATURES, f'{n} has no ctypes signature'
    # the _ex forms take the plain forms' arguments, then the configuration, then the stream
    for n in ('ssd_op_multibox_loss', 'ssd_op_multibox_loss_grad'):
        res, args = _lib.SIGNATURES[n]
        res_ex, args_ex = _lib.SIGNATURES[n + '_ex']
        assert res_ex is res and args_ex[:len(args) - 1] == args[:-1] and len(args_ex) == len(args) + 1
    assert re.search(r'typedef\s+struct\s*\{\s*int\s+kind;\s*float\s+focal_gamma;\s*float\s+focal_alpha;\s*\}\s*ssd_loss_config;', code)


def test_enum_values():
    from ssd_tensorflow_amd import ssdvgg
    code = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    assert re.search(r'enum\s*\{\s*SSD_LOSS_MINING\s*=\s*0\s*,\s*SSD_LOSS_FOCAL\s*=\s*1\s*\}', code)
    assert ssdvgg.LOSS_KINDS == {'mining': 0, 'focal': 1}
    assert C.sizeof(ssdvgg.LossConfig) == 12 and [f[0] for f in ssdvgg.LossConfig._fields_] == ['kind', 'focal_gamma', 'focal_alpha']


BAD = [(2, 2.0, 0.25), (-1, 2.0, 0.25), (1, -0.125, 0.25), (1, 5.5, 0.25), (1, float('nan'), 0.25), (1, 2.0, 0.0), (1, 2.0, 1.0),
       (1, 2.0, -0.5), (1, 2.0, float('nan'))]


@pytest.mark.parametrize('bad', BAD, ids=[f'kind {k} gamma {g} alpha {a}' for k, g, a in BAD])
def test_bad_configuration_is_refused_on_the_host(bad):
    from ssd_tensorflow_amd._lib import lib, last_error
    from ssd_tensorflow_amd.ssdvgg import LossConfig
    cfg = LossConfig(*bad)
    hw = (C.c_int * 1)(4); nj = (C.c_int * 1)(4)
    calls = [
        lambda: lib.ssd_set_loss(None, C.byref(cfg)),
        lambda: lib.ssd_op_multibox_loss_ex(1, hw, nj, 20, None, None, None, None, 1, 0, 1, 0.0, None, 0, 0.0, C.byref(cfg), None),
        lambda: lib.ssd_op_multibox_loss_grad_ex(1, hw, nj, 20, None, 0, None, None, None, 1, 0, 1, C.byref(cfg), None),
    ]
    for call in calls:
        assert call() != 0
        assert 'loss' in last_error(), last_error()


def test_null_arguments_are_refused():
    from ssd_tensorflow_amd._lib import lib, last_error
    from ssd_tensorflow_amd.ssdvgg import LossConfig
    assert lib.ssd_get_loss(None, None) != 0 and 'loss' in last_error()
    assert lib.ssd_set_loss(None, None) != 0 and 'loss' in last_error()
    good = LossConfig(1, 2.0, 0.25)
    assert lib.ssd_set_loss(None, C.byref(good)) != 0 and last_error() == 'null handle'       # a good configuration gets further
    assert lib.ssd_get_loss(None, C.byref(good)) != 0 and last_error() == 'null handle'
    # a focal call with null buffers stops at the buffers, a mining one goes to the old entry point's own checks
    hw = (C.c_int * 1)(4); nj = (C.c_int * 1)(4)
    for cfg in (good, LossConfig(0, 9.0, 9.0), None):       # (gamma and alpha are not read under mining)
        ref = None if cfg is None else C.byref(cfg)
        assert lib.ssd_op_multibox_loss_ex(1, hw, nj, 20, None, None, None, None, 1, 0, 1, 0.0, None, 0, 0.0, ref, None) != 0
        assert last_error() == 'null buffer'
        assert lib.ssd_op_multibox_loss_grad_ex(1, hw, nj, 20, None, 0, None, None, None, 1, 0, 1, ref, None) != 0
        assert last_error() == 'null buffer'


def test_python_names():
    from ssd_tensorflow_amd import ssdvgg
    cfg = ssdvgg.loss_config('focal', 1.5, 0.75)
    assert (cfg.kind, cfg.focal_gamma, cfg.focal_alpha) == (1, 1.5, 0.75)
    assert ssdvgg.loss_config().kind == 0 and ssdvgg.loss_config('mining', 9, 9).kind == 0
    for bad in ('Focal', 'ohem', '', None):
        with pytest.raises(ValueError, match='loss'):
            ssdvgg.loss_config(bad)
    for g, a in ((-1, 0.25), (5.01, 0.25), (2, 0), (2, 1), (float('nan'), 0.25)):
        with pytest.raises(ValueError, match='loss'):
            ssdvgg.loss_config('focal', g, a)
    # build_optimizer refuses a bad name before it touches the handle
    import inspect
    sig = inspect.signature(ssdvgg.SSDVGG.build_optimizer)
    assert [sig.parameters[k].default for k in ('loss', 'focal_gamma', 'focal_alpha')] == ['mining', 2.0, 0.25]
    assert inspect.signature(ssdvgg.SSDVGG.build_from_vgg).parameters['background_prior'].default is None
    net = ssdvgg.SSDVGG(None, 'vgg300')
    net.training = True
    with pytest.raises(ValueError, match='loss'):
        net.build_optimizer(loss='hinge')


def test_checkpoint_without_the_keys_is_mining(tmp_path):
    import numpy as np
    from ssd_tensorflow_amd import ssdvgg, train
    p = str(tmp_path / 'old.npz')
    np.savez(p, __match__=np.array('paper'))
    assert train.checkpoint_loss(p) == ('mining', 2.0, 0.25)
    np.savez(p, __loss__=np.array('focal'), __focal_gamma__=np.array(1.5), __focal_alpha__=np.array(0.5))
    assert train.checkpoint_loss(p) == ('focal', 1.5, 0.5)
    with np.load(p) as ck:
        assert ssdvgg.checkpoint_loss(ck) == ('focal', 1.5, 0.5)
