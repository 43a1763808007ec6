"""CPU: the localization-loss selection of the C ABI (ssd_set_loc_loss / ssd_get_loc_loss / ssd_op_multibox_loss_ex2 /
ssd_op_multibox_loss_grad_ex2): declared, exported and given ctypes signatures; the enum values and the struct; a bad kind or weight
is refused on the host, before any device work (every device pointer here is NULL and no GPU is needed), with an error that names
the localization loss; the Python names, the checkpoint helper and the driver's flags."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ssd_set_loc_loss', 'ssd_get_loc_loss', 'ssd_op_multibox_loss_ex2', 'ssd_op_multibox_loss_grad_ex2')


def _code():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ssdvgg_hip.h')).read(), flags=re.S)


def test_symbols_declared_exported_and_signed():
    from ssd_tensorflow_amd import _lib
    code = _code()
    for n in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % n, code), f'{n} is not declared in include/ssdvgg_hip.h'
        assert hasattr(_lib.lib, n), f'{n} is not exported'
        assert n in _lib.SIGNATURES, f'{n} has no ctypes signature'
    # the _ex2 forms take the _ex forms' arguments, then the localization configuration, then the stream
    for n in ('ssd_op_multibox_loss', 'ssd_op_multibox_loss_grad'):
        res, args = _lib.SIGNATURES[n + '_ex']
        res2, args2 = _lib.SIGNATURES[n + '_ex2']
        assert res2 is res and args2[:len(args) - 1] == args[:-1] and len(args2) == len(args) + 1
        assert re.search(r'%s_ex2\s*\([^)]*const\s+ssd_loss_config\s*\*\s*cfg\s*,\s*const\s+ssd_loc_loss_config\s*\*\s*loc\s*,\s*void\s*\*\s*stream\s*\)'
                         % n, code)
    assert re.search(r'typedef\s+struct\s*\{\s*int\s+kind;\s*float\s+weight;\s*\}\s*ssd_loc_loss_config;', code)
    assert re.search(r'enum\s*\{\s*SSD_LOC_SMOOTH_L1\s*=\s*0\s*,\s*SSD_LOC_GIOU\s*=\s*1\s*\}', code)
    # ssd_loss_config keeps its layout
    assert re.search(r'typedef\s+struct\s*\{\s*int\s+kind;\s*float\s+focal_gamma;\s*float\s+focal_alpha;\s*\}\s*ssd_loss_config;', code)


def test_struct_and_names():
    from ssd_tensorflow_amd import ssdvgg
    assert ssdvgg.LOC_LOSS_KINDS == {'smooth_l1': 0, 'giou': 1}
    assert C.sizeof(ssdvgg.LocLossConfig) == 8 and [f[0] for f in ssdvgg.LocLossConfig._fields_] == ['kind', 'weight']
    assert C.sizeof(ssdvgg.LossConfig) == 12
    cfg = ssdvgg.loc_loss_config('giou', 2.5)
    assert (cfg.kind, cfg.weight) == (1, 2.5)
    d = ssdvgg.loc_loss_config()
    assert (d.kind, d.weight) == (0, 1.0)
    s = ssdvgg.loc_loss_config('smooth_l1', 7.0)          # ignored under smooth_l1, stored as 1
    assert (s.kind, s.weight) == (0, 1.0)
    sig = inspect.signature(ssdvgg.SSDVGG.build_optimizer)
    assert [sig.parameters[k].default for k in ('loss', 'focal_gamma', 'focal_alpha', 'loc_loss', 'loc_weight')] == \
        ['mining', 2.0, 0.25, 'smooth_l1', 1.0]
    assert [p.default for p in inspect.signature(ssdvgg.loc_loss_config).parameters.values()] == ['smooth_l1', 1.0]
    assert hasattr(ssdvgg.SSDVGG, 'set_loc_loss') and hasattr(ssdvgg.SSDVGG, 'get_loc_loss')


def test_python_refuses_a_bad_configuration_by_name():
    from ssd_tensorflow_amd import ssdvgg
    for w in (0, 0.0, -1.0, float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match='localization loss'):
            ssdvgg.loc_loss_config('giou', w)
    for bad in ('GIoU', 'diou', 'ciou', 'iou', '', None):
        with pytest.raises(ValueError, match='localization loss'):
            ssdvgg.loc_loss_config(bad)
    # build_optimizer refuses before it touches the handle's localization loss: set_loss comes first and needs a handle, so the
    # configuration is checked on its own here
    net = ssdvgg.SSDVGG(None, 'vgg300')
    with pytest.raises(ValueError, match='localization loss'):
        net.set_loc_loss('giou', 0.0)
    with pytest.raises(ValueError, match='localization loss'):
        net.set_loc_loss('l2')


BAD = [(2, 1.0), (-1, 1.0), (1, 0.0), (1, -1.0), (1, float('nan')), (1, float('inf')), (1, -float('inf'))]


@pytest.mark.parametrize('bad', BAD, ids=[f'kind {k} weight {w}' for k, w in BAD])
def test_bad_configuration_is_refused_on_the_host(bad):
    from ssd_tensorflow_amd._lib import lib, last_error
    from ssd_tensorflow_amd.ssdvgg import LocLossConfig, LossConfig
    loc = LocLossConfig(*bad)
    hw = (C.c_int * 1)(4); nj = (C.c_int * 1)(4)
    for cfg in (None, LossConfig(0, 2.0, 0.25), LossConfig(1, 2.0, 0.25)):
        ref = None if cfg is None else C.byref(cfg)
        calls = [
            lambda: lib.ssd_set_loc_loss(None, C.byref(loc)),
            lambda: lib.ssd_op_multibox_loss_ex2(1, hw, nj, 20, None, None, None, None, 1, 0, 1, 0.0, None, 0, 0.0, ref, C.byref(loc), None),
            lambda: lib.ssd_op_multibox_loss_grad_ex2(1, hw, nj, 20, None, 0, None, None, None, 1, 0, 1, ref, C.byref(loc), None),
        ]
        for call in calls:
            assert call() != 0
            assert 'localization loss' in last_error(), last_error()


def test_null_arguments_are_refused():
    from ssd_tensorflow_amd._lib import lib, last_error
    from ssd_tensorflow_amd.ssdvgg import LocLossConfig, LossConfig
    assert lib.ssd_get_loc_loss(None, None) != 0 and 'localization loss' in last_error()
    assert lib.ssd_set_loc_loss(None, None) != 0 and 'localization loss' in last_error()
    good = LocLossConfig(1, 2.0)
    assert lib.ssd_set_loc_loss(None, C.byref(good)) != 0 and last_error() == 'null handle'       # a good configuration gets further
    assert lib.ssd_get_loc_loss(None, C.byref(good)) != 0 and last_error() == 'null handle'
    # a call with null buffers stops at the buffers, whatever the two configurations; smooth-L1 (its weight is not read) and NULL
    # go to the _ex entry points' own checks
    hw = (C.c_int * 1)(4); nj = (C.c_int * 1)(4)
    focal = LossConfig(1, 2.0, 0.25)
    for loc in (good, LocLossConfig(0, float('nan')), None):
        for cfg in (focal, None):
            lref = None if loc is None else C.byref(loc)
            cref = None if cfg is None else C.byref(cfg)
            assert lib.ssd_op_multibox_loss_ex2(1, hw, nj, 20, None, None, None, None, 1, 0, 1, 0.0, None, 0, 0.0, cref, lref, None) != 0
            assert last_error() == 'null buffer'
            assert lib.ssd_op_multibox_loss_grad_ex2(1, hw, nj, 20, None, 0, None, None, None, 1, 0, 1, cref, lref, None) != 0
            assert last_error() == 'null buffer'
    # a bad confidence configuration is still refused by name under GIoU
    bad = LossConfig(1, 9.0, 0.25)
    assert lib.ssd_op_multibox_loss_ex2(1, hw, nj, 20, None, None, None, None, 1, 0, 1, 0.0, None, 0, 0.0, C.byref(bad), C.byref(good), None) != 0
    assert 'gamma' in last_error()


def test_checkpoint_without_the_keys_is_smooth_l1(tmp_path):
    from ssd_tensorflow_amd import ssdvgg, train
    p = str(tmp_path / 'old.npz')
    np.savez(p, __match__=np.array('paper'), __loss__=np.array('focal'), __focal_gamma__=np.array(1.5), __focal_alpha__=np.array(0.5))
    assert train.checkpoint_loc_loss(p) == ('smooth_l1', 1.0)
    assert train.checkpoint_loss(p) == ('focal', 1.5, 0.5)
    np.savez(p, __loc_loss__=np.array('giou'), __loc_weight__=np.array(2.5))
    assert train.checkpoint_loc_loss(p) == ('giou', 2.5)
    with np.load(p) as ck:
        assert ssdvgg.checkpoint_loc_loss(ck) == ('giou', 2.5)


def test_train_help_lists_the_flags(capsys):
    from ssd_tensorflow_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(['--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert '--loc-loss' in out and '--loc-weight' in out and 'smooth_l1' in out and 'giou' in out
