"""CPU: the update rule in the C ABI (ssd_set_update_rule / ssd_get_update_rule / ssd_get_adam_step / ssd_set_adam_step /
ssd_save_second_moment / ssd_load_second_moment / ssd_op_adamw_update): declared, exported and given ctypes signatures; the struct
and the enum; hyper-parameters outside their ranges are refused on the host before any device work (every pointer here is NULL and
no GPU is needed), by name and in the order beta1, beta2, eps, decay, kind, while good ones get as far as the null-handle / null-buffer
check; the Python names and defaults, the checkpoint helper, the driver's flags and the resolved --weight-decay."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ssd_set_update_rule', 'ssd_get_update_rule', 'ssd_get_adam_step', 'ssd_set_adam_step', 'ssd_save_second_moment',
       'ssd_load_second_moment', 'ssd_op_adamw_update')
INF, NAN = float('inf'), float('nan')


def _code():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ssdvgg_hip.h')).read(), flags=re.S)


def test_symbols_declared_exported_and_signed():
    from ssd_tensorflow_amd import _lib
    code = _code()
    for n in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % n, code), f'{n} is not declared in include/ssdvgg_hip.h'
        assert hasattr(_lib.lib, n), f'{n} is not exported'
        assert n in _lib.SIGNATURES, f'{n} has no ctypes signature'
    assert re.search(r'enum\s*\{\s*SSD_UPDATE_MOMENTUM\s*=\s*0\s*,\s*SSD_UPDATE_ADAMW\s*=\s*1\s*\}\s*;', code)
    assert re.search(r'typedef\s+struct\s*\{\s*int\s+kind;\s*float\s+beta1\s*,\s*beta2\s*,\s*eps\s*,\s*decay;\s*\}\s*ssd_update_rule_config;', code)
    assert re.search(r'ssd_set_update_rule\s*\(\s*ssd_handle\s+h\s*,\s*const\s+ssd_update_rule_config\s*\*\s*cfg\s*\)', code)
    assert re.search(r'ssd_get_adam_step\s*\(\s*ssd_handle\s+h\s*,\s*long\s+long\s*\*\s*t\s*\)', code)
    assert re.search(r'ssd_save_second_moment\s*\(\s*ssd_handle\s+h\s*,\s*const\s+char\s*\*\s*name\s*,\s*float\s*\*\s*data\s*,\s*size_t\s+count\s*\)', code)
    assert re.search(r'ssd_op_adamw_update\s*\(\s*float\s*\*\s*w\s*,\s*float\s*\*\s*m\s*,\s*float\s*\*\s*v\s*,\s*const\s+float\s*\*\s*g\s*,\s*size_t\s+n\s*,'
                     r'\s*size_t\s+n_decay\s*,\s*float\s+lr\s*,\s*float\s+beta1\s*,\s*float\s+beta2\s*,\s*float\s+eps\s*,\s*float\s+decay\s*,'
                     r'\s*long\s+long\s+t\s*,\s*float\s+grad_scale\s*,\s*float\s+max_norm\s*,\s*void\s*\*\s*ws_dev\s*,\s*float\s*\*\s*report_dev\s*,'
                     r'\s*void\s*\*\s*stream\s*\)', code)
    res, args = _lib.SIGNATURES['ssd_op_adamw_update']
    assert res is C.c_int and len(args) == 17 and args[4] is C.c_size_t and args[5] is C.c_size_t
    assert args[6:11] == [C.c_float] * 5 and args[11] is C.c_longlong and args[12:14] == [C.c_float] * 2
    assert _lib.SIGNATURES['ssd_set_adam_step'][1][1] is C.c_longlong
    # the contract comment names what the tests hold the kernel to
    text = open(os.path.join(ROOT, 'include', 'ssdvgg_hip.h')).read()
    for word in ('update rule', 'rounded to nearest', 'multiply-add', "m'  = (b1 * m[i]) + (omb1 * gs)", "den = (sqrtf(v') * rs2) + eps",
                 'i < n_decay', 'filter_floats', 'skipped', 'zeroes m, v and t', 'rounded to float once'):
        assert word in text, word


def test_the_kernel_has_its_own_translation_unit_without_contraction():
    mk = open(os.path.join(ROOT, 'ssd_tensorflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^EXTRA_optim\s*=\s*-ffp-contract=off\s*$', mk, flags=re.M) and '$(B)/optim.o' in mk
    ops = open(os.path.join(ROOT, 'ssd_tensorflow_amd', 'csrc', 'ops.hip')).read()
    assert 'adamw_kernel' not in ops
    optim = open(os.path.join(ROOT, 'ssd_tensorflow_amd', 'csrc', 'optim.hip')).read()
    assert re.search(r'template\s*<bool CLIPPED>\s*__global__', optim) and 'adamw_kernel<false>' in optim and 'adamw_kernel<true>' in optim
    assert '"adamw_update"' in optim and '"adamw_update_clipped"' in optim


def test_struct_and_names():
    from ssd_tensorflow_amd import ssdvgg, train
    cfg = ssdvgg.UpdateRuleConfig
    assert C.sizeof(cfg) == 20 and [f[0] for f in cfg._fields_] == ['kind', 'beta1', 'beta2', 'eps', 'decay']
    assert [getattr(cfg, f).offset for f in ('kind', 'beta1', 'beta2', 'eps', 'decay')] == [0, 4, 8, 12, 16]
    assert ssdvgg.UPDATE_KINDS == {'momentum': 0, 'adamw': 1}
    d = ssdvgg.update_rule_config()
    assert (d.kind, d.beta1, d.beta2, d.eps, d.decay) == (0, np.float32(0.9), np.float32(0.999), np.float32(1e-8), np.float32(0.01))
    assert ssdvgg.update_rule_config('adamw', 0.0, 0.0, 1e-6, 0.0).kind == 1
    p = inspect.signature(ssdvgg.SSDVGG.build_optimizer).parameters
    assert [p[k].default for k in ('optimizer', 'adam_beta1', 'adam_beta2', 'adam_eps', 'adam_decay')] == ['momentum', 0.9, 0.999, 1e-8, 0.01]
    assert p['weight_decay'].default == 0.0005 and p['momentum'].default == 0.9 and p['clip_norm'].default == 0.0
    for name in ('set_update_rule', 'get_update_rule', 'save_second_moment', 'adam_step'):
        assert hasattr(ssdvgg.SSDVGG, name)
    assert callable(train.checkpoint_update_rule) and callable(ssdvgg.checkpoint_update_rule) and callable(train.resolved_weight_decay)


BAD = [('beta1', dict(adam_beta1=1.0)), ('beta1', dict(adam_beta1=-0.1)), ('beta1', dict(adam_beta1=NAN)),
       ('beta2', dict(adam_beta2=1.0)), ('beta2', dict(adam_beta2=NAN)), ('beta2', dict(adam_beta2=0.99999999)),      # (1.0 as float32)
       ('eps', dict(adam_eps=0.0)), ('eps', dict(adam_eps=-1e-8)), ('eps', dict(adam_eps=INF)), ('eps', dict(adam_eps=NAN)),
       ('decay', dict(adam_decay=-0.01)), ('decay', dict(adam_decay=INF)), ('decay', dict(adam_decay=NAN))]


@pytest.mark.parametrize('name,kw', BAD, ids=['%s %r' % (n, list(k.values())[0]) for n, k in BAD])
def test_python_refuses_a_bad_value_by_name(name, kw):
    from ssd_tensorflow_amd import ssdvgg
    with pytest.raises(ValueError, match='update rule: ' + name):
        ssdvgg.update_rule_config('adamw', **kw)
    with pytest.raises(ValueError, match='update rule: ' + name):
        ssdvgg.update_rule_config('momentum', **kw)
    net = ssdvgg.SSDVGG(None, 'vgg300')
    with pytest.raises(ValueError, match='update rule: ' + name):
        net.set_update_rule('adamw', **kw)


def test_python_refuses_a_bad_name_last():
    from ssd_tensorflow_amd import ssdvgg
    with pytest.raises(ValueError, match='update rule must be one of'):
        ssdvgg.update_rule_config('adam')
    with pytest.raises(ValueError, match='update rule: beta1'):
        ssdvgg.update_rule_config('adam', adam_beta1=2.0)


def _cfg(kind=1, b1=0.9, b2=0.999, eps=1e-8, decay=0.01):
    from ssd_tensorflow_amd.ssdvgg import UpdateRuleConfig
    return UpdateRuleConfig(kind, b1, b2, eps, decay)


def _op(b1=0.9, b2=0.999, eps=1e-8, decay=0.01, t=1, max_norm=0.0, n=1024, n_decay=1024):
    from ssd_tensorflow_amd._lib import lib
    return lib.ssd_op_adamw_update(None, None, None, None, n, n_decay, 1e-3, b1, b2, eps, decay, t, 1.0, max_norm, None, None, None)


LIB_BAD = [('beta1', dict(b1=1.0)), ('beta1', dict(b1=-0.5)), ('beta1', dict(b1=NAN)), ('beta2', dict(b2=1.0)), ('beta2', dict(b2=NAN)),
           ('eps', dict(eps=0.0)), ('eps', dict(eps=-1.0)), ('eps', dict(eps=INF)), ('eps', dict(eps=NAN)),
           ('decay', dict(decay=-1.0)), ('decay', dict(decay=INF)), ('decay', dict(decay=NAN))]


@pytest.mark.parametrize('name,kw', LIB_BAD, ids=['%s %r' % (n, list(k.values())[0]) for n, k in LIB_BAD])
def test_bad_hyper_parameters_are_refused_on_the_host(name, kw):
    from ssd_tensorflow_amd._lib import lib, last_error
    for kind in (0, 1):
        cfg = _cfg(kind, **kw)
        assert lib.ssd_set_update_rule(None, C.byref(cfg)) != 0
        assert 'update rule' in last_error() and name in last_error(), last_error()
    assert _op(**kw) != 0
    assert 'update rule' in last_error() and name in last_error(), last_error()


def test_the_order_of_the_refusals():
    """beta1, beta2, eps, decay, then the kind; and gradient clipping's own check behind the rule's"""
    from ssd_tensorflow_amd._lib import lib, last_error
    bad = dict(b1=1.5, b2=1.5, eps=0.0, decay=-1.0)
    for name in ('beta1', 'beta2', 'eps', 'decay'):
        cfg = _cfg(7, **bad)
        assert lib.ssd_set_update_rule(None, C.byref(cfg)) != 0 and name in last_error(), (name, last_error())
        assert _op(max_norm=-1.0, **bad) != 0 and name in last_error(), (name, last_error())
        del bad[dict(beta1='b1', beta2='b2').get(name, name)]
    cfg = _cfg(7)
    assert lib.ssd_set_update_rule(None, C.byref(cfg)) != 0
    assert 'update rule' in last_error() and 'kind 7' in last_error() and 'SSD_UPDATE_ADAMW' in last_error()
    assert _op(max_norm=-1.0) != 0 and 'gradient clipping' in last_error()


def test_good_values_get_to_the_null_checks():
    from ssd_tensorflow_amd._lib import lib, last_error
    for cfg in (_cfg(0), _cfg(1), _cfg(1, 0.0, 0.0, 1e-30, 0.0)):
        assert lib.ssd_set_update_rule(None, C.byref(cfg)) != 0 and last_error() == 'null handle'
        assert lib.ssd_get_update_rule(None, C.byref(cfg)) != 0 and last_error() == 'null handle'
    assert lib.ssd_set_update_rule(None, None) != 0 and 'update rule' in last_error()
    assert lib.ssd_get_update_rule(None, None) != 0 and 'update rule' in last_error()
    t = C.c_longlong()
    assert lib.ssd_get_adam_step(None, C.byref(t)) != 0 and last_error() == 'null handle'
    assert lib.ssd_set_adam_step(None, 3) != 0 and last_error() == 'null handle'
    buf = (C.c_float * 4)()
    assert lib.ssd_save_second_moment(None, b'conv1_1/filter', buf, 4) != 0 and last_error() == 'null handle'
    assert lib.ssd_load_second_moment(None, b'conv1_1/filter', buf, 4) != 0 and last_error() == 'null handle'
    for mn in (0.0, 1.5, INF):
        assert _op(max_norm=mn) != 0 and last_error() == 'null buffer'


def test_checkpoint_without_the_key_is_a_momentum_run(tmp_path):
    from ssd_tensorflow_amd import ssdvgg, train
    p = str(tmp_path / 'old.npz')
    np.savez(p, __clip_norm__=np.array(7.5), __momentum__=np.array(0.9))
    assert train.checkpoint_update_rule(p) == ('momentum', 0.9, 0.999, 1e-8, 0.01)
    assert train.checkpoint_clip_norm(p) == 7.5
    np.savez(p, __optimizer__=np.array('adamw'), __adam_beta1__=np.array(0.8, np.float32), __adam_beta2__=np.array(0.99, np.float32),
             __adam_eps__=np.array(1e-6, np.float32), __adam_decay__=np.array(0.0, np.float32), __adam_step__=np.array(12, np.int64))
    want = ('adamw',) + tuple(float(np.float32(x)) for x in (0.8, 0.99, 1e-6, 0.0))
    assert train.checkpoint_update_rule(p) == want
    with np.load(p) as ck:
        assert ssdvgg.checkpoint_update_rule(ck) == want and int(ck['__adam_step__']) == 12


def test_train_help_lists_the_flags(capsys):
    from ssd_tensorflow_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(['--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ('--optimizer', '{momentum,adamw}', '--adam-beta1', '--adam-beta2', '--adam-eps', '--adam-decay', '--weight-decay'):
        assert flag in out, flag


def test_weight_decay_default_resolves_by_the_rule():
    from ssd_tensorflow_amd import train
    assert train.resolved_weight_decay(None, 'momentum') == 0.0005
    assert train.resolved_weight_decay(None, 'adamw') == 0.0
    assert train.resolved_weight_decay(0.001, 'adamw') == 0.001 and train.resolved_weight_decay(0.0, 'momentum') == 0.0
