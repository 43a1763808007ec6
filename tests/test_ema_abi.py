"""CPU: the weight EMA in the C ABI (ssd_set_ema / ssd_get_ema / ssd_set_ema_step / ssd_save_ema / ssd_load_ema / ssd_ema_swap /
ssd_op_ema_update / ssd_op_ema_swap): declared, exported and given ctypes signatures; the contract comment holds the formulas the
tests hold the kernel to; the kernels live in the translation unit compiled without contraction; a bad decay, a negative count and an
arena size that is no multiple of 4 are refused on the host before any device work (every pointer here is NULL and no GPU is needed),
by name, while good values get as far as the null-handle / null-buffer check; the Python names and defaults, the checkpoint helper
and the drivers' flags."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ssd_set_ema', 'ssd_get_ema', 'ssd_set_ema_step', 'ssd_save_ema', 'ssd_load_ema', 'ssd_ema_swap', 'ssd_op_ema_update',
       'ssd_op_ema_swap')
INF, NAN = float('inf'), float('nan')
BAD_DECAYS = [-0.1, 1.0, 0.99999999, NAN, INF]          # (0.99999999 is 1.0 as a float32)


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _code():
    return re.sub(r'/\*.*?\*/', '', _read('include', 'ssdvgg_hip.h'), flags=re.S)


def test_symbols_declared_exported_and_signed():
    from ssd_tensorflow_amd import _lib
    code = _code()
    for n in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % n, code), f'{n} is not declared in include/ssdvgg_hip.h'
        assert hasattr(_lib.lib, n), f'{n} is not exported'
        assert n in _lib.SIGNATURES, f'{n} has no ctypes signature'
    assert re.search(r'ssd_set_ema\s*\(\s*ssd_handle\s+h\s*,\s*float\s+decay\s*\)', code)
    assert re.search(r'ssd_get_ema\s*\(\s*ssd_handle\s+h\s*,\s*float\s*\*\s*decay\s*,\s*long\s+long\s*\*\s*t\s*,\s*int\s*\*\s*swapped\s*\)', code)
    assert re.search(r'ssd_set_ema_step\s*\(\s*ssd_handle\s+h\s*,\s*long\s+long\s+t\s*\)', code)
    assert re.search(r'ssd_save_ema\s*\(\s*ssd_handle\s+h\s*,\s*const\s+char\s*\*\s*name\s*,\s*float\s*\*\s*data\s*,\s*size_t\s+count\s*\)', code)
    assert re.search(r'ssd_load_ema\s*\(\s*ssd_handle\s+h\s*,\s*const\s+char\s*\*\s*name\s*,\s*const\s+float\s*\*\s*data\s*,\s*size_t\s+count\s*\)', code)
    assert re.search(r'ssd_ema_swap\s*\(\s*ssd_handle\s+h\s*\)', code)
    assert re.search(r'ssd_op_ema_update\s*\(\s*float\s*\*\s*e\s*,\s*const\s+float\s*\*\s*w\s*,\s*size_t\s+n\s*,\s*float\s+decay\s*,'
                     r'\s*long\s+long\s+t\s*,\s*void\s*\*\s*stream\s*\)', code)
    assert re.search(r'ssd_op_ema_swap\s*\(\s*float\s*\*\s*a\s*,\s*float\s*\*\s*b\s*,\s*size_t\s+n\s*,\s*void\s*\*\s*stream\s*\)', code)
    sig = _lib.SIGNATURES
    assert all(sig[n][0] is C.c_int for n in NEW)
    assert sig['ssd_set_ema'][1][1] is C.c_float and sig['ssd_set_ema_step'][1][1] is C.c_longlong
    assert len(sig['ssd_get_ema'][1]) == 4 and len(sig['ssd_ema_swap'][1]) == 1
    args = sig['ssd_op_ema_update'][1]
    assert len(args) == 6 and args[2] is C.c_size_t and args[3] is C.c_float and args[4] is C.c_longlong
    assert len(sig['ssd_op_ema_swap'][1]) == 4 and sig['ssd_op_ema_swap'][1][2] is C.c_size_t


def test_the_contract_comment_holds_the_formulas():
    text = _read('include', 'ssdvgg_hip.h')
    for word in ('weight EMA', 'd   = min((double)decay, (1 + t) / (10 + t))', 'omd = (float)(1 - d)', 'diff = e[i] - w[i]',
                 'e[i] = e[i] - (omd * diff)', 'rounded to nearest', 'multiply-add', 'fixed point', 'swapped', '"weight EMA:"',
                 'bit for bit', 'padding'):
        assert word in text, word


def test_the_kernels_live_in_the_translation_unit_without_contraction():
    mk = _read('ssd_tensorflow_amd', 'csrc', 'Makefile')
    assert re.search(r'^EXTRA_optim\s*=\s*-ffp-contract=off\s*$', mk, flags=re.M) and '$(B)/optim.o' in mk
    ops = _read('ssd_tensorflow_amd', 'csrc', 'ops.hip')
    assert 'ema_kernel' not in ops and 'swap_kernel' not in ops
    optim = _read('ssd_tensorflow_amd', 'csrc', 'optim.hip')
    assert re.search(r'__global__[^;{]*\bema_kernel\s*\(', optim) and re.search(r'__global__[^;{]*\bswap_kernel\s*\(', optim)
    assert '"ema_update"' in optim and '"ema_swap"' in optim and 'fp contract(off)' in optim
    hdr = _read('ssd_tensorflow_amd', 'csrc', 'ops.h')
    assert re.search(r'void\s+ema_update\s*\(\s*float\*\s*e\s*,\s*const\s+float\*\s*w\s*,\s*size_t\s+n\s*,\s*float\s+decay\s*,\s*long\s+long\s+t\s*,'
                     r'\s*hipStream_t\s+s\s*\)', hdr)
    assert re.search(r'void\s+ema_swap\s*\(\s*float\*\s*a\s*,\s*float\*\s*b\s*,\s*size_t\s+n\s*,\s*hipStream_t\s+s\s*\)', hdr)
    assert re.search(r'void\s+ema_check\s*\(\s*float\s+decay\s*\)', hdr)
    assert hdr.index('void adamw_update') < hdr.index('void ema_update')


def _update(decay=0.9, t=0, n=1024):
    from ssd_tensorflow_amd._lib import lib
    return lib.ssd_op_ema_update(None, None, n, decay, t, None)


@pytest.mark.parametrize('decay', BAD_DECAYS, ids=[repr(d) for d in BAD_DECAYS])
def test_a_bad_decay_is_refused_on_the_host_by_name(decay):
    from ssd_tensorflow_amd._lib import lib, last_error
    assert lib.ssd_set_ema(None, decay) != 0
    assert last_error().startswith('weight EMA: decay'), last_error()
    assert _update(decay=decay) != 0
    assert last_error().startswith('weight EMA: decay'), last_error()
    # ... in front of the other checks
    assert _update(decay=decay, t=-1, n=6) != 0 and last_error().startswith('weight EMA: decay')


def test_zero_is_off_not_a_bad_decay():
    from ssd_tensorflow_amd._lib import lib, last_error
    assert lib.ssd_set_ema(None, 0.0) != 0 and last_error() == 'null handle'
    assert _update(decay=0.0) != 0 and last_error().startswith('weight EMA: decay')       # the kernel itself has no "off"


def test_a_negative_count_and_a_ragged_size_are_refused_on_the_host():
    from ssd_tensorflow_amd._lib import lib, last_error
    assert lib.ssd_set_ema_step(None, -1) != 0
    assert last_error().startswith('weight EMA:') and 'count' in last_error() and '-1' in last_error()
    assert _update(t=-1) != 0
    assert last_error().startswith('weight EMA:') and 'count' in last_error()
    for n in (1, 6, 1023):
        assert _update(n=n) != 0
        assert last_error().startswith('weight EMA:') and 'multiple of 4' in last_error()
        assert lib.ssd_op_ema_swap(None, None, n, None) != 0
        assert last_error().startswith('weight EMA:') and 'multiple of 4' in last_error()


def test_misaligned_and_overlapping_buffers_are_refused_on_the_host():
    """(addresses that are never dereferenced: every call is refused before any device work)"""
    from ssd_tensorflow_amd._lib import lib, last_error
    base = 1 << 20
    for a, b in ((base + 4, base + 4096), (base, base + 4096 + 8)):
        assert lib.ssd_op_ema_update(a, b, 1024, 0.9, 0, None) != 0 and last_error() == 'weight EMA: the buffers must be 16-byte aligned'
        assert lib.ssd_op_ema_swap(a, b, 1024, None) != 0 and last_error() == 'weight EMA: the buffers must be 16-byte aligned'
    for a, b in ((base, base), (base, base + 4096 - 16), (base + 16, base)):
        assert lib.ssd_op_ema_update(a, b, 1024, 0.9, 0, None) != 0 and last_error() == 'weight EMA: the two buffers overlap'
        assert lib.ssd_op_ema_swap(a, b, 1024, None) != 0 and last_error() == 'weight EMA: the two buffers overlap'


def test_good_values_get_to_the_null_checks():
    from ssd_tensorflow_amd._lib import lib, last_error
    for decay in (0.0, 0.5, 0.9, 0.999, 0.9999999, 1e-6):
        assert lib.ssd_set_ema(None, decay) != 0 and last_error() == 'null handle', (decay, last_error())
    d, t, s = C.c_float(), C.c_longlong(), C.c_int()
    assert lib.ssd_get_ema(None, C.byref(d), C.byref(t), C.byref(s)) != 0 and last_error() == 'null handle'
    for step in (0, 3, 10 ** 12):
        assert lib.ssd_set_ema_step(None, step) != 0 and last_error() == 'null handle'
    buf = (C.c_float * 4)()
    assert lib.ssd_save_ema(None, b'conv1_1/filter', buf, 4) != 0 and last_error() == 'null handle'
    assert lib.ssd_load_ema(None, b'conv1_1/filter', buf, 4) != 0 and last_error() == 'null handle'
    assert lib.ssd_ema_swap(None) != 0 and last_error() == 'null handle'
    for decay, step, n in ((0.9, 0, 1024), (0.999, 10 ** 7, 4), (0.5, 0, 0)):
        assert _update(decay, step, n) != 0 and last_error() == 'null buffer'
    assert lib.ssd_op_ema_swap(None, None, 1024, None) != 0 and last_error() == 'null buffer'


def test_python_names_and_defaults():
    from ssd_tensorflow_amd import ssdvgg, train
    p = inspect.signature(ssdvgg.SSDVGG.build_optimizer).parameters
    assert p['ema_decay'].default == 0.0
    assert p['optimizer'].default == 'momentum' and p['clip_norm'].default == 0.0 and p['weight_decay'].default == 0.0005
    p = inspect.signature(ssdvgg.SSDVGG.build_from_metagraph).parameters
    assert p['weights'].default == 'auto' and p['training'].default is False and p['dtype'].default == 'f32'
    assert ssdvgg.WEIGHT_SETS == ('auto', 'raw', 'ema')
    for name in ('set_ema', 'get_ema', 'save_ema', 'swap_ema', 'averaged_weights'):
        assert callable(getattr(ssdvgg.SSDVGG, name)), name
    assert inspect.signature(ssdvgg.SSDVGG.save_ema).parameters['names'].default is None
    assert callable(ssdvgg.checkpoint_ema) and callable(train.checkpoint_ema)
    assert ssdvgg.ema_decay_config() == 0.0 and ssdvgg.ema_decay_config(-0.0) == 0.0
    assert ssdvgg.ema_decay_config(0.999) == float(np.float32(0.999))
    net = ssdvgg.SSDVGG(None, 'vgg300')
    assert net.weights == 'raw'                  # (before any build_from_*)
    assert callable(ssdvgg.checkpoint_has_ema) and "weights='ema'" in ssdvgg.NO_EMA_IN_FILE
    for decay in BAD_DECAYS:
        with pytest.raises(ValueError, match='weight EMA: decay'):
            ssdvgg.ema_decay_config(decay)
        with pytest.raises(ValueError, match='weight EMA: decay'):
            net.set_ema(decay)
    with pytest.raises(ValueError, match='weights must be one of'):
        net.build_from_metagraph(None, 'no-such-file.npz', weights='average')


def test_checkpoint_without_the_key_is_a_run_without_the_average(tmp_path):
    from ssd_tensorflow_amd import ssdvgg, train
    p = str(tmp_path / 'old.npz')
    np.savez(p, __clip_norm__=np.array(7.5), __momentum__=np.array(0.9))
    assert train.checkpoint_ema(p) == 0.0
    with np.load(p) as ck:
        assert ssdvgg.checkpoint_ema(ck) == 0.0
    np.savez(p, __ema_decay__=np.array(0.999, np.float32), __ema_step__=np.array(12, np.int64))
    assert train.checkpoint_ema(p) == float(np.float32(0.999))
    with np.load(p) as ck:
        assert ssdvgg.checkpoint_ema(ck) == float(np.float32(0.999)) and int(ck['__ema_step__']) == 12


def _help(main, capsys):
    with pytest.raises(SystemExit) as e:
        main(['--help'])
    assert e.value.code == 0
    return capsys.readouterr().out


def test_train_help_lists_the_flag(capsys):
    from ssd_tensorflow_amd import train
    out = _help(train.main, capsys)
    assert '--ema-decay' in out and 'DESIGN.md 37' in out


def test_infer_and_detect_help_list_the_weights(capsys):
    from ssd_tensorflow_amd import infer, detect
    for main in (infer.main, detect.main):
        out = _help(main, capsys)
        assert '--weights' in out and '{auto,raw,ema}' in out
