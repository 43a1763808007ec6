"""CPU, no GPU call: the Soft-NMS entry points are exported with the signatures include/ssdvgg_hip.h declares;
ssd_nms_params has the header's layout; the four refusals come by name and in order before anything touches a device; the Python
layers and the two drivers carry the keywords and options."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from ssd_tensorflow_amd import _lib
from ssd_tensorflow_amd import ssdutils as su
from ssd_tensorflow_amd._lib import lib, last_error
from test_detection_output_abi import prototypes, ctype_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['ssd_detection_output_soft', 'ssd_detection_output_soft_dev', 'ssd_detect_last_all_soft_dev', 'ssd_detout_tiles_merge_soft_dev',
       'ssd_detout_tiles_soft', 'ssd_soft_nms_boxes']
KEYWORDS = ['soft_nms', 'soft_nms_iou', 'soft_nms_sigma', 'soft_nms_min_score']


def header():
    return open(os.path.join(ROOT, 'include', 'ssdvgg_hip.h')).read()


@pytest.mark.parametrize('name', NEW)
def test_symbol_and_signature(name):
    protos = prototypes()
    assert name in protos, name + ' is not declared in include/ssdvgg_hip.h'
    assert hasattr(lib, name), name + ' is not exported'
    ret, args = protos[name]
    res, argtypes = _lib.SIGNATURES[name]
    assert res is _lib.i32 and ret == 'int'
    assert len(argtypes) == len(args), (args, argtypes)
    for decl, t in zip(args, argtypes):
        assert t is (_lib.p_i32 if name == 'ssd_soft_nms_boxes' and decl == 'int* n_keep' else ctype_of(decl)), (name, decl, t)


def _names(proto):
    return [re.search(r'[A-Za-z0-9_]*$', a).group(0) for a in proto[1]]


def test_the_soft_entries_take_their_namesakes_arguments_plus_nms():
    protos = prototypes()
    for soft, hard in (('ssd_detection_output_soft', 'ssd_detection_output'), ('ssd_detout_tiles_soft', 'ssd_detout_tiles'),
                       ('ssd_detect_last_all_soft_dev', 'ssd_detect_last_all_dev')):
        assert protos[soft][1] == protos[hard][1] + ['const ssd_nms_params* nms'], soft      # at the end
    for soft, hard in (('ssd_detection_output_soft_dev', 'ssd_detection_output_dev'),
                       ('ssd_detout_tiles_merge_soft_dev', 'ssd_detout_tiles_merge_dev')):
        assert protos[soft][1] == protos[hard][1][:-1] + ['const ssd_nms_params* nms', 'void* stream'], soft      # the last before stream
    assert _names(protos['ssd_soft_nms_boxes']) == ['device', 'n', 'box_abs', 'conf', 'nms', 'order_out', 'conf_out', 'n_keep']
    assert 'ssd_detout_tiles_add_soft_dev' not in protos and not hasattr(lib, 'ssd_detout_tiles_add_soft_dev')      # no suppression there


def test_struct_layout_and_enum_values():
    src = re.sub(r'/\*.*?\*/', '', header(), flags=re.S)
    assert re.search(r'enum\s*\{\s*SSD_NMS_HARD\s*=\s*0\s*,\s*SSD_NMS_SOFT_LINEAR\s*=\s*1\s*,\s*SSD_NMS_SOFT_GAUSSIAN\s*=\s*2\s*\}\s*;', src)
    assert re.search(r'typedef\s+struct\s+ssd_nms_params\s*\{\s*int\s+kind\s*;\s*float\s+iou_thr\s*,\s*sigma\s*,\s*min_score\s*;\s*\}\s*ssd_nms_params\s*;', src)
    assert C.sizeof(su.NmsParams) == 16
    assert [(n, t) for n, t in su.NmsParams._fields_] == [('kind', C.c_int), ('iou_thr', C.c_float), ('sigma', C.c_float), ('min_score', C.c_float)]
    assert [getattr(su.NmsParams, n).offset for n in ('kind', 'iou_thr', 'sigma', 'min_score')] == [0, 4, 8, 12]
    assert su.SOFT_NMS_KINDS == {'linear': 1, 'gaussian': 2}


def _pp(*fields):
    nms = su.NmsParams(*fields)
    return nms, C.cast(C.pointer(nms), C.c_void_p)


def _calls(ptr):
    """every new entry point that can refuse without a handle, with arguments that are otherwise in range (z: a host buffer no
    kernel may see -- nothing below reaches a launch)"""
    z = (C.c_int * 64)()
    a = C.addressof(z)
    tile = (C.c_int * 8)(0, 0, 300, 300, 300, 300, 0, 0)
    nk = C.c_int(0)
    return {
        'ssd_detection_output_soft': lambda: lib.ssd_detection_output_soft(b'vgg300', 3, 0, a, 1, 0.01, 400, 200, 200, a, a, a, a, a, ptr),
        'ssd_detection_output_soft_dev': lambda: lib.ssd_detection_output_soft_dev(b'vgg300', 3, a, a, 1, 0.01, 400, 200, 200, a, a, a, a, a, a, 0,
                                                                                   ptr, None),
        'ssd_detout_tiles_merge_soft_dev': lambda: lib.ssd_detout_tiles_merge_soft_dev(3, C.addressof(tile), 1, 1, 400, 200, 200, a, a, a, a, a, a, a,
                                                                                       0, ptr, None),
        'ssd_detout_tiles_soft': lambda: lib.ssd_detout_tiles_soft(b'vgg300', 3, 0, a, C.addressof(tile), 1, 1, 0.01, 400, 200, 2, 200, a, a, a, a, a,
                                                                   a, ptr),
        'ssd_soft_nms_boxes': lambda: lib.ssd_soft_nms_boxes(0, 1025, a, a, ptr, a, a, C.byref(nk)),
    }


REFUSALS = [  # in the order of the checks: each row is wrong in its own field AND in every later one
    ((7, float('nan'), -1.0, -1.0), 'nms kind'),
    ((1, 1.5, -1.0, -1.0), 'iou_thr'),
    ((1, float('nan'), 0.5, -1.0), 'iou_thr'),
    ((1, -0.1, 0.5, 0.0), 'iou_thr'),
    ((2, 7.0, 0.0, -1.0), 'sigma'),            # (iou_thr is not read under the gaussian rule)
    ((2, 0.45, float('inf'), -1.0), 'sigma'),
    ((2, 0.45, float('nan'), 0.0), 'sigma'),
    ((1, 0.45, -3.0, -1.0), 'min_score'),      # (sigma is not read under the linear rule)
    ((2, 0.45, 0.5, float('inf')), 'min_score'),
    ((1, 1.0, 0.5, float('nan')), 'min_score'),
]


@pytest.mark.parametrize('fields,word', REFUSALS, ids=['%s-%d' % (w, i) for i, (_, w) in enumerate(REFUSALS)])
def test_the_four_refusals_by_name_and_in_order(fields, word):
    nms, ptr = _pp(*fields)
    for name, call in _calls(ptr).items():
        assert call() != 0, name
        msg = last_error()
        assert msg.startswith(name + ':') and word in msg, (name, msg)
        assert not any(w in msg for w in ('nms kind', 'iou_thr', 'sigma', 'min_score') if w != word), (name, msg)


def test_a_null_parameter_block_is_refused():
    for name, call in _calls(None).items():
        assert call() != 0 and 'null' in last_error(), name


def test_kind_hard_ignores_garbage_in_the_other_fields():
    """the parameters pass; what refuses these calls is the next check of the hard path, with its message"""
    nms, ptr = _pp(0, float('nan'), -1.0, float('-inf'))
    calls = _calls(ptr)
    assert calls['ssd_detection_output_soft_dev']() != 0 and 'workspace' in last_error()
    assert calls['ssd_detout_tiles_merge_soft_dev']() != 0 and 'workspace' in last_error()
    assert calls['ssd_soft_nms_boxes']() != 0 and 'ssd_nms_boxes' in last_error()      # the rule alone has no hard form here
    # in range under a soft kind: the same next check
    good, gptr = _pp(2, 0.45, 0.5, 0.01)
    assert _calls(gptr)['ssd_detection_output_soft_dev']() != 0 and 'workspace' in last_error()
    assert _calls(gptr)['ssd_soft_nms_boxes']() != 0 and '0..1024' in last_error()
    # min_score and iou_thr at their closed ends
    for fields in ((1, 0.0, 0.5, 0.0), (1, 1.0, 0.5, 0.0), (2, 9.0, 1e-30, 3e38)):
        assert _calls(_pp(*fields)[1])['ssd_detection_output_soft_dev']() != 0 and 'workspace' in last_error(), fields


def test_python_keywords():
    from ssd_tensorflow_amd import tiling
    from ssd_tensorflow_amd.ssdvgg import SSDVGG
    for fn in (su.detection_output, su.detection_output_batch, su.detection_output_tiles, su.detect_tiles, SSDVGG.detect_last_launch,
               SSDVGG.detect_last, tiling.TiledDetector.__init__):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in KEYWORDS] == [None, 0.45, 0.5, None], fn
        assert list(p)[-4:] == KEYWORDS, fn              # appended: every positional call of before means what it meant
    assert inspect.signature(SSDVGG.detect_last).parameters['nms'].default is True
    assert su.soft_nms_params(None, float('nan'), -1.0, -5.0) is None
    nms = su.soft_nms_params('gaussian', 0.3, 0.25, None, thr=0.125)
    assert (nms.kind, nms.iou_thr, nms.sigma, nms.min_score) == (2, np.float32(0.3), 0.25, 0.125)
    assert su.soft_nms_params('linear', soft_nms_min_score=0.5, thr=0.125).min_score == 0.5
    with pytest.raises(ValueError, match='soft_nms'):
        su.soft_nms_params('hard')
    with pytest.raises(ValueError, match="decode='all'"):
        su.detect_tiles(np.zeros((1, 8732, 8), np.float32), None, [], 0.5, soft_nms='linear')
    with pytest.raises(ValueError, match="decode='all'"):
        tiling.TiledDetector(None, 300, soft_nms='gaussian')
    assert callable(su.soft_nms_boxes)


@pytest.mark.parametrize('driver', ['infer', 'detect'])
def test_driver_help_and_argument_errors(driver, capsys, tmp_path):
    import importlib
    main = importlib.import_module('ssd_tensorflow_amd.' + driver).main
    with pytest.raises(SystemExit) as e:
        main(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert '--soft-nms {off,linear,gaussian}' in text
    for opt in ('--soft-nms-iou', '--soft-nms-sigma', '--soft-nms-min-score'):
        assert opt in text
    base = (['--name', str(tmp_path / 'none')] if driver == 'infer' else []) + [str(tmp_path / 'x.npy')]
    for extra, why in ((['--soft-nms', 'linear'], 'needs --decode all'),
                       (['--soft-nms', 'gaussian', '--decode', 'argmax'], 'needs --decode all'),
                       (['--soft-nms', 'gaussian', '--tile', '300'], 'needs --tile-decode all'),
                       (['--soft-nms', 'matrix', '--decode', 'all'], 'invalid choice'),
                       (['--soft-nms', 'gaussian', '--decode', 'all', '--soft-nms-sigma', '0'], '--soft-nms-sigma')):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2, extra
        assert why in capsys.readouterr().err, extra


def test_banner_names_the_rule():
    import argparse
    from ssd_tensorflow_amd import infer
    p = argparse.ArgumentParser()
    infer.add_decode_arguments(p)
    assert infer.nms_rule_text(p.parse_args([])) == '' and infer.soft_nms_keywords(p.parse_args([])) == {}
    a = p.parse_args(['--soft-nms', 'gaussian', '--soft-nms-sigma', '0.3'])
    assert infer.nms_rule_text(a) == ', soft nms gaussian, sigma 0.3, min score the threshold'
    assert infer.soft_nms_keywords(a) == dict(soft_nms='gaussian', soft_nms_iou=0.45, soft_nms_sigma=0.3, soft_nms_min_score=None)
    a = p.parse_args(['--soft-nms', 'linear', '--soft-nms-min-score', '0.05'])
    assert infer.nms_rule_text(a) == ', soft nms linear, iou 0.45, min score 0.05'
