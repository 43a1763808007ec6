"""CPU: the DetectionOutput entry points are exported with the signatures include/ssdvgg_hip.h declares, and
ssd_detection_output_ws_bytes follows the formula the header documents."""
import ctypes as C
import os
import re

import pytest

from ssd_tensorflow_amd import _lib
from ssd_tensorflow_amd._lib import lib, last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['ssd_detection_output_ws_bytes', 'ssd_detection_output_dev', 'ssd_detection_output', 'ssd_detect_last_all_dev']


def prototypes():
    src = open(os.path.join(ROOT, 'include', 'ssdvgg_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r'\b(size_t|int)\s+(ssd_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        out[name] = (ret, [' '.join(a.split()) for a in args.split(',')])
    return out


def ctype_of(decl):
    """the ctypes type _lib.py uses for a parameter declared as `decl`"""
    kind = decl[:len(decl) - len(re.search(r'[A-Za-z0-9_]*$', decl).group(0))].strip()      # without the parameter's name
    if kind == 'const char*':
        return _lib.cstr
    if kind == 'ssd_handle':
        return _lib.handle
    if kind.endswith('**'):
        return C.POINTER(_lib.vp)
    if kind.endswith('*'):
        return _lib.vp
    return {'int': _lib.i32, 'float': _lib.f32, 'size_t': _lib.sz}[kind]


@pytest.mark.parametrize('name', NEW)
def test_symbol_and_signature(name):
    protos = prototypes()
    assert name in protos, name + ' is not declared in include/ssdvgg_hip.h'
    assert hasattr(lib, name), name + ' is not exported'
    ret, args = protos[name]
    res, argtypes = _lib.SIGNATURES[name]
    assert res is {'int': _lib.i32, 'size_t': _lib.sz}[ret]
    assert len(argtypes) == len(args), (args, argtypes)
    for decl, t in zip(args, argtypes):
        assert t is ctype_of(decl), (name, decl, t)


def test_header_states_the_parameter_order():
    protos = prototypes()
    names = [re.search(r'[A-Za-z0-9_]*$', a).group(0) for a in protos['ssd_detection_output_dev'][1]]
    assert names == ['preset', 'num_classes', 'anchors_dev', 'pred_dev', 'b', 'conf_thr', 'nms_top_k', 'keep_top_k', 'out_cap', 'count_dev',
                     'conf_dev', 'cls_dev', 'idx_dev', 'box_dev', 'ws_dev', 'ws_bytes', 'stream']
    names = [re.search(r'[A-Za-z0-9_]*$', a).group(0) for a in protos['ssd_detection_output'][1]]
    assert names == ['preset', 'num_classes', 'device', 'pred', 'b', 'conf_thr', 'nms_top_k', 'keep_top_k', 'out_cap', 'count', 'conf', 'cls',
                     'idx', 'box']
    names = [re.search(r'[A-Za-z0-9_]*$', a).group(0) for a in protos['ssd_detect_last_all_dev'][1]]
    assert names == ['h', 'b', 'conf_thr', 'nms_top_k', 'keep_top_k', 'out_cap', 'count_dev', 'conf_dev', 'cls_dev', 'idx_dev', 'box_dev']


def align256(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize('pname', ['vgg300', 'vgg512'])
@pytest.mark.parametrize('ncls,b,k', [(1, 1, 1), (3, 2, 400), (20, 32, 400), (80, 128, 400), (127, 4096, 1024), (27, 3, 7), (28, 5, 1023)])
def test_ws_bytes_formula(pname, ncls, b, k):
    want = align256(4 * b * ncls) + align256(8 * b * ncls * k) + 16 * b * ncls * k
    assert lib.ssd_detection_output_ws_bytes(pname.encode(), ncls, b, k) == want
    # bounded by b (A + C k) up to a constant: no term holds b * A * C
    assert want <= 32 * b * ncls * k + 512


@pytest.mark.parametrize('args', [(b'vgg999', 3, 1, 400), (b'vgg300', 0, 1, 400), (b'vgg300', 128, 1, 400), (b'vgg300', 3, 0, 400),
                                  (b'vgg300', 3, 4097, 400), (b'vgg300', 3, 1, 0), (b'vgg300', 3, 1, 1025), (b'vgg300', 3, -1, 400),
                                  (None, 3, 1, 400)])
def test_ws_bytes_is_zero_on_bad_arguments(args):
    assert lib.ssd_detection_output_ws_bytes(*args) == 0
    assert last_error()


def test_host_side_refusals_need_no_gpu():
    """every limit is checked before the first HIP call: these fail with the limit's message on a machine without a GPU too"""
    z = (C.c_int * 16)()
    for kw, word in ((dict(k=0), 'nms_top_k'), (dict(keep=1025), 'keep_top_k'), (dict(thr=-1.0), 'threshold'), (dict(out_cap=0), 'out_cap'),
                     (dict(b=0), 'images'), (dict(ncls=128), 'num_classes')):
        a = dict(ncls=3, b=1, thr=0.01, k=400, keep=200, out_cap=200); a.update(kw)
        rc = lib.ssd_detection_output_dev(b'vgg300', a['ncls'], C.addressof(z), C.addressof(z), a['b'], a['thr'], a['k'], a['keep'], a['out_cap'],
                                          C.addressof(z), C.addressof(z), C.addressof(z), C.addressof(z), C.addressof(z), C.addressof(z), 1 << 40,
                                          None)
        assert rc != 0 and word in last_error(), (kw, last_error())
    rc = lib.ssd_detection_output_dev(b'vgg300', 3, C.addressof(z), C.addressof(z), 1, 0.01, 400, 200, 200, C.addressof(z), C.addressof(z),
                                      C.addressof(z), C.addressof(z), C.addressof(z), C.addressof(z),
                                      lib.ssd_detection_output_ws_bytes(b'vgg300', 3, 1, 400) - 1, None)
    assert rc != 0 and 'workspace' in last_error()
