"""the C ABI of the mxfp6 feature: the library exports the four ops, _lib.py declares them with the mxfp8 ops' argument
lists (wscales in the place of s_w), the Python dtype table knows 'mxfp6', and a training handle is refused.  No GPU."""
import ctypes as C

import pytest

OPS = ('ssd_op_quantize_mxfp6', 'ssd_op_quantize_filter_mxfp6', 'ssd_op_conv2d_fwd_mxfp6', 'ssd_op_maxpool_fwd_mxfp6')


def test_library_exports_the_mxfp6_ops():
    from ssd_tensorflow_amd._lib import lib, SIGNATURES
    for name in OPS:
        assert callable(getattr(lib, name)) and name in SIGNATURES
        assert getattr(lib, name).argtypes == SIGNATURES[name][1] and getattr(lib, name).restype is C.c_int


def test_signatures_are_the_mxfp8_ops():
    from ssd_tensorflow_amd._lib import SIGNATURES
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    assert SIGNATURES['ssd_op_quantize_mxfp6'] == SIGNATURES['ssd_op_quantize_mxfp8'] == (i32, [vp, i32, sz, i32, vp, vp, vp])
    assert SIGNATURES['ssd_op_maxpool_fwd_mxfp6'] == SIGNATURES['ssd_op_maxpool_fwd_mxfp8']
    # x6, xscales, w6, wscales, bias, y, y6, yscales, out_mode, 13 geometry ints, relu, stream
    res, args = SIGNATURES['ssd_op_conv2d_fwd_mxfp6']
    assert res is i32 and len(args) == 24 and args == SIGNATURES['ssd_op_conv2d_fwd_mxfp8'][1]
    assert SIGNATURES['ssd_op_quantize_filter_mxfp6'] == (i32, [vp, vp, vp, i32, i32, i32, vp])      # w, w6, wscales, taps, ci, co, stream


def test_header_declares_the_ops_and_the_dtype():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'ssdvgg_hip.h')).read()
    assert '#define SSD_DTYPE_MXFP6 4' in text
    for name in OPS:
        assert 'int %s(' % name in text


def test_dtype_table_accepts_mxfp6():
    from ssd_tensorflow_amd import ssdvgg
    assert ssdvgg.DTYPES['mxfp6'] == 4 and ssdvgg.DTYPES['mxfp8'] == 3
    net = ssdvgg.SSDVGG(None, 'vgg300')
    with pytest.raises(ValueError, match='inference only'):
        net._create(20, 2, True, 0, 'mxfp6')
    with pytest.raises(ValueError, match='dtype must be'):
        net._create(20, 2, False, 0, 'mxfp4')


def test_library_refuses_mxfp6_training_handle_and_unknown_dtype():
    from ssd_tensorflow_amd._lib import lib, last_error
    h = C.c_void_p()
    rc = lib.ssd_create_dtype(b'vgg300', 20, 2, 0, 1, 0, None, None, None, 4, C.byref(h))
    assert rc != 0 and not h.value
    assert last_error() == 'SSD_DTYPE_MXFP6 is inference only: create the handle with training = 0'
    rc = lib.ssd_create_graph(b'vgg300', 20, 2, 0, 1, 0, None, None, None, 4, 1, C.byref(h))
    assert rc != 0 and 'inference only' in last_error()
