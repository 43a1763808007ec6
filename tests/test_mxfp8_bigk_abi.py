"""the C ABI of the mxfp8 convolution with more than 9 taps: the library exports it and _lib.py declares it.  No GPU."""
import ctypes as C


def test_library_exports_the_mxfp8_bigk_op():
    from ssd_tensorflow_amd._lib import lib
    assert callable(getattr(lib, 'ssd_op_conv2d_fwd_mxfp8_bigk'))


def test_signature_is_the_mxfp8_convolutions():
    from ssd_tensorflow_amd._lib import lib, SIGNATURES
    res, args = SIGNATURES['ssd_op_conv2d_fwd_mxfp8_bigk']
    assert res is C.c_int and len(args) == 24
    assert (res, args) == SIGNATURES['ssd_op_conv2d_fwd_mxfp8']      # the same argument list and contract, for 10 ... 121 taps
    assert lib.ssd_op_conv2d_fwd_mxfp8_bigk.argtypes == args
