"""CPU: the mxfp8 oracle (tests/mxfp8_ref.py) against torch.float8_e8m0fnu / torch.float8_e4m3fn and against the scale rule's
definition, and what of the mxfp8 feature can be seen without a GPU: the exported ops and the refusal of a training handle."""
import ctypes as C

import numpy as np
import pytest
import torch

import fp8_ref as f8
import mxfp8_ref as mx


def bits(u):
    return np.array(u, np.uint32).view(np.float32)


def boundary_values():
    """448 * 2^k and 1.75 * 2^k, each with its neighbours one ulp down and up, over the whole fp32-normal range of the rule"""
    out = []
    for k in range(-126, 128):
        base = np.float32(np.ldexp(1.75, k)).view(np.uint32)      # (448 * 2^k is 1.75 * 2^(k + 8))
        out += [base - 1, base, base + 1]
    v = bits(out)
    return v[np.isfinite(v)]


def test_scale_bytes_agree_with_torch_e8m0():
    assert torch.tensor([1.0]).to(torch.float8_e8m0fnu).view(torch.uint8).item() == 127
    assert torch.tensor([2.0 ** -127]).to(torch.float8_e8m0fnu).view(torch.uint8).item() == 0
    e = np.arange(255, dtype=np.uint8)                            # (255 is NaN in E8M0: never written)
    theirs = torch.from_numpy(e).view(torch.float8_e8m0fnu).float().numpy().astype(np.float64)
    assert np.array_equal(mx.scale_values(e), theirs)
    # and the other way: the byte the rule picks for a block whose absmax is 448 * 2^x is torch's byte of 2^x
    x = np.arange(-126, 120)
    am = np.ldexp(np.float32(448.0), x).astype(np.float32)
    want = torch.from_numpy(np.ldexp(np.float32(1.0), x).astype(np.float32)).to(torch.float8_e8m0fnu).view(torch.uint8).numpy()
    assert np.array_equal((mx.scale_exponent(am) + 127).astype(np.uint8), want)


def test_codes_agree_with_torch_e4m3():
    rng = np.random.default_rng(21)
    v = (rng.normal(0, 1, (500, 64)) * np.exp2(rng.integers(-20, 20, (500, 2)).repeat(32, 1))).astype(np.float32)
    codes, scales = mx.quantize(v)
    x = np.repeat(scales.astype(np.int32) - 127, 32, axis=-1)
    scaled = torch.from_numpy(np.ldexp(v, -x)).clamp(-448.0, 448.0)
    assert np.array_equal(codes, scaled.to(torch.float8_e4m3fn).view(torch.uint8).numpy())
    # every block uses its range: absmax / 2^x lies in (224, 448]
    top = np.abs(f8.decode(codes)).reshape(500, 2, 32).max(-1)
    assert np.all(top >= 224.0) and np.all(top <= 448.0)
    back = mx.dequantize(codes, scales)
    assert np.all(np.abs(back - v) <= np.repeat(mx.scale_values(scales), 32, -1) * f8.e4m3_step(f8.decode(codes)) / 2)


def test_rule_equals_definition_at_boundaries():
    v = boundary_values()
    assert v.size > 700
    assert np.array_equal(mx.scale_exponent(v), mx.scale_exponent_by_definition(v))
    rng = np.random.default_rng(22)
    r = bits(rng.integers(0x00800000, 0x7F800000, 5000, dtype=np.uint32))
    assert np.array_equal(mx.scale_exponent(r), mx.scale_exponent_by_definition(r))
    # the named points
    se = lambda a: int(mx.scale_exponent(np.array([a], np.float32))[0])
    assert se(448.0) == 0 and se(np.nextafter(np.float32(448.0), np.float32(1e9))) == 1 and se(np.nextafter(np.float32(448.0), np.float32(0))) == 0
    assert se(1.75) == -8 and se(np.nextafter(np.float32(1.75), np.float32(2))) == -7 and se(1.0) == -8 and se(2.0) == -7
    z = np.zeros((1, 32), np.float32)
    codes, scales = mx.quantize(z)
    assert scales[0, 0] == 0 and not codes.any()                   # an all-zero block: byte 0, no special case
    big = np.full((1, 32), np.finfo(np.float32).max, np.float32)
    codes, scales = mx.quantize(big)
    assert scales[0, 0] == 127 + 120 and scales.max() < 255         # largest finite: 2^128 (1 - 2^-24) / 2^120 = 256 (1 - 2^-24): no byte 255
    assert np.all(f8.decode(codes) == 256.0)


def test_quantize_dequantize_identity_on_small_integer_blocks():
    rng = np.random.default_rng(23)
    i = rng.integers(0, 8, (300, 96))
    i[:, ::32] = 7                                                  # (any block content works; this one has its maximum at 7)
    s = rng.integers(-40, 40, (300, 3)).repeat(32, 1)
    v = np.ldexp(i.astype(np.float32), s).astype(np.float32)
    v[5] = 0
    v[6, :32] = np.ldexp(np.arange(32) % 8, 3)                      # a block without a 7
    codes, scales = mx.quantize(v)
    assert np.array_equal(mx.dequantize(codes, scales), v.astype(np.float64))
    # signs too
    codes, scales = mx.quantize(-v)
    assert np.array_equal(mx.dequantize(codes, scales), -v.astype(np.float64))


def test_pool_requantises_per_block():
    codes = np.zeros((1, 2, 2, 32), np.uint8)
    scales = np.array([127, 130, 120, 127], np.uint8).reshape(1, 2, 2, 1)
    codes[0, 0, 0, :] = f8.encode(np.full(32, 3.0))                 # 3
    codes[0, 0, 1, :] = f8.encode(np.full(32, 1.0))                 # 8: the window's maximum
    codes[0, 1, 0, :] = f8.encode(np.full(32, 448.0))               # 448 / 128 = 3.5
    codes[0, 1, 1, 0] = f8.encode(np.array([20.0]))[0]              # channel 0: 20
    y8, ys = mx.maxpool(codes, scales, 2, 2)
    assert y8.shape == (1, 1, 1, 32) and ys.shape == (1, 1, 1, 1)
    got = mx.dequantize(y8, ys)[0, 0, 0]
    assert got[0] == 20.0 and np.all(got[1:] == 8.0) and ys[0, 0, 0, 0] == 127 + int(mx.scale_exponent(np.array([20.0], np.float32))[0])


def test_library_exports_the_mxfp8_ops():
    from ssd_tensorflow_amd._lib import lib
    for name in ('ssd_op_quantize_mxfp8', 'ssd_op_conv2d_fwd_mxfp8', 'ssd_op_maxpool_fwd_mxfp8'):
        assert callable(getattr(lib, name))


def test_library_refuses_mxfp8_training_handle():
    from ssd_tensorflow_amd._lib import lib, last_error
    h = C.c_void_p()
    rc = lib.ssd_create_dtype(b'vgg300', 20, 2, 0, 1, 0, None, None, None, 3, C.byref(h))
    assert rc != 0 and not h.value
    assert last_error() == 'SSD_DTYPE_MXFP8 is inference only: create the handle with training = 0'
    rc = lib.ssd_create_graph(b'vgg300', 20, 2, 0, 1, 0, None, None, None, 3, 1, C.byref(h))
    assert rc != 0 and 'inference only' in last_error()
