"""CPU: the fp8 oracle (tests/fp8_ref.py) against torch.float8_e4m3fn, and the host-only refusals of the fp8 handle."""
import ctypes as C

import numpy as np
import pytest
import torch

import fp8_ref as f8


def torch_decode(codes):
    return torch.from_numpy(np.asarray(codes, np.uint8)).view(torch.float8_e4m3fn).float().numpy()


def torch_encode_clamped(v):
    """clamp first: torch's own cast turns 480 into NaN"""
    t = torch.from_numpy(np.asarray(v, np.float32)).clamp(-448.0, 448.0)
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_all_codes_decode_like_torch_and_round_trip():
    codes = np.arange(256, dtype=np.uint8)
    mine, theirs = f8.decode(codes), torch_decode(codes)
    finite = np.isfinite(theirs)
    assert finite.sum() == 254 and np.array_equal(np.isnan(mine), ~finite)
    assert np.array_equal(mine[finite], theirs[finite].astype(np.float64))
    assert np.array_equal(np.signbit(mine[finite]), np.signbit(theirs[finite]))
    assert np.array_equal(f8.encode(mine[finite]), codes[finite])
    assert mine[0x7E] == 448.0 and mine[0xFE] == -448.0 and mine[0x01] == 2.0 ** -9 and mine[0x08] == 2.0 ** -6


def test_ties_subnormals_saturation():
    d = lambda v: float(f8.decode(f8.encode(np.array([v])))[0])
    assert d(1.0625) == 1.0 and d(1.1875) == 1.25              # ties to the even code
    assert d(-1.0625) == -1.0 and d(-1.1875) == -1.25
    assert d(2.0 ** -10) == 0.0                                 # half the smallest subnormal: tie to 0
    assert d(1.5 * 2.0 ** -9) == 2.0 ** -8 and d(2.5 * 2.0 ** -9) == 2.0 ** -8
    assert d(2.0 ** -9) == 2.0 ** -9 and d(7.5 * 2.0 ** -9) == 2.0 ** -6
    for v in (464.0, 480.0, 1e6):
        assert d(v) == 448.0 and d(-v) == -448.0
    assert f8.encode(np.array([-0.0]))[0] == 0x80 and f8.encode(np.array([0.0]))[0] == 0x00


def test_random_floats_match_clamped_torch_cast():
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.normal(0, 1, 40000), rng.normal(0, 200, 30000), rng.normal(0, 0.01, 20000),
                        rng.uniform(-500, 500, 10000)]).astype(np.float32)
    assert v.size == 100000
    assert np.array_equal(f8.encode(v), torch_encode_clamped(v))
    # ... and every tie between two neighbouring codes
    pos = f8.decode(np.arange(0x7F, dtype=np.uint8))
    mids = ((pos[1:] + pos[:-1]) / 2).astype(np.float32)
    both = np.concatenate([mids, -mids])
    assert np.array_equal(f8.encode(both), torch_encode_clamped(both))


def test_quantize_filter_layout_and_scales():
    rng = np.random.default_rng(2)
    w = rng.normal(0, 1, (3, 3, 8, 5)).astype(np.float32)
    w[..., 1] = 0
    w[0, 0, 0, 2] = -7.0
    codes, s = f8.quantize_filter(w)
    assert codes.shape == (9, 5, 8) and s.dtype == np.float32
    assert s[1] == 1.0 and np.all(codes[:, 1, :] == 0) and s[2] == np.float32(7.0) / np.float32(448.0)
    assert codes[0, 2, 0] == 0xFE                              # the channel's absmax maps to -448
    back = f8.decode(codes) * s[None, :, None]
    assert np.abs(back - np.transpose(w.reshape(9, 8, 5), (0, 2, 1))).max() <= np.abs(w).max() / 16


def test_python_refuses_fp8_training_before_any_gpu_call():
    from ssd_tensorflow_amd.ssdvgg import SSDVGG
    with pytest.raises(ValueError, match='fp8'):
        SSDVGG(None, 'vgg300')._create(20, 2, True, 0, dtype='fp8')
    with pytest.raises(ValueError, match="'f32', 'bf16' or 'fp8'"):
        SSDVGG(None, 'vgg300')._create(20, 2, False, 0, dtype='fp16')


def test_library_refuses_fp8_training_handle():
    from ssd_tensorflow_amd._lib import lib, last_error
    h = C.c_void_p()
    rc = lib.ssd_create_dtype(b'vgg300', 20, 2, 0, 1, 0, None, None, None, 2, C.byref(h))
    assert rc != 0 and not h.value
    assert last_error() == 'SSD_DTYPE_FP8 is inference only: create the handle with training = 0'
    rc = lib.ssd_create_graph(b'vgg300', 20, 2, 0, 1, 0, None, None, None, 2, 0, C.byref(h))
    assert rc != 0 and 'inference only' in last_error()
