"""-m gpu: quantised inference on TWO forward lanes.  Every other quantised model test runs at batch 2: one lane, whose samples start at
offset 0 of every code and scale tensor.  From batch 8 on the forward pass cuts the batch in two lanes, and the second lane's quantise
passes, convolutions and pools address their operands at a non-zero sample offset (Net::q_at) -- the path of tools/infer_rate.py and
detect at batch 128.  Batch 9 is the smallest odd batch that takes it: 5 + 4 samples, lane 1 starts at sample 5, and the full-batch heads
run behind both lanes.

The same 9 images are inferred as one call (two lanes) and as calls of 2, 2, 2, 2, 1 (one lane: the covered path), on a quantised and on
a bf16 handle.  The bound is measured inside the test, on the covered path: with e1[i] the quantised result's error against bf16 on the
chunked passes, e2[i] the same on the batch-9 passes and d[i] quantised batch-9 against quantised chunked, every sample must satisfy
e2[i] <= 2 max(e1) and d[i] <= max(e1).  The only legitimate difference between the two ways is another tile's summation order in front
of a bf16 rounding (1e-3, test_step_lane_settings_agree), ten times below the quantisation error itself; a wrong sample offset reads
another sample's codes or scales, an error of order 1."""
import ctypes as C

import numpy as np
import pytest

from gpu_util import lib, check, rel_err
from ssd_tensorflow_amd.ssdvgg import DTYPES
from test_gpu_mxfp8 import build

pytestmark = pytest.mark.gpu

B = 9
CHUNKS = (2, 2, 2, 2, 1)


@pytest.fixture(scope='module')
def setup():
    from oracle import boxes as ob, ssdvgg_ref as ref
    from ssd_tensorflow_amd.ssdvgg import Session
    preset = ob.get_preset('vgg300')
    w = ref.init_params(preset, 20, seed=42, alive=True)
    x = ref.synth_images(np.random.default_rng(99), B, preset)
    sess = Session(0)
    bf16 = build(sess, 'vgg300', w, B, 'bf16')
    yield dict(w=w, x=x, sess=sess, bf16=both_ways(bf16, x))
    sess.close()


def both_ways(net, x):
    """(the result of one call at b = 9, the results of the chunked calls joined)"""
    whole = net.infer(x)
    starts = np.cumsum((0,) + CHUNKS)
    chunked = np.concatenate([net.infer(x[a:a + n]) for a, n in zip(starts, CHUNKS)])
    assert whole.shape == chunked.shape and whole.shape[0] == B
    return whole, chunked


@pytest.mark.parametrize('dtype', ['fp8', 'mxfp8', 'mxfp6'])
def test_two_lanes_agree_with_one(setup, dtype, capsys):
    x = setup['x']
    net = build(setup['sess'], 'vgg300', setup['w'], B, dtype)
    code = C.c_int(-1)
    check(lib.ssd_get_dtype(net._h, C.byref(code)))      # what the handle itself reports, not the string it was asked for
    assert code.value == DTYPES[dtype] and net.dtype == dtype
    if dtype == 'fp8':
        net.calibrate_fp8(x)      # once, on the 9 images: every pass below uses these scales
        scales = net.fp8_scales
        assert len(scales) > 0 and all(v > 0 for v in scales.values())
    q9, qc = both_ways(net, x)
    r9, rc = setup['bf16']
    e1 = [rel_err(qc[i], rc[i]) for i in range(B)]
    e2 = [rel_err(q9[i], r9[i]) for i in range(B)]
    d = [rel_err(q9[i], qc[i]) for i in range(B)]
    with capsys.disabled():
        print(f'\n[quant lanes] {dtype}: max(e1) = {max(e1):.4e}, max(e2) = {max(e2):.4e}, max(d) = {max(d):.4e}')
    assert 0 < max(e1) < 0.5, e1
    for i in range(B):
        assert e2[i] <= 2 * max(e1), (i, e2[i], max(e1))
        assert d[i] <= max(e1), (i, d[i], max(e1))
