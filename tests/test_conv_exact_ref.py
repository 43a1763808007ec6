"""tests/conv_exact_ref.py without a GPU: the numpy reference equals oracle.ssdvgg_ref.conv2d_tf plus autograd in float64 on the exact
operands of every case the GPU tests use, the operands are admissible (asserted by the generator), and they SEE the bugs the exact
tests are for: each mutation below changes the expected tensor it bears on, for every case it can apply to (a swapped tap or another
dilation has no meaning for a 1x1 filter or a 1x1 image, a (ci, co) transpose needs ci == co)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_exact_ref as cx
from oracle import ssdvgg_ref as ref
from gpu_util import conv_geom
from test_gpu_conv_exact import FP32_CASES, BF16_CASES, CHAIN_CASES, FIRST_CASES, C64_CASE, operands, c64_operands


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if c[1:11] not in seen:
            seen.add(c[1:11])
            out.append(c[:11])
    return out


CASES = _unique(FP32_CASES + BF16_CASES + CHAIN_CASES + FIRST_CASES + [C64_CASE])
IDS = [c[0] for c in CASES]


def test_the_lists_hold_the_shapes_the_exact_tests_are_for():
    names = ' | '.join(c[0] for c in CASES)
    for part in ('1x3x2', 'one pixel over a 128-row tile', '64->8', '136->64', 'dil6', 's2', 'VALID', 'pad-BR', '1x1', 'head', '7x7', 'smallC'):
        assert part in names, part
    m = [c for c in CASES if 'one pixel over' in c[0]][0]
    assert m[1] * m[2] * m[3] == 129


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_reference_equals_the_oracle_with_autograd(case):
    name, b, hi, wi, ci, co, k, stride, dil, padding, relu = case
    o = operands(case)
    g = o.g
    assert (g.ph, g.pw, g.ho, g.wo) == conv_geom(hi, wi, k, stride, dil, padding)
    xt = torch.tensor(o.x).permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.tensor(o.w).requires_grad_(True)
    bt = torch.tensor(o.bias).requires_grad_(True)
    xin = F.pad(xt, (0, 1, 0, 1)) if padding == 'BR1' else xt
    pre = ref.conv2d_tf(xin, wt, stride, 'SAME' if padding == 'SAME' else 'VALID', dil) + bt.view(1, -1, 1, 1)
    assert pre.dtype == torch.float64
    y = F.relu(pre) if relu else pre
    assert np.array_equal(y.detach().permute(0, 2, 3, 1).numpy(), o.y)
    pre.backward(torch.tensor(o.dy).permute(0, 3, 1, 2))
    dx = xt.grad.permute(0, 2, 3, 1).numpy()
    assert np.array_equal(dx, o.dx)
    assert np.array_equal((dx + o.prev) * (o.mask > 0), o.dxm)
    assert np.array_equal(cx.dgrad(o.dy, o.w, g, o.prev, o.mask, absacc=False)[0], o.dxm)
    assert np.array_equal(wt.grad.numpy() + o.wd * o.w, o.dw)
    assert np.array_equal(bt.grad.numpy(), o.db)
    # the sums of magnitudes are the same functions of the magnitudes
    _, ay = cx.forward(o.x, o.w, o.bias, relu, g)
    assert np.array_equal(ay, cx.forward(np.abs(o.x), np.abs(o.w), 0 * o.bias, False, g, absacc=False)[0])
    # every expectation is an fp32 value, and a bf16 store would round some of them (the RNE check is not vacuous) unless all fit
    for v in (o.y, o.dx, o.dxm, o.dw, o.db):
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    assert relu is False or (o.y == 0).any() and (o.y > 0).any()


def _rot(a):
    """one 32-channel block (the first; all channels of a narrower tensor) rotated by one channel"""
    a = a.copy()
    n = min(32, a.shape[-1])
    a[..., :n] = np.roll(a[..., :n], 1, axis=-1)
    return a


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_the_operands_see_the_bugs(case):
    o = operands(case)
    g, k, relu = o.g, case[6], o.relu
    fwd = lambda x=o.x, w=o.w, gg=g: cx.forward(x, w, o.bias, relu, gg, absacc=False)[0]
    dgr = lambda dy=o.dy, w=o.w, gg=g: cx.dgrad(dy, w, gg, absacc=False)[0]
    wgr = lambda x=o.x, dy=o.dy, gg=g, wd=o.wd: cx.wgrad(x, dy, o.w, wd, gg, absacc=False)[0]
    differs = lambda a, b: not np.array_equal(a, b)
    if k > 1 and g.hi * g.wi > 1:      # (a 1x1 image under a SAME 3x3 filter meets the centre tap alone)
        wt = np.ascontiguousarray(o.w.transpose(1, 0, 2, 3))
        assert differs(fwd(w=wt), o.y) and differs(dgr(w=wt), o.dx) and differs(o.dw.transpose(1, 0, 2, 3), o.dw), 'kh / kw swapped'
        g2 = g.replace(dil=g.dil + 1)
        assert differs(fwd(gg=g2), o.y) and differs(dgr(gg=g2), o.dx) and differs(wgr(gg=g2), o.dw), 'dilation off by one'
    if g.ci == g.co:
        wt = np.ascontiguousarray(o.w.transpose(0, 1, 3, 2))
        assert differs(fwd(w=wt), o.y) and differs(dgr(w=wt), o.dx) and differs(o.dw.transpose(0, 1, 3, 2), o.dw), 'filter transposed in (ci, co)'
    for g2 in (g.replace(ph=g.ph + 1), g.replace(pw=g.pw + 1)):
        assert differs(fwd(gg=g2), o.y) and differs(dgr(gg=g2), o.dx) and differs(wgr(gg=g2), o.dw), 'pad shifted by one'
    assert differs(fwd(x=_rot(o.x)), o.y) and differs(wgr(x=_rot(o.x)), o.dw), 'a 32-channel block of x rotated'
    assert differs(dgr(dy=_rot(o.dy)), o.dx) and differs(wgr(dy=_rot(o.dy)), o.dw), 'a 32-channel block of dy rotated'
    nz = o.w != 0
    assert np.all(wgr(wd=0.0)[nz] != o.dw[nz]), 'wd term dropped'
    assert differs(cx.dgrad(o.dy, o.w, g, o.prev, o.mask, mask_ge=True, absacc=False)[0], o.dxm), 'mask > replaced by >='
    assert differs(cx.dgrad(o.dy, o.w, g, None, o.mask, absacc=False)[0], o.dxm), 'accumulate dropped'
    assert differs(o.dxm, o.dx + o.prev), 'mask dropped'


def test_bf16_round_is_round_to_nearest_even():
    v = np.array([1.0, 257.0, 258.0, 259.0, 261.0, 262.0, -259.0, 1023.0, 0.0, 3.0 * 2 ** 20 + 2 ** 12], np.float64)
    want = torch.tensor(v, dtype=torch.float32).bfloat16().double().numpy()
    assert np.array_equal(cx.bf16_round(v), want)
    assert cx.bf16_round(np.array([257.0]))[0] == 256.0 and cx.bf16_round(np.array([259.0]))[0] == 260.0      # both ties: to even
    o = operands(CASES[2])
    assert not np.array_equal(cx.bf16_round(o.dx), o.dx), 'the exact data gradient must not fit bf16, or RNE is never exercised'


def test_c64_operands_are_admissible():
    o, g1, image, w1, dw1, db1 = c64_operands()
    assert image.min() == 0 and image.max() == 3 and np.array_equal(dw1.astype(np.float32).astype(np.float64), dw1)
    assert not np.array_equal(cx.wgrad(image, o.dx * (o.mask > 0), w1, cx.WD, g1, absacc=False)[0], dw1), 'the bf16 rounding of dx must show'
