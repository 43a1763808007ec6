"""-m gpu: the fp32, bf16 and conv1_1 training convolutions against tests/conv_exact_ref.py, through the C ABI.

  * Value for value on operands whose sums are exact in fp32 in any order (conv_exact_ref.operands: i * 2^s, asymmetric in every
    index, zeros and negative values in x, the relu mask and the accumulated tensor; weight decay 0.25).  A bf16 store is the
    round-to-nearest-even of the exact value.  No tolerance: a term that is missing, doubled, misplaced or masked with >= shows.
  * The weight decay of every weight-gradient entry point made visible: with dy = 0 (and with x = 0) dw is the single fp32 product
    wd * w of a real-valued w at wd = 0.0005, db is exactly 0 (x = 0: the exact column sums); with wd = 0 a non-null w changes nothing.
  * The fp32 direct kernels on the Gaussian inputs of tests/test_gpu_kernels.py against float64, per element:
    |err| <= K * 2^-23 * sum |x * w| (mxfp6_ref.accumulation_bound), K the length of the sum.
  * All of it again in child processes under the forced kernel variants (the library reads its switches once per process).

The case lists are the kernels' own (test_gpu_kernels.CONV_CASES, test_gpu_bf16.CONV_CASES / FIRST_CASES, test_gpu_tail.TAIL_CASES)
plus conv_exact_ref.EXTRA_CASES and a 7x7 layer (csrc/conv_bigk.hip); tests/test_conv_exact_ref.py shows on the CPU that the operands
of every case see a swapped tap, a transposed filter, a shifted pad, a wrong dilation, a rotated channel block, a dropped weight decay,
a >= mask and a dropped accumulate.

That these tests can fail was shown with one-line edits of the kernels, one library each, all tests of before passing on every "wd" edit:
  "+ wd * w" dropped from                          caught by
  wgrad_reduce_kernel (conv_igemm.hip)             test_fp32_exact, test_bf16_exact, test_first_layer_bf16_exact, test_weight_decay_* (96 tests)
  wgrad_reduce_wide_kernel (32 ... 255 slabs)      test_weight_decay_first_layer_many_slabs[160x160]
  wgrad_reduce_many_kernel (256 slabs and more)    test_weight_decay_first_layer_many_slabs[512x512]
  the direct epilogue of conv_bf16.hip             test_bf16_chain_exact, test_weight_decay_bf16_direct (every case)
  conv_bigk.hip                                    the 7x7 case of test_fp32_exact, test_bf16_exact, test_weight_decay_fp32 / _bf16
  wino_wgrad_reduce_kernel (winograd.hip)          tests/test_gpu_wino_bound.py, every case of both tests
  (conv1_1's weight gradients, the one inside conv1_2's data gradient included, end in the first three)
  mask "> 0" turned into ">= 0" in                 caught by
  conv_gather_dma_kernel (conv_igemm.hip)          test_fp32_exact, every case with a data gradient
  the bf16 gather kernels' epilogue                test_bf16_exact, every case;  the persistent 64 -> 64 kernel: test_dgrad_first_wgrad_in_c64_child
  tail_bf16.hip                                    test_bf16_chain_exact, every case
  (conv_gather_kernel's data-gradient mask is not reached: only a stride that is no power of two under SSD_DGRAD_PARITY=0 runs it, and
  the default configuration refuses such a stride)

Found by test_bf16_chain_exact (64 -> 8 and 64 -> 64 on maps below 64 pixels): the chain's k split left a task without a k group when 9
groups met 4 splits, and that task still primed its filter stream 4 KB past the packed filter (csrc/tail_bf16.hip, fixed in the planner)."""
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import conv_exact_ref as cx
import mxfp6_ref as m6
from gpu_util import lib, check, dev, ptr, host
import test_gpu_kernels as tk
import test_gpu_bf16 as tb
import test_gpu_tail as tt
from test_gpu_bf16 import bdev, bhost

pytestmark = pytest.mark.gpu

BIGK = ('7x7 (more than 9 taps) 5x7 40->72', 1, 5, 7, 40, 72, 7, 1, 1, 'SAME', True)
# (name, b, hi, wi, ci, co, k, stride, dil, padding, relu)
FP32_CASES = list(tk.CONV_CASES) + cx.EXTRA_CASES + [BIGK]
# (..., y_f32): the extra shapes with both kinds of output
BF16_CASES = list(tb.CONV_CASES) + [c + (f,) for c in cx.EXTRA_CASES + [BIGK] for f in (False, True)]
CHAIN_CASES = list(tt.TAIL_CASES) + [c + (False,) for c in cx.EXTRA_CASES]
# conv1_1 (3 -> 64) on image values 0 ... 255; the full-size image is left out (its sums of magnitudes pass 2^24 LSB)
FIRST_CASES = [(n, b, h, w, 3, 64, 3, 1, 1, 'SAME', True) for n, b, h, w in tb.FIRST_CASES if h * w < 300 * 300]
C64_CASE = ('conv1_2 on conv1_1, 2x40x33', 2, 40, 33, 64, 64, 3, 1, 1, 'SAME', True)
WD_REAL = 0.0005


def ids(cases):
    return [c[0] + (' f32 out' if len(c) > 11 and c[11] and 'f32 out' not in c[0] else '') for c in cases]


@functools.lru_cache(maxsize=None)
def operands(case):
    """the exact operands and expectations of a case: computed once per process, shared and read-only"""
    o = cx.operands(case[:11], image=case[4] == 3)
    for v in vars(o).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


def same(got, want, what):
    """value for value (a zero's sign does not matter); the first mismatches on failure"""
    want32 = np.asarray(want, np.float32)
    assert np.array_equal(want32.astype(np.float64), want), f'{what}: the expectation itself is not an fp32 value'
    assert got.shape == want32.shape, (what, got.shape, want32.shape)
    if not np.array_equal(got, want32):
        bad = np.argwhere(got != want32)
        first = [(tuple(int(j) for j in i), float(got[tuple(i)]), float(want32[tuple(i)])) for i in bad[:6]]
        pytest.fail(f'{what}: {len(bad)} of {got.size} values differ; (index, got, want) {first}')


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def full(shape, v, dtype=torch.float32):
    return torch.full(tuple(shape), v, dtype=dtype, device='cuda')


def wgrad_ws(fn, geom):
    return torch.empty((max(int(fn(*geom)), 1),), dtype=torch.float32, device='cuda')


# ---- fp32 direct ---------------------------------------------------------------------------------------------------------------------

def run_fp32(x, w, bias, dy, prev, mask, wd, geom, relu, dgrad):
    """-> y, dw, db, dx, dxm (numpy) of the fp32 entry points"""
    b, hi, wi, ci, ho, wo, co, kh, kw = geom[:9]
    x_, w_, b_, dy_ = dev(f32(x)), dev(f32(w)), dev(f32(bias)), dev(f32(dy))
    y_ = full((b, ho, wo, co), 9.0)
    check(lib.ssd_op_conv2d_fwd(ptr(x_), ptr(w_), ptr(b_), ptr(y_), *geom, int(relu), None))
    ws_ = wgrad_ws(lib.ssd_op_conv2d_wgrad_ws_floats, geom)
    gw_, gb_ = full((kh, kw, ci, co), 7.0), full((co,), 7.0)
    check(lib.ssd_op_conv2d_wgrad(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_), wd, ptr(ws_), *geom, None))
    out = [host(y_), host(gw_), host(gb_), None, None]
    if dgrad:
        gx_ = full((b, hi, wi, ci), 3.0)
        check(lib.ssd_op_conv2d_dgrad(ptr(dy_), ptr(w_), ptr(gx_), None, 0, *geom, None))
        ga_, m_ = dev(f32(prev)), dev(f32(mask))
        check(lib.ssd_op_conv2d_dgrad(ptr(dy_), ptr(w_), ptr(ga_), ptr(m_), 1, *geom, None))
        out[3:] = [host(gx_), host(ga_)]
    return out


@pytest.mark.parametrize('case', FP32_CASES, ids=ids(FP32_CASES))
def test_fp32_exact(case):
    o = operands(case)
    name, dgrad = case[0], o.g.ci % 4 == 0
    y, dw, db, dx, dxm = run_fp32(o.x, o.w, o.bias, o.dy, o.prev, o.mask, o.wd, o.g.abi(), o.relu, dgrad)
    same(y, o.y, f'{name}: forward')
    same(dw, o.dw, f'{name}: weight gradient + wd * w')
    same(db, o.db, f'{name}: bias gradient')
    if dgrad:
        same(dx, o.dx, f'{name}: data gradient')
        same(dxm, o.dxm, f'{name}: data gradient, accumulate + mask')


# ---- bf16 ----------------------------------------------------------------------------------------------------------------------------

def cast_filter(w, k, ci, co):
    w_ = dev(f32(w))
    wio_ = torch.empty((k * k, ci, co), dtype=torch.bfloat16, device='cuda')
    woi_ = torch.empty((k * k, co, ci), dtype=torch.bfloat16, device='cuda')
    check(lib.ssd_op_cast_filter(ptr(w_), ptr(wio_), ptr(woi_), k * k, ci, co, None))
    return w_, wio_, woi_


def check_bf16(case, chain):
    o = operands(case)
    name, y_f32, g = case[0], bool(case[11]), o.g
    geom = g.abi()
    w_, wio_, woi_ = cast_filter(o.w, g.kh, g.ci, g.co)
    same(bhost(wio_).reshape(o.w.shape), o.w, f'{name}: filter mirror [tap][Ci][Co]')
    same(bhost(woi_), np.transpose(o.w.reshape(g.kh * g.kw, g.ci, g.co), (0, 2, 1)), f'{name}: filter mirror [tap][Co][Ci]')
    fwd = lib.ssd_op_conv2d_fwd_bf16_chain if chain else lib.ssd_op_conv2d_fwd_bf16
    dgrad = lib.ssd_op_conv2d_dgrad_bf16_chain if chain else lib.ssd_op_conv2d_dgrad_bf16
    x_, b_, dy_ = bdev(f32(o.x)), dev(f32(o.bias)), bdev(f32(o.dy))
    y_ = full((g.b, g.ho, g.wo, g.co), 9.0, torch.float32 if y_f32 else torch.bfloat16)
    check(fwd(ptr(x_), ptr(woi_), ptr(b_), ptr(y_), int(y_f32), *geom, int(o.relu), None))
    same(bhost(y_), o.y if y_f32 else cx.bf16_round(o.y), f'{name}: forward, {"fp32" if y_f32 else "bf16 (RNE)"} out')
    gw_, gb_ = full(o.w.shape, 7.0), full((g.co,), 7.0)
    if chain:
        check(lib.ssd_op_conv2d_wgrad_bf16_direct(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_), o.wd, *geom, None))
    else:
        ws_ = wgrad_ws(lib.ssd_op_conv2d_wgrad_bf16_ws_floats, geom)
        check(lib.ssd_op_conv2d_wgrad_bf16(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_), o.wd, ptr(ws_), *geom, None))
    same(host(gw_), o.dw, f'{name}: weight gradient + wd * w')
    same(host(gb_), o.db, f'{name}: bias gradient')
    gx_ = full(o.x.shape, 3.0, torch.bfloat16)
    check(dgrad(ptr(dy_), ptr(wio_), ptr(gx_), None, 0, *geom, None))
    same(bhost(gx_), cx.bf16_round(o.dx), f'{name}: data gradient, RNE(dx)')
    ga_, m_ = bdev(f32(o.prev)), bdev(f32(o.mask))
    check(dgrad(ptr(dy_), ptr(wio_), ptr(ga_), ptr(m_), 1, *geom, None))
    same(bhost(ga_), cx.bf16_round(o.dxm), f'{name}: data gradient, RNE(prev + dx) under the mask')


@pytest.mark.parametrize('case', BF16_CASES, ids=ids(BF16_CASES))
def test_bf16_exact(case):
    check_bf16(case, chain=False)


@pytest.mark.parametrize('case', CHAIN_CASES, ids=ids(CHAIN_CASES))
def test_bf16_chain_exact(case):
    check_bf16(case, chain=True)


# ---- conv1_1 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', FIRST_CASES, ids=ids(FIRST_CASES))
def test_first_layer_bf16_exact(case):
    """fp32 image 0 ... 255 and fp32 master filter in, bf16 activations out, fp32 gradients"""
    o = operands(case)
    name, g = case[0], o.g
    geom = g.abi()
    assert o.x.min() >= 0 and o.x.max() <= 255 and np.array_equal(o.x, np.round(o.x)) and len(np.unique(o.x)) > 40
    x_, w_, b_, dy_ = dev(f32(o.x)), dev(f32(o.w)), dev(f32(o.bias)), bdev(f32(o.dy))
    y_ = full((g.b, g.ho, g.wo, g.co), 9.0, torch.bfloat16)
    check(lib.ssd_op_conv2d_first_fwd_bf16(ptr(x_), ptr(w_), ptr(b_), ptr(y_), *geom, 1, None))
    same(bhost(y_), cx.bf16_round(o.y), f'{name}: forward, bf16 (RNE) out')
    ws_ = wgrad_ws(lib.ssd_op_conv2d_first_wgrad_bf16_ws_floats, geom)
    gw_, gb_ = full(o.w.shape, 7.0), full((g.co,), 7.0)
    check(lib.ssd_op_conv2d_first_wgrad_bf16(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_), o.wd, ptr(ws_), *geom, None))
    same(host(gw_), o.dw, f'{name}: weight gradient + wd * w')
    same(host(gb_), o.db, f'{name}: bias gradient')


def c64_operands():
    """conv1_2's data gradient with conv1_1's weight gradient inside: dy, w2 and the mask from the 64 -> 64 case, an image of small
    integers (0 ... 3: the sums of magnitudes stay below 2^24 LSB), conv1_1's filter w1.
    Expectation: dw1, db1 of RNE_bf16(dgrad(dy, w2) * (mask > 0)), the dx the kernel never writes."""
    o = operands(C64_CASE)
    g1 = cx.Geom(o.g.b, o.g.hi, o.g.wi, 3, 64, 3, 1, 1, 'SAME')
    first = cx.make_operands(g1, (0, 1, 0), True)
    image, w1 = first.x % 4, first.w
    dx = cx.bf16_round(o.dx * (o.mask > 0))
    dw1, db1, adw, adb = cx.wgrad(image, dx, w1, cx.WD, g1)
    assert max(adw.max() + np.abs(cx.WD * w1).max(), adb.max()) / cx.LSB < 2 ** 24
    assert cx.distinct_enough(dw1) and cx.distinct_enough(db1)
    return o, g1, image, w1, dw1, db1


def run_dgrad_first_wgrad(dy, w2, mask, image, w1, wd, b, h, w):
    _, wio_, _ = cast_filter(w2, 3, 64, 64)
    dy_, m_, img_, w1_ = bdev(f32(dy)), bdev(f32(mask)), dev(f32(image)), dev(f32(w1))
    ws_ = torch.empty((lib.ssd_op_conv2d_dgrad_first_wgrad_bf16_ws_floats(b, h, w),), dtype=torch.float32, device='cuda')
    gw_, gb_ = full((3, 3, 3, 64), 9.0), full((64,), 9.0)
    check(lib.ssd_op_conv2d_dgrad_first_wgrad_bf16(ptr(dy_), ptr(wio_), ptr(m_), ptr(img_), ptr(gw_), ptr(gb_), ptr(w1_), wd, ptr(ws_), b, h, w, None))
    return host(gw_), host(gb_)


def c64_child():
    """what test_dgrad_first_wgrad_in_c64_child runs under SSD_C64_BF16=2: the exact operands, then the weight decay made visible"""
    assert os.environ.get('SSD_C64_BF16') == '2'
    o, g1, image, w1, dw1, db1 = c64_operands()
    b, h, wi = g1.b, g1.hi, g1.wi
    name = 'conv1_1 weight gradient inside the conv1_2 data gradient'
    dw, db = run_dgrad_first_wgrad(o.dy, o.w, o.mask, image, w1, cx.WD, b, h, wi)
    same(dw, dw1, f'{name}: dw + wd * w')
    same(db, db1, f'{name}: db')
    w, wdw = real_filter(('conv1_1 under conv1_2', b, h, wi, 3, 64, 3))
    dw, db = run_dgrad_first_wgrad(np.zeros_like(o.dy), o.w, o.mask, image, w, WD_REAL, b, h, wi)
    same(dw, wdw, f'{name}: dy = 0, dw must be wd * w')
    same(db, np.zeros(64), f'{name}: dy = 0, db must be 0')
    dw, db = run_dgrad_first_wgrad(o.dy, o.w, o.mask, np.zeros_like(image), w, WD_REAL, b, h, wi)
    same(dw, wdw, f'{name}: image = 0, dw must be wd * w')
    same(db, db1, f'{name}: image = 0, db')
    dw, db = run_dgrad_first_wgrad(o.dy, o.w, o.mask, image, w, 0.0, b, h, wi)
    same(dw, dw1 - cx.WD * w1, f'{name}: wd = 0 with a non-null w')
    same(db, db1, f'{name}: wd = 0, db')
    print('c64 child ok')


def test_dgrad_first_wgrad_in_c64_child():
    """ssd_op_conv2d_dgrad_first_wgrad_bf16 runs the persistent 64 -> 64 kernel, which small layers take only under SSD_C64_BF16=2
    (read once per process): a child process"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f'import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_conv_exact as t; t.c64_child()'
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, SSD_C64_BF16='2'), cwd=os.path.dirname(here),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'c64 child ok' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the weight decay, visible ---------------------------------------------------------------------------------------------------------

def real_filter(case):
    name, b, hi, wi, ci, co, k = case[:7]
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    w = (rng.normal(0, 1, (k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
    return w, (np.float32(WD_REAL) * w).astype(np.float32)          # the one fp32 product


def check_weight_decay(name, o, w, wdw, call):
    """call(x, dy, w, wd) -> (dw, db) of one entry point on float64 / float32 host arrays"""
    zx, zdy = np.zeros_like(o.x), np.zeros_like(o.dy)
    dw, db = call(o.x, zdy, w, WD_REAL)
    same(dw, wdw, f'{name}: dy = 0, dw must be wd * w')
    same(db, np.zeros(o.g.co), f'{name}: dy = 0, db must be 0')
    dw, db = call(zx, o.dy, w, WD_REAL)
    same(dw, wdw, f'{name}: x = 0, dw must be wd * w')
    same(db, o.db, f'{name}: x = 0, db')
    dw, db = call(o.x, o.dy, w, 0.0)
    same(dw, o.dw - o.wd * o.w, f'{name}: wd = 0 with a non-null w')
    same(db, o.db, f'{name}: wd = 0, db')


@pytest.mark.parametrize('case', FP32_CASES, ids=ids(FP32_CASES))
def test_weight_decay_fp32(case):
    o = operands(case)
    w, wdw = real_filter(case)

    def call(x, dy, w, wd):
        return run_fp32(x, w, o.bias, dy, None, None, wd, o.g.abi(), False, False)[1:3]
    check_weight_decay(case[0], o, w, wdw, call)


def wgrad_bf16_call(g, direct):
    geom = g.abi()

    def call(x, dy, w, wd):
        x_, dy_, w_ = bdev(f32(x)), bdev(f32(dy)), dev(f32(w))
        gw_, gb_ = full(w.shape, 7.0), full((g.co,), 7.0)
        if direct:
            check(lib.ssd_op_conv2d_wgrad_bf16_direct(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_), wd, *geom, None))
        else:
            ws_ = wgrad_ws(lib.ssd_op_conv2d_wgrad_bf16_ws_floats, geom)
            check(lib.ssd_op_conv2d_wgrad_bf16(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_), wd, ptr(ws_), *geom, None))
        return host(gw_), host(gb_)
    return call


# (the weight gradient has no fp32-out form: a shape that is listed with both kinds of output runs once)
WD_BF16_CASES = [c for i, c in enumerate(BF16_CASES) if c[1:11] not in [d[1:11] for d in BF16_CASES[:i]]]


@pytest.mark.parametrize('case', WD_BF16_CASES, ids=ids(WD_BF16_CASES))
def test_weight_decay_bf16(case):
    o = operands(case)
    check_weight_decay(case[0], o, *real_filter(case), wgrad_bf16_call(o.g, False))


@pytest.mark.parametrize('case', CHAIN_CASES, ids=ids(CHAIN_CASES))
def test_weight_decay_bf16_direct(case):
    o = operands(case)
    check_weight_decay(case[0], o, *real_filter(case), wgrad_bf16_call(o.g, True))


@pytest.mark.parametrize('case', FIRST_CASES, ids=ids(FIRST_CASES))
def test_weight_decay_first_layer_bf16(case):
    o = operands(case)
    geom = o.g.abi()

    def call(x, dy, w, wd):
        x_, dy_, w_ = dev(f32(x)), bdev(f32(dy)), dev(f32(w))
        ws_ = wgrad_ws(lib.ssd_op_conv2d_first_wgrad_bf16_ws_floats, geom)
        gw_, gb_ = full(w.shape, 7.0), full((o.g.co,), 7.0)
        check(lib.ssd_op_conv2d_first_wgrad_bf16(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_), wd, ptr(ws_), *geom, None))
        return host(gw_), host(gb_)
    check_weight_decay(case[0], o, *real_filter(case), call)


@pytest.mark.parametrize('hw', [160, 512], ids=['160x160: 17 / 25 splits', '512x512: 171 / 256 splits'])
def test_weight_decay_first_layer_many_slabs(hw):
    """The split slabs of conv1_1's weight gradient are reduced by one of three kernels, by their number (csrc/conv_igemm.hip
    wgrad_reduce: below 32, below 256, and more); the last two are met at image sizes whose exact sums no longer fit 2^24 LSB.  The
    weight decay needs no sum: dy = 0 (x = 0) leaves wd * w; with x = 0 the bias gradient is the exact column sum of dy."""
    g = cx.Geom(1, hw, hw, 3, 64, 3, 1, 1, 'SAME')
    geom = g.abi()
    image = cx.pattern((1, hw, hw, 3), None, 0, 0, 0, image=True)
    dy = cx.pattern((1, hw, hw, 64), (3, 5, 2, 1), -4, 9, 1)
    db_want = dy.sum((0, 1, 2))
    assert np.abs(dy).sum((0, 1, 2)).max() < 2 ** 24 and cx.distinct_enough(db_want)
    w, wdw = real_filter((f'conv1_1 {hw}', 1, hw, hw, 3, 64, 3))
    zero = np.zeros(64)

    def bf16_call(x, dy, w, wd):
        x_, dy_, w_ = dev(f32(x)), bdev(f32(dy)), dev(f32(w))
        ws_ = wgrad_ws(lib.ssd_op_conv2d_first_wgrad_bf16_ws_floats, geom)
        gw_, gb_ = full(w.shape, 7.0), full((64,), 7.0)
        check(lib.ssd_op_conv2d_first_wgrad_bf16(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_), wd, ptr(ws_), *geom, None))
        return host(gw_), host(gb_)

    def fp32_call(x, dy, w, wd):
        return run_fp32(x, w, zero, dy, None, None, wd, geom, False, False)[1:3]

    for name, call in (('ssd_op_conv2d_first_wgrad_bf16', bf16_call), ('ssd_op_conv2d_wgrad, ci = 3', fp32_call)):
        dw, db = call(image, np.zeros_like(dy), w, WD_REAL)
        same(dw, wdw, f'{name} {hw}x{hw}: dy = 0, dw must be wd * w')
        same(db, zero, f'{name} {hw}x{hw}: dy = 0, db must be 0')
        dw, db = call(np.zeros_like(image), dy, w, WD_REAL)
        same(dw, wdw, f'{name} {hw}x{hw}: x = 0, dw must be wd * w')
        same(db, db_want, f'{name} {hw}x{hw}: x = 0, db')


# ---- fp32 direct kernels on real-valued data: a bound per element ----------------------------------------------------------------------

BOUND_CASES = [c for c in tk.CONV_CASES if c[0] in ('conv4-like 256->512', 'mod_conv6 dil6', 'conv8_2 s2 19->10', 'conv8_1 1x1 ->256',
                                                    'head 6 types N=152')]


def within(name, what, got, ref, absacc, K):
    bound = m6.accumulation_bound(absacc, K)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err[bound > 0] / bound[bound > 0]).max())
    print(f'\n[conv exact] {name}: {what}: largest error / bound = {worst:.5f} (K = {K})')
    assert np.all(err <= bound), f'{name}: {what}: {int((err > bound).sum())} values beyond K * 2^-23 * sum|x * w|; first {np.argwhere(err > bound)[:4].tolist()}'


@pytest.mark.parametrize('case', BOUND_CASES, ids=ids(BOUND_CASES))
def test_fp32_per_element_bound(case):
    """the Gaussian inputs of test_gpu_kernels.test_conv_fwd_dgrad_wgrad (same generator, same order), float64 reference"""
    name, b, hi, wi, ci, co, k, stride, dil, padding, relu = case
    assert len(BOUND_CASES) == 5
    g = cx.Geom(b, hi, wi, ci, co, k, stride, dil, padding)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.normal(0, 1, (b, hi, wi, ci)).astype(np.float32)
    w = (rng.normal(0, 1, (k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.normal(0, 0.1, (co,)).astype(np.float32)
    if co == 152:
        w[..., 150:] = 0; bias[150:] = 0
    dy = rng.normal(0, 1, (b, g.ho, g.wo, co)).astype(np.float32)
    prev = rng.normal(0, 1, x.shape).astype(np.float32)
    y, dw, db, dx, dxm = run_fp32(x, w, bias, dy, prev, x, WD_REAL, g.abi(), relu, True)
    y_ref, ay = cx.forward(x, w, bias, relu, g)
    within(name, 'forward', y, y_ref, ay + np.abs(bias), k * k * ci)
    dx_ref, adx = cx.dgrad(dy, w, g)
    within(name, 'data gradient', dx, dx_ref, adx, k * k * co)
    within(name, 'data gradient, accumulate + mask', dxm, (dx_ref + prev) * (x > 0), adx + np.abs(prev), k * k * co)
    dw_ref, db_ref, adw, adb = cx.wgrad(x, dy, w, np.float64(np.float32(WD_REAL)), g)
    within(name, 'weight gradient', dw, dw_ref, adw + np.abs(WD_REAL * w), b * g.ho * g.wo)
    within(name, 'bias gradient', db, db_ref, adb, b * g.ho * g.wo)


# ---- forced variants: the same tests in child processes --------------------------------------------------------------------------------

FP32_TESTS = 'test_fp32_exact or test_weight_decay_fp32 or test_weight_decay_first_layer_many_slabs or test_fp32_per_element_bound'
BF16_TESTS = 'test_bf16_exact or test_bf16_chain_exact or test_weight_decay_bf16 or test_dgrad_first_wgrad_in_c64_child'
FIRST_TESTS = 'test_first_layer_bf16_exact or test_weight_decay_first_layer'
BF16_FORCED = [dict(SSD_GATHER_ROWS256_BF16='2', SSD_C64_BF16='2'), dict(SSD_GATHER_ROWS_N64_BF16='2'),
               dict(SSD_GATHER_ROWS_N64_BF16='0', SSD_SMALL_TILE='0'), dict(SSD_SMALL_KSPLIT='0')]      # test_gpu_bf16's four
VARIANTS = ([(v, FP32_TESTS) for v in tk.FP32_VARIANTS]
            + [(v, BF16_TESTS) for v in BF16_FORCED]
            + [(dict(SSD_FIRST_ROWS_BF16='0'), FIRST_TESTS), (dict(SSD_FIRST_GRID='16'), FIRST_TESTS)])


@pytest.mark.parametrize('variant,tests', VARIANTS, ids=[' '.join(f'{k[4:]}={v}' for k, v in d.items()) for d, _ in VARIANTS])
def test_exact_under_forced_variants(variant, tests):
    """one child after another, each under its own time limit; nothing is retried"""
    env = dict(os.environ, **variant)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-x', '-q', '-k', tests, '-p', 'no:cacheprovider'],
                       env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and ' failed' not in r.stdout, r.stdout[-1000:]
