"""-m gpu: every max-pool and L2-norm launch of csrc/ops.hip against tests/pool_l2_ref.py (numpy float64), through the C ABI only,
in fp32 and in bf16 storage.

Pooling, value for value (no tolerance).  pool_l2_ref.operands draws x from bf16 values with exact zeros of both signs, negatives
and positives j / 8 that tie inside most windows, dy and the accumulated tensor from integers of at most 12: every expected value
is an integer below 256, exact in fp32 and a bf16 value.  tests/test_pool_l2_ref.py shows on the CPU that these operands see a
last-instead-of-first maximum, a >= mask, a dropped accumulate, a mask applied before the accumulation, a shifted pad, swapped
kh / kw, reversed record fields and a "positive" bit taken from >= 0.  Every output buffer is prefilled with a sentinel and
carries 64 sentinel elements past its end.

  launch (ops.hip)                                   reached by                                           cases
  maxpool_taps_kernel<T, 2>  (y)                     ssd_op_maxpool_fwd[_bf16], k = 2                     2x2 cases, k2 s1, k2 s2 pad 1
  maxpool_taps_kernel<T, 3>  (y)                     ssd_op_maxpool_fwd[_bf16], k = 3                     3x3 cases, k3 s2
  maxpool_taps_kernel<T, 3>  (y + record)            ssd_op_maxpool_arg_fwd                               3x3 cases
  maxpool_taps_kernel<T, 3>  (record only)           ssd_op_maxpool_bwd[_bf16], 3x3 stride 1              3x3 cases
  maxpool_fwd_kernel<T>                              ssd_op_maxpool_fwd[_bf16], k = 5                     k5 s3
  maxpool2x2_bwd_kernel<float, 4>, <bf16_t, 8 | 4>   ssd_op_maxpool_bwd[_bf16], 2x2 stride 2 unpadded     2x2 cases (C = 12: <bf16_t, 4>)
  maxpool2x2_fwd_rec_kernel / _bwd_rec_kernel, same  ssd_op_maxpool_rec_fwd / _bwd                        2x2 cases
  maxpool_bwd_arg_s1_kernel<T, 3>                    ssd_op_maxpool_bwd[_bf16] and ssd_op_maxpool_arg_bwd 3x3 cases
  maxpool_argmax_kernel + maxpool_bwd_arg_kernel     ssd_op_maxpool_bwd[_bf16], anything else with scratch k3 s2, k2 s1, k5 s3
  maxpool_bwd_kernel<T> (no scratch)                 ssd_op_maxpool_bwd[_bf16], 2x2 stride 2 with padding k2 s2 pad 1
  l2norm_fwd_kernel / l2norm_bwd_kernel<T, 1 | 2 | 4>, colsum_kernel   ssd_op_l2norm_fwd / _bwd[_bf16]    L2_CASES
3x37x38x136 takes the per-row loop of the 2x2 kernels twice (19 windows x 34 or 17 channel groups > 256 threads, the second trip
partial); 1x129x129x512 has 2,130,048 channel quads, past the 2,097,152 threads of the capped grid, so the grid-stride loops of
maxpool_taps_kernel<T, 3> and maxpool_bwd_arg_s1_kernel take a second trip.  The switch to 64-bit indices at 2e9 elements
(maxpool_fwd_t small_idx, maxpool_arg_applicable) is out of reach of a small test and is not exercised.

L2 norm, per element within the bounds derived in pool_l2_ref's docstring from the kernels' operation counts (the norm cannot
be exact: rsqrtf is not correctly rounded): y within (2J + 8) 2^-24 |y|, dx within (10J + 30) 2^-24 (|s g r| + |x| r^3 sum|s g x|),
dscale within (K_chain + 2J + 8) 2^-23 sum|g x r|; bf16 stores add half a bf16 ulp of the reference.  One pixel is all zero, one
holds a single 2^-21 (sum of squares below the clamp with a nonzero x: y = s x 1e6, dx = s dy 1e6), one a single 2^-19.

Measured on an MI355X, largest error / bound over the twelve cases (a ratio above 1 fails; the smallest of the twelve in brackets):
  entry point                    fp32              bf16
  ssd_op_l2norm_fwd[_bf16]  y    0.317  (0.050)    0.9998  (0.649)
  ssd_op_l2norm_bwd[_bf16]  dx   0.072  (0.031)    0.9991  (0.987)
                        dscale   0.033  (0.004)    0.030   (0.0001)
The bf16 ratios are the store's rounding, which comes as close to half an ulp as it likes: one bf16 ulp of error fails.  The fp32
bounds count every rounding at its worst while the roundings met add up like a random walk (the fp32 numpy emulation of the
kernels' order in tests/test_pool_l2_ref.py gives the same ratios: 0.31, 0.08, 0.04), and dscale is bounded against sum |g x r| of
terms of both signs, about sqrt(npix) above the partial sums it stands for: the operation counts leave nothing to tighten, and a
wrong or missing term is an error of order 1 in these units.  No test here found a bug in the kernels.

That these tests can fail was shown with one-line edits of comparisons and masks in ops.hip, one library each (never of an address or
a bound).  "before": the pooling and L2-norm tests there were, run on the same library: test_gpu_kernels.py test_maxpool / test_l2norm
(11 tests), the kernel-level tests of test_gpu_pool_fusion.py (12), test_gpu_bf16.py test_bf16_step_layer_local[vgg300-2].
  edit                                                     caught here by                                before
  > -> >= in the first-maximum test of
    maxpool2x2_bwd_kernel                                  test_pool_2x2_stride2, 10 of 12 (a)           the bf16 step only
    maxpool2x2_fwd_rec_kernel                              test_pool_2x2_stride2, 10 of 12 (a)           pool fusion 9 of 12, the bf16 step
    maxpool_taps_kernel                                    test_pool_3x3_stride1, 10 of 12 (a)           the bf16 step only
    maxpool_argmax_kernel                                  test_pool_fallbacks, 6 of 8 (b)               all passed
    maxpool_bwd_kernel (": v[e] > self[e]")                test_pool_fallbacks, k2 s2 pad 1, both types  all passed
  > 0.f -> >= 0.f in the relu mask of
    maxpool_bwd_kernel                                     test_pool_fallbacks, k2 s2 pad 1, both types  all passed
    maxpool2x2_bwd_kernel                                  test_pool_2x2_stride2, 12 of 12               test_maxpool 3 of 4, the bf16 step
    maxpool2x2_fwd_rec_kernel (the record's "positive")    test_pool_2x2_stride2, 12 of 12               pool fusion 9 of 12, the bf16 step
    maxpool_bwd_arg_kernel                                 test_pool_fallbacks, 6 of 8 (b)               all passed
    maxpool_bwd_arg_s1_kernel                              test_pool_3x3_stride1, 12 of 12               test_maxpool 1 of 4, the bf16 step
  3 * (e & 3) -> 3 * (3 - (e & 3)) in
    maxpool2x2_fwd_rec_kernel                              test_pool_2x2_stride2, 12 of 12               pool fusion 9 of 12, the bf16 step
    maxpool2x2_bwd_rec_kernel                              test_pool_2x2_stride2, 12 of 12               pool fusion 12 of 12, the bf16 step
  accumulate ignored in maxpool2x2_bwd_kernel              test_pool_2x2_stride2, 12 of 12               test_maxpool 3 of 4, the bf16 step
  "ss > 1e-12f ?" dropped in l2norm_bwd_kernel             test_l2norm_within_bounds, 24 of 24           all passed (test_l2norm too)
  (a) all but 1x1x1x4, whose windows hold one cell   (b) all but k2 s2 pad 1, which takes the scratch-free kernel
The early exit of maxpool_bwd_kernel ("every component is masked") with >= is no edit to catch: the mask behind it decides."""
import functools

import numpy as np
import pytest
import torch

import pool_l2_ref as pr
from gpu_util import lib, check, ptr

pytestmark = pytest.mark.gpu

TAIL = 64
SENTINEL = 1000.0            # a bf16 value no expectation reaches (|dx| < 256, |y| < 1)
DTYPES = ['fp32', 'bf16']


# ---- buffers with a guarded tail -----------------------------------------------------------------------------------------------------

def tdtype(dtype):
    return {'fp32': torch.float32, 'bf16': torch.bfloat16, 'u16': torch.int16, 'u32': torch.int32}[dtype]


def fill_of(dtype):
    return -1 if dtype in ('u16', 'u32') else SENTINEL      # all bits set: no record has its top bits set


def out_buf(shape, dtype):
    """an output of `shape`, every element and 64 more behind it set to the sentinel"""
    return torch.full((int(np.prod(shape)) + TAIL,), fill_of(dtype), dtype=tdtype(dtype), device='cuda')


def in_buf(a, dtype):
    """host values -> device (fp32 values that bf16 holds are cast exactly), with the guarded tail: also an accumulated output"""
    t = out_buf(a.shape, dtype)
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).to('cuda').to(tdtype(dtype))
    return t


def take(t, shape, what):
    """the first prod(shape) elements on the host (floats as fp32, records unsigned), after checking the tail"""
    torch.cuda.synchronize()
    n = int(np.prod(shape))
    assert t.numel() == n + TAIL
    h = t.float().cpu().numpy() if t.dtype in (torch.float32, torch.bfloat16) else t.cpu().numpy()
    fill = -1 if t.dtype in (torch.int16, torch.int32) else SENTINEL
    assert (h[n:] == fill).all(), f'{what}: wrote past the end of the buffer: {h[n:].tolist()}'
    if t.dtype == torch.int16:
        h = h.view(np.uint16)
    if t.dtype == torch.int32:
        h = h.view(np.uint32)
    return h[:n].reshape(shape)


def bits(t, shape):
    """the raw words of a float buffer's first prod(shape) elements"""
    torch.cuda.synchronize()
    n = int(np.prod(shape))
    return t[:n].view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def same(got, want, what):
    """value for value (a zero's sign does not matter); the count and the first mismatches on failure"""
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.dtype.kind == 'f':
        assert np.array_equal(pr.bf16_round(want), want), f'{what}: the expectation itself is not a bf16 value'
        got = got.astype(np.float64)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        first = [(tuple(int(j) for j in i), got[tuple(i)].item(), want[tuple(i)].item()) for i in bad[:6]]
        pytest.fail(f'{what}: {len(bad)} of {got.size} values differ; (index, got, want) {first}')


# ---- pooling -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pool_case(case):
    """operands and expectation of a case: computed once per process, shared by both storage types, read-only"""
    o = pr.operands(case)
    e = pr.expectation(o)
    for v in (o.x, o.dy, o.prev, *e.values()):
        v.setflags(write=False)
    return o, e


FLAGS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def pool_fwd(x_, case, dtype):
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = case
    y_ = out_buf((b, ho, wo, c), dtype)
    fn = lib.ssd_op_maxpool_fwd_bf16 if dtype == 'bf16' else lib.ssd_op_maxpool_fwd
    check(fn(ptr(x_), ptr(y_), b, hi, wi, c, ho, wo, k, stride, pad_h, pad_w, None))
    return y_


def pool_bwd(x_, dy_, o, dtype, acc, mask):
    """-> the dx buffer: prefilled with prev when it is accumulated into, with the sentinel otherwise"""
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = o.case
    dx_ = in_buf(o.prev, dtype) if acc else out_buf(o.x.shape, dtype)
    fn = lib.ssd_op_maxpool_bwd_bf16 if dtype == 'bf16' else lib.ssd_op_maxpool_bwd
    check(fn(ptr(x_), ptr(dy_), ptr(dx_), acc, mask, b, hi, wi, c, ho, wo, k, stride, pad_h, pad_w, None))
    return dx_


def check_fwd_bwd(case, dtype):
    """ssd_op_maxpool_fwd / _bwd [_bf16] with the four combinations of accumulate and relu_mask -> (o, e, x_, dy_, {flags: dx_})"""
    o, e = pool_case(case)
    name = f'{pr.case_id(case)} {dtype}'
    x_, dy_ = in_buf(o.x, dtype), in_buf(o.dy, dtype)
    same(take(pool_fwd(x_, case, dtype), e['y'].shape, f'{name}: maxpool_fwd'), e['y'], f'{name}: maxpool_fwd')
    dx = {}
    for acc, mask in FLAGS:
        what = f'{name}: maxpool_bwd accumulate={acc} relu_mask={mask}'
        dx[acc, mask] = pool_bwd(x_, dy_, o, dtype, acc, mask)
        same(take(dx[acc, mask], o.x.shape, what), e[f'dx acc={acc} mask={mask}'], what)
    return o, e, x_, dy_, dx


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', pr.POOL2_CASES, ids=pr.case_id)
def test_pool_2x2_stride2(case, dtype):
    o, e, x_, dy_, dx = check_fwd_bwd(case, dtype)
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = case
    name, bf = f'{pr.case_id(case)} {dtype}', int(dtype == 'bf16')
    y_, rec_ = out_buf((b, ho, wo, c), dtype), out_buf((b, ho, wo, c // 4), 'u16')
    check(lib.ssd_op_maxpool_rec_fwd(ptr(x_), ptr(y_), ptr(rec_), bf, b, hi, wi, c, None))
    same(take(y_, e['y'].shape, f'{name}: rec_fwd y'), e['y'], f'{name}: maxpool_rec_fwd y')
    same(take(rec_, e['rec'].shape, f'{name}: rec_fwd record'), e['rec'], f'{name}: maxpool_rec_fwd record')
    for mask in (0, 1):
        what = f'{name}: maxpool_rec_bwd relu_mask={mask}'
        dx_ = out_buf(o.x.shape, dtype)
        check(lib.ssd_op_maxpool_rec_bwd(ptr(rec_), ptr(dy_), ptr(dx_), mask, bf, b, hi, wi, c, None))
        same(take(dx_, o.x.shape, what), e[f'rec dx mask={mask}'], what)
        if mask:
            assert np.array_equal(bits(dx_, o.x.shape), bits(dx[0, 1], o.x.shape)), \
                f'{name}: maxpool_rec_bwd with the mask and maxpool_bwd (accumulate=0, relu_mask=1) differ in bits'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', pr.POOL3_CASES, ids=pr.case_id)
def test_pool_3x3_stride1(case, dtype):
    o, e, x_, dy_, dx = check_fwd_bwd(case, dtype)
    b, hi, wi, c = case[:4]
    name, bf = f'{pr.case_id(case)} {dtype}', int(dtype == 'bf16')
    y_, arg_ = out_buf(o.x.shape, dtype), out_buf((b, hi, wi, c // 4), 'u32')
    check(lib.ssd_op_maxpool_arg_fwd(ptr(x_), ptr(y_), ptr(arg_), bf, b, hi, wi, c, None))
    same(take(y_, e['y'].shape, f'{name}: arg_fwd y'), e['y'], f'{name}: maxpool_arg_fwd y')
    same(take(arg_, e['arg'].shape, f'{name}: arg_fwd record'), e['arg'], f'{name}: maxpool_arg_fwd record')
    for acc, mask in FLAGS:
        what = f'{name}: maxpool_arg_bwd accumulate={acc} relu_mask={mask}'
        dx_ = in_buf(o.prev, dtype) if acc else out_buf(o.x.shape, dtype)
        check(lib.ssd_op_maxpool_arg_bwd(ptr(x_), ptr(arg_), ptr(dy_), ptr(dx_), acc, mask, bf, b, hi, wi, c, None))
        same(take(dx_, o.x.shape, what), e[f'dx acc={acc} mask={mask}'], what)
        assert np.array_equal(bits(dx_, o.x.shape), bits(dx[acc, mask], o.x.shape)), f'{what}: differs in bits from maxpool_bwd'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', pr.FALLBACK_CASES, ids=pr.case_id)
def test_pool_fallbacks(case, dtype):
    check_fwd_bwd(case, dtype)


def test_pool_refusals():
    """C not a multiple of 4, and the forward-recorded 3x3 pool without its record: an error code and a message, nothing launched"""
    x_, y_ = out_buf((1, 4, 4, 8), 'fp32'), out_buf((1, 4, 4, 8), 'fp32')
    geom2, geom3 = (1, 4, 4, 6, 2, 2, 2, 2, 0, 0), (1, 4, 4, 6, 4, 4, 3, 1, 1, 1)
    calls = []
    for geom in (geom2, geom3):
        calls += [lambda g=geom: lib.ssd_op_maxpool_fwd(ptr(x_), ptr(y_), *g, None),
                  lambda g=geom: lib.ssd_op_maxpool_fwd_bf16(ptr(x_), ptr(y_), *g, None),
                  lambda g=geom: lib.ssd_op_maxpool_bwd(ptr(x_), ptr(x_), ptr(y_), 0, 0, *g, None),
                  lambda g=geom: lib.ssd_op_maxpool_bwd_bf16(ptr(x_), ptr(x_), ptr(y_), 0, 0, *g, None)]
    for bf in (0, 1):
        calls += [lambda bf=bf: lib.ssd_op_maxpool_rec_fwd(ptr(x_), ptr(y_), ptr(y_), bf, 1, 4, 4, 6, None),
                  lambda bf=bf: lib.ssd_op_maxpool_arg_fwd(ptr(x_), ptr(y_), ptr(y_), bf, 1, 4, 4, 6, None),
                  lambda bf=bf: lib.ssd_op_maxpool_arg_bwd(ptr(x_), ptr(y_), ptr(x_), ptr(y_), 0, 0, bf, 1, 4, 4, 6, None),
                  lambda bf=bf: lib.ssd_op_maxpool_arg_fwd(ptr(x_), ptr(y_), None, bf, 1, 4, 4, 8, None),
                  lambda bf=bf: lib.ssd_op_maxpool_arg_bwd(ptr(x_), None, ptr(x_), ptr(y_), 0, 0, bf, 1, 4, 4, 8, None)]
    for i, call in enumerate(calls):
        assert call() != 0, f'call {i} was not refused'
        msg = lib.ssd_last_error().decode()
        assert 'multiple of 4' in msg or 'record' in msg, (i, msg)
    torch.cuda.synchronize()
    assert (x_.cpu().numpy() == SENTINEL).all() and (y_.cpu().numpy() == SENTINEL).all()


# ---- L2 norm -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def l2_case(npix, C, bf16):
    x, scale, dy, special = pr.l2_operands(npix, C, bf16)
    r = pr.l2norm(x, scale, dy)
    return x, scale, dy, special, r, pr.l2_bounds(r, npix, C, bf16)


def ratio(name, what, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    nz = bound > 0
    worst = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    print(f'\n[pool l2 exact] {name}: {what}: largest error / bound = {worst:.4f}')
    assert (err <= bound).all(), (f'{name}: {what}: {int((err > bound).sum())} of {err.size} values beyond the bound, largest error / bound '
                                  f'{worst:.3f}; first (index, got, want, bound) '
                                  f'{[(tuple(map(int, i)), float(got[tuple(i)]), float(want[tuple(i)]), float(bound[tuple(i)])) for i in np.argwhere(err > bound)[:4]]}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('npix,C', pr.L2_CASES)
def test_l2norm_within_bounds(npix, C, dtype):
    bf = dtype == 'bf16'
    x, scale, dy, special, r, (by, bdx, bds) = l2_case(npix, C, bf)
    name = f'l2norm {npix}x{C} {dtype}'
    x_, s_, dy_ = in_buf(x, dtype), in_buf(scale, 'fp32'), in_buf(dy, dtype)
    y_ = out_buf(x.shape, dtype)
    check((lib.ssd_op_l2norm_fwd_bf16 if bf else lib.ssd_op_l2norm_fwd)(ptr(x_), ptr(s_), ptr(y_), npix, C, None))
    y = take(y_, x.shape, f'{name}: y')
    ratio(name, 'forward', y, r['y'], by)
    nws = int(lib.ssd_op_l2norm_bwd_ws_floats(npix, C))
    assert nws == pr.l2_blocks(npix) * C
    dx_, ds_, ws_ = out_buf(x.shape, dtype), out_buf((C,), 'fp32'), out_buf((nws,), 'fp32')
    check((lib.ssd_op_l2norm_bwd_bf16 if bf else lib.ssd_op_l2norm_bwd)(ptr(x_), ptr(s_), ptr(dy_), ptr(dx_), ptr(ds_), ptr(ws_), npix, C, None))
    dx, ds = take(dx_, x.shape, f'{name}: dx'), take(ds_, (C,), f'{name}: dscale')
    take(ws_, (nws,), f'{name}: scratch')
    ratio(name, 'dx', dx, r['dx'], bdx)
    ratio(name, 'dscale', ds, r['dscale'], bds)
    if 'zero' in special:
        p = special['zero']
        assert not y[p].any(), f'{name}: y of the all-zero pixel'
    p, s64 = special['below'], scale.astype(np.float64)       # below the clamp: the norm is the constant 1e-6, k = 0
    lim = (pr.k_fwd(pr.chunks(C)) * pr.U + (2.0 ** -8 if bf else 0) + 3e-9)
    assert (np.abs(y[p] - s64 * x[p] * 1e6) <= lim * np.abs(s64 * x[p] * 1e6)).all(), f'{name}: y below the clamp'
    assert (np.abs(dx[p] - s64 * dy[p] * 1e6) <= lim * np.abs(s64 * dy[p] * 1e6)).all(), f'{name}: dx below the clamp'
