"""-m gpu: the Winograd F(4x4, 3x3) passes (csrc/winograd.hip) against float64 with a bound per element that is MEASURED on the CPU, not
1e-3 of the tensor's maximum.

    rho = max |got - ref64| / (2^-24 * A),  A = ref64's own sum over the operands' magnitudes        (tests/wino_emul.py)

rho_emul comes from the fp32 numpy restatement of the algorithm on the very inputs of this test (sequential fp32 channel and tile sums:
the least favourable order); the kernels must stay within rho_gpu <= 2 * rho_emul, per pass and per case -- the factor 2 for another
association inside the transforms and for split accumulators.  Nothing here is derived from the kernels' own output.  The limit is
also capped at 1e-4 of max |ref|, the level the project already asserts for Winograd against the direct kernels
(test_gpu_model.py): where A is nearly empty -- single taps of the weight gradient of relu-like inputs on small maps -- the measured
limit alone would be no sharper than that.  For the weight gradient a second figure takes A summed over the nine taps, which the
inverse transform G^T dU G mixes ('wgrad, taps pooled').

rho_emul as measured (profiles/wino_error_bound.txt, checked against the restatement by tests/test_wino_emul.py):

    case                                     forward   dgrad   dgrad acc+mask   wgrad      wgrad, taps pooled   bias grad
    tiny 3x2 32->32 b5                       8.81      9.16    5.70             1.88e+09   5.78                 3.97
    exact tiles 8x12 128->96                 13.2      21.4    18.1             1.71e+03   3.72                 0.98
    dil 2 odd 13x9 64->64                    13.3      15.3    13.7             2.45e+06   2.71                 0.976
    mod_conv6 dil 6 19x19 64->96             15.6      20.5    12.8             76.1       1.94                 1.72
    12 output channels 9x9 32->12            5.60      16.6    11.9             29.1       2.19                 0.564
    128 -> 64 channels 21x10                 9.04      12.3    11.5             61.8       2.17                 0.955

Every case runs under both values of SSD_WINO_FUSE_OUT and every SSD_WINO_TILE (0 ... 3) in child processes: the library reads them
once.  The weight decay is made visible as in tests/test_gpu_conv_exact.py: dy = 0 or x = 0 leave exactly wd * w."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wino_emul as we
from gpu_util import lib, check, dev, ptr, host

pytestmark = pytest.mark.gpu
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'wino_error_bound.txt')


def full(shape, v):
    return torch.full(tuple(shape), v, dtype=torch.float32, device='cuda')


def run_wgrad(g, x, dy, w, wd, flags):
    """-> (dw, db); flags 3: the filter transforms and the input's transform are those a forward call on the same x left in ws"""
    geom = g.abi()
    ws_ = torch.zeros((lib.ssd_op_conv2d_wino_ws_floats(*geom),), dtype=torch.float32, device='cuda')
    x_, dy_, w_ = dev(x), dev(dy), dev(w)
    if flags == 3:
        y_ = full((g.b, g.hi, g.wi, g.co), 7.0)
        check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), None, ptr(y_), None, None, None, ptr(ws_), 0, *geom, 1, None))
    gw_, gb_ = full(w.shape, 7.0), full((g.co,), 7.0)
    check(lib.ssd_op_conv2d_wino_wgrad(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_), wd, ptr(ws_), flags, *geom, None))
    return host(gw_), host(gb_)


def run_all(o):
    """-> {pass: tensor} of the Winograd entry points on the inputs o, in the order the step calls them"""
    g = o.g
    geom = g.abi()
    ws_ = torch.empty((lib.ssd_op_conv2d_wino_ws_floats(*geom),), dtype=torch.float32, device='cuda')
    x_, w_, b_, dy_ = dev(o.x), dev(o.w), dev(o.bias), dev(o.dy)
    y_ = full((g.b, g.hi, g.wi, g.co), 7.0)
    check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), ptr(b_), ptr(y_), None, None, None, ptr(ws_), 0, *geom, 1, None))
    gw_, gb_ = full(o.w.shape, 7.0), full((g.co,), 7.0)
    check(lib.ssd_op_conv2d_wino_wgrad(ptr(x_), ptr(dy_), ptr(gw_), ptr(gb_), ptr(w_), we.WD, ptr(ws_), 3, *geom, None))
    gx_ = full(o.x.shape, 3.0)
    check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(gx_), None, None, 0, None, 0, 0, ptr(ws_), 0, *geom, None))
    ga_ = dev(o.prev)
    check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(ga_), ptr(x_), None, 1, None, 0, 0, ptr(ws_), 1, *geom, None))
    return {'forward': host(y_), 'dgrad': host(gx_), 'dgrad accumulate+mask': host(ga_), 'wgrad': host(gw_), 'bias grad': host(gb_)}


@pytest.mark.parametrize('case', we.CASES, ids=[c[0] for c in we.CASES])
def test_winograd_within_twice_the_emulations_error(case):
    o = we.inputs(case)
    emul = we.read_profile(PROFILE)
    got = run_all(o)
    got['wgrad, taps pooled'] = got['wgrad']
    # ... and the weight gradient from scratch (the call transforms x itself): the same bits, so the same figures
    dw0, db0 = run_wgrad(o.g, o.x, o.dy, o.w, we.WD, 0)
    assert np.array_equal(dw0, got['wgrad']) and np.array_equal(db0, got['bias grad'])
    bad = []
    for p in we.PASSES:
        ref, A = o.ref[p]
        r_gpu, r_emul = we.rho(got[p], ref, A), emul[case[0], p]
        limit = np.minimum(2 * r_emul * 2.0 ** -24 * A, 1e-4 * np.abs(ref).max())
        err = np.abs(got[p].astype(np.float64) - ref)
        sharper = 2 * r_emul * 2.0 ** -24 * A.max() < 1e-4 * np.abs(ref).max()
        print(f'\n[wino bound] {case[0]}: {p}: rho_gpu {r_gpu:.4g}  rho_emul {r_emul:.4g}  largest error / max|ref| {err.max() / np.abs(ref).max():.2e}'
              f'{"" if sharper else "  (the measured limit passes 1e-4 of max|ref|: capped there)"}')
        if not (r_gpu <= 2 * r_emul and np.all(err <= limit)):
            bad.append((p, r_gpu, r_emul, int((err > limit).sum())))
    assert not bad, f'{case[0]}: (pass, rho_gpu, rho_emul, elements beyond the limit) {bad}'


@pytest.mark.parametrize('flags', [3, 0])
@pytest.mark.parametrize('case', we.CASES, ids=[c[0] for c in we.CASES])
def test_winograd_weight_decay_is_visible(case, flags):
    """dy = 0 (and x = 0): every transform of zeros is zero, so dw is the one fp32 product wd * w and db (dy = 0) exactly 0; wd = 0: the
    filter must not reach the result at all"""
    o = we.inputs(case)
    wdw = (np.float32(we.WD) * o.w).astype(np.float32)          # one fp32 product
    dw, db = run_wgrad(o.g, o.x, np.zeros_like(o.dy), o.w, we.WD, flags)
    assert np.array_equal(dw, wdw), f'dy = 0: {int((dw != wdw).sum())} values are not wd * w; first {np.argwhere(dw != wdw)[:4].tolist()}'
    assert np.array_equal(db, np.zeros_like(db))
    dw, db = run_wgrad(o.g, np.zeros_like(o.x), o.dy, o.w, we.WD, flags)
    assert np.array_equal(dw, wdw), f'x = 0: {int((dw != wdw).sum())} values are not wd * w; first {np.argwhere(dw != wdw)[:4].tolist()}'
    ref, A = o.ref['bias grad']
    assert we.rho(db, ref, A) <= 2 * we.read_profile(PROFILE)[case[0], 'bias grad']
    dw_a, db_a = run_wgrad(o.g, o.x, o.dy, o.w, 0.0, flags)
    dw_b, db_b = run_wgrad(o.g, o.x, o.dy, np.zeros_like(o.w), 0.0, 0)
    assert np.array_equal(dw_a, dw_b) and np.array_equal(db_a, db_b), 'wd = 0: a non-null w changed the weight gradient'
    with_wd, _ = run_wgrad(o.g, o.x, o.dy, o.w, we.WD, flags)
    want = dw_a + wdw                                            # fp32: the epilogue's one multiply-add, fused or not
    fused = (dw_a.astype(np.float64) + np.float64(np.float32(we.WD)) * o.w.astype(np.float64)).astype(np.float32)
    ok = (with_wd == want) | (with_wd == fused)
    assert ok.all(), f'wd * w is not what the epilogue adds: {int((~ok).sum())} values; first {np.argwhere(~ok)[:4].tolist()}'


SWITCHES = [dict(SSD_WINO_FUSE_OUT=f, **({} if t is None else dict(SSD_WINO_TILE=t))) for f in ('1', '0') for t in (None, '0', '1', '2', '3')][1:]


@pytest.mark.parametrize('switches', SWITCHES, ids=[' '.join(f'{k[9:]}={v}' for k, v in d.items()) for d in SWITCHES])
def test_winograd_bound_under_forced_switches(switches):
    """one child after another, each under its own time limit; nothing is retried"""
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-x', '-q', '-s', '-k',
                        'test_winograd_within_twice or test_winograd_weight_decay', '-p', 'no:cacheprovider'],
                       env=dict(os.environ, **switches), cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and ' failed' not in r.stdout, r.stdout[-1000:]
