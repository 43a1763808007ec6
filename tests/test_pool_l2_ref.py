"""CPU: tests/pool_l2_ref.py is right (it agrees with the oracle and with torch autograd where those are defined: without ties),
its pooling operands can tell a right kernel from a wrong one (every mutant reference changes the expectation of every case it
can touch), and its L2-norm bounds hold for an fp32 emulation of the kernels' summation order."""
import functools

import numpy as np
import pytest
import torch

from oracle import ssdvgg_ref as ref
import pool_l2_ref as pr

ALL_CASES = pr.POOL2_CASES + pr.POOL3_CASES + pr.FALLBACK_CASES
BIG = 4_000_000      # elements: the one case above it is sampled by a band of rows (nine references of the whole tensor take a minute)


@functools.lru_cache(maxsize=None)
def operands(case):
    return pr.operands(case)


@functools.lru_cache(maxsize=None)
def expectation(case):
    return pr.expectation(operands(case))


# ---- the reference agrees with the oracle ------------------------------------------------------------------------------------------

TIE_FREE = [pr.same_case(2, 9, 7, 8, 2, 2), pr.same_case(2, 6, 5, 4, 3, 1), pr.same_case(1, 10, 7, 8, 3, 2), pr.same_case(1, 6, 5, 8, 2, 1),
            pr.same_case(1, 11, 9, 4, 5, 3)]


@pytest.mark.parametrize('case', TIE_FREE, ids=pr.case_id)
def test_maxpool_matches_oracle_and_autograd(case):
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = case
    rng = np.random.default_rng(5)
    x = rng.permutation(b * hi * wi * c).reshape(b, hi, wi, c) / 8.0 - 40.0        # all distinct: no ties, both signs
    dy = rng.integers(-12, 13, (b, ho, wo, c)).astype(np.float64)
    y, tap, dx = pr.maxpool(x, k, stride, pad_h, pad_w, ho, wo, dy)
    xt = torch.tensor(x).permute(0, 3, 1, 2).requires_grad_(True)
    yt = ref.maxpool_tf(xt, k, stride)
    yt.backward(torch.tensor(dy).permute(0, 3, 1, 2))
    assert np.array_equal(y, yt.detach().permute(0, 2, 3, 1).numpy())
    assert np.array_equal(dx, xt.grad.permute(0, 2, 3, 1).numpy())
    prev = rng.integers(-12, 13, x.shape).astype(np.float64)
    assert np.array_equal(pr.maxpool(x, k, stride, pad_h, pad_w, ho, wo, dy, prev, True, True)[2], (dx + prev) * (x > 0))
    # the tap is the cell the maximum came from
    for idx in [(0, 0, 0, 0), (b - 1, ho - 1, wo - 1, c - 1), (0, ho // 2, wo // 2, 1)]:
        n, oh, ow, ch = idx
        kh, kw = divmod(int(tap[idx]), k)
        assert x[n, oh * stride - pad_h + kh, ow * stride - pad_w + kw, ch] == y[idx]


def test_explicit_leading_padding():
    """2x2 stride 2 with one cell of padding in front: windows of 1, 2 and 4 cells, by hand"""
    x = np.arange(1, 10, dtype=np.float64).reshape(1, 3, 3, 1)
    y, tap, dx = pr.maxpool(x, 2, 2, 1, 1, 2, 2, np.array([1.0, 2, 3, 4]).reshape(1, 2, 2, 1))
    assert np.array_equal(y[0, :, :, 0], [[1, 3], [7, 9]]) and np.array_equal(tap[0, :, :, 0], [[3, 3], [3, 3]])
    assert np.array_equal(dx[0, :, :, 0], [[1, 0, 2], [0, 0, 0], [3, 0, 4]])


def test_first_maximum_and_records_by_hand():
    x = np.zeros((1, 2, 2, 4))
    x[0, :, :, 0] = [[0.5, 0.5], [0.5, 0.25]]        # tie of three: cell 0
    x[0, :, :, 1] = [[-1, 0.0], [-0.0, -2]]          # zeros of both signs tie: cell 1, not positive
    x[0, :, :, 2] = [[-3, -1], [-1, -2]]             # negative tie: cell 1
    x[0, :, :, 3] = [[0.125, 0.25], [0.75, 0.75]]    # tie in the last row: cell 2
    rec = pr.record_2x2(x)
    assert rec.shape == (1, 1, 1, 1) and rec.dtype == np.uint16
    assert int(rec[0, 0, 0, 0]) == (0 | 4) | (1 << 3) | (1 << 6) | ((2 | 4) << 9)
    dy = np.array([5.0, 6, 7, 8]).reshape(1, 1, 1, 4)
    dx = pr.rec_bwd(rec, dy, True, 2, 2)
    assert dx[0, 0, 0, 0] == 5 and dx[0, 1, 0, 3] == 8 and dx.sum() == 13
    assert np.array_equal(dx, pr.maxpool(x, 2, 2, 0, 0, 1, 1, dy, None, False, True)[2])
    assert pr.rec_bwd(rec, dy, False, 2, 2).sum() == 26
    arg = pr.arg_3x3(x)                               # 3x3 SAME on 2x2: window (0, 0) sees taps 4, 5, 7, 8
    assert arg.dtype == np.uint32 and int(arg[0, 0, 0, 0]) == 4 | (5 << 8) | (5 << 16) | (7 << 24)
    assert int(arg[0, 1, 1, 0]) == 0 | (1 << 8) | (1 << 16) | (3 << 24)


@pytest.mark.parametrize('npix,C', [(5, 8), (6, 260), (4, 1000)])
def test_l2norm_matches_oracle_and_autograd(npix, C):
    rng = np.random.default_rng(7)
    x, scale, dy = rng.normal(0, 1, (npix, C)), 20 + rng.normal(0, 1, C), rng.normal(0, 1, (npix, C))
    x[1] = 0
    r = pr.l2norm(x, scale, dy, eps=1e-12)
    xt = torch.tensor(x).t().reshape(1, C, npix, 1).contiguous().requires_grad_(True)
    st = torch.tensor(scale).requires_grad_(True)
    yt = ref.l2norm_tf(xt, st)
    yt.backward(torch.tensor(dy).t().reshape(1, C, npix, 1))
    for got, want in ((r['y'], yt.detach().reshape(C, npix).t().numpy()), (r['dx'], xt.grad.reshape(C, npix).t().numpy()),
                      (r['dscale'], st.grad.numpy())):
        assert np.abs(got - want).max() <= 64 * 2.0 ** -53 * np.abs(want).max()
    assert np.allclose(r['dx'][1], scale * dy[1] / np.sqrt(1e-12), rtol=1e-15, atol=0)


# ---- the operands can tell right from wrong ------------------------------------------------------------------------------------------

def cannot_show(case, mutant, name):
    """where a mutant has nothing to change, by construction of the case"""
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = case
    if hi * wi == 1 and mutant in ('last_max', 'swap_khkw'):
        return True                                  # one cell per window: no order among cells, and its tap is on the diagonal
    if min(hi, wi) == 1 and mutant == 'swap_khkw' and name.startswith('dx'):
        return True                                  # a window of one row or one column is scanned in the same order either way
    if hi * wi == 1 and mutant == 'reverse_fields' and name in ('arg', 'rec dx mask=0'):
        return True                                  # the four fields name the same cell (the 2x2 record's sign bits differ)
    return False


def sample(case):
    """the case itself, or for the one large case its first 5 rows as an image of their own (windows are local)"""
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = case
    if b * hi * wi * c <= BIG:
        return operands(case), expectation(case)
    assert (k, stride) == (3, 1)
    o = pr.Operands()
    o.case, o.dtype = pr.same_case(b, 5, wi, c, k, stride), 'fp32'
    full = operands(case)
    o.x, o.dy, o.prev = full.x[:, :5], full.dy[:, :5], full.prev[:, :5]
    return o, pr.expectation(o)


# which outputs a mutant has to change
TOUCHES = {
    'last_max': ('dx acc=0 mask=0', 'dx acc=1 mask=1', 'rec', 'arg'),
    'mask_ge': ('dx acc=0 mask=1', 'dx acc=1 mask=1'),
    'drop_accumulate': ('dx acc=1 mask=0', 'dx acc=1 mask=1'),
    'mask_before_accumulate': ('dx acc=1 mask=1',),
    'pad_shift': ('dx acc=0 mask=0', 'rec', 'arg'),
    'swap_khkw': ('dx acc=0 mask=0', 'rec', 'arg'),
    'reverse_fields': ('rec', 'arg', 'rec dx mask=0', 'rec dx mask=1'),
    'positive_ge': ('rec',),
}


@pytest.mark.parametrize('case', ALL_CASES, ids=pr.case_id)
def test_mutants_change_the_expectation(case):
    o, good = sample(case)
    assert set(TOUCHES) == set(pr.MUTANTS)
    for mutant in pr.MUTANTS:
        bad = pr.expectation(o, mutant)
        assert bad.keys() == good.keys()
        for name in TOUCHES[mutant]:
            if name not in good or cannot_show(case, mutant, name):
                continue
            if mutant == 'pad_shift' and name.startswith('dx') and o.case[1] * o.case[2] == 1:
                continue                             # one cell: every window still holds it (the records show the shift)
            assert not np.array_equal(good[name], bad[name]), f'{pr.case_id(case)}: {mutant} leaves {name} unchanged'


@pytest.mark.parametrize('case', ALL_CASES, ids=pr.case_id)
def test_operands_are_exact_and_varied(case):
    o, e = sample(case)
    b, hi, wi, c, k, stride, pad_h, pad_w, ho, wo = o.case
    assert np.array_equal(pr.bf16_round(o.x), o.x) and np.array_equal(pr.bf16_round(o.dy), o.dy) and np.array_equal(pr.bf16_round(o.prev), o.prev)
    for name, v in e.items():
        if v.dtype == np.float64:
            assert np.array_equal(pr.bf16_round(v), v), f'{name}: not a bf16 value'
            assert np.abs(v).max() < 256
    neg_zero = (o.x == 0) & np.signbit(o.x)
    if o.x.size >= 64:
        assert neg_zero.any() and ((o.x == 0) & ~np.signbit(o.x)).any() and (o.x < 0).any() and len(np.unique(o.x[o.x > 0])) == 6
    tied, none, unique = pr.window_kinds(o)
    print(f'\n[pool operands] {pr.case_id(case)}: {b * ho * wo} windows; tied positive maximum {tied:.3f}, no positive cell {none:.3f}, '
          f'unique positive maximum {unique:.3f}')
    if b * ho * wo >= 16:
        assert tied >= 0.10 and none >= 0.05 and unique >= 0.20
    if 'rec' in e:
        assert e['rec'].dtype == np.uint16 and (e['rec'] >> 12 == 0).all()
        assert np.array_equal(e['rec dx mask=1'], e['dx acc=0 mask=1'])       # the record's sign bit is the relu mask of the maximum


def test_large_case_crosses_the_grid_cap():
    b, hi, wi, c = pr.POOL3_CASES[-1][:4]
    assert b * hi * wi * (c // 4) == 2_130_048 > 256 * 32 * 256 == 2_097_152


# ---- the L2 bounds hold for an fp32 emulation of the kernels' order --------------------------------------------------------------------

def test_bound_constants():
    assert [pr.chunks(c) for c in (4, 256, 260, 512, 516, 1024)] == [1, 1, 2, 2, 4, 4]
    assert pr.k_fwd(4) == 16 < 64 and pr.k_bwd(4) == 70
    assert {pr.chunks(c) for _, c in pr.L2_CASES} == {1, 2, 4}
    # 2888 pixels, 512 workgroups: a wave has 4 pixels at most, a row group of the column sums 32 rows in four running sums
    assert pr.chain_length(2888, 2) == 4 + 2 + 8 + 2 + 16 and pr.chain_length(1, 1) == 1 + 2 + 1 + 2 + 16


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('npix,C', pr.L2_CASES)
def test_l2_emulation_within_bounds(npix, C, bf16):
    x, scale, dy, special = pr.l2_operands(npix, C, bf16)
    assert (x < 0).any() or npix <= 3
    r = pr.l2norm(x, scale, dy)
    if 'zero' in special:
        assert not x[special['zero']].any() and not r['y'][special['zero']].any()
    p = special['below']
    assert np.count_nonzero(x[p]) == 1 and 0 < (x[p].astype(np.float64) ** 2).sum() < pr.EPS
    assert np.allclose(r['y'][p], scale.astype(np.float64) * x[p] * 1e6, rtol=1e-8, atol=0)
    assert np.allclose(r['dx'][p], scale.astype(np.float64) * dy[p] * 1e6, rtol=1e-8, atol=0)
    if 'above' in special:
        assert (x[special['above']].astype(np.float64) ** 2).sum() > pr.EPS
    y, dx, ds = pr.l2norm_f32_emulation(x, scale, dy)
    if bf16:
        y, dx = pr.bf16_round(y), pr.bf16_round(dx)
    by, bdx, bds = pr.l2_bounds(r, npix, C, bf16)
    for name, got, want, bound in (('y', y, r['y'], by), ('dx', dx, r['dx'], bdx), ('dscale', ds, r['dscale'], bds)):
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), f'{name}: {int((err > bound).sum())} beyond the bound, worst ratio {(err[bound > 0] / bound[bound > 0]).max()}'
        nz = bound > 0
        print(f'\n[l2 emulation] {npix}x{C} {"bf16" if bf16 else "fp32"} {name}: largest error / bound = {(err[nz] / bound[nz]).max() if nz.any() else 0:.4f}')
