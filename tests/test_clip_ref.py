"""CPU: the float64 oracle of tests/clip_ref.py is itself checked -- f = 1 at and below the threshold, the clipped gradient's norm equals
max_norm to fp64 rounding, zeros give norm 0 and f = 1, a non-finite gradient skips -- and the operands of the GPU test's cases are
shown to tell: each seeded mistake (a deliberately wrong restatement of the contract) moves the norm, the factor, w or acc of those
very operands by far more than the GPU test allows (1 ulp on norm and factor, the bit on w and acc)."""
import numpy as np
import pytest

import clip_ref as cr

QUICK = [c for c in cr.CASES if c[0] <= 2 ** 20 + 4]          # (the CPU suite stays quick)
# A mistake must move a reported value by at least this many fp32 ulps, 16 times what the GPU test allows.  One heavy group is about
# 110 / n of the norm (4 values of ~1.5 * 2^20 against n values whose squares average 0.042 * 2^40): 40 ulps at the largest size, 29 M.
FAR_ULPS = 16


def test_factor_is_one_at_and_below_the_threshold():
    for n in (4, 252, 1028):
        g = cr.operands(n)[2]
        for s in (1.0, 0.25, -0.5):
            nv = cr.norm(g, s)
            at = np.float32(nv)
            if float(at) >= nv:       # the two float32 thresholds around the fp64 norm
                up, below = at, np.nextafter(at, np.float32(0))
            else:
                up, below = np.nextafter(at, np.float32(np.inf)), at
            assert float(below) <= nv <= float(up)
            assert cr.factor(g, s, up) == 1.0
            assert cr.factor(g, s, 2 * nv) == 1.0 and cr.factor(g, s, np.inf) == 1.0
            if float(below) < nv:
                assert 0.0 < cr.factor(g, s, below) <= 1.0 and cr.factor(g, s, below) == np.float32(float(below) / nv)
            assert cr.factor(g, s, 0.5 * nv) == np.float32(float(np.float32(0.5 * nv)) / nv)


def test_clipped_gradient_has_the_threshold_norm():
    for n in (8, 1020, 2 ** 20 + 4):
        g = cr.operands(n)[2]
        for s, rel in ((1.0, 0.5), (0.25, 0.01), (-0.5, 0.9)):
            nv = cr.norm(g, s)
            m = rel * nv
            f64 = m / nv                                   # the factor before its one rounding to float
            assert abs(cr.norm(g.astype(np.float64) * f64, s) - m) <= 8 * np.finfo(np.float64).eps * m
            f = cr.factor(g, s, np.float32(m))
            assert abs(cr.norm(g.astype(np.float64) * float(f), s) - float(np.float32(m))) <= 2.0 ** -23 * m   # ... and after it: half an ulp


def test_zeros_and_non_finite():
    z = np.zeros(64, np.float32)
    for m in (1.0, 1e-30, np.inf):
        assert cr.norm(z, 0.5) == 0.0 and cr.factor(z, 0.5, m) == 1.0 and not cr.skipped(z)
    w, acc, g = cr.operands(252)
    w2, a2, n32, f = cr.update(w, acc, np.zeros(252, np.float32), 0.5, 1.0)
    assert f == 1.0 and n32 == 0.0 and np.array_equal(a2, cr.MOMENTUM * acc) and np.array_equal(w2, w - cr.LR * a2)
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 126, 251):
            gb = g.copy(); gb[at] = bad
            assert cr.skipped(gb) and cr.factor(gb, 1.0, np.inf) == 0.0 and not np.isfinite(cr.norm(gb, 1.0))
            w2, a2, n32, f = cr.update(w, acc, gb, 1.0, 5.0)
            assert f == 0.0 and not np.isfinite(n32) and w2.tobytes() == w.tobytes() and a2.tobytes() == acc.tobytes()


def test_operands_are_what_the_cases_promise():
    for n in [n for n in cr.SIZES if n <= cr.GRID_FLOATS + 4] + [max(cr.SIZES)]:      # (one generator: the sizes between add seconds, no path)
        w, acc, g = cr.operands(n)
        assert g.size == n and n % 4 == 0
        assert np.all(g != 0) and np.all(w != 0) and np.all(acc != 0) and np.all(np.isfinite(g))
        assert (g > 0).any() and (g < 0).any()
        a = np.abs(g)
        assert a.min() >= 2.0 ** -20 and a.max() < 2.0 ** 21
        if n >= 252:
            assert a.min() < 2.0 ** -14 and a.max() > 2.0 ** 19          # spread over the range
    # a float32 running sum of the squares would not pass: it is off by many ulps of the norm
    g = cr.operands(2 ** 20 + 4)[2]
    run = np.cumsum(np.square(g), dtype=np.float32)[-1]
    assert cr.ulps(np.sqrt(np.float32(run)), np.float32(cr.norm(g, 1.0))) > 4


@pytest.mark.parametrize('case', cr.CASES, ids=cr.CASE_IDS)
def test_a_group_lost_or_counted_twice_shows(case):
    """at every size of the GPU test, for every heavy group: the first, middle and last one and thread 0's group of every pass"""
    n, s, rel = case
    g = cr.operands(n)[2]
    S = cr.sum_squares(g)
    want = np.float32(cr.norm(g, s))
    m = cr.max_norm_of(n, s, min(rel, 0.5))
    f_want = np.float32(float(m) / cr.norm(g, s))
    for grp in cr.heavy_groups(n):
        part = cr.sum_squares(g[4 * grp:4 * grp + 4])
        lost, twice = abs(np.float32(s)) * np.sqrt(S - part), abs(np.float32(s)) * np.sqrt(S + part)
        assert cr.ulps(np.float32(lost), want) >= FAR_ULPS, ('lost', grp)
        assert cr.ulps(np.float32(twice), want) >= FAR_ULPS, ('twice', grp)
        assert cr.ulps(np.float32(float(m) / twice), f_want) >= FAR_ULPS          # ... and so moves the factor of a clipped case


def test_the_sizes_reach_both_loops_of_the_norm_kernel():
    """thread 0 of block 0, walked as the kernel walks: which sizes enter the main loop, how often, and what is left to the one-pass loop"""
    def trips(n):
        n4, stride = n // 4, min(-(-(n // 4) // cr.GROUPS_PER_BLOCK), cr.GRID_CAP) * cr.GROUPS_PER_BLOCK
        i = main = 0
        while i + (cr.UNROLL - 1) * stride < n4:
            main, i = main + 1, i + cr.UNROLL * stride
        tail = len(range(i, n4, stride))
        return main, tail
    G, U = cr.GRID_FLOATS, cr.UNROLL
    assert trips(cr.MAIN_FLOATS - 4) == (0, U - 1) and trips(cr.MAIN_FLOATS) == (0, U - 1)
    assert trips(cr.MAIN_FLOATS + 4) == (1, 0) and trips(U * G + 4) == (1, 1) and trips((2 * U - 1) * G + 4) == (2, 0)
    assert all(trips(n)[0] == 0 for n in cr.SIZES if n <= cr.MAIN_FLOATS)
    for n in (cr.MAIN_FLOATS - 4, cr.MAIN_FLOATS, cr.MAIN_FLOATS + 4, U * G + 4, (2 * U - 1) * G + 4):
        assert n in cr.SIZES
    # thread 0's loads of the main loop are heavy groups: a v[u] taken from the wrong pass shows
    heavy = cr.heavy_groups(cr.MAIN_FLOATS + 4)
    assert all(k * cr.GRID_CAP * cr.GROUPS_PER_BLOCK in heavy for k in range(U))


SCALED = [c for c in QUICK if c[1] != 1.0]          # (grad_scale 1 cannot tell; the test below shows every size has another setting)


@pytest.mark.parametrize('case', SCALED, ids=['n%d-s%g-x%g' % c for c in SCALED])
def test_norm_before_grad_scale_shows(case):
    n, s, rel = case
    g = cr.operands(n)[2]
    wrong = np.float32(cr.norm(g, 1.0))             # the norm of g, not of s * g
    assert cr.ulps(wrong, np.float32(cr.norm(g, s))) >= FAR_ULPS
    if np.isfinite(rel):
        m = cr.max_norm_of(n, s, rel)
        assert cr.ulps(cr.factor(g, 1.0, m), cr.factor(g, s, m)) >= FAR_ULPS


def test_every_size_has_a_setting_with_a_grad_scale_other_than_one():
    for n in cr.SIZES:
        assert any(c[0] == n and c[1] != 1.0 and c[2] < 1.0 for c in cr.CASES)


@pytest.mark.parametrize('n', [n for n in cr.SIZES if n <= 2 ** 20 + 4])
def test_factor_on_the_learning_rate_shows(n):
    """w -= (lr * f) * (m * acc + s * g) scales the old momentum too and leaves acc unclipped: needs acc != 0 and f < 1"""
    w, acc, g = cr.operands(n)
    s, rel = cr.SETTINGS[0]
    m = cr.max_norm_of(n, s, rel)
    w2, a2, _, f = cr.update(w, acc, g, s, m)
    assert 0.0 < f < 1.0
    a_wrong = cr.MOMENTUM * acc + np.float32(s) * g
    w_wrong = w - (cr.LR * f) * a_wrong
    assert np.abs(a_wrong - a2).max() > 1e-3 * np.abs(a2).max()
    assert np.abs((w_wrong - w2).astype(np.float64)).max() > 1e-4          # the m * acc * lr * (1 - f) term: ~ 0.9 * 1e-3 * 0.5 * |acc|


def test_a_skipped_step_that_decays_the_momentum_shows():
    w, acc, g = cr.operands(1028)
    gb = g.copy(); gb[5] = np.nan
    w2, a2, _, f = cr.update(w, acc, gb, 1.0, 1.0)
    assert f == 0.0 and a2.tobytes() == acc.tobytes() and w2.tobytes() == w.tobytes()
    decayed = cr.MOMENTUM * acc                     # gscale' = 0 through the plain expression: acc = m * acc, w -= lr * acc
    assert np.all(decayed != acc) and np.all(w - cr.LR * decayed != w)
