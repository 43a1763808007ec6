"""CPU: the AdamW oracle of tests/adamw_ref.py.  Its identities, its agreement with a float64 restatement, and that the operands
of the shared cases TELL: every mistake an implementation of the contract is likely to make, restated here on purpose, changes at
least one element of at least one case -- so a GPU test that compares bits against the oracle on those cases would catch it."""
import math

import numpy as np
import pytest

import adamw_ref as ar

F = np.float32


def test_launcher_constants_and_case_table():
    assert ar.BLOCK == 256 and ar.GRID_CAP == 4096 and ar.G == 4194304
    sizes = {c.n for c in ar.CASES}
    assert sizes == {4, 8, 1020, 1024, 1028, ar.G - 4, ar.G, ar.G + 4, 2 * ar.G + 4}
    assert {c.t for c in ar.CASES} == {1, 2, 1000, 10 ** 7}
    for n in sizes:
        assert all(c.n % 4 == 0 and 0 <= c.n_decay <= c.n for c in ar.CASES)
    for n in ar.SMALL:
        assert {c.n_decay for c in ar.CASES if c.n == n} >= set(ar.decays(n))
    assert ar.decays(1028) == [0, 1, 6, 1025, 1028] and ar.decays(4) == [0, 1, 4]
    big = {(c.n_decay - c.n if c.n_decay > 6 else c.n_decay) for c in ar.CASES if c.n >= ar.G - 4}
    assert big == {0, 1, 6, -3}
    assert any(c.b1 == 0 and c.b2 != 0 for c in ar.CASES) and any(c.b2 == 0 and c.b1 != 0 for c in ar.CASES)
    assert any(c.b1 == 0 and c.b2 == 0 for c in ar.CASES)


def test_host_scalars():
    a = ar.host_scalars(ar.DEFAULT, 1)
    assert a.omb1 == F(1.0 - float(F(0.9))) and a.omb2 == F(1.0 - float(F(0.999)))
    assert a.omb1 != F(0.1)                              # (1 - float32(0.9), not float32(0.1))
    assert a.ss == F(float(F(1e-3)) / (1.0 - float(F(0.9)))) and a.ld == F(float(F(1e-3)) * float(F(0.01)))
    assert a.rs2 == F(1.0 / math.sqrt(1.0 - float(F(0.999))))
    z = ar.host_scalars(ar.hyper(b1=0.0, b2=0.0), 1)
    assert z.omb1 == 1.0 and z.omb2 == 1.0 and z.rs2 == 1.0 and z.ss == F(1e-3)
    # t -> inf: both corrections go to 1
    for t in (10 ** 7, 10 ** 9):
        a = ar.host_scalars(ar.DEFAULT, t)
        assert a.rs2 == 1.0 and a.ss == F(1e-3)
    a = ar.host_scalars(ar.DEFAULT, 1000)
    assert a.ss == F(1e-3) and 1.0 < a.rs2 < 1.3         # beta1^1000 is gone, beta2^1000 = 0.37 is not


def test_operands_hold_what_the_cases_need():
    w, m, v, g = ar.operands(1028)
    for a in (w, m, v, g):
        assert a.dtype == F and not a.flags.writeable
    assert np.signbit(g[3]) and g[3] == 0 and g[2] == 0 and not np.signbit(g[2])
    assert np.signbit(m[3]) and m[3] == 0 and m[4] == 0 and v[3] == 0 and v[5] == 0
    assert (g > 0).any() and (g < 0).any() and (v >= 0).all() and (w != 0).all()
    nz = np.abs(g[g != 0])
    assert nz.min() >= 2.0 ** -20 and nz.max() <= 2.0 ** 21
    # no subnormal intermediate under any case's scale
    tiny = float(np.finfo(F).tiny)
    for c in ar.SMALL_CASES:
        w, m, v, g = ar.operands(c.n)
        a = ar.host_scalars(ar.case_hyper(c), c.t)
        gs = F(c.s) * g
        wn, mn, vn = ar.adamw(w, m, v, g, c.n_decay, ar.case_hyper(c), c.t, c.s)
        for x in (gs, gs * gs, a.omb2 * (gs * gs), a.omb1 * gs, a.b1 * m, a.b2 * v, mn, vn, a.ld * w, wn):
            x = np.abs(x)
            assert np.isfinite(x).all() and (x[x != 0] >= tiny).all()


@pytest.mark.parametrize('case', ar.SMALL_CASES, ids=[i for c, i in zip(ar.CASES, ar.CASE_IDS) if c.n <= 1028])
def test_float32_oracle_rounds_the_float64_restatement(case):
    """each of m', v', w' is a handful of roundings (e = 2^-24 relative each) away from the float64 value.  m': one on each product, one
    more on gs, one on the sum: 4e of |b1 m| + |omb1 gs|.  v' (all terms >= 0): gs, its square, omb2 *, b2 * v, the sum: 6e.  w': e |w|
    for x and e (|x| + |ss u|) for the last difference; u inherits 3e of m's operands over den, 5.5e from den (v' through the root,
    rs2, eps) and its own e, and ss * u one more: 16e ss max(|u|, m's operands / den) covers them with room."""
    w, m, v, g = ar.operands(case.n)
    hp = ar.case_hyper(case)
    w32, m32, v32 = ar.adamw(w, m, v, g, case.n_decay, hp, case.t, case.s)
    w64, m64, v64 = ar.adamw64(w, m, v, g, case.n_decay, hp, case.t, case.s)
    e = 2.0 ** -24
    a = ar.host_scalars(hp, case.t)
    gs = float(F(case.s)) * g.astype(np.float64)
    assert (np.abs(m32 - m64) <= 4 * e * (np.abs(float(a.b1) * m) + np.abs(float(a.omb1) * gs)) + 1e-45).all()
    assert (np.abs(v32 - v64) <= 6 * e * np.abs(v64) + 1e-45).all()
    u64 = m64 / (np.sqrt(v64) * float(a.rs2) + float(a.eps))
    # the quotient's error includes m's, relative to m's operands, not to a cancelled m'
    mag = (np.abs(float(a.b1) * m) + np.abs(float(a.omb1) * gs)) / (np.sqrt(v64) * float(a.rs2) + float(a.eps))
    assert (np.abs(w32 - w64) <= 4 * e * np.abs(w.astype(np.float64)) + 16 * e * float(a.ss) * np.maximum(mag, np.abs(u64)) + 1e-45).all()


def test_zero_gradient_only_decays():
    n, nd = 1028, 1025
    w, m, v, _ = ar.operands(n)
    z = np.zeros(n, F)
    hp = ar.hyper(b1=0.0)
    wn, mn, vn = ar.adamw(w, z, v, z, nd, hp, 5, 1.0)       # beta1 = 0 and m = 0: u = 0
    assert (mn == 0).all() and np.array_equal(vn, hp.b2 * v)
    ld = F(float(hp.lr) * float(hp.decay))
    assert np.array_equal(wn[:nd], w[:nd] - ld * w[:nd]) and np.array_equal(wn[nd:], w[nd:])
    assert not np.array_equal(wn[:nd], w[:nd])


def test_without_decay_filters_and_biases_are_alike():
    n = 1028
    w, m, v, g = ar.operands(n)
    hp = ar.hyper(decay=0.0)
    ref = ar.adamw(w, m, v, g, 0, hp, 3, 0.5)
    for nd in (1, 6, n - 3, n):
        got = ar.adamw(w, m, v, g, nd, hp, 3, 0.5)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref))
    # and with decay the split matters exactly in front of n_decay
    a = ar.adamw(w, m, v, g, 6, ar.DEFAULT, 3, 0.5)[0]
    b = ar.adamw(w, m, v, g, 0, ar.DEFAULT, 3, 0.5)[0]
    assert (a[:6] != b[:6]).all() and np.array_equal(a[6:], b[6:])


def test_large_t_is_the_uncorrected_update():
    n = 1024
    w, m, v, g = ar.operands(n)
    a = ar.host_scalars(ar.DEFAULT, 10 ** 7)
    wn, mn, vn = ar.adamw(w, m, v, g, n, ar.DEFAULT, 10 ** 7, 1.0)
    x = w - a.ld * w
    assert np.array_equal(wn, x - ar.DEFAULT.lr * (mn / (np.sqrt(vn) + a.eps)))


# ---------------------------------------------------------------------------------------------------------------------------------
# deliberately wrong restatements
def fma32(a, b, c):
    """float32 fused multiply-add, emulated: the product of two floats is exact in float64, the sum is rounded to 53 bits and then to 24"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


MISTAKES = ('decay past n_decay', 'decay through the gradient', 't off by one', 'no bias correction on m', 'no bias correction on v',
            'eps inside the root', 'v from the unscaled g', 'old m in the quotient', 'old v in the quotient', 'fused b1*m + omb1*gs',
            'fused x - ss*u')


def wrong(mistake, w, m, v, g, n_decay, hp, t, gscale):
    """adamw_ref.adamw with one mistake"""
    assert mistake in MISTAKES
    a = ar.host_scalars(hp, t + 1 if mistake == 't off by one' else t)
    if mistake == 'no bias correction on m':
        a = a._replace(ss=hp.lr)
    if mistake == 'no bias correction on v':
        a = a._replace(rs2=F(1.0))
    gs = F(gscale) * g
    if mistake == 'decay through the gradient':
        gs = gs.copy()
        gs[:n_decay] = gs[:n_decay] + hp.decay * w[:n_decay]
    mn = fma32(a.b1, m, a.omb1 * gs) if mistake == 'fused b1*m + omb1*gs' else (a.b1 * m) + (a.omb1 * gs)
    g2 = g * g if mistake == 'v from the unscaled g' else gs * gs
    vn = (a.b2 * v) + (a.omb2 * g2)
    vq = v if mistake == 'old v in the quotient' else vn
    den = np.sqrt(vq + a.eps) * a.rs2 if mistake == 'eps inside the root' else (np.sqrt(vq) * a.rs2) + a.eps
    u = (m if mistake == 'old m in the quotient' else mn) / den
    x = w.copy()
    nd = len(w) if mistake == 'decay past n_decay' else 0 if mistake == 'decay through the gradient' else n_decay
    x[:nd] = w[:nd] - (a.ld * w[:nd])
    wn = fma32(-a.ss, u, x) if mistake == 'fused x - ss*u' else x - (a.ss * u)
    return wn.astype(F), mn.astype(F), vn.astype(F)


def _exposed(mistake, c):
    w, m, v, g = ar.operands(c.n)
    hp = ar.case_hyper(c)
    ref = ar.adamw(w, m, v, g, c.n_decay, hp, c.t, c.s)
    got = wrong(mistake, w, m, v, g, c.n_decay, hp, c.t, c.s)
    return sum(int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in zip(ref, got))


@pytest.mark.parametrize('mistake', MISTAKES)
def test_the_cases_expose_the_mistake(mistake):
    hit = {c: _exposed(mistake, c) for c in ar.SMALL_CASES}
    print(mistake, {('n%d d%d t%d' % (c.n, c.n_decay, c.t)): k for c, k in hit.items() if k})
    assert any(hit.values()), mistake
    # ... and where the mistake CAN show in a case, it does: a decay in the wrong place in every case that has elements behind (or in
    # front of) n_decay, the corrections in every case whose t leaves them away from 1, the rest everywhere
    for c, k in hit.items():
        if c.n < 1020:
            continue
        can = {'decay past n_decay': c.n_decay < c.n, 'decay through the gradient': c.n_decay > 0,
               't off by one': c.t <= 1000 and (c.b1 > 0 or c.b2 > 0), 'no bias correction on m': c.t <= 2 and c.b1 > 0,
               'no bias correction on v': c.t <= 1000 and c.b2 > 0, 'v from the unscaled g': c.s != 1.0,
               'old m in the quotient': True, 'old v in the quotient': True, 'eps inside the root': True,
               # (whether a fused form rounds differently depends on the operands: the cases together must show it, above)
               'fused b1*m + omb1*gs': False, 'fused x - ss*u': False}[mistake]
        if can:
            assert k > 0, (mistake, c)


def test_the_emulated_fma_differs_from_two_roundings():
    """operands for which the fused and the unfused form differ exist among the cases' own, and a hand-made one to show the emulation works"""
    a, b, c = F(1.0 + 2.0 ** -12), F(1.0 + 2.0 ** -12), F(-1.0)
    assert fma32(a, b, c) != F(a * b) + c
    assert float(fma32(a, b, c)) == 2.0 ** -11 + 2.0 ** -24
    w, m, v, g = ar.operands(1028)
    s = ar.host_scalars(ar.DEFAULT, 2)
    gs = F(0.25) * g
    assert (fma32(s.b1, m, s.omb1 * gs) != (s.b1 * m) + (s.omb1 * gs)).sum() > 50
