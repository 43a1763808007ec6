"""CPU: the oracle of the weight EMA (tests/ema_ref.py) is itself right, and its operands and cases tell a wrong kernel from a right
one.

* the float32 result lies within half an ulp per operation of the same expressions in float64 (the bound is written out below);
* e == w is a fixed point, bit for bit, signed zeros included;
* the host scalar is 0.9 at t = 0 under every decay (d = 1 / 10) and f32(1 - decay), one rounding, past the crossover;
* no intermediate of any case is subnormal;
* mistakes show, in at least one element of every case they can show in: `w - e` for `e - w` and the form d * e + (1 - d) * w
  change the arithmetic and show in EVERY case; a dropped warm-up and `t + 1` for `t` change the host scalar alone, so they show in
  every case whose scalar they change -- for the dropped warm-up those are the cases under the warm-up, ema_ref.WARM, at every size;
  past the crossover (t = 80 ... under 0.9, t = 8991 under 0.999) both leave omd = f32(1 - decay) and the kernel's input is the same.
"""
import numpy as np
import pytest

import ema_ref as er

F = np.float32
ALL = er.CASES          # every case, the four large sizes too (a few seconds)
ALL_IDS = er.CASE_IDS
TINY = float(np.finfo(F).tiny)


def test_the_cases_are_the_ones_the_sizes_and_scalars_span():
    assert er.BLOCK == 256 and er.GRID_CAP == 4096 and er.G == 4194304
    assert sorted({c.n for c in er.CASES}) == sorted([4, 8, 1020, 1024, 1028, er.G - 4, er.G, er.G + 4, 2 * er.G + 4])
    for n in er.SIZES:
        got = {(c.decay, c.t) for c in er.CASES if c.n == n}
        assert {(0.9, t) for t in (0, 1, 89, 90, 10 ** 7)} | {(0.999, t) for t in (0, 8990, 8991)} | {(0.5, 0)} <= got
        assert {(0.9, 79), (0.9, 80)} <= got          # the sides of the min under 0.9
    assert all(c.n % 4 == 0 for c in er.CASES)


def test_host_scalar():
    for decay in (0.5, 0.9, 0.999):
        assert er.host_decay(decay, 0) == 0.1 and er.host_scalar(decay, 0) == F(0.9)
    # under the warm-up the scalar is the warm-up's, past the crossover f32(1 - decay) from the float32 decay, rounded once
    for decay, t in er.SCALARS:
        warm = (1.0 + t) / (10.0 + t)
        if (decay, t) in er.WARM:
            assert warm < float(F(decay)) and er.host_scalar(decay, t) == F(1.0 - warm), (decay, t)
        else:
            assert warm >= float(F(decay)) and er.host_scalar(decay, t) == F(1.0 - float(F(decay))), (decay, t)
    # where the min changes sides
    assert (0.9, 79) in er.WARM and (0.9, 80) not in er.WARM and (0.999, 8990) in er.WARM and (0.999, 8991) not in er.WARM
    assert er.host_scalar(0.9, 89) == er.host_scalar(0.9, 90) == er.host_scalar(0.9, 10 ** 7) == F(1.0 - float(F(0.9)))
    assert er.host_scalar(0.9, 79) != er.host_scalar(0.9, 80) and er.host_scalar(0.999, 8990) != er.host_scalar(0.999, 8991)
    # f32(1 - f32(decay)) is not f32(1) - f32(decay) rounded twice, nor 1 - decay of the double
    assert float(er.host_scalar(0.999, 10 ** 6)) == float(F(1.0 - float(F(0.999)))) != 1.0 - 0.999


@pytest.mark.parametrize('n', er.SIZES)
def test_operands_are_what_the_docstring_says(n):
    e, w = er.operands(n)
    assert e.dtype == w.dtype == F and e.size == w.size == n and not e.flags.writeable and not w.flags.writeable
    for i in er.ties(n):
        assert e[i].tobytes() == w[i].tobytes(), i
    assert 1 in er.ties(n) and (n < 8 or n - 2 in er.ties(n)) and min(er.ties(n)) < 4 and max(er.ties(n)) >= n - 4
    plain = np.flatnonzero((e != 0) & (w != 0) & (e != w))
    assert plain.size >= 2
    rel = np.abs((e[plain].astype(np.float64) - w[plain]) / w[plain])
    assert rel.min() >= 2.0 ** -21 and rel.max() <= 2.0 + 2.0 ** -20
    assert (np.abs(w[plain]) >= 0.5).all() and (np.abs(w[plain]) <= 2.0).all()
    if n >= 1020:
        assert rel.min() < 2.0 ** -18 and rel.max() > 1.0                       # the span is used
        assert (w[plain] > 0).any() and (w[plain] < 0).any() and (np.sign(e[plain]) != np.sign(w[plain])).any()
    sign = lambda a: bool(np.signbit(a))
    if n >= 8:
        assert e[3] == 0 and sign(e[3]) and e[n - 2] == 0 and not sign(e[n - 2])
        assert e[n - 1] == 0 and sign(e[n - 1]) and w[n - 1] == 0 and not sign(w[n - 1])
    if n >= 1020:
        assert w[9] == 0 and sign(w[9]) and e[9] != 0 and e[10] == 0 and not sign(e[10]) and w[10] != 0


@pytest.mark.parametrize('case', ALL, ids=ALL_IDS)
def test_float32_is_within_half_an_ulp_per_operation_of_float64(case):
    """diff32 = diff (1 + a), prod32 = omd diff32 (1 + b), out32 = (e - prod32)(1 + c) with |a|, |b|, |c| <= half an ulp of the
    value rounded: the distance to the float64 result is at most omd * ulp(diff) / 2 + ulp(prod) / 2 + ulp(out) / 2.  The ulps are
    taken at the larger of the float32 and the float64 value (they can lie either side of a power of two); the float64
    expressions' own rounding is 2^-29 of that."""
    e, w = er.operands(case.n)
    omd = er.host_scalar(case.decay, case.t)
    d32, p32, o32 = er.ema_parts(e, w, omd)
    d64, p64, o64 = er.ema64(e, w, case.decay, case.t)
    assert np.array_equal(o32, er.ema(e, w, case.decay, case.t))

    def ulp(a32, a64):
        return np.spacing(np.maximum(np.abs(a32), np.abs(a64).astype(F))).astype(np.float64)

    assert np.array_equal(d32.astype(np.float64), d64) or (np.abs(d32 - d64) <= 0.5 * ulp(d32, d64)).all()
    bound = 0.5 * (float(omd) * ulp(d32, d64) + ulp(p32, p64) + ulp(o32, o64))
    err = np.abs(o32.astype(np.float64) - o64)
    worst = int(np.argmax(err / bound))
    print('largest error %.3f of the bound, at %d' % (err[worst] / bound[worst], worst))
    assert (err <= bound * (1.0 + 2.0 ** -20)).all()
    assert err.max() > 0.0                      # (float32 does round: the bound is not met by identity)


@pytest.mark.parametrize('case', ALL, ids=ALL_IDS)
def test_a_tie_is_a_fixed_point_bit_for_bit(case):
    e, w = er.operands(case.n)
    out = er.ema(e, w, case.decay, case.t)
    for i in er.ties(case.n):
        assert out[i].tobytes() == e[i].tobytes() == w[i].tobytes(), i
    # the whole arena at rest: e == w everywhere, both signs of zero among them
    for a in (w, e):
        assert er.ema(a, a, case.decay, case.t).tobytes() == a.tobytes()
    assert not np.array_equal(out, e)


@pytest.mark.parametrize('case', ALL, ids=ALL_IDS)
def test_no_intermediate_is_subnormal(case):
    e, w = er.operands(case.n)
    for a in er.ema_parts(e, w, er.host_scalar(case.decay, case.t)) + (e, w):
        mag = np.abs(a[a != 0])
        assert (mag >= TINY).all() and np.isfinite(a).all()
    assert float(er.host_scalar(case.decay, case.t)) >= 2.0 ** -10


def _differs(a, b):
    return bool((np.asarray(a, F).view(np.uint32) != np.asarray(b, F).view(np.uint32)).any())


@pytest.mark.parametrize('case', ALL, ids=ALL_IDS)
def test_the_cases_tell_the_mistakes(case):
    e, w = er.operands(case.n)
    omd = er.host_scalar(case.decay, case.t)
    want = er.ema(e, w, case.decay, case.t)
    # the arithmetic: in every case
    assert _differs(e - (omd * (w - e)), want), 'w - e for e - w'
    d = F(er.host_decay(case.decay, case.t))
    assert _differs((d * e) + (omd * w), want), 'd * e + (1 - d) * w'
    # the host scalar: in every case whose scalar the mistake changes
    no_warmup = F(1.0 - float(F(case.decay)))
    assert (no_warmup != omd) == ((case.decay, case.t) in er.WARM)
    if no_warmup != omd:
        assert _differs(er.ema_parts(e, w, no_warmup)[2], want), 'a dropped warm-up'
    late = er.host_scalar(case.decay, case.t + 1)
    assert (late != omd) == ((case.decay, case.t) in er.WARM)
    if late != omd:
        assert _differs(er.ema_parts(e, w, late)[2], want), 't + 1 for t'


def test_every_size_has_cases_that_tell_the_scalar_mistakes():
    for n in er.SIZES:
        assert sum(1 for c in er.CASES if c.n == n and (c.decay, c.t) in er.WARM) >= 6


def test_ulps():
    a = np.array([1.0, -1.0, 0.0], F)
    assert er.ulps(a, a) == 0 and er.ulps(a, np.nextafter(a, F(2.0))) == 1 and er.ulps(F(0.0), F(-0.0)) == 0
