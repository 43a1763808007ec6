"""-m gpu: the clipped momentum update through ssd_op_momentum_update_clipped, the launcher the handle uses, against
the float64 oracle of tests/clip_ref.py (itself checked, and its operands shown to tell, in tests/test_clip_ref.py).

Bounds.  The norm pass squares in fp64 (exact: 48 bits of product) and sums in fp64: a sum of n <= 2^25 non-negative terms is off by
at most n * 2^-53 relative in any order, the oracle's likewise; both are far below half an fp32 ulp (2^-24), so the reported norm and
factor can differ from the oracle's by their final rounding alone: 1 ulp each.  w and acc are compared to the BIT with a twin: the
same operands through the same entry with max_norm = 0 -- the plain update's launch -- and grad_scale = float32(s) * float32(f
reported), which pins the clipped kernel to the arithmetic of the unclipped one, not to itself."""
import numpy as np
import pytest
import torch

import clip_ref as cr
from gpu_util import DEV
from ssd_tensorflow_amd._lib import lib, check

pytestmark = pytest.mark.gpu
GUARD = 64          # floats (256 bytes: the buffers between them stay 16-byte aligned)
INF = float('inf')


def _guarded(a):
    """device tensor [guard | a | guard], the guards NaN"""
    t = torch.full((a.size + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    t[GUARD:GUARD + a.size] = torch.from_numpy(np.array(a, np.float32)).to(DEV)
    return t


def _split(t, n):
    h = t.cpu().numpy()
    guards_intact = bool(np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + n:]).all())
    return h[GUARD:GUARD + n].copy(), guards_intact


def run(w, acc, g, s, max_norm, with_report=True):
    """-> (w', acc', [norm, factor] or None): one call on guarded copies; asserts every guard word (and g) intact"""
    n = g.size
    tw, ta, tg = _guarded(w), _guarded(acc), _guarded(g)
    wsb = lib.ssd_op_grad_norm_ws_bytes(n)
    assert wsb % 8 == 0
    tws = torch.full((wsb // 4 + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    trep = torch.full((2 + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    off = 4 * GUARD
    check(lib.ssd_op_momentum_update_clipped(tw.data_ptr() + off, ta.data_ptr() + off, tg.data_ptr() + off, n, float(cr.LR), float(cr.MOMENTUM),
                                             float(s), float(max_norm), tws.data_ptr() + off,
                                             trep.data_ptr() + off if with_report else None, None))
    torch.cuda.synchronize()
    w2, ok_w = _split(tw, n)
    a2, ok_a = _split(ta, n)
    g2, ok_g = _split(tg, n)
    _, ok_ws = _split(tws, wsb // 4)
    rep, ok_r = _split(trep, 2)
    assert ok_w and ok_a and ok_g and ok_ws and ok_r, 'a guard word was written'
    assert g2.tobytes() == np.ascontiguousarray(g, np.float32).tobytes()
    if not with_report:
        assert np.isnan(rep).all()
    return w2, a2, (rep if with_report else None)


def test_the_launcher_has_the_shape_the_sizes_assume():
    """the block and the grid cap that tests/clip_ref.py reads from csrc/ops.h are what the library was built with"""
    def blocks(n):
        return (lib.ssd_op_grad_norm_ws_bytes(n) - 16) // 8
    assert blocks(cr.BLOCK_FLOATS) == 1 and blocks(cr.BLOCK_FLOATS + 4) == 2
    assert blocks(cr.GRID_FLOATS - cr.BLOCK_FLOATS) == cr.GRID_CAP - 1 and blocks(cr.GRID_FLOATS) == cr.GRID_CAP == blocks(cr.GRID_FLOATS + 4)


@pytest.mark.parametrize('case', cr.CASES, ids=cr.CASE_IDS)
def test_clipped_update(case):
    n, s, rel = case
    w, acc, g = cr.operands(n)
    m = cr.max_norm_of(n, s, rel)
    want_norm, want_f = np.float32(cr.norm(g, s)), cr.factor(g, s, m)
    w2, a2, rep = run(w, acc, g, s, m)
    print('n %d s %g max_norm %r: norm %r (oracle %r), factor %r (oracle %r)' % (n, s, m, rep[0], want_norm, rep[1], want_f))
    assert np.isfinite(rep).all()
    assert cr.ulps(rep[0], want_norm) <= 1
    assert cr.ulps(rep[1], want_f) <= 1
    # f == 1 exactly when the oracle's norm is below max_norm by more than an ulp; every case here is a factor of 2 from the threshold
    if float(np.nextafter(want_norm, np.float32(INF))) < float(m):
        assert rep[1] == 1.0
    if float(np.nextafter(want_norm, np.float32(0))) > float(m):
        assert 0.0 < rep[1] < 1.0
    assert (rel < 1.0) == (rep[1] < 1.0)
    # the twin: the plain update under grad_scale = s * f
    wt, at, none = run(w, acc, g, np.float32(s) * np.float32(rep[1]), 0.0, with_report=False)
    assert a2.tobytes() == at.tobytes() and w2.tobytes() == wt.tobytes()
    assert not np.array_equal(a2, acc) and not np.array_equal(w2, w)
    # (and it is the contract's update to rounding: fused or not, one product and one sum per value)
    wo, ao, _, _ = cr.update(w, acc, g, s, m)
    assert np.allclose(a2, ao, rtol=1e-6, atol=1e-6) and np.allclose(w2, wo, rtol=1e-5, atol=1e-6)
    # run to run
    w3, a3, rep3 = run(w, acc, g, s, m)
    assert w3.tobytes() == w2.tobytes() and a3.tobytes() == a2.tobytes() and rep3.tobytes() == rep.tobytes()


def test_report_may_be_null():
    n = cr.BLOCK_FLOATS + 4
    w, acc, g = cr.operands(n)
    m = cr.max_norm_of(n, 0.25, 0.5)
    w2, a2, rep = run(w, acc, g, 0.25, m)
    w3, a3, none = run(w, acc, g, 0.25, m, with_report=False)
    assert none is None and w3.tobytes() == w2.tobytes() and a3.tobytes() == a2.tobytes()


SKIP_SIZES = (252, cr.BLOCK_FLOATS + 4, cr.GRID_FLOATS + 4)


@pytest.mark.parametrize('bad', [float('nan'), INF, -INF], ids=['nan', '+inf', '-inf'])
@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
@pytest.mark.parametrize('n', SKIP_SIZES)
def test_a_non_finite_gradient_skips_the_update(n, where, bad):
    w, acc, g = cr.operands(n)
    gb = g.copy()
    gb[dict(first=0, middle=n // 2 + 1, last=n - 1)[where]] = bad
    for m in (cr.max_norm_of(n, 1.0, 0.5), INF):
        w2, a2, rep = run(w, acc, gb, 1.0, m)
        assert w2.tobytes() == w.tobytes() and a2.tobytes() == acc.tobytes()
        assert rep[1] == 0.0 and not np.isfinite(rep[0])


MAIN_N = cr.UNROLL * cr.GRID_FLOATS + 4          # every thread takes one trip of the norm kernel's main loop, thread 0 one more of the one-pass loop
MAIN_AT = [('pass %d' % k, k * cr.GRID_FLOATS + 4 * 12345 + 1) for k in range(cr.UNROLL)] + [('thread 0 pass %d' % k, k * cr.GRID_FLOATS) for k in range(1, cr.UNROLL)] \
    + [('last', MAIN_N - 1)]


@pytest.mark.parametrize('at', MAIN_AT, ids=[a[0] for a in MAIN_AT])
def test_a_non_finite_value_in_each_load_of_the_main_loop_skips_the_update(at):
    """one NaN, +Inf or -Inf (taken in turn) where only load v[k] of the main loop reads it, for every k, in an arbitrary thread and in
    thread 0; and in the group the one-pass loop takes after it"""
    w, acc, g = cr.operands(MAIN_N)
    gb = g.copy()
    gb[at[1]] = (float('nan'), INF, -INF)[MAIN_AT.index(at) % 3]
    w2, a2, rep = run(w, acc, gb, 1.0, cr.max_norm_of(MAIN_N, 1.0, 0.5))
    assert w2.tobytes() == w.tobytes() and a2.tobytes() == acc.tobytes()
    assert rep[1] == 0.0 and not np.isfinite(rep[0])


@pytest.mark.parametrize('n', (8, cr.BLOCK_FLOATS + 4))
def test_a_zero_gradient_is_norm_zero_factor_one_and_decays_the_momentum(n):
    w, acc, _ = cr.operands(n)
    z = np.zeros(n, np.float32)
    for m in (1.0, INF):
        w2, a2, rep = run(w, acc, z, 0.5, m)
        assert rep[0] == 0.0 and rep[1] == 1.0
        wt, at, _ = run(w, acc, z, 0.5, 0.0, with_report=False)          # as the plain update decays it
        assert a2.tobytes() == at.tobytes() and w2.tobytes() == wt.tobytes()
        assert np.array_equal(a2, cr.MOMENTUM * acc)
