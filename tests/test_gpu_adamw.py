"""-m gpu: the AdamW update through ssd_op_adamw_update, the launcher the handle uses, against the float32 oracle of
tests/adamw_ref.py (itself checked, and its operands shown to tell, in tests/test_adamw_ref.py).

The contract rounds every operation once and fuses none, so w, m and v are compared to the BIT (np.array_equal on the float32 arrays,
and on their bytes where signed zeros matter).  The clipped launcher is pinned three ways: with max_norm = +inf and with a threshold
above the norm it gives the bits of the plain one; at half the norm the bits of the oracle under gscale = float32(s) * f, f the factor
the finish kernel reported (itself held to 1 ulp of the float64 oracle in tests/test_gpu_grad_clip.py); a gradient that is not finite
leaves all three arrays alone.  NaN guard words lie around w, m, v, the workspace and the report."""
import numpy as np
import pytest
import torch

import adamw_ref as ar
import clip_ref as cr
from gpu_util import DEV
from ssd_tensorflow_amd._lib import lib, check

pytestmark = pytest.mark.gpu
GUARD = 64          # floats (256 bytes: the buffers between them stay 16-byte aligned)
INF = float('inf')
F = np.float32


def _guarded(a):
    """device tensor [guard | a | guard], the guards NaN"""
    t = torch.full((a.size + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    t[GUARD:GUARD + a.size] = torch.from_numpy(np.array(a, F)).to(DEV)
    return t


def _split(t, n):
    h = t.cpu().numpy()
    guards_intact = bool(np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + n:]).all())
    return h[GUARD:GUARD + n].copy(), guards_intact


def run(w, m, v, g, n_decay, hp, t, s, max_norm=0.0, with_report=True):
    """-> (w', m', v', [norm, factor] or None): one call on guarded copies; asserts every guard word (and g) intact"""
    n = g.size
    tw, tm, tv, tg = _guarded(w), _guarded(m), _guarded(v), _guarded(g)
    wsb = lib.ssd_op_grad_norm_ws_bytes(n)
    tws = torch.full((wsb // 4 + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    trep = torch.full((2 + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    off = 4 * GUARD
    clipped = float(max_norm) != 0.0
    check(lib.ssd_op_adamw_update(tw.data_ptr() + off, tm.data_ptr() + off, tv.data_ptr() + off, tg.data_ptr() + off, n, int(n_decay),
                                  float(hp.lr), float(hp.b1), float(hp.b2), float(hp.eps), float(hp.decay), int(t), float(s),
                                  float(max_norm), tws.data_ptr() + off if clipped else None,
                                  trep.data_ptr() + off if with_report and clipped else None, None))
    torch.cuda.synchronize()
    w2, ok_w = _split(tw, n)
    m2, ok_m = _split(tm, n)
    v2, ok_v = _split(tv, n)
    g2, ok_g = _split(tg, n)
    ws, ok_ws = _split(tws, wsb // 4)
    rep, ok_r = _split(trep, 2)
    assert ok_w and ok_m and ok_v and ok_g and ok_ws and ok_r, 'a guard word was written'
    assert g2.tobytes() == np.ascontiguousarray(g, F).tobytes()
    if not clipped:
        assert np.isnan(ws).all()                # the plain update has no norm pass and reads no workspace
    if not (with_report and clipped):
        assert np.isnan(rep).all()
    return w2, m2, v2, (rep if with_report and clipped else None)


def same(got, want):
    return all(np.array_equal(a, b) and a.tobytes() == b.tobytes() for a, b in zip(got, want))


def test_the_launcher_has_the_shape_the_sizes_assume():
    """block 256, grid cap 4096: one pass of the grid is G = 4 194 304 floats (csrc/ops.h; the norm pass shares the shape)"""
    assert ar.BLOCK == 256 and ar.GRID_CAP == 4096 and ar.G == 4194304 == cr.GRID_FLOATS


@pytest.mark.parametrize('case', ar.CASES, ids=ar.CASE_IDS)
def test_update_has_the_bits_of_the_oracle(case):
    w, m, v, g = ar.operands(case.n)
    hp = ar.case_hyper(case)
    want = ar.adamw(w, m, v, g, case.n_decay, hp, case.t, case.s)
    got = run(w, m, v, g, case.n_decay, hp, case.t, case.s)
    for name, a, b in zip('wmv', got, want):
        bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
        print('%s: %d of %d elements differ%s' % (name, bad.size, a.size, '' if not bad.size else ', first at %d: %r against %r' % (bad[0], a[bad[0]], b[bad[0]])))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert same(got[:3], want)                  # the signs of the zeros too
    assert not np.array_equal(got[0], w) and not np.array_equal(got[2], v)
    # run to run
    again = run(w, m, v, g, case.n_decay, hp, case.t, case.s)
    assert same(again[:3], got[:3])


CLIP_CASES = [c for c in ar.CASES if c.n in (8, 1028, ar.G + 4)][::2] + [c for c in ar.CASES if c.n == 2 * ar.G + 4][:1]


@pytest.mark.parametrize('case', CLIP_CASES, ids=[ar.CASE_IDS[ar.CASES.index(c)] for c in CLIP_CASES])
def test_clipped_update(case):
    w, m, v, g = ar.operands(case.n)
    hp = ar.case_hyper(case)
    plain = run(w, m, v, g, case.n_decay, hp, case.t, case.s)
    norm = cr.norm(g, case.s)
    # measured only, and a threshold above the norm: factor 1, the bits of the plain update
    for max_norm in (INF, F(2.0 * norm)):
        got = run(w, m, v, g, case.n_decay, hp, case.t, case.s, max_norm)
        assert got[3][1] == 1.0 and cr.ulps(got[3][0], F(norm)) <= 1
        assert same(got[:3], plain[:3])
    # half the norm: the oracle under gscale = s * f, one float32 product, f as reported
    half = F(0.5 * norm)
    got = run(w, m, v, g, case.n_decay, hp, case.t, case.s, half)
    f = got[3][1]
    print('n %d: norm %r (oracle %r), factor %r (oracle %r)' % (case.n, got[3][0], F(norm), f, cr.factor(g, case.s, half)))
    assert 0.0 < f < 1.0 and cr.ulps(f, cr.factor(g, case.s, half)) <= 1
    want = ar.adamw(w, m, v, g, case.n_decay, hp, case.t, F(case.s) * F(f))
    assert same(got[:3], want)
    assert not same(got[:3], plain[:3])
    # run to run, and without a report
    again = run(w, m, v, g, case.n_decay, hp, case.t, case.s, half, with_report=False)
    assert again[3] is None and same(again[:3], got[:3])


@pytest.mark.parametrize('bad', [float('nan'), INF, -INF], ids=['nan', '+inf', '-inf'])
@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
@pytest.mark.parametrize('n', (1028, ar.G + 4))
def test_a_non_finite_gradient_skips_the_update(n, where, bad):
    w, m, v, g = ar.operands(n)
    gb = g.copy()
    gb[dict(first=0, middle=n // 2 + 1, last=n - 1)[where]] = bad
    for max_norm in (F(0.5 * cr.norm(g, 1.0)), INF):
        got = run(w, m, v, gb, n - 3, ar.DEFAULT, 2, 1.0, max_norm)
        assert got[0].tobytes() == w.tobytes() and got[1].tobytes() == m.tobytes() and got[2].tobytes() == v.tobytes()
        assert got[3][1] == 0.0 and not np.isfinite(got[3][0])
