"""-m gpu: the weight EMA's two kernels through ssd_op_ema_update and ssd_op_ema_swap, the launchers the handle uses,
against the float32 oracle of tests/ema_ref.py (itself checked, and its operands shown to tell, in tests/test_ema_ref.py).

The contract rounds every operation once and fuses none, so e is compared to the BIT (on the bytes: the signs of the zeros count).
w is read only.  NaN guard words lie around both buffers."""
import numpy as np
import pytest
import torch

import ema_ref as er
from gpu_util import DEV
from ssd_tensorflow_amd._lib import lib, check

pytestmark = pytest.mark.gpu
GUARD = 64          # floats (256 bytes: the buffers between them stay 16-byte aligned)
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


def update(e, w, steps):
    """-> e after one launch per (decay, t) of `steps` on guarded copies; asserts every guard word (and w) intact"""
    n = e.size
    te, tw = _guarded(e), _guarded(w)
    off = 4 * GUARD
    for decay, t in steps:
        check(lib.ssd_op_ema_update(te.data_ptr() + off, tw.data_ptr() + off, n, float(decay), int(t), None))
    torch.cuda.synchronize()
    e2, ok_e = _split(te, n)
    w2, ok_w = _split(tw, n)
    assert ok_e and ok_w, 'a guard word was written'
    assert w2.tobytes() == np.ascontiguousarray(w, F).tobytes()
    return e2


def swap(a, b, times=1):
    n = a.size
    ta, tb = _guarded(a), _guarded(b)
    off = 4 * GUARD
    for _ in range(times):
        check(lib.ssd_op_ema_swap(ta.data_ptr() + off, tb.data_ptr() + off, n, None))
    torch.cuda.synchronize()
    a2, ok_a = _split(ta, n)
    b2, ok_b = _split(tb, n)
    assert ok_a and ok_b, 'a guard word was written'
    return a2, b2


def test_the_launcher_has_the_shape_the_sizes_assume():
    """block 256, grid cap 4096: one pass of the grid is G = 4 194 304 floats (csrc/ops.h; the AdamW update's shape)"""
    assert er.BLOCK == 256 and er.GRID_CAP == 4096 and er.G == 4194304


@pytest.mark.parametrize('case', er.CASES, ids=er.CASE_IDS)
def test_update_has_the_bits_of_the_oracle(case):
    e, w = er.operands(case.n)
    want = er.ema(e, w, case.decay, case.t)
    got = update(e, w, [(case.decay, case.t)])
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print('%d of %d elements differ%s' % (bad.size, got.size, '' if not bad.size else ', first at %d: %r against %r' % (bad[0], got[bad[0]], want[bad[0]])))
    assert got.tobytes() == want.tobytes()
    for i in er.ties(case.n):
        assert got[i].tobytes() == e[i].tobytes()
    assert got.tobytes() != e.tobytes()


SECOND = [c for c in er.CASES if (c.decay, c.t) in ((0.9, 0), (0.9, 79), (0.999, 8990))]


@pytest.mark.parametrize('case', SECOND, ids=[er.CASE_IDS[er.CASES.index(c)] for c in SECOND])
def test_a_second_launch_continues_from_the_first(case):
    """t and t + 1 on the same buffers: the second launch reads what the first wrote (79 -> 80 and 8990 -> 8991 cross from the
    warm-up to the decay)"""
    e, w = er.operands(case.n)
    first = er.ema(e, w, case.decay, case.t)
    want = er.ema(first, w, case.decay, case.t + 1)
    got = update(e, w, [(case.decay, case.t), (case.decay, case.t + 1)])
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() != first.tobytes()


@pytest.mark.parametrize('n', er.SIZES)
def test_swap_exchanges_two_buffers_bit_for_bit(n):
    e, w = er.operands(n)
    a, b = swap(e, w)
    assert a.tobytes() == w.tobytes() and b.tobytes() == e.tobytes()
    a, b = swap(e, w, times=2)
    assert a.tobytes() == e.tobytes() and b.tobytes() == w.tobytes()


def test_swap_carries_any_bit_pattern():
    """NaN payloads, infinities and subnormals cross unchanged: the kernel moves bits"""
    rng = np.random.default_rng(37)
    a = rng.integers(0, 2 ** 32, 1028, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 2 ** 32, 1028, dtype=np.uint64).astype(np.uint32)
    ta = torch.from_numpy(a.view(np.int32)).to(DEV)
    tb = torch.from_numpy(b.view(np.int32)).to(DEV)
    check(lib.ssd_op_ema_swap(ta.data_ptr(), tb.data_ptr(), 1028, None))
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy().view(np.uint32), b) and np.array_equal(tb.cpu().numpy().view(np.uint32), a)
