"""tests/wino_emul.py without a GPU: the restatement is the algorithm (in float64 it equals the float64 convolution to rounding), in
fp32 it stays at the 1e-4 level the project asserts for Winograd against the direct kernels (tests/test_gpu_model.py), the figures in
profiles/wino_error_bound.txt are what it measures, and the limit the GPU test derives from them is sharper than 1e-4 of max |ref|
for every pass but the single taps of the weight gradient (where the GPU test caps it there and adds the taps-pooled figure)."""
import os

import numpy as np
import pytest

import wino_emul as we

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'wino_error_bound.txt')
IDS = [c[0] for c in we.CASES]


def max_rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def test_the_matrices_are_the_minimal_filtering_identity():
    """y = A^T [(G g) . (B^T d)] in exact fractions, one dimension: F(4, 3)"""
    from fractions import Fraction as Fr
    d = [Fr(n) for n in (3, -1, 4, 1, -5, 9)]
    g = [Fr(n) for n in (2, -7, 1)]
    Gg = [sum(r[j] * g[j] for j in range(3)) for r in we.G]
    Bd = [sum(r[j] * d[j] for j in range(6)) for r in we.BT]
    y = [sum(r[j] * Gg[j] * Bd[j] for j in range(6)) for r in we.AT]
    assert y == [sum(d[i + k] * g[k] for k in range(3)) for i in range(4)]
    assert [sum(we.BIAS_C[k] * we.AT[i][k] for k in range(6)) for i in range(4)] == [1, 1, 1, 1]


@pytest.mark.parametrize('case', we.CASES, ids=IDS)
def test_restatement_against_float64(case):
    o = we.inputs(case)
    exact = we.emulate(o, np.float64)
    fp32 = we.emulate(o)
    for p in we.PASSES:
        ref, A = o.ref[p]
        assert max_rel(exact[p], ref) < 1e-12, p
        assert fp32[p].dtype == np.float32 and max_rel(fp32[p], ref) < 1e-4, (p, max_rel(fp32[p], ref))
    assert (o.x == 0).mean() > 0.3 and (o.dy == 0).mean() > 0.2      # relu-like input, dy masked by the layer's relu


@pytest.mark.parametrize('case', we.CASES, ids=IDS)
def test_profile_holds_the_measured_figures_and_the_limit_is_sharp(case):
    o = we.inputs(case)
    prof = we.read_profile(PROFILE)
    assert len(prof) == len(we.CASES) * len(we.PASSES)
    for p, v in we.rho_emul(o).items():
        assert abs(prof[case[0], p] - v) <= 1e-4 * v, (p, prof[case[0], p], v)
        ref, A = o.ref[p]
        limit = 2 * v * 2.0 ** -24 * A.max() / np.abs(ref).max()
        assert limit < 1e-4 or p == 'wgrad', (p, limit)
