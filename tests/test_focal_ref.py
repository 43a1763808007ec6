"""CPU: the float64 focal-loss oracle of tests/focal_ref.py is itself checked -- against torch autograd of the same formula written
directly on logits, against plain cross entropy at gamma = 0 (and through that against loss_ref.stage_b where mining takes every
negative), at its limits, and for its power to tell: each seeded mistake moves the sums or gradients of the GPU test's own
inputs (focal_cases.py) by at least 1e-3, a hundred times the 1e-5 the GPU test allows."""
import numpy as np
import pytest
import torch

import focal_cases as fc
import focal_ref as fr
import loss_ref as lr

FAR = 1e-3            # 100 x the caps of test_gpu_focal.py (1e-5 on sums and on gradients)


def _torch_loss(out, y, C_, gamma, alpha, bnorm=0.0):
    """the definition on logits, nothing factored: fl = alpha_t * (1 - p_t)^gamma * -log p_t, smooth-L1 on positives"""
    nc = C_ + 1
    B = out.shape[0]
    bn = bnorm if bnorm > 0 else float(B)
    logp = torch.log_softmax(out[:, :, :nc], -1)
    ce = -(y[:, :, :nc] * logp).sum(-1)
    pos = y[:, :, nc - 1] == 0
    at = torch.where(pos, torch.tensor(alpha, dtype=torch.float64), torch.tensor(1.0 - alpha, dtype=torch.float64))
    mod = (1.0 - torch.exp(-ce)) ** gamma if gamma != 0 else torch.ones_like(ce)
    fl = at * mod * ce
    d = out[:, :, nc:] - y[:, :, nc:]
    sl1 = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).sum(-1) * pos
    n = pos.sum(1).clamp(min=1).to(torch.float64)
    conf = (fl.sum(1) / n).sum() / bn
    loc = (sl1.sum(1) / n).sum() / bn
    return conf, loc


@pytest.mark.parametrize('gamma', [0.0, 0.5, 1.0, 2.0, 5.0])
@pytest.mark.parametrize('alpha', [0.25, 0.75])
def test_gradient_is_autograd_of_the_definition(gamma, alpha):
    rng = np.random.default_rng(int(gamma * 10 + alpha * 100))
    C_, A = 5, 300
    out, y = lr.continuous_batch(rng, A, C_, [12, 0, 300, 1])
    a, f, d = fr.full_chain(out, y, C_, gamma, alpha, bnorm=2.5)
    t = torch.tensor(out, dtype=torch.float64, requires_grad=True)
    conf, loc = _torch_loss(t, torch.tensor(y, dtype=torch.float64), C_, gamma, alpha, bnorm=2.5)
    (conf + loc).backward()
    g = t.grad.numpy()
    assert np.abs(d - g).max() <= 1e-12 * np.abs(g).max()
    assert abs(f['losses'][2] - conf.item()) <= 1e-12 * conf.item() and abs(f['losses'][1] - loc.item()) <= 1e-12 * loc.item()
    assert np.abs(d[1, :, :C_ + 1]).max() > 0            # the sample without positives trains its background anchors
    assert not d[1, :, C_ + 1:].any()


def test_gamma_0_is_weighted_cross_entropy():
    """gamma 0, alpha 0.5: half of plain cross entropy over ALL anchors -- which is what mining computes when it takes every
    negative (k == neg_n), so half of loss_ref.stage_b's there"""
    rng = np.random.default_rng(5)
    C_, A = 20, 64
    out, y = lr.continuous_batch(rng, A, C_, [20, 30, 64])          # 3 * pos_n >= neg_n on every sample
    a = lr.stage_a(out, y, C_)
    sb = lr.stage_b(a['ce'], a['pos'], a['sl1'])
    assert (sb['k'] == A - sb['pos_n']).all()
    f = fr.stage_f(a['ce'], a['pos'], a['sl1'], 0.0, 0.5)
    assert np.allclose(f['sample'][:, 0], 0.5 * a['ce'].sum(1) / sb['pos_n'], rtol=1e-13, atol=0)
    assert np.allclose(f['sample'][:, 0], 0.5 * sb['sample'][:, 0], rtol=1e-13, atol=0)
    assert np.allclose(f['sample'][:, 1:], sb['sample'][:, 1:], rtol=1e-13, atol=0)
    assert np.isclose(f['losses'][2], 0.5 * sb['losses'][2], rtol=1e-13) and np.isclose(f['losses'][1], sb['losses'][1], rtol=1e-13)
    # ... and the gradient: kappa is alpha_t everywhere, sel is all ones
    d = fr.grad(a['result'], y, a['ce'], a['pos'], f['sample'][:, 2], C_, 0.0, 0.5)
    dm = lr.grad(a['result'], y, sb['sel'], a['pos'], sb['sample'][:, 2], C_)
    assert sb['sel'].all()
    assert np.allclose(d[:, :, :C_ + 1], 0.5 * dm[:, :, :C_ + 1], rtol=1e-13, atol=0) and np.array_equal(d[:, :, C_ + 1:], dm[:, :, C_ + 1:])


@pytest.mark.parametrize('gamma', [0.0, 0.5, 2.0])
def test_limit_ce_zero(gamma):
    """a saturated anchor (ce == 0 exactly): the term is 0 for every gamma, kappa is alpha_t at gamma 0 and 0 otherwise; nothing
    is NaN or infinite although q^(gamma - 1) is for 0 < gamma < 1"""
    ce = np.array([[0.0, 0.0, 1.5, 1e-30]]); pos = np.array([[True, False, True, False]])
    fl = fr.terms(ce, pos, gamma, 0.25)
    k = fr.kappa(ce, pos, gamma, 0.25)
    assert np.isfinite(fl).all() and np.isfinite(k).all()
    assert fl[0, 0] == 0 and fl[0, 1] == 0 and fl[0, 2] > 0
    assert list(k[0, :2]) == ([0.25, 0.75] if gamma == 0 else [0.0, 0.0])
    f = fr.stage_f(ce, pos, np.zeros_like(ce), gamma, 0.25)
    assert np.isfinite(f['sample']).all() and np.isfinite(f['losses']).all()


def test_limit_sample_without_positives():
    rng = np.random.default_rng(11)
    out, y = lr.continuous_batch(rng, 64, 20, [0, 5])
    a, f, d = fr.full_chain(out, y, 20, 2.0, 0.25)
    assert f['sample'][0, 3] == 0 and f['sample'][0, 1] == 0 and f['sample'][0, 2] == 0.5 and f['sample'][0, 0] > 0
    assert np.isclose(f['sample'][0, 0], f['fl'][0].sum(), rtol=1e-15)
    assert np.abs(d[0, :, :21]).max() > 0 and not d[0, :, 21:].any()
    assert lr.stage_b(a['ce'], a['pos'], a['sl1'])['sample'][0].tolist() == [0, 0, 0, 0]        # mining: exactly nothing


# ---- seeded mistakes on the GPU test's inputs ---------------------------------------------------------------------------------
def _shows(mistake, case):
    """does the case's configuration let the mistake show at all"""
    name, layout, C_, pos_counts, kind, gamma, alpha, easy = case
    return {'alpha_swapped': alpha != 0.5, 'no_second_term': gamma > 0, 'no_max': 0 in pos_counts, 'gamma_plus_one': True,
            'naive_q': easy is not None}[mistake]


def _moved(case, mistake):
    """(largest relative change of sample / losses, change of the gradient relative to its largest magnitude) under the mistake,
    on fp32 cross entropies (saturated rows are exact zeros there, as on the GPU)"""
    name, layout, C_, pos_counts, kind, gamma, alpha, easy = case
    out, y = fc.make(name, layout, C_, pos_counts, kind, easy)
    a = lr.stage_a(out, y, C_)
    ce = lr.ce_fp32(out, y, C_)
    res = []
    for m in (None, mistake):
        f = fr.stage_f(ce, a['pos'], a['sl1'], gamma, alpha, mistake=m)
        d = fr.grad(a['result'], y, ce, a['pos'], f['sample'][:, 2], C_, gamma, alpha, mistake=m)
        res.append((np.concatenate([f['sample'][:, :3].ravel(), f['losses']]), d))
    (s0, d0), (s1, d1) = res
    with np.errstate(divide='ignore', invalid='ignore'):
        ds = np.where(s0 != 0, np.abs(s1 - s0) / np.abs(s0), np.where(s1 == s0, 0.0, np.inf))
        dg = np.abs(d1 - d0).max() / np.abs(d0).max()
    return float(np.nan_to_num(ds, nan=np.inf).max()), float(np.nan_to_num(dg, nan=np.inf))


SMALL = [c for c in fc.CASES if lr.layout(*c[1], c[2])['A'] * len(c[3]) <= 8000]          # (the CPU suite stays quick)


@pytest.mark.parametrize('mistake', fr.MISTAKES)
def test_seeded_mistake_moves_the_gpu_inputs(mistake):
    cases = [c for c in SMALL if _shows(mistake, c)]
    assert len(cases) >= 2, mistake
    for c in cases:
        ds, dg = _moved(c, mistake)
        print(f'{mistake} on {c[0]!r}: sums move by {ds:.2e}, gradients by {dg:.2e}')
        assert max(ds, dg) >= FAR, f'{mistake} on {c[0]!r}: sums {ds:.2e}, gradients {dg:.2e}'


def test_expm1_matters_on_small_cross_entropies():
    """the easy samples hold what the palette alone does not: cross entropies small but not 0"""
    for c in fc.CASES:
        if c[7] is None:
            continue
        out, y = fc.make(*c[:5], c[7])
        ce = lr.ce_fp32(out, y, c[2])[c[7]]
        neg = y[c[7], :, c[2]] != 0
        assert ((ce[neg] > 0) & (ce[neg] < 1e-4)).all()
