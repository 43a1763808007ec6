"""CPU: the float64 GIoU oracle of tests/giou_ref.py is itself checked -- against torch autograd of the definition written directly,
against the same loss in absolute image coordinates under random anchors (the design fact: no anchor table is needed), at its
limits (identical boxes, the clamp, the range of L, linearity in the weight), for the separation condition on the inputs of
giou_cases.py, and for its power to tell: each seeded mistake moves the sums or gradients of the GPU test's own inputs by at least
1e-3, a hundred times the 1e-5 the GPU test allows."""
import numpy as np
import pytest
import torch

import focal_ref as fr
import giou_cases as gc
import giou_ref as gr
import loss_ref as lr

FAR = 1e-3            # 100 x the caps of test_gpu_giou.py (1e-5 on terms and on gradients)
SMALL = [c for c in gc.CASES if lr.layout(*c[1], c[2])['A'] * len(c[3]) <= 8000]          # (the CPU suite stays quick)


def _torch_L(t, g):
    """1 - GIoU of the definition, nothing factored, on torch float64 [..., 4]"""
    def box(v):
        v = v.clamp(-100.0, 100.0)
        cx, cy, w, h = v[..., 0] / 10, v[..., 1] / 10, torch.exp(v[..., 2] / 5), torch.exp(v[..., 3] / 5)
        return cx - w / 2, cx + w / 2, cy - h / 2, cy + h / 2
    x0p, x1p, y0p, y1p = box(t)
    x0g, x1g, y0g, y1g = box(g)
    iw = (torch.minimum(x1p, x1g) - torch.maximum(x0p, x0g)).clamp(min=0)
    ih = (torch.minimum(y1p, y1g) - torch.maximum(y0p, y0g)).clamp(min=0)
    inter = iw * ih
    union = (x1p - x0p) * (y1p - y0p) + (x1g - x0g) * (y1g - y0g) - inter
    enc = (torch.maximum(x1p, x1g) - torch.minimum(x0p, x0g)) * (torch.maximum(y1p, y1g) - torch.minimum(y0p, y0g))
    giou = inter / union - (enc - union) / enc
    return 1 - giou


def _positives(case):
    """(t, g, tie) [n, 4], [n, 4], [n] of a case's positive anchors"""
    name, layout, C_, pos_counts, kind = case[:5]
    out, y, tie = gc.make(name, layout, C_, pos_counts, kind)
    pos = y[:, :, C_] == 0
    return out[pos][:, C_ + 1:], y[pos][:, C_ + 1:], tie[pos]


@pytest.mark.parametrize('case', SMALL, ids=[c[0] for c in SMALL])
def test_inputs_are_separated_and_gradient_is_autograd(case):
    t, g, tie = _positives(case)
    assert len(t) and gr.separated(t[~tie], g[~tie]).all(), 'a fixture outside the tie entries is not separated: re-seed it'
    # (width by width the clamp's own kink is no tie of the definition's max / min: autograd's clamp passes the gradient at exactly
    # +-100 as the definition does, and zeroes it beyond)
    tt = torch.tensor(t[~tie], dtype=torch.float64, requires_grad=True)
    L = _torch_L(tt, torch.tensor(g[~tie], dtype=torch.float64))
    L.sum().backward()
    L_ref, d_ref = gr.loss_and_grad(t[~tie], g[~tie])
    assert np.abs(L_ref - L.detach().numpy()).max() <= 1e-12
    assert np.abs(d_ref - tt.grad.numpy()).max() <= 1e-12 * max(np.abs(d_ref).max(), 1.0)
    assert (L_ref >= 0).all() and (L_ref < 2).all()


def test_every_palette_entry_is_used_and_the_tie_flags_are_right():
    seen = set()
    for c in SMALL:
        t, g, tie = _positives(c)
        for pt, pg, is_tie in gc.PALETTE:
            hit = (t == np.array(pt, np.float32)).all(1) & (g == np.array(pg, np.float32)).all(1)
            if hit.any():
                seen.add((pt, pg))
                assert (tie[hit] == is_tie).all()
    assert len(seen) == len(gc.PALETTE)
    for pt, pg, is_tie in gc.PALETTE:
        assert bool(gr.separated(np.array(pt, np.float32), np.array(pg, np.float32))) != is_tie, (pt, pg)


def test_anchor_normalised_equals_absolute_coordinates():
    """GIoU of the decoded boxes in image coordinates (ssdutils.decode_location: centre = anchor centre + t / 10 * anchor size,
    size = anchor size * exp(t / 5)) equals the value in units of the anchor"""
    rng = np.random.default_rng(2)
    n = 10000
    t = rng.normal(0, 3, (n, 4)); g = rng.normal(0, 2, (n, 4))
    t[::3, :2] += rng.choice([-1.0, 1.0], (len(t[::3]), 2)) * rng.uniform(8, 40, (len(t[::3]), 2))
    acx, acy = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    aw, ah = rng.uniform(0.02, 0.9, n), rng.uniform(0.02, 0.9, n)

    def absolute(v):
        cx, cy = acx + v[:, 0] / 10 * aw, acy + v[:, 1] / 10 * ah
        w, h = aw * np.exp(v[:, 2] / 5), ah * np.exp(v[:, 3] / 5)
        return cx - w / 2, cx + w / 2, cy - h / 2, cy + h / 2, w, h
    x0p, x1p, y0p, y1p, wp, hp = absolute(t)
    x0g, x1g, y0g, y1g, wg, hg = absolute(g)
    iw = np.maximum(np.minimum(x1p, x1g) - np.maximum(x0p, x0g), 0)
    ih = np.maximum(np.minimum(y1p, y1g) - np.maximum(y0p, y0g), 0)
    I = iw * ih
    U = wp * hp + wg * hg - I
    C = (np.maximum(x1p, x1g) - np.minimum(x0p, x0g)) * (np.maximum(y1p, y1g) - np.minimum(y0p, y0g))
    L_abs = 2 - I / U - U / C
    L, _ = gr.loss_and_grad(t, g)
    assert (I == 0).sum() > n // 10 and (I > 0).sum() > n // 10
    assert np.abs(L - L_abs).max() <= 1e-12


def test_identical_boxes_and_touching_boxes():
    t = np.array([[1.5, -2.25, 3.0, -4.0], [0, 0, 0, 0], [99.5, -100.0, 100.0, -7.0]])
    L, d = gr.loss_and_grad(t, t)
    assert (L[:2] == 0).all() and not d[:2].any()
    # (x1 - x0 is w only up to the rounding of the centre's magnitude: the third box, at cx = 9.95 with w = exp(20), and random
    # ones are 0 to float64 rounding)
    assert np.abs(L).max() <= 1e-14 and np.abs(d).max() <= 1e-14
    rng = np.random.default_rng(9)
    t = rng.normal(0, 3, (1000, 4))
    L, d = gr.loss_and_grad(t, t)
    assert np.abs(L).max() <= 1e-14 and np.abs(d).max() <= 1e-14
    # touching in x: not live, the intersection's derivative is off; L = 2 - 0 - U / C = 2 - 2 / 2 = 1
    L, d = gr.loss_and_grad(np.array([10.0, 0, 0, 0]), np.array([0.0, 0, 0, 0]))
    assert L == 1.0 and d[0] > 0 and d[1] == 0


def test_clamp_zeroes_exactly_the_clamped_components():
    rng = np.random.default_rng(4)
    g = rng.normal(0, 1, (64, 4))
    for comp in range(4):
        for v in (100.5, -100.5, 1e30, -1e30):
            t = g + rng.normal(0, 0.5, g.shape)
            t[:, comp] = v
            L, d = gr.loss_and_grad(t, g)
            assert np.isfinite(L).all() and np.isfinite(d).all()
            assert not d[:, comp].any()
            others = [k for k in range(4) if k != comp]
            assert (d[:, others] != 0).any()          # (not every column: a box of width exp(20) contains the other in x, no pull on t0)
            tc = t.copy(); tc[:, comp] = np.sign(v) * 100.0          # the value at the clamp: same loss, and there the gradient is kept
            Lc, dc = gr.loss_and_grad(tc, g)
            assert np.array_equal(L, Lc) and np.array_equal(d[:, others], dc[:, others])
    _, d = gr.loss_and_grad(np.array([0.5, -0.25, 100.0, -100.0]), np.array([0.25, 0.5, 0.0, 0.0]))
    assert d[2] != 0 and d[3] != 0          # |t| == 100 is not beyond the clamp


def test_weight_scales_linearly_and_negatives_are_zero():
    name, layout, C_, pos_counts, kind = gc.CASES[3][:5]
    out, y, _ = gc.make(name, layout, C_, pos_counts, kind)
    assert len(pos_counts) == 4
    wb = np.array([0.25, 0.0, 0.125, 0.5])
    pos = y[:, :, C_] == 0
    t1, t3 = gr.terms(out, y, C_, 1.0), gr.terms(out, y, C_, 3.0)
    g1, g3 = gr.grad(out, y, C_, 1.0, wb), gr.grad(out, y, C_, 3.0, wb)
    assert np.allclose(t3, 3 * t1, rtol=1e-15, atol=0) and np.allclose(g3, 3 * g1, rtol=1e-15, atol=0)
    assert not t1[~pos].any() and not g1[~pos].any() and (t1[pos] >= 0).all() and np.abs(g1).max() > 0


# ---- seeded mistakes on the GPU test's inputs ---------------------------------------------------------------------------------
def _moved(case, mistake):
    """(largest relative change of sample / losses, change of the gradient relative to its largest magnitude) under the mistake"""
    name, layout, C_, pos_counts, kind, conf, gamma, alpha, weight = case
    out, y, _ = gc.make(name, layout, C_, pos_counts, kind)
    a = lr.stage_a(out, y, C_)
    res = []
    for m in (None, mistake):
        sl1 = gr.terms(out, y, C_, weight, m)
        if conf == 'focal':
            s = fr.stage_f(a['ce'], a['pos'], sl1, gamma, alpha)
            d = fr.grad(a['result'], y, a['ce'], a['pos'], s['sample'][:, 2], C_, gamma, alpha)
        else:
            s = lr.stage_b(a['ce'], a['pos'], sl1)
            d = lr.grad(a['result'], y, s['sel'], a['pos'], s['sample'][:, 2], C_)
        d = gr.with_loc_grad(d, out, y, C_, weight, s['sample'][:, 2], m)
        res.append((np.concatenate([s['sample'][:, :3].ravel(), s['losses']]), d))
    (s0, d0), (s1, d1) = res
    with np.errstate(divide='ignore', invalid='ignore'):
        ds = np.where(s0 != 0, np.abs(s1 - s0) / np.abs(s0), np.where(s1 == s0, 0.0, np.inf))
        dg = np.abs(d1 - d0).max() / np.abs(d0).max()
    return float(np.nan_to_num(ds, nan=np.inf).max()), float(np.nan_to_num(dg, nan=np.inf))


@pytest.mark.parametrize('mistake', gr.MISTAKES)
def test_seeded_mistake_moves_the_gpu_inputs(mistake):
    cases = [c for c in SMALL if mistake != 'no_weight_grad' or c[8] != 1.0]
    assert len(cases) >= 2, mistake
    for c in cases:
        ds, dg = _moved(c, mistake)
        print(f'{mistake} on {c[0]!r}: sums move by {ds:.2e}, gradients by {dg:.2e}')
        assert max(ds, dg) >= FAR, f'{mistake} on {c[0]!r}: sums {ds:.2e}, gradients {dg:.2e}'
