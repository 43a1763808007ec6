"""float64 numpy restatement of the GIoU localization loss (Rezatofighi et al. 2019; DESIGN.md 31, include/ssdvgg_hip.h
SSD_LOC_GIOU) for the tests of the LOC_GIOU instantiations of the head and gradient kernels (csrc/ops.hip).  It composes with
loss_ref.stage_b / grad and with focal_ref's stage F: `terms` takes the place of stage A's sl1, `grad` of the four loc columns of
either gradient (`with_loc_grad`).

For a positive anchor with predicted offsets t (the four loc columns of result) and label offsets g:
  tc = clamp(t, -100, 100), gc likewise
  predicted box: cx = tc0 / 10, cy = tc1 / 10, w = exp(tc2 / 5), h = exp(tc3 / 5), x0 = cx - w / 2, x1 = cx + w / 2, y0, y1;
  the ground-truth box from gc in the same way (both in units of their own anchor: GIoU is invariant under a scaling and shift per axis)
  iw = max(min(x1p, x1g) - max(x0p, x0g), 0), ih likewise, I = iw * ih, U = wp * hp + wg * hg - I
  cw = max(x1p, x1g) - min(x0p, x0g), ch likewise, C = cw * ch
  L = 1 - GIoU = 2 - I / U - U / C in [0, 2);  term = weight * L on a positive anchor, 0 elsewhere
  kI = -1/U - I/U^2 + 1/C, kA = I/U^2 - 1/C, kC = U/C^2, live = iw > 0 and ih > 0
  dL/dx0p = kI * (-ih * [live and x0p >= x0g]) + kA * (-hp) + kC * (-ch * [x0p <= x0g])
  dL/dx1p = kI * (+ih * [live and x1p <= x1g]) + kA * (+hp) + kC * (+ch * [x1p >= x1g])          (y with iw, wp, cw)
  dL/dt0 = (dL/dx0p + dL/dx1p) / 10, dL/dt2 = (dL/dx1p - dL/dx0p) * wp / 10 (t1, t3 likewise), exactly 0 where |t| > 100
  head gradient = pos * weight * w_b * dL/dt

`mistake` seeds one wrong reading of the definition (test_giou_ref.py shows that each one moves the sums or gradients of the GPU
test's own inputs by far more than its bounds): see MISTAKES."""
import numpy as np

MISTAKES = ('no_enclosing', 'enclosing_sign', 'intersection_unclamped', 'w_over_5', 'clamp_grad', 'no_weight_grad', 'swap_xy')
CLAMP = 100.0


def boxes(t, mistake=None):
    """offsets [..., 4] -> dict of x0, x1, y0, y1, w, h (float64), in units of the anchor"""
    t = np.asarray(t, np.float64)
    tc = np.clip(t, -CLAMP, CLAMP)
    cx, cy = tc[..., 0] / 10, tc[..., 1] / 10
    w, h = np.exp(tc[..., 2] / 5), np.exp(tc[..., 3] / 5)
    if mistake == 'swap_xy':
        w, h = h, w
    return dict(x0=cx - w / 2, x1=cx + w / 2, y0=cy - h / 2, y1=cy + h / 2, w=w, h=h)


def loss_and_grad(t, g, mistake=None):
    """t, g [..., 4] -> (L [...], dL/dt [..., 4]) in float64, every row treated as a positive anchor"""
    t = np.asarray(t, np.float64); g = np.asarray(g, np.float64)
    p, q = boxes(t, mistake), boxes(g, mistake)
    iw = np.minimum(p['x1'], q['x1']) - np.maximum(p['x0'], q['x0'])
    ih = np.minimum(p['y1'], q['y1']) - np.maximum(p['y0'], q['y0'])
    if mistake != 'intersection_unclamped':
        iw, ih = np.maximum(iw, 0), np.maximum(ih, 0)
    live = np.ones(iw.shape, bool) if mistake == 'intersection_unclamped' else (iw > 0) & (ih > 0)
    I = iw * ih
    U = p['w'] * p['h'] + q['w'] * q['h'] - I
    cw = np.maximum(p['x1'], q['x1']) - np.minimum(p['x0'], q['x0'])
    ch = np.maximum(p['y1'], q['y1']) - np.minimum(p['y0'], q['y0'])
    C = cw * ch
    # L = c0 - I / U - s * U / C: the definition has c0 = 2, s = 1
    c0, s = {'no_enclosing': (1.0, 0.0), 'enclosing_sign': (0.0, -1.0)}.get(mistake, (2.0, 1.0))
    L = c0 - I / U - s * U / C
    kI = -1 / U - I / U ** 2 + s / C
    kA = I / U ** 2 - s / C
    kC = s * U / C ** 2
    gx0 = kI * (-ih * (live & (p['x0'] >= q['x0']))) + kA * -p['h'] + kC * (-ch * (p['x0'] <= q['x0']))
    gx1 = kI * (ih * (live & (p['x1'] <= q['x1']))) + kA * p['h'] + kC * (ch * (p['x1'] >= q['x1']))
    gy0 = kI * (-iw * (live & (p['y0'] >= q['y0']))) + kA * -p['w'] + kC * (-cw * (p['y0'] <= q['y0']))
    gy1 = kI * (iw * (live & (p['y1'] <= q['y1']))) + kA * p['w'] + kC * (cw * (p['y1'] >= q['y1']))
    ws = 5.0 if mistake == 'w_over_5' else 10.0
    dw, dh = (gx1 - gx0) * p['w'] / ws, (gy1 - gy0) * p['h'] / ws          # by the offset that made w, and h
    if mistake == 'swap_xy':      # t3 made w and t2 made h there
        dw, dh = dh, dw
    d = np.stack([(gx0 + gx1) / 10, (gy0 + gy1) / 10, dw, dh], -1)
    if mistake != 'clamp_grad':
        d = np.where(np.abs(t) > CLAMP, 0.0, d)
    return L, d


def _split(out, labels, num_classes):
    nc = num_classes + 1
    y = np.asarray(labels, np.float64)
    return np.asarray(out, np.float64)[:, :, nc:], y[:, :, nc:], y[:, :, nc - 1] == 0


def terms(out, labels, num_classes, weight=1.0, mistake=None):
    """[B, A] float64: weight * (1 - GIoU) on the positive anchors, 0 elsewhere -- what takes the place of stage A's sl1.  out: raw
    head outputs or result (the loc columns are the same values)"""
    t, g, pos = _split(out, labels, num_classes)
    with np.errstate(over='ignore', invalid='ignore'):
        L, _ = loss_and_grad(t, g, mistake)
    return np.where(pos, weight * L, 0.0)


def grad(out, labels, num_classes, weight, sample_weight, mistake=None):
    """[B, A, 4] float64: pos * weight * w_b * dL/dt, w_b = sample_weight [B]"""
    t, g, pos = _split(out, labels, num_classes)
    with np.errstate(over='ignore', invalid='ignore'):
        _, d = loss_and_grad(t, g, mistake)
    w = 1.0 if mistake == 'no_weight_grad' else weight
    return np.where(pos[:, :, None], d * w * np.asarray(sample_weight, np.float64)[:, None, None], 0.0)


def with_loc_grad(d, out, labels, num_classes, weight, sample_weight, mistake=None):
    """a gradient of loss_ref.grad / focal_ref.grad with its four loc columns replaced by GIoU's"""
    d = np.array(d, np.float64)
    d[:, :, num_classes + 1:] = grad(out, labels, num_classes, weight, sample_weight, mistake)
    return d


def separated(t, g, rel=1e-5):
    """[...] bool: every pair of coordinates the definition compares (x0p/x0g, x1p/x1g, x1p/x0g, x1g/x0p, the same in y) differs
    by more than rel * max(|a|, |b|, 1): the fp32 branch decisions are then the float64 ones"""
    p, q = boxes(t), boxes(g)
    ok = np.ones(p['x0'].shape, bool)
    for a, b in ((p['x0'], q['x0']), (p['x1'], q['x1']), (p['x1'], q['x0']), (q['x1'], p['x0']),
                 (p['y0'], q['y0']), (p['y1'], q['y1']), (p['y1'], q['y0']), (q['y1'], p['y0'])):
        ok &= np.abs(a - b) > rel * np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0)
    return ok
