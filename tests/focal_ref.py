"""float64 numpy restatement of the focal loss (Lin et al. 2017, softmax form) for the tests of focal_sample_kernel
and focal_grad_kernel (csrc/ops.hip), in the two-stage manner of loss_ref.py: stage A (loss_ref.stage_a) goes from raw head
outputs and labels to what the head kernels store per anchor; stage F goes from a GIVEN cross-entropy array to the per-sample
entries and the losses, so a kernel is judged on its OWN cross entropies (the layer-local principle of loss_ref.py's stage B).

With ce = -log p_t:   p_t = exp(-ce),  q = 1 - p_t = -expm1(-ce),  alpha_t = alpha on a positive anchor, 1 - alpha on background
  fl     = alpha_t * q^gamma * ce                                      (exactly 0 at ce == 0, for gamma == 0 too)
  kappa  = alpha_t * (q^gamma + gamma * p_t * ce * q^(gamma - 1))      (q == 0: alpha_t at gamma == 0, else 0)
  sample = (sum_a fl / n, sum_pos sl1 / n, 1 / (n * bnorm), pos_n),  n = max(pos_n, 1): a sample without positives still counts
  d/d(logit c) = w_b * kappa * (softmax_c - label_c);   d/d(offset) = pos * clip(offset - gt, -1, 1) * w_b

`mistake` seeds one wrong reading of the definition (test_focal_ref.py shows that each one moves the results by far more than
the GPU tests' bounds): 'alpha_swapped', 'no_second_term', 'no_max', 'gamma_plus_one', 'naive_q'."""
import numpy as np

import loss_ref as lr

MISTAKES = ('alpha_swapped', 'no_second_term', 'no_max', 'gamma_plus_one', 'naive_q')


def _q(ce, mistake=None):
    if mistake == 'naive_q':          # 1 - exp(-ce) as fp32 arithmetic does it: every digit of a small cross entropy is lost
        ce32 = np.asarray(ce, np.float32)
        return (np.float32(1) - np.exp(-ce32, dtype=np.float32)).astype(np.float64)
    return -np.expm1(-np.asarray(ce, np.float64))


def _alpha_t(pos, alpha, mistake=None):
    pos = np.asarray(pos).astype(bool)
    if mistake == 'alpha_swapped':
        pos = ~pos
    return np.where(pos, alpha, 1.0 - alpha)


def terms(ce, pos, gamma, alpha, mistake=None):
    """per-anchor focal terms fl [B,A], float64"""
    ce = np.asarray(ce, np.float64)
    g = gamma + 1 if mistake == 'gamma_plus_one' else gamma
    q = _q(ce, mistake)
    with np.errstate(divide='ignore', invalid='ignore'):
        fl = _alpha_t(pos, alpha, mistake) * np.power(q, g) * ce
    return np.where(ce == 0, 0.0, fl)


def kappa(ce, pos, gamma, alpha, mistake=None):
    """d fl / d(-log-probability chain): the factor of (softmax - label), [B,A] float64"""
    ce = np.asarray(ce, np.float64)
    g = gamma + 1 if mistake == 'gamma_plus_one' else gamma
    q = _q(ce, mistake)
    p = np.exp(-ce)
    at = _alpha_t(pos, alpha, mistake)
    qs = np.where(q > 0, q, 1.0)                    # the q == 0 branch is decided apart
    second = 0.0 if mistake == 'no_second_term' else g * p * ce * np.power(qs, g - 1)
    k = at * (np.power(qs, g) + second)
    return np.where(q > 0, k, at if g == 0 else 0.0)


def stage_f(ce, pos, sl1, gamma=2.0, alpha=0.25, bnorm=0.0, sumsq=0.0, weight_decay=0.0, mistake=None):
    """ce, sl1 [B,A] (any float type, taken exactly), pos [B,A].  bnorm <= 0: B.  -> dict(sample [B,4], losses [4] = total,
    localization, confidence, l2; sel [B,A] all ones; pos_n [B])"""
    ce = np.asarray(ce, np.float64); sl1 = np.asarray(sl1, np.float64); pos = np.asarray(pos).astype(bool)
    B, A = ce.shape
    bn = float(bnorm) if bnorm > 0 else float(B)
    fl = terms(ce, pos, gamma, alpha, mistake)
    pos_n = pos.sum(1).astype(np.float64)
    n = pos_n.copy() if mistake == 'no_max' else np.maximum(pos_n, 1.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        sample = np.stack([fl.sum(1) / n, np.where(pos, sl1, 0.0).sum(1) / n, 1.0 / (n * bn), pos_n], 1)
    conf = sample[:, 0].sum() / bn
    loc = sample[:, 1].sum() / bn
    l2 = weight_decay * 0.5 * sumsq
    return dict(sample=sample, losses=np.array([conf + loc + l2, loc, conf, l2]), sel=np.ones((B, A), np.uint8), pos_n=pos_n, fl=fl)


def grad(result, labels, ce, pos, weight, num_classes, gamma=2.0, alpha=0.25, mistake=None):
    """d(confidence + localization)/d(head outputs) [B,A,nv] from a given result (softmax, offsets), cross entropies, positive mask
    and per-sample weight w_b = 1 / (n_b * bnorm)"""
    r = np.asarray(result, np.float64); y = np.asarray(labels, np.float64)
    nc = num_classes + 1
    w = np.asarray(weight, np.float64)[:, None, None]
    d = np.zeros_like(r)
    with np.errstate(invalid='ignore'):             # (an infinite weight: the seeded 'no_max' on a sample without positives)
        d[:, :, :nc] = (r[:, :, :nc] - y[:, :, :nc]) * w * kappa(ce, pos, gamma, alpha, mistake)[:, :, None]
        d[:, :, nc:] = np.clip(r[:, :, nc:] - y[:, :, nc:], -1, 1) * w * np.asarray(pos).astype(bool)[:, :, None]
    return d


def full_chain(out, labels, num_classes, gamma=2.0, alpha=0.25, bnorm=0.0, sumsq=0.0, weight_decay=0.0, mistake=None):
    """loss_ref.stage_a, stage F on its float64 cross entropies, and the gradient: (stage A dict, stage F dict, d_out)"""
    a = lr.stage_a(out, labels, num_classes)
    f = stage_f(a['ce'], a['pos'], a['sl1'], gamma, alpha, bnorm, sumsq, weight_decay, mistake)
    return a, f, grad(a['result'], labels, a['ce'], a['pos'], f['sample'][:, 2], num_classes, gamma, alpha, mistake)
