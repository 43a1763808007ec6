"""float64 numpy restatement of the multibox loss (ssdvgg.py:375-580) in two stages, for the op-level tests of the loss kernels
(csrc/ops.hip: heads_kernel / heads_wide_kernel, loss_sample_kernel, loss_grad_kernel, sumsq_partial_kernel).

Stage A goes from raw head outputs and labels to what the head kernels store per anchor: result, cross entropy, smooth-L1 and
the positive mask.  Stage B goes from a GIVEN cross-entropy array to the hard-negative selection and everything after it.  The
selection is a rule on values (value descending, then anchor index ascending, tf.nn.top_k), and equal values are only equal
in the precision they were computed in: a float64 cross entropy of a saturated row is ~1e-13 where fp32 gives exactly 0.  So a
kernel's selection is judged by stage B on the kernel's OWN cross entropies, the layer-local principle of test_gpu_model.py;
on tie-free input stage A + stage B agree with oracle.ssdvgg_ref.loss_numpy (test_loss_ref.py).

Also here: the head-buffer layout of the C ABI's ssd_op_multibox_loss (restated, not imported) and the generators of the
tests' inputs (logit rows drawn from a small palette, so that ties are exact in fp32 and in float64)."""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------------
# layout: anchor a = off[i] + j * hw[i] + cell lives in row (b * hw[i] + cell), columns j * nv .. of map i's [b * hw][ld] buffer
# ---------------------------------------------------------------------------------------------------------------------
def layout(hw, nj, num_classes):
    hw = [int(v) for v in hw]; nj = [int(v) for v in nj]
    nv = num_classes + 5
    off = np.concatenate([[0], np.cumsum([h * j for h, j in zip(hw, nj)])]).astype(int)
    return dict(nmaps=len(hw), hw=hw, nj=nj, nv=nv, num_classes=num_classes, ld=[(j * nv + 7) // 8 * 8 for j in nj],
                off=[int(v) for v in off], A=int(off[-1]))


PRESET_LAYOUTS = {                       # (cells per map, box types per map) of the two presets (ssdutils.py:36-62)
    'vgg300': ([38 * 38, 19 * 19, 10 * 10, 5 * 5, 3 * 3, 1], [4, 6, 6, 6, 4, 4]),
    'vgg512': ([64 * 64, 32 * 32, 16 * 16, 8 * 8, 4 * 4, 2 * 2, 1], [4, 6, 6, 6, 6, 4, 4]),
}


def pack_heads(out, lay, pad_value=0.0):
    """[B, A, nv] in anchor order -> per map [B * hw, ld] (pad columns = pad_value)"""
    B = out.shape[0]
    bufs = []
    for i in range(lay['nmaps']):
        hw, nj, nv, ld = lay['hw'][i], lay['nj'][i], lay['nv'], lay['ld'][i]
        blk = out[:, lay['off'][i]:lay['off'][i + 1]].reshape(B, nj, hw, nv)
        buf = np.full((B, hw, ld), pad_value, out.dtype)
        buf[:, :, :nj * nv] = blk.transpose(0, 2, 1, 3).reshape(B, hw, nj * nv)
        bufs.append(buf.reshape(B * hw, ld))
    return bufs


def unpack_heads(bufs, lay, B):
    """per map [B * hw, ld] -> ([B, A, nv] in anchor order, list of the pad columns [B * hw, ld - nj * nv])"""
    outs, pads = [], []
    for i in range(lay['nmaps']):
        hw, nj, nv, ld = lay['hw'][i], lay['nj'][i], lay['nv'], lay['ld'][i]
        buf = np.asarray(bufs[i]).reshape(B, hw, ld)
        outs.append(buf[:, :, :nj * nv].reshape(B, hw, nj, nv).transpose(0, 2, 1, 3).reshape(B, nj * hw, nv))
        pads.append(buf[:, :, nj * nv:].reshape(B * hw, ld - nj * nv))
    return np.concatenate(outs, 1), pads


# ---------------------------------------------------------------------------------------------------------------------
# stage A: raw head outputs + labels -> per-anchor quantities
# ---------------------------------------------------------------------------------------------------------------------
def stage_a(out, labels, num_classes):
    """-> dict(result [B,A,nv] = (softmax, offsets), ce [B,A], sl1 [B,A] (0 off the positives, as the kernels store it),
    pos [B,A] bool), all float64"""
    out = np.asarray(out, np.float64); y = np.asarray(labels, np.float64)
    nc = num_classes + 1
    z = out[:, :, :nc]
    m = z.max(-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(z - m).sum(-1))
    p = np.exp(z - lse[..., None])
    ce = (y[:, :, :nc] * (lse[..., None] - z)).sum(-1)
    pos = y[:, :, nc - 1] == 0
    d = out[:, :, nc:] - y[:, :, nc:]
    ad = np.abs(d)
    sl1 = np.where(ad < 1, 0.5 * d * d, ad - 0.5).sum(-1)
    return dict(result=np.concatenate([p, out[:, :, nc:]], -1), ce=ce, sl1=np.where(pos, sl1, 0.0), pos=pos)


def ce_fp32(out, labels, num_classes):
    """the cross entropy in fp32 arithmetic, lse = max + log(sum exp(z - max)) as the head kernels evaluate it (numpy's exp and
    log, not the hardware's: for CPU statements about saturation, not for comparing bits)"""
    out = np.asarray(out, np.float32); y = np.asarray(labels, np.float32)
    nc = num_classes + 1
    z = out[:, :, :nc]
    m = z.max(-1, keepdims=True)
    se = np.exp(z - m, dtype=np.float32).sum(-1, dtype=np.float32)
    lse = (m[..., 0] + np.log(se, dtype=np.float32)).astype(np.float32)
    return (y[:, :, :nc] * (lse[..., None] - z)).sum(-1, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# stage B: cross entropies -> selection, per-sample entries, losses
# ---------------------------------------------------------------------------------------------------------------------
def stage_b(ce, pos, sl1, bnorm=0.0, sumsq=0.0, weight_decay=0.0):
    """ce, sl1 [B,A] (any float type, taken exactly), pos [B,A] bool.  bnorm <= 0: B.  sumsq: sum of squares of the filters.
    -> dict:
      k [B]            min(neg_n, 3 * pos_n)  (0 for a sample without positives, which contributes nothing)
      picked [B,A]     the k entries of  where(pos, 0, ce)  first by value descending, then by index ascending: positives count
                       as zeros and take slots
      sel [B,A] uint8  the reported mask  pos | picked
      T, n_eq, n_eq_taken [B]   the k-th value, how many entries equal it (positives included when it is 0), how many of those
                       are picked
      sample [B,4]     confidence sum / pos_n, localization sum / pos_n, 1 / (pos_n * bnorm), pos_n  (zeros without positives)
      losses [4]       total, localization, confidence, l2"""
    ce = np.asarray(ce, np.float64); sl1 = np.asarray(sl1, np.float64); pos = np.asarray(pos).astype(bool)
    B, A = ce.shape
    bn = float(bnorm) if bnorm > 0 else float(B)
    r = dict(k=np.zeros(B, int), picked=np.zeros((B, A), bool), T=np.full(B, np.nan), n_eq=np.zeros(B, int),
             n_eq_taken=np.zeros(B, int), sample=np.zeros((B, 4)), pos_n=pos.sum(1))
    for b in range(B):
        pos_n = int(pos[b].sum())
        if pos_n == 0:
            continue
        k = min(A - pos_n, 3 * pos_n)
        negv = np.where(pos[b], 0.0, ce[b])
        order = np.lexsort((np.arange(A), -negv))[:k]
        r['k'][b] = k
        r['picked'][b, order] = True
        if k > 0:
            T = negv[order[-1]]
            r['T'][b] = T
            r['n_eq'][b] = int((negv == T).sum())
            r['n_eq_taken'][b] = k - int((negv > T).sum())
        r['sample'][b] = ((ce[b][pos[b]].sum() + negv[order].sum()) / pos_n, sl1[b][pos[b]].sum() / pos_n, 1.0 / (pos_n * bn), pos_n)
    r['sel'] = (pos | r['picked']).astype(np.uint8)
    conf = r['sample'][:, 0].sum() / bn
    loc = r['sample'][:, 1].sum() / bn
    l2 = weight_decay * 0.5 * sumsq
    r['losses'] = np.array([conf + loc + l2, loc, conf, l2])
    return r


def grad(result, labels, sel, pos, weight, num_classes):
    """d(confidence + localization)/d(head outputs) [B,A,nv]:  sel * (softmax - labels) * w_b  and  pos * clip(offsets - gt, -1, 1) * w_b
    from a given result (softmax, offsets), reported mask, positive mask and per-sample weight w_b = 1 / (pos_n * bnorm)"""
    r = np.asarray(result, np.float64); y = np.asarray(labels, np.float64)
    nc = num_classes + 1
    w = np.asarray(weight, np.float64)[:, None, None]
    d = np.zeros_like(r)
    d[:, :, :nc] = (r[:, :, :nc] - y[:, :, :nc]) * w * np.asarray(sel).astype(bool)[:, :, None]
    d[:, :, nc:] = np.clip(r[:, :, nc:] - y[:, :, nc:], -1, 1) * w * np.asarray(pos).astype(bool)[:, :, None]
    return d


def full_chain(out, labels, num_classes, bnorm=0.0, sumsq=0.0, weight_decay=0.0):
    """stage A, stage B on stage A's float64 cross entropies, and the gradient: (stage A dict, stage B dict, d_out)"""
    a = stage_a(out, labels, num_classes)
    b = stage_b(a['ce'], a['pos'], a['sl1'], bnorm, sumsq, weight_decay)
    return a, b, grad(a['result'], labels, b['sel'], a['pos'], b['sample'][:, 2], num_classes)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
N_SATURATED = 3          # palette rows 0..2 have a background cross entropy of exactly 0 in fp32
LOC_DIFFS = np.array([0.0, 1.0, -1.0, 0.5, -0.25, 0.96875, 2.25, -3.0, 1.5, -1.0625], np.float32)   # +-1 and 0 exactly, |d| > 1


def palette(rng, num_classes, n_rows=12):
    """n_rows (8..16) distinct logit rows [n_rows, num_classes + 1], multiples of 1/16 (exact in fp32):
       0, 1: the background logit leads by 30 and by 40 (exp(-30) * 127 < 2^-24: the sum of exponentials is 1, ce exactly 0)
       2:    background +80, every class -80;   3: class 0 +80, background -80, the rest near -80 (ce 160)
       4..:  moderate rows"""
    assert 8 <= n_rows <= 16
    nc = num_classes + 1
    rows = (np.round(rng.normal(0, 2, (n_rows, nc)) * 16) / 16).astype(np.float32)
    rows[:, -1] += np.float32(1.0)
    for r, lead in ((0, 30.0), (1, 40.0)):
        rows[r, -1] = rows[r, :-1].max() + np.float32(lead)
    rows[2, :-1] = -80.0; rows[2, -1] = 80.0
    rows[3, :-1] = np.float32(-80.0) + np.abs(rows[3, :-1]) / 4; rows[3, 0] = 80.0; rows[3, -1] = -80.0
    rows[4:, -1] += np.arange(n_rows - 4, dtype=np.float32) / 8          # distinct background cross entropies
    return rows


def palette_batch(rng, A, num_classes, pos_counts, zero_frac=0.25, n_rows=12):
    """(out [B,A,nv] f32, labels [B,A,nv] f32) with pos_counts[b] positives at random anchors.  Every anchor's logits are a
    palette row (a saturated one with probability zero_frac); a positive's class is random, its offsets differ from the ground
    truth by LOC_DIFFS; a negative's offsets are noise against a ground truth of 0."""
    nc, nv, B = num_classes + 1, num_classes + 5, len(pos_counts)
    pal = palette(rng, num_classes, n_rows)
    prob = np.concatenate([np.full(N_SATURATED, zero_frac / N_SATURATED), np.full(n_rows - N_SATURATED, (1 - zero_frac) / (n_rows - N_SATURATED))])
    out = np.zeros((B, A, nv), np.float32); y = np.zeros((B, A, nv), np.float32)
    for b, pn in enumerate(pos_counts):
        out[b, :, :nc] = pal[rng.choice(n_rows, A, p=prob)]
        out[b, :, nc:] = rng.normal(0, 2, (A, 4)).astype(np.float32)
        y[b, :, nc - 1] = 1.0
        idx = np.sort(rng.choice(A, pn, replace=False))
        y[b, idx, nc - 1] = 0.0
        y[b, idx, rng.integers(0, num_classes, pn)] = 1.0
        gt = (rng.integers(-16, 17, (pn, 4)) / 8).astype(np.float32)
        y[b, idx, nc:] = gt
        out[b, idx, nc:] = gt + LOC_DIFFS[rng.integers(0, len(LOC_DIFFS), (pn, 4))]
    return out, y


def continuous_batch(rng, A, num_classes, pos_counts):
    """tie-free control: continuous random logits and offsets"""
    nc, nv, B = num_classes + 1, num_classes + 5, len(pos_counts)
    out = rng.normal(0, 3, (B, A, nv)).astype(np.float32)
    y = np.zeros((B, A, nv), np.float32)
    for b, pn in enumerate(pos_counts):
        y[b, :, nc - 1] = 1.0
        idx = rng.choice(A, pn, replace=False)
        y[b, idx, nc - 1] = 0.0
        y[b, idx, rng.integers(0, num_classes, pn)] = 1.0
        y[b, idx, nc:] = rng.normal(0, 1, (pn, 4)).astype(np.float32)
    return out, y
