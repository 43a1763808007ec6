"""
Numpy oracle of the label encoder's two matching rules, built on oracle.boxes.  Test infrastructure only.

  match_labels(gt_boxes, gt_cls, preset, num_classes, match) -> (vec [A, C+5] f32, match [A] int32)

match[a] is the index of the box that won anchor a, -1 for a background row.

'reference' is LabelCreatorTransform as oracle.boxes.encode_labels restates it, written as "who wins the anchor":
pass 1 gives an anchor the box of greatest IoU above 0.5 (the earlier box keeps a tie), pass 2 puts a box's single best
anchor (np.argmax: the first maximum, if above 0.5) on top, again greatest IoU first and the earlier box on a tie.

'paper' is the SSD paper's matching (section 2.2) as Caffe's MultiBoxLoss runs it (match_type PER_PREDICTION):
  stage 1, bipartite: repeatedly, among all pairs (box not yet matched, anchor not yet taken) with a positive
      intersection, the pair of greatest IoU; exact ties go to the lower anchor index, then to the lower box index.
      The anchor is matched to the box and both leave the pool.  It ends when no such pair is left.
  stage 2, per anchor: every anchor stage 1 left free takes the box of greatest IoU with it if that IoU exceeds 0.5
      (strictly), the lower box index on a tie.

IoU is oracle.boxes.iou_plus1: integer boxes on the 1000 grid, +1 pixel convention, float64 division.  Comparing the
float64 quotients orders them exactly as the GPU's cross-multiplied 64-bit integers do: intersections and unions are
integers below 4e6 (a box or an anchor that reaches beyond the grid may exceed it, by far less than the factor 1e3 that
is to spare), so two different ratios i1/u1 != i2/u2 differ by at least 1/(u1 u2) > 6e-14 relative to values <= 1, while
a correctly rounded float64 quotient is off by at most 1.2e-16; equal ratios of different integers (2/4, 3/6) round to
the same float64, because division is correctly rounded.  "Positive intersection" is iou > 0, also exact.
"""
import numpy as np

from oracle import boxes as ob

RULES = ('reference', 'paper')


def tables(preset):
    anch = ob.anchors(preset)
    return anch, ob.anchors_abs(anch)


def iou_matrix(gt_boxes, anch_abs):
    """[n, A] float64 IoU of every box with every anchor."""
    gt_boxes = np.asarray(gt_boxes, np.float64).reshape(-1, 4)
    out = np.zeros((gt_boxes.shape[0], anch_abs.shape[0]), np.float64)
    for i, g in enumerate(gt_boxes):
        x0, x1, y0, y1 = ob.prop2abs(g[0], g[1], g[2], g[3])
        out[i] = ob.iou_plus1(np.array([x0, x1, y0, y1], np.float64), anch_abs)
    return out


def bipartite(iou):
    """Stage 1 on an [n, A] IoU matrix -> {box: anchor}."""
    n = iou.shape[0]
    work = iou.copy()
    work[work <= 0] = -1.0                 # pairs that do not intersect are never matched
    out = {}
    for _ in range(n):
        best = work.max()
        if not best > 0:
            break
        # ties: lower anchor first, then lower box -- the first hit of a scan that walks anchors outside, boxes inside
        g, a = np.nonzero(work == best)
        k = np.lexsort((g, a))[0]
        g, a = int(g[k]), int(a[k])
        out[g] = a
        work[g, :] = -1.0
        work[:, a] = -1.0
    return out


def per_anchor(iou):
    """Every anchor's box of greatest IoU above 0.5 (the lower box on a tie), -1 if none: [A] int32."""
    A = iou.shape[1]
    if iou.shape[0] == 0:
        return np.full(A, -1, np.int32)
    g = np.argmax(iou, axis=0)             # first maximum: the lower box index
    return np.where(iou[g, np.arange(A)] > 0.5, g, -1).astype(np.int32)


def match_anchors(iou, match):
    """[A] int32 winner per anchor under `match`."""
    if match not in RULES:
        raise ValueError(match)
    win = per_anchor(iou)
    if match == 'paper':
        for g, a in bipartite(iou).items():
            win[a] = g
        return win
    best = {}
    for g in range(iou.shape[0]):          # pass 2 of the reference: a box's best anchor, if above 0.5
        a = int(np.argmax(iou[g]))
        if iou[g, a] > 0.5 and (a not in best or iou[g, a] > iou[best[a], a]):
            best[a] = g
    for a, g in best.items():
        win[a] = g
    return win


def rows(gt_boxes, gt_cls, win, anch, num_classes):
    """The label rows of a matching: one-hot class, background flag, four offsets (f64, stored as f32)."""
    gt_boxes = np.asarray(gt_boxes, np.float64).reshape(-1, 4)
    C = num_classes
    vec = np.zeros((anch.shape[0], C + 5), np.float32)
    vec[:, C] = 1
    for a in np.nonzero(win >= 0)[0]:
        g = int(win[a])
        vec[a, C] = 0
        vec[a, int(gt_cls[g])] = 1
        vec[a, C + 1:] = ob.encode_location(gt_boxes[g], anch[a])
    return vec


def match_labels(gt_boxes, gt_cls, preset, num_classes, match, anch=None, anch_abs=None):
    if anch is None:
        anch, anch_abs = tables(preset)
    iou = iou_matrix(gt_boxes, anch_abs)
    win = match_anchors(iou, match)
    return rows(gt_boxes, gt_cls, win, anch, num_classes), win


def random_boxes(rng, lo, hi, images=40, max_boxes=8, num_classes=20):
    """The seeded set of DESIGN.md 29: per image 1..max_boxes boxes, centre uniform in the image, sides uniform in
    lo..hi of the image side.  Draw order per image: count, then per box cx, cy, w, h, class."""
    out = []
    for _ in range(images):
        n = int(rng.integers(1, max_boxes + 1))
        b = np.zeros((n, 4), np.float64)
        c = np.zeros(n, np.int32)
        for i in range(n):
            b[i] = [rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(lo, hi), rng.uniform(lo, hi)]
            c[i] = int(rng.integers(0, num_classes))
        out.append((b, c))
    return out
