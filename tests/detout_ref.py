"""Numpy oracle of DetectionOutput, the decode of the SSD paper, built on oracle/boxes.py.

Per image, pred [A, C+5] f32 (C foreground classes, background, 4 offsets):
  1. per foreground class c the anchors with !(pred[a, c] < conf_thr), by confidence descending (by float value), exact ties
     by lower anchor; the first nms_top_k.  The background column yields nothing.
  2. their boxes as the argmax path decodes them: offsets > 100 clamped on a copy, decode_location_np2, normalize_abs_np2.
  3. greedy suppression per class: oracle.boxes.nms_class (20 inter > 9 union after the abs2prop / prop2abs round trip).
  4. the survivors of all classes by (confidence descending, anchor ascending, class ascending); the first keep_top_k.
Selection comes before decoding, and a box depends on its anchor alone, so an image decodes at most min(A, C * nms_top_k) boxes.

`mutant` switches one rule to a plausible wrong one; tests/test_detout_ref.py shows that the cases the GPU tests use tell every
mutant from the oracle."""
import numpy as np

from oracle import boxes as ob

F32 = np.float32
MUTANTS = ('threshold_gt', 'nms_top_k_off_by_one', 'nms_top_k_plus_one', 'cut_ties_by_higher_anchor', 'keep_top_k_before_nms',
           'class_agnostic_nms', 'final_ties_by_class_first', 'background_admitted')


def _empty():
    return dict(idx=np.zeros(0, np.int64), cls=np.zeros(0, np.int64), conf=np.zeros(0, F32), box=np.zeros((0, 4), np.int64))


def detection_output(pred, anch, thr, nms_top_k=400, keep_top_k=200, mutant=None):
    """-> dict(idx, cls, conf f32, box int64 [n, 4]) of one image, in step 4's order."""
    assert mutant is None or mutant in MUTANTS, mutant
    pred = np.asarray(pred, F32)
    A, nv = pred.shape
    C = nv - 5
    thr = F32(thr)
    k = nms_top_k - 1 if mutant == 'nms_top_k_off_by_one' else nms_top_k + 1 if mutant == 'nms_top_k_plus_one' else nms_top_k
    boxes = {}

    def box_of(a):
        if a not in boxes:
            loc = pred[a, C + 1:].copy()
            loc[loc > 100] = 100
            boxes[a] = ob.normalize_abs_np2(*ob.decode_location_np2(loc, anch[a]))
        return boxes[a]

    # step 1: (conf, anchor, class) of every class' first k candidates
    sel = []
    for c in range(C + 1 if mutant == 'background_admitted' else C):
        col = pred[:, c]
        cand = np.nonzero(col > thr if mutant == 'threshold_gt' else ~(col < thr))[0]
        tie = -cand if mutant == 'cut_ties_by_higher_anchor' else cand
        cand = cand[np.lexsort((tie, -col[cand].astype(np.float64)))][:max(k, 0)]
        sel.append([(col[a], int(a), c) for a in cand])

    def final_order(recs):
        if mutant == 'final_ties_by_class_first':
            return sorted(recs, key=lambda r: (-float(r[0]), r[2], r[1]))
        return sorted(recs, key=lambda r: (-float(r[0]), r[1], r[2]))

    if mutant == 'keep_top_k_before_nms':
        kept = final_order([r for s in sel for r in s])[:keep_top_k]
        sel = [[r for r in kept if r[2] == c] for c in range(C)]
    # steps 2, 3
    out = []
    if mutant == 'class_agnostic_nms':
        recs = final_order([r for s in sel for r in s])
        if recs:
            out = [recs[i] for i in ob.nms_class(np.array([box_of(r[1]) for r in recs], np.int64).reshape(-1, 4))]
    else:
        for s in sel:
            if s:
                out.extend(s[i] for i in ob.nms_class(np.array([box_of(r[1]) for r in s], np.int64).reshape(-1, 4)))
    # step 4
    out = final_order(out)
    if mutant != 'keep_top_k_before_nms':
        out = out[:keep_top_k]
    if not out:
        return _empty()
    return dict(idx=np.array([r[1] for r in out], np.int64), cls=np.array([r[2] for r in out], np.int64),
                conf=np.array([r[0] for r in out], F32), box=np.array([box_of(r[1]) for r in out], np.int64).reshape(-1, 4))


def same(a, b):
    """two results agree in count, confidence bits, class, anchor and box"""
    return (len(a['idx']) == len(b['idx']) and np.array_equal(a['conf'].view(np.uint32), b['conf'].view(np.uint32))
            and np.array_equal(a['cls'], b['cls']) and np.array_equal(a['idx'], b['idx']) and np.array_equal(a['box'], b['box']))


# ---------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_detection_output.py (and of the mutant checks in tests/test_detout_ref.py)
# ---------------------------------------------------------------------------------------------------------------
def softmax_rows(rng, b, A, C, spread):
    """seeded softmax rows [b, A, C+5]: class logits N(0, spread), offsets N(0, 1)"""
    z = rng.normal(0.0, spread, (b, A, C + 1))
    e = np.exp(z - z.max(-1, keepdims=True))
    pred = np.empty((b, A, C + 5), F32)
    pred[..., :C + 1] = (e / e.sum(-1, keepdims=True)).astype(F32)
    pred[..., C + 1:] = rng.normal(0.0, 1.0, (b, A, 4)).astype(F32)
    return pred


def quiet_rows(rng, b, A, C):
    """rows whose foreground columns all lie below 0.01 (background 0.99), offsets N(0, 0.5)"""
    pred = np.zeros((b, A, C + 5), F32)
    pred[..., :C] = rng.uniform(0.0, 0.009, (b, A, C)).astype(F32) / F32(max(C, 1))
    pred[..., C] = F32(0.99)
    pred[..., C + 1:] = rng.normal(0.0, 0.5, (b, A, 4)).astype(F32)
    return pred


def plant(rng, pred, img, c, n, lo=0.02, hi=0.9, values=None):
    """n distinct anchors of image img get a confidence for class c (distinct seeded values in [lo, hi), or `values`)"""
    A = pred.shape[1]
    at = rng.choice(A, n, replace=False)
    if values is None:
        values = np.unique(rng.uniform(lo, hi, 4 * n).astype(F32))[:n]
        rng.shuffle(values)
    pred[img, at, c] = np.asarray(values, F32)
    return at
