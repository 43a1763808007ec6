"""Numpy float32 oracle of Soft-NMS in the DetectionOutput decode (include/ssdvgg_hip.h, ssd_detection_output_soft).

The rule, per list of candidates with scores s (f32, non-negative), unique low key words and boxes (the integers the hard rule
compares, i.e. after oracle.boxes.nms_roundtrip):
    repeat:
      i = the remaining candidate with the largest key  s[i] bits << 32 | low[i]
      if s[i] < min_score: stop
      emit (s[i], i); remove i
      for every remaining j:  iou = uni > 0 ? f32(inter) / f32(uni) : 0     (+1 pixel areas, one rounding)
          linear:    w = iou > iou_thr ? 1 - iou : 1
          gaussian:  w = expw(-((iou * iou) / sigma))
          s[j] = s[j] * w
Every operation below is a numpy float32 operation, rounded once, in the order written: the GPU kernels are compared with it
bit for bit.  `expw` is the fixed sequence of the header, not a library call.

Four parts: the rule on a list (soft_nms), detection_output with the soft step 3 (on tests/detout_ref.py's steps), the tiled form
(on tests/tiledet_ref.py's steps), and a float64 restatement (soft_nms_f64) plus named mutants.  `mutant` switches one rule to a
plausible wrong one; tests/test_softnms_ref.py shows that the cases the GPU tests use tell every mutant from the oracle."""
import numpy as np

import tiledet_ref as tr
from oracle import boxes as ob

F32 = np.float32
HARD, LINEAR, GAUSSIAN = 0, 1, 2
KINDS = {'linear': LINEAR, 'gaussian': GAUSSIAN}
MUTANTS = ('no_rerank',                   # picks in the initial order, scores decayed, each tested against min_score on its turn
           'ties_by_higher_anchor',       # equal scores go to the smaller low word
           'min_score_le',                # s <= min_score stops
           'drop_test_before_argmax',     # the stop test reads the scores as they stood before the round's decay and re-rank
           'gaussian_threshold',          # the gaussian weight only above iou_thr
           'iou_f64',                     # the quotient and the weight's argument in float64, rounded to f32 at the end
           'linear_ge',                   # 1 - iou applied at iou >= iou_thr
           'fma_poly',                    # p * r + c contracted (one rounding, emulated in float64)
           'class_agnostic',              # a pick decays the candidates of every class (image level only)
           'raw_boxes')                   # overlaps of the boxes before the abs2prop / prop2abs round trip
LIST_MUTANTS = tuple(m for m in MUTANTS if m != 'class_agnostic')

_LOG2E, _C1, _C2 = F32(1.44269504088896341), F32(0.693359375), F32(-2.12194440e-4)
_P0 = F32(1.9875691500e-4)
_P = tuple(F32(c) for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1))


def expw(x, fma=False):
    """exp(x) for an f32 array x <= 0 as the header's fixed sequence"""
    x = np.asarray(x, F32)
    small = x < F32(-87.0)
    xs = np.where(small, F32(0.0), x)
    n = np.rint(xs * _LOG2E)
    r = (xs - n * _C1) - n * _C2
    p = np.full(x.shape, _P0, F32)
    for c in _P:
        if fma:
            p = (p.astype(np.float64) * r.astype(np.float64) + np.float64(c)).astype(F32)
        else:
            p = p * r + c
    y = (p * (r * r) + r) + F32(1.0)
    scale = ((n.astype(np.int32) + 127) << 23).astype(np.uint32).view(F32)
    return np.where(small, F32(0.0), y * scale).astype(F32)


def overlap_ints(pivot, boxes):
    """inter, uni (int64) of one box with an array of boxes, +1 pixel areas: what overlaps45 computes"""
    w = np.maximum(0, np.minimum(pivot[1], boxes[:, 1]) - np.maximum(pivot[0], boxes[:, 0]) + 1)
    h = np.maximum(0, np.minimum(pivot[3], boxes[:, 3]) - np.maximum(pivot[2], boxes[:, 2]) + 1)
    inter = w * h
    area = (boxes[:, 1] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 2] + 1)
    uni = (pivot[1] - pivot[0] + 1) * (pivot[3] - pivot[2] + 1) + area - inter
    return inter, uni


def weights(inter, uni, kind, iou_thr, sigma, mutant=None):
    """the f32 weight of every overlap"""
    if kind == HARD:                         # the hard rule as a weight: 0 deletes (soft_nms removes the candidate), 1 keeps
        return np.where(20 * inter > 9 * uni, F32(0.0), F32(1.0)).astype(F32)
    iou_thr, sigma = F32(iou_thr), F32(sigma)
    ok = uni > 0
    den = np.where(ok, uni, 1)
    if mutant == 'iou_f64':
        iou = np.where(ok, inter.astype(np.float64) / den.astype(np.float64), 0.0)
        if kind == LINEAR:
            return np.where(iou > np.float64(iou_thr), 1.0 - iou, 1.0).astype(F32)
        return expw((-((iou * iou) / np.float64(sigma))).astype(F32))
    iou = np.where(ok, inter.astype(F32) / den.astype(F32), F32(0.0)).astype(F32)
    one = F32(1.0)
    if kind == LINEAR:
        hit = iou >= iou_thr if mutant == 'linear_ge' else iou > iou_thr
        return np.where(hit, one - iou, one).astype(F32)
    w = expw(-((iou * iou) / sigma), fma=mutant == 'fma_poly')
    if mutant == 'gaussian_threshold':
        w = np.where(iou > iou_thr, w, one).astype(F32)
    return w


def _bits(s):
    return np.asarray(s, F32).view(np.uint32).astype(np.uint64)


def soft_nms(conf, low, box, kind, iou_thr=0.45, sigma=0.5, min_score=0.0, mutant=None):
    """The rule on one list.  conf [n] f32 >= 0; low [n] unique ints < 2^32 (the low key words); box [n, 4] ints (xmin, xmax, ymin,
    ymax) BEFORE the round trip.  -> (order: positions in pick order, scores f32: their decayed scores).
    kind = HARD runs the greedy suppression through the same loop (a weight of 0 removes the candidate, min_score is not read):
    what the *_soft entry points compute with kind = hard, and the check that the loop and the steps around it are detout_ref's."""
    assert kind in (HARD, LINEAR, GAUSSIAN) and (mutant is None or mutant in MUTANTS), (kind, mutant)
    conf = np.asarray(conf, F32)
    n = conf.shape[0]
    box = np.asarray(box, np.int64).reshape(n, 4)
    b = box if mutant == 'raw_boxes' else ob.nms_roundtrip(box)
    low = np.asarray(low, np.uint64)
    rank = (np.uint64(0xFFFFFFFF) - low) if mutant == 'ties_by_higher_anchor' else low
    min_score = F32(min_score)
    s = conf.copy()
    before = s.copy()                        # the scores before the latest decay (one mutant reads them)
    alive = np.ones(n, bool)
    order, scores = [], []
    first = np.lexsort((-low.astype(np.int64), -_bits(conf).astype(np.int64))) if mutant == 'no_rerank' else None
    for turn in range(n):
        if mutant == 'no_rerank':
            i = int(first[turn])
            if s[i] < min_score:
                alive[i] = False
                continue
        else:
            rem = np.nonzero(alive)[0]
            if rem.size == 0:
                break
            key = (_bits(s[rem]) << np.uint64(32)) | rank[rem]
            i = int(rem[np.argmax(key)])
            tested = before[i] if mutant == 'drop_test_before_argmax' else s[i]
            if kind != HARD and ((tested <= min_score) if mutant == 'min_score_le' else (tested < min_score)):
                break
        order.append(i)
        scores.append(s[i])
        alive[i] = False
        rem = np.nonzero(alive)[0]
        if rem.size:
            inter, uni = overlap_ints(b[i], b[rem])
            before = s.copy()
            w = weights(inter, uni, kind, iou_thr, sigma, mutant)
            if kind == HARD:
                alive[rem[w == 0]] = False
            else:
                s[rem] = s[rem] * w
    return np.array(order, np.int64), np.array(scores, F32)


def soft_nms_f64(conf, low, box, kind, iou_thr=0.45, sigma=0.5, min_score=0.0):
    """The rule restated in float64 with numpy's exp: what the f32 sequence approximates.  -> (order, scores f64)"""
    conf = np.asarray(conf, F32).astype(np.float64)
    n = conf.shape[0]
    b = ob.nms_roundtrip(np.asarray(box, np.int64).reshape(n, 4))
    low = np.asarray(low, np.int64)
    s, alive = conf.copy(), np.ones(n, bool)
    order, scores = [], []
    for _ in range(n):
        rem = np.nonzero(alive)[0]
        i = int(rem[np.lexsort((-low[rem], -s[rem]))[0]])
        if s[i] < np.float64(F32(min_score)):
            break
        order.append(i)
        scores.append(s[i])
        alive[i] = False
        rem = np.nonzero(alive)[0]
        if rem.size:
            inter, uni = overlap_ints(b[i], b[rem])
            iou = np.where(uni > 0, inter / np.where(uni > 0, uni, 1), 0.0)
            if kind == LINEAR:
                s[rem] *= np.where(iou > np.float64(F32(iou_thr)), 1.0 - iou, 1.0)
            else:
                s[rem] *= np.exp(-(iou * iou) / np.float64(F32(sigma)))
    return np.array(order, np.int64), np.array(scores, np.float64)


def soft_nms_boxes(conf, box, kind, iou_thr=0.45, sigma=0.5, min_score=0.0, mutant=None):
    """ssd_soft_nms_boxes: the key's anchor field is the input index, the class field 127"""
    n = len(conf)
    low = ((32767 - np.arange(n, dtype=np.int64)) << 8) | 127
    return soft_nms(conf, low, box, kind, iou_thr, sigma, min_score, mutant)


# ---------------------------------------------------------------------------------------------------------------
# DetectionOutput with the soft step 3
# ---------------------------------------------------------------------------------------------------------------
def _empty():
    return dict(idx=np.zeros(0, np.int64), cls=np.zeros(0, np.int64), conf=np.zeros(0, F32), box=np.zeros((0, 4), np.int64))


def _by_key(recs, tiled=False):
    """records (score, [tile,] anchor, class) in descending key order: score bits, then tile, anchor, class ascending"""
    return sorted(recs, key=lambda r: (-int(np.array(r[0], F32).view(np.uint32)),) + tuple(r[1:]))


def detection_output(pred, anch, thr, nms_top_k=400, keep_top_k=200, kind=LINEAR, iou_thr=0.45, sigma=0.5, min_score=None, mutant=None):
    """-> dict(idx, cls, conf f32 (decayed), box int64 [n, 4]) of one image.  min_score None = thr.  Steps 1, 2 and 4 are
    tests/detout_ref.py's."""
    pred = np.asarray(pred, F32)
    A, nv = pred.shape
    C = nv - 5
    thr = F32(thr)
    min_score = thr if min_score is None else F32(min_score)
    boxes = {}

    def box_of(a):
        if a not in boxes:
            loc = pred[a, C + 1:].copy()
            loc[loc > 100] = 100
            boxes[a] = ob.normalize_abs_np2(*ob.decode_location_np2(loc, anch[a]))
        return boxes[a]

    sel = []
    for c in range(C):
        col = pred[:, c]
        cand = np.nonzero(~(col < thr))[0]
        cand = cand[np.lexsort((cand, -col[cand].astype(np.float64)))][:nms_top_k]
        sel.append([(col[a], int(a), c) for a in cand])
    if mutant == 'class_agnostic':
        sel = [[r for s in sel for r in s]]
    out = []
    for s in sel:
        if not s:
            continue
        low = [((32767 - a) << 8) | (127 - c) for _, a, c in s]
        order, scores = soft_nms([r[0] for r in s], low, np.array([box_of(r[1]) for r in s], np.int64).reshape(-1, 4), kind, iou_thr,
                                 sigma, min_score, None if mutant == 'class_agnostic' else mutant)
        out.extend((sc, s[i][1], s[i][2]) for i, sc in zip(order, scores))
    out = _by_key(out)[:keep_top_k]
    if not out:
        return _empty()
    return dict(idx=np.array([r[1] for r in out], np.int64), cls=np.array([r[2] for r in out], np.int64),
                conf=np.array([r[0] for r in out], F32), box=np.array([box_of(r[1]) for r in out], np.int64).reshape(-1, 4))


# ---------------------------------------------------------------------------------------------------------------
# the tiled form: tests/tiledet_ref.py's steps 1-3 and 5, Soft-NMS in step 4 (the low key word carries the tile)
# ---------------------------------------------------------------------------------------------------------------
def detout_tiles(preds, tiles, size, anch, thr, nms_top_k=400, keep_top_k=200, edge_margin=2, kind=LINEAR, iou_thr=0.45, sigma=0.5,
                 min_score=None, mutant=None):
    """one picture -> dict(idx, cls, tile, conf f32 (decayed), box int64 [n, 4] on the picture's grid)"""
    preds = np.asarray(preds, F32)
    T, A, nv = preds.shape
    C = nv - 5
    W, H = int(size[0]), int(size[1])
    thr = F32(thr)
    min_score = thr if min_score is None else F32(min_score)
    tbox, pbox = {}, {}

    def tile_box(t, a):
        if (t, a) not in tbox:
            loc = preds[t, a, C + 1:].copy()
            loc[loc > 100] = 100
            tbox[t, a] = ob.normalize_abs_np2(*ob.decode_location_np2(loc, anch[a]))
        return tbox[t, a]

    def pic_box(t, a):
        if (t, a) not in pbox:
            x0, y0, w, h, _ = tiles[t]
            xmin, xmax, ymin, ymax = tile_box(t, a)
            pbox[t, a] = (min((1000 * x0 + xmin * w) // W, 999), min((1000 * x0 + xmax * w) // W, 999),
                          min((1000 * y0 + ymin * h) // H, 999), min((1000 * y0 + ymax * h) // H, 999))
        return pbox[t, a]

    per_tile = []
    for t in range(T):
        recs = []
        for c in range(C):
            col = preds[t, :, c]
            cand = np.nonzero(~(col < thr))[0]
            cand = cand[np.lexsort((cand, -col[cand].astype(np.float64)))][:nms_top_k]
            recs += [(col[a], t, int(a), c) for a in cand if not tr._cut(tile_box(t, int(a)), tiles[t][4], edge_margin)]
        per_tile.append(recs)
    out = []
    for c in range(C):
        union = _by_key([r for recs in per_tile for r in recs if r[3] == c])[:nms_top_k]
        if not union:
            continue
        low = [tr.key(0.0, t, a, cc) & 0xFFFFFFFF for _, t, a, cc in union]
        order, scores = soft_nms([r[0] for r in union], low, np.array([pic_box(r[1], r[2]) for r in union], np.int64).reshape(-1, 4), kind,
                                 iou_thr, sigma, min_score, mutant)
        out.extend((sc,) + union[i][1:] for i, sc in zip(order, scores))
    out = _by_key(out)[:keep_top_k]
    if not out:
        return tr._empty()
    return dict(idx=np.array([r[2] for r in out], np.int64), cls=np.array([r[3] for r in out], np.int64),
                tile=np.array([r[1] for r in out], np.int64), conf=np.array([r[0] for r in out], F32),
                box=np.array([pic_box(r[1], r[2]) for r in out], np.int64).reshape(-1, 4))


def detout_tiles_all(preds, tiles, anch, thr, nms_top_k=400, keep_top_k=200, edge_margin=2, **soft):
    """tiles = [(image, (x0, y0, w, h, interior), (W, H))] as tests/tiledet_ref.py takes them -> one result per picture"""
    out = []
    for i in range(max(t[0] for t in tiles) + 1):
        sel = [j for j, t in enumerate(tiles) if t[0] == i]
        out.append(detout_tiles(preds[sel], [tuple(tiles[j][1]) for j in sel], tiles[sel[0]][2], anch, thr, nms_top_k, keep_top_k,
                                edge_margin, **soft))
    return out
