"""The inputs of tests/test_gpu_softnms.py, built once per process, and their oracle results (tests/softnms_ref.py), computed once
per (case, kind) and shared.  tests/test_softnms_ref.py runs the mutants over the same cases and checks that every case reaches
the edge it is named for.

Op-level cases (ssd_soft_nms_boxes): name -> dict(conf [n] f32, box [n, 4] on the 1000 grid, and per kind the parameters
(iou_thr, sigma, min_score)).  Image-level cases: tests/detout_cases.py's by import (1, 27, 28 and 127 classes and vgg512 are among
them) plus the ones below: name -> (pname, pred, thr, nms_top_k, keep_top_k, min_score)."""
import functools

import numpy as np

import detout_cases as dc
import detout_ref as dr
import softnms_ref as sr

F32 = np.float32
LINEAR, GAUSSIAN = sr.LINEAR, sr.GAUSSIAN
KIND_NAMES = ('linear', 'gaussian')
SIZES = (1, 2, 63, 64, 65, 128, 129, 400, 1023, 1024)      # the lane-ownership edges and the top
DEFAULT = (0.45, 0.5, 0.01)


def _crowd(rng, n):
    """n boxes with heavy overlap: centres in the middle fifth of the grid, sides 100..400"""
    cx, cy = rng.integers(400, 600, n), rng.integers(400, 600, n)
    w, h = rng.integers(100, 400, n), rng.integers(100, 400, n)
    x0, y0 = cx - w // 2, cy - h // 2        # (odd and even extents: the round trip moves the odd ones)
    return np.stack([x0, x0 + w, y0, y0 + h], 1).astype(np.int32)


def _confs(rng, n, lo=0.02, hi=1.0):
    v = np.unique(rng.uniform(lo, hi, 4 * n + 8).astype(F32))
    rng.shuffle(v)
    return v[:n]


def _both(p):
    return {LINEAR: p, GAUSSIAN: p}


def _overlap(n):
    rng = np.random.default_rng(3800 + n)
    conf = _confs(rng, n)
    best = int(np.argmax(conf))
    conf[[best, n - 1]] = conf[[n - 1, best]]      # the first pick is the last candidate: the last lane and slot in use
    return dict(conf=conf, box=_crowd(rng, n), params=_both(DEFAULT))


def _disjoint():
    """100 boxes of 50 x 50 on a 10 x 10 lattice of pitch 90: no pixel shared, every weight exactly 1"""
    rng = np.random.default_rng(3801)
    gx, gy = np.meshgrid(np.arange(10) * 90 + 10, np.arange(10) * 90 + 10)
    x0, y0 = gx.ravel(), gy.ravel()
    return dict(conf=_confs(rng, 100), box=np.stack([x0, x0 + 49, y0, y0 + 49], 1).astype(np.int32), params=_both((0.0, 0.5, 0.01)))


def _identical(conf):
    n = len(conf)
    return np.asarray(conf, F32), np.tile(np.array([[200, 700, 300, 800]], np.int32), (n, 1))


def _identical_equal():
    """70 identical boxes with equal confidences, min_score 0: linear weights are exactly 0, gaussian weights equal, so every
    later pick is a tie that the index resolves"""
    conf, box = _identical(np.full(70, 0.5, F32))
    return dict(conf=conf, box=box, params=_both((0.45, 0.5, 0.0)))


def _equal_conf():
    rng = np.random.default_rng(3802)
    return dict(conf=np.full(129, 0.5, F32), box=_crowd(rng, 129), params=_both(DEFAULT))


def _min_score_edge(ulps):
    """Box 1 overlaps box 0 (the first pick) and lands on a known score; box 2 touches neither and scores less.  min_score is that
    score (`ulps` = 0: box 1 stays, box 2 is dropped as below it) or one ulp above it (box 1 is dropped with everything behind
    it, though it is the best that remains)."""
    conf = np.array([0.9, 0.8, 0.05], F32)
    box = np.array([[100, 400, 100, 400], [150, 450, 100, 400], [600, 700, 600, 700]], np.int32)
    params = {}
    for kind in (LINEAR, GAUSSIAN):
        _, s = sr.soft_nms_boxes(conf, box, kind, 0.45, 0.5, 0.0)
        landed = s[1]
        assert landed < conf[1] and landed > conf[2]
        params[kind] = (0.45, 0.5, float(np.nextafter(landed, F32(1.0))) if ulps else float(landed))
    return dict(conf=conf, box=box, params=params)


def _drop_after_first():
    """identical boxes, min_score 0.5: one pick, whose decay takes every other candidate below min_score"""
    conf, box = _identical(np.linspace(0.9, 0.6, 65).astype(F32))
    return dict(conf=conf, box=box, params=_both((0.45, 0.5, 0.5)))


def _thr(iou_thr):
    d = _overlap(129)
    return dict(conf=d['conf'], box=d['box'], params=_both((iou_thr, 0.5, 0.01)))


def _identical_thr1():
    """identical boxes at iou_thr = 1: iou == iou_thr is not above it, nothing decays under the linear rule"""
    conf, box = _identical(np.linspace(0.9, 0.2, 40).astype(F32))
    return dict(conf=conf, box=box, params=_both((1.0, 0.5, 0.01)))


def _sigma_small():
    """sigma 0.01 with ten copies of box 0 among a crowd: iou = 1 gives x = -100 < -87, the weight is exactly 0"""
    rng = np.random.default_rng(3803)
    box = _crowd(rng, 100)
    box[50:60] = box[0]
    return dict(conf=_confs(rng, 100), box=box, params=_both((0.45, 0.01, 0.0)))


def _denormal():
    """confidences near 2^-120, min_score 0: after a few decays the products are denormals, which the rule keeps"""
    rng = np.random.default_rng(3804)
    conf = (np.float32(2.0) ** -120 * (1.0 + np.arange(64) / 64.0)).astype(F32)
    rng.shuffle(conf)
    return dict(conf=conf, box=_crowd(rng, 64), params=_both((0.45, 0.5, 0.0)))


_LISTS = {f'overlap-{n}': functools.partial(_overlap, n) for n in SIZES}
_LISTS.update({
    'disjoint': _disjoint,
    'identical-equal': _identical_equal,
    'equal-conf': _equal_conf,
    'on-min-score': functools.partial(_min_score_edge, 0),
    'ulp-below-min-score': functools.partial(_min_score_edge, 1),
    'drop-after-first': _drop_after_first,
    'iou-thr-0': functools.partial(_thr, 0.0),
    'iou-thr-1': functools.partial(_thr, 1.0),
    'identical-iou-thr-1': _identical_thr1,
    'sigma-0.01': _sigma_small,
    'denormal': _denormal,
})
LIST_NAMES = list(_LISTS)


@functools.lru_cache(maxsize=None)
def list_case(name):
    d = _LISTS[name]()
    conf, box = np.ascontiguousarray(d['conf'], F32), np.ascontiguousarray(d['box'], np.int32)
    conf.setflags(write=False)
    box.setflags(write=False)
    return dict(conf=conf, box=box, params=d['params'])


@functools.lru_cache(maxsize=None)
def list_expected(name, kind, mutant=None):
    """-> (order, scores) of the oracle"""
    d = list_case(name)
    return sr.soft_nms_boxes(d['conf'], d['box'], kind, *d['params'][kind], mutant=mutant)


# ---------------------------------------------------------------------------------------------------------------
# image level
# ---------------------------------------------------------------------------------------------------------------
def _full_frame():
    """anchors with offsets (0, 0, 100, 100) decode to the full frame whatever the anchor: identical boxes in two classes, among
    ordinary candidates"""
    rng = np.random.default_rng(3810)
    pred = dr.quiet_rows(rng, 2, dc.A300, 3)
    for img in range(2):
        for c in range(2):
            at = dr.plant(rng, pred, img, c, 40)
            pred[img, at[:12], 4:] = np.array([0, 0, 100, 100], F32)
        pred[img, 77, 0] = pred[img, 78, 0] = F32(0.5)      # equal scores on identical boxes
        pred[img, 77:79, 4:] = np.array([0, 0, 100, 100], F32)
    return pred


def _softmax1():
    return dc._softmax(3)[:1]


# name -> (builder, pname, thr, nms_top_k, keep_top_k, min_score (None = thr))
_IMAGES = {
    'full-frame': (_full_frame, 'vgg300', 0.01, 400, 200, None),
    'keep-top-k-50': (_softmax1, 'vgg300', 0.01, 400, 50, None),        # every class has more than keep_top_k picks
    'min-score-above-thr': (_softmax1, 'vgg300', 0.2, 300, 1024, 0.4),
    'min-score-below-thr': (_softmax1, 'vgg300', 0.2, 300, 1024, 0.05),
}
IMAGE_NAMES = list(dc.NAMES) + list(_IMAGES)


@functools.lru_cache(maxsize=None)
def image_case(name):
    """-> (pname, pred (read-only), thr, nms_top_k, keep_top_k, min_score)"""
    if name in _IMAGES:
        build, pname, thr, k, keep, min_score = _IMAGES[name]
        pred = np.ascontiguousarray(build(), F32)
        pred.setflags(write=False)
        return pname, pred, thr, k, keep, min_score
    return dc.case(name) + (None,)


@functools.lru_cache(maxsize=None)
def image_expected(name, kind, mutant=None):
    pname, pred, thr, k, keep, min_score = image_case(name)
    return [sr.detection_output(pred[i], dc.anchors(pname), thr, k, keep, kind, 0.45, 0.5, min_score, mutant) for i in range(pred.shape[0])]


# ---------------------------------------------------------------------------------------------------------------
# tiled: 2 pictures x 4 windows, 3 classes
# ---------------------------------------------------------------------------------------------------------------
TILED = ('vgg300', 0.01, 60, 150, 2)     # pname, thr, nms_top_k, keep_top_k, edge_margin


@functools.lru_cache(maxsize=None)
def tiled_case():
    """-> (pred [8, A, 8] read-only, tiles [(image, (x0, y0, w, h, interior), (W, H))]): four 500 x 500 windows of an 800 x 800
    picture and four 400 x 300 windows of a 600 x 450 one; per (window, class) 25..45 planted candidates on consecutive anchors
    (neighbours in a feature map: heavy overlap), so the per-class union of a picture exceeds nms_top_k, and a few confidences
    shared across windows"""
    rng = np.random.default_rng(3820)
    tiles = []
    for img, (W, H, w, h) in enumerate(((800, 800, 500, 500), (600, 450, 400, 300))):
        for j, y0 in enumerate((0, H - h)):
            for i, x0 in enumerate((0, W - w)):
                interior = (2 if i == 0 else 1) | (8 if j == 0 else 4)
                tiles.append((img, (x0, y0, w, h, interior), (W, H)))
    pred = dr.quiet_rows(rng, 8, dc.A300, 3)
    for t in range(8):
        for c in range(3):
            n = 25 + 10 * ((t + c) % 3)
            start = int(rng.integers(0, 5000))
            pred[t, start:start + n, c] = _confs(rng, n, 0.02, 0.9)
    pred[0, 100, 1] = pred[1, 100, 1] = pred[2, 50, 1] = F32(0.95)
    pred[3, 200:204, 2] = F32(0.9)                                        # equal scores on neighbouring (overlapping) anchors     # equal scores: lower tile, then lower anchor
    pred.setflags(write=False)
    return pred, tiles


@functools.lru_cache(maxsize=None)
def tiled_expected(kind, mutant=None):
    pname, thr, k, keep, m = TILED
    pred, tiles = tiled_case()
    return sr.detout_tiles_all(pred, tiles, dc.anchors(pname), thr, k, keep, m, kind=kind, mutant=mutant)
