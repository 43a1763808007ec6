"""The inputs of tests/test_gpu_tiledet.py, built once per process, and their oracle results (tests/tiledet_ref.py), computed once
per case and shared.  tests/test_tiledet_ref.py runs the mutants over the same cases on the CPU.

A case is (pname, pred [n_tiles, A, C+5], tiles [(image, (x0, y0, w, h, interior), (W, H))], thr, nms_top_k, keep_top_k,
edge_margin).  The presets fix A, so the cases stay small in tiles x classes."""
import functools

import numpy as np

import detout_ref as dr
import tiles_ref as tr
import tiledet_ref as R
from oracle import boxes as ob

F32 = np.float32
A300 = 8732
W, H = 1000, 700


@functools.lru_cache(maxsize=None)
def anchors(pname):
    return ob.anchors(ob.get_preset(pname))


@functools.lru_cache(maxsize=None)
def anchors_abs(pname):
    return ob.anchors_abs(anchors(pname))


def _second_class(pred):
    """every other hot anchor also speaks for a second class, 2/64 below its first: anchors that carry two classes, boxes of
    different classes that coincide, more ties"""
    C = pred.shape[2] - 5
    for t in range(pred.shape[0]):
        hot = np.nonzero(pred[t, :, :C].max(1) > 0)[0]
        for a in hot[::2]:
            c = int(np.argmax(pred[t, a, :C]))
            pred[t, a, (c + 7) % C] = pred[t, a, c] - F32(2 / 64)
    return pred


def _scene(pname='vgg300', size=(W, H), seed=5, n_objects=25, image=0):
    pred, tiles, _ = tr.planted_scene(pname, size, 400, 0.25, n_objects, 20, seed)
    return _second_class(pred), [(image, tuple(t), size) for t in tiles]


def _two_pictures():
    p0, t0 = _scene()
    p1, t1 = _scene(size=(700, 400), seed=9, n_objects=12, image=1)
    return np.concatenate([p0, p1], 0), t0 + t1


def _rules():
    """One 800 x 400 picture: the left half (its right edge interior), the right half (its left edge interior), the whole.  Four
    classes, nms_top_k = 4; every box has one hot anchor.
    class 3, tile 0: A (0.9) touches the right edge and is dropped; B (0.8) overlaps A without touching: it survives, unless A
      suppresses it inside the tile first; four lone boxes at 0.7, 0.65, 0.5, 0.4: the cut keeps A, B, 0.7, 0.65, the drop leaves
      three -- a drop before the cut lets 0.5 in.
    class 1: lone boxes 0.9 (tile 0), 0.8 (tile 2), then three at 0.75: one low in tile 0 (a high anchor), two high up in tile 1 (low
      anchors), and 0.3 in tile 2: the picture's cut at 4 keeps tile 0's 0.75 and the lower anchor of tile 1's.
    class 2 and class 0 in tile 1 at 0.6: (low anchor, class 2) comes before (high anchor, class 0)."""
    pname = 'vgg300'
    anch, aabs = anchors(pname), anchors_abs(pname)
    size = (800, 400)
    tiles = [(0, 0, 400, 400, 2), (400, 0, 400, 400, 1), (0, 0, 800, 400, 0)]
    pred = np.zeros((3, A300, 9), F32)
    pred[:, :, 4] = 1

    def put(t, part, c, conf):
        tr.plant(pred[t], anch, aabs, part, c, [F32(conf)])

    put(0, (800, 999, 100, 300), 3, 0.9)
    put(0, (780, 985, 100, 300), 3, 0.8)
    for j, cf in enumerate((0.7, 0.65, 0.5, 0.4)):
        put(0, (50 + 150 * j, 150 + 150 * j, 500, 600), 3, cf)
    put(0, (100, 200, 350, 450), 1, 0.9)
    put(2, (850, 950, 700, 900), 1, 0.8)
    put(0, (300, 400, 800, 900), 1, 0.75)
    put(1, (300, 400, 50, 150), 1, 0.75)
    put(1, (600, 700, 50, 150), 1, 0.75)
    put(2, (600, 650, 100, 300), 1, 0.3)
    put(1, (100, 200, 300, 400), 2, 0.6)
    put(1, (500, 600, 700, 800), 0, 0.6)
    return pred, [(0, t, size) for t in tiles]


def _classes(C, seed):
    """3 tiles of a 700 x 400 picture, C classes: quiet rows plus planted candidates (random anchors, so random boxes) in a few
    classes of every tile, more than nms_top_k = 30 in one of them"""
    rng = np.random.default_rng(seed)
    size = (700, 400)
    tiles = tr.plan_tiles_ref(size[0], size[1], 400)
    assert len(tiles) == 3
    pred = dr.quiet_rows(rng, 3, A300, C)
    for t in range(3):
        for c in sorted({0, C // 2, C - 1}):
            dr.plant(rng, pred, t, c, 60 if (t, c) == (1, 0) else 25)
    return pred, [(0, tuple(t), size) for t in tiles]


def _empty_and_dropped():
    """picture 0 has no candidate; every candidate of picture 1 touches an interior edge; picture 2 has one that stays"""
    pname = 'vgg300'
    anch, aabs = anchors(pname), anchors_abs(pname)
    pred = np.zeros((4, A300, 7), F32)
    pred[:, :, 2] = 1
    tiles = [(0, (0, 0, 300, 300, 0), (300, 300)), (1, (0, 0, 200, 200, 2), (400, 200)), (1, (200, 0, 200, 200, 1), (400, 200)),
             (2, (0, 0, 300, 300, 0), (300, 300))]
    tr.plant(pred[1], anch, aabs, (700, 999, 200, 500), 0, [F32(0.9), F32(0.8)])
    tr.plant(pred[2], anch, aabs, (0, 300, 200, 500), 1, [F32(0.7)])
    tr.plant(pred[3], anch, aabs, (0, 300, 200, 500), 1, [F32(0.7)])
    return pred, tiles


def _many_tiles():
    """256 tiles (16 x 16 windows of 100 pixels) of one picture, one class, a handful of candidates in a few tiles, the last
    one included; nms_top_k = 3 makes the picture's cut search all 256 lists"""
    pname = 'vgg300'
    anch, aabs = anchors(pname), anchors_abs(pname)
    size = (1600, 1600)
    tiles = []
    for j in range(16):
        for i in range(16):
            interior = (1 if i > 0 else 0) | (2 if i < 15 else 0) | (4 if j > 0 else 0) | (8 if j < 15 else 0)
            tiles.append((0, (100 * i, 100 * j, 100, 100, interior), size))
    pred = np.zeros((256, A300, 6), F32)
    pred[:, :, 1] = 1
    for t, conf in ((0, 0.5), (17, 0.75), (100, 0.75), (101, 0.25), (254, 0.5), (255, 0.75), (255, 0.625)):
        part = (200, 500, 300, 600) if conf != 0.625 else (600, 900, 300, 600)
        tr.plant(pred[t], anch, aabs, part, 0, [F32(conf)])
    return pred, tiles


# name -> (builder of (pred, tiles), pname, thr, nms_top_k, keep_top_k, edge_margin)
_CASES = {
    'scene': (_scene, 'vgg300', 0.01, 400, 200, 2),
    'scene-k8-keep5': (_scene, 'vgg300', 0.01, 8, 5, 2),
    'scene-no-edge-drop': (_scene, 'vgg300', 0.01, 400, 200, -1),
    'rules': (_rules, 'vgg300', 0.01, 4, 200, 2),
    'one-class': (lambda: _classes(1, 31), 'vgg300', 0.01, 30, 200, 2),
    'classes-127': (lambda: _classes(127, 32), 'vgg300', 0.01, 30, 200, 2),
    'vgg512': (lambda: _scene('vgg512', (700, 400), 11, 10), 'vgg512', 0.01, 400, 200, 2),
    'two-pictures': (_two_pictures, 'vgg300', 0.01, 400, 200, 2),
    'empty-and-dropped': (_empty_and_dropped, 'vgg300', 0.01, 400, 200, 2),
    'tiles-256': (_many_tiles, 'vgg300', 0.01, 3, 200, 2),
}
NAMES = list(_CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (pname, pred, tiles, thr, nms_top_k, keep_top_k, edge_margin); pred is read-only"""
    build, pname, thr, k, keep, m = _CASES[name]
    pred, tiles = build()
    pred = np.ascontiguousarray(pred, F32)
    pred.setflags(write=False)
    return pname, pred, tiles, thr, k, keep, m


@functools.lru_cache(maxsize=None)
def expected(name, mutant=None):
    """the oracle's result for every picture of the case"""
    pname, pred, tiles, thr, k, keep, m = case(name)
    return R.detout_tiles_all(pred, tiles, anchors(pname), thr, k, keep, m, mutant)
