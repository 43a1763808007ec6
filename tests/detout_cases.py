"""The inputs of tests/test_gpu_detection_output.py, built once per process, and their oracle results (tests/detout_ref.py),
computed once per case and shared by the tests that need them.  tests/test_detout_ref.py runs the mutants over the same cases.

A case is (pname, pred [b, A, C+5], thr, nms_top_k, keep_top_k).  The anchor count is the preset's, so the cases stay small in the
other dimensions: b <= 3, few classes wherever the class count is not the point, and with many classes a smaller nms_top_k (the
oracle's suppression is a Python loop per kept box: 127 classes at 400 take it 7 s)."""
import functools

import numpy as np

import detout_ref as dr
from oracle import boxes as ob

F32 = np.float32
A300, A512 = 8732, 24564


@functools.lru_cache(maxsize=None)
def anchors(pname):
    return ob.anchors(ob.get_preset(pname))


def _softmax(C, b=3, pname='vgg300', seed=0, spread=1.0):
    A = A300 if pname == 'vgg300' else A512
    rng = np.random.default_rng(1000 + 7 * C + seed)
    pred = dr.softmax_rows(rng, b, A, C, spread)
    pred[0, 5, C + 1:] = F32(150.0)          # offsets above the clamp
    pred[b - 1, A - 1, C + 3] = F32(101.0)
    return pred


def _sparse():
    """a few hundred pairs above the threshold in images 0 and 2, none in image 1; a value exactly at the threshold; anchors
    that carry two classes"""
    rng = np.random.default_rng(21)
    pred = dr.quiet_rows(rng, 3, A300, 3)
    for img, c, n in ((0, 0, 150), (0, 1, 90), (0, 2, 70), (2, 1, 130), (2, 2, 40)):
        dr.plant(rng, pred, img, c, n)
    pred[0, 4000, 0] = F32(0.01)             # !(conf < thr): a candidate
    pred[0, 4000, 2] = F32(0.5)              # the same anchor under another class
    pred[2, 17, 1] = pred[2, 17, 2] = F32(0.7)
    return pred


def _all_equal():
    """every confidence of class 1 equal, in both images: the kept set is the lowest nms_top_k anchors"""
    rng = np.random.default_rng(22)
    pred = dr.quiet_rows(rng, 2, A300, 3)
    pred[:, :, 1] = F32(0.25)
    dr.plant(rng, pred, 1, 0, 30)
    return pred


def _counts(k, seed=39):
    """exactly k - 1, k and k + 1 candidates of class 0 in images 0, 1, 2 (a seed with which the k-th and the (k+1)-th survive
    the suppression, so that a cut one too early or too late shows in the output)"""
    rng = np.random.default_rng(seed)
    pred = dr.quiet_rows(rng, 3, A300, 3)
    for img, n in ((0, k - 1), (1, k), (2, k + 1)):
        dr.plant(rng, pred, img, 0, n)
    return pred


def _cut_ties(k):
    """exactly k + 5 candidates of class 2, the last 10 of them sharing the cut value: the 5 lowest anchors of the 10 stay"""
    rng = np.random.default_rng(24)
    pred = dr.quiet_rows(rng, 1, A300, 3)
    values = np.unique(rng.uniform(0.3, 0.9, 4 * k).astype(F32))[:k - 5]
    rng.shuffle(values)
    dr.plant(rng, pred, 0, 2, k + 5, values=np.concatenate([values, np.full(10, 0.125, F32)]))
    return pred


def _final_ties():
    """300 candidates per class; the best confidence shared by (anchor 6000, class 0) and (anchor 200, class 2), the next by
    two classes of anchor 3000, the next by two anchors of class 1"""
    rng = np.random.default_rng(25)
    pred = dr.quiet_rows(rng, 1, A300, 3)
    for c in range(3):
        dr.plant(rng, pred, 0, c, 300, lo=0.02, hi=0.8)
    pred[0, 6000, 0] = pred[0, 200, 2] = F32(0.95)
    pred[0, 3000, 0] = pred[0, 3000, 1] = F32(0.93)
    pred[0, 100, 1] = pred[0, 8000, 1] = F32(0.91)
    return pred


def _one_class():
    """one class, 300 candidates (<= nms_top_k): the argmax path sees the same candidates"""
    rng = np.random.default_rng(26)
    pred = dr.quiet_rows(rng, 2, A300, 1)
    dr.plant(rng, pred, 0, 0, 300)
    dr.plant(rng, pred, 1, 0, 64)
    pred[0, 9, 0] = F32(0.6)
    pred[0, 9, 2:] = F32(150.0)          # offsets above the clamp
    return pred


# name -> (builder of pred, pname, thr, nms_top_k, keep_top_k)
_CASES = {
    'softmax-C1': (lambda: _softmax(1), 'vgg300', 0.01, 400, 200),
    'softmax-C3': (lambda: _softmax(3), 'vgg300', 0.01, 400, 200),
    'softmax-C27': (lambda: _softmax(27), 'vgg300', 0.01, 150, 200),
    'softmax-C28': (lambda: _softmax(28), 'vgg300', 0.01, 150, 200),
    'softmax-C127': (lambda: _softmax(127, spread=1.5), 'vgg300', 0.01, 100, 200),
    'softmax-vgg512-C3': (lambda: _softmax(3, b=1, pname='vgg512'), 'vgg512', 0.01, 400, 200),
    'sparse': (_sparse, 'vgg300', 0.01, 400, 1024),      # (every survivor is output: the one at the threshold too)
    'thr-0': (lambda: _softmax(2, b=2, seed=1), 'vgg300', 0.0, 400, 200),
    'thr-above-all': (lambda: _softmax(2, b=2, seed=1), 'vgg300', 1.5, 400, 200),
    'all-equal': (_all_equal, 'vgg300', 0.01, 400, 1024),
    'counts-k-1-k-k+1': (lambda: _counts(400), 'vgg300', 0.01, 400, 1024),
    'cut-ties': (lambda: _cut_ties(400), 'vgg300', 0.01, 400, 1024),
    'nms-top-k-1': (lambda: _softmax(3)[:1], 'vgg300', 0.01, 1, 200),
    'nms-top-k-1024': (lambda: _softmax(3)[:1], 'vgg300', 0.01, 1024, 200),
    'keep-top-k-1': (_final_ties, 'vgg300', 0.01, 400, 1),
    'keep-top-k-2': (_final_ties, 'vgg300', 0.01, 400, 2),
    'keep-top-k-200': (_final_ties, 'vgg300', 0.01, 400, 200),
    'keep-top-k-1024': (_final_ties, 'vgg300', 0.01, 400, 1024),
    'one-class': (_one_class, 'vgg300', 0.01, 400, 200),
}
NAMES = list(_CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (pname, pred, thr, nms_top_k, keep_top_k); pred is read-only"""
    build, pname, thr, k, keep = _CASES[name]
    pred = np.ascontiguousarray(build(), F32)
    pred.setflags(write=False)
    return pname, pred, thr, k, keep


@functools.lru_cache(maxsize=None)
def expected(name, mutant=None):
    """the oracle's result for every image of the case"""
    pname, pred, thr, k, keep = case(name)
    return [dr.detection_output(pred[i], anchors(pname), thr, k, keep, mutant) for i in range(pred.shape[0])]
