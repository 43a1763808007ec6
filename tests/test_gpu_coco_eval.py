"""-m gpu: COCO's box evaluation on the GPU -- ssd_coco_eval, the accumulator's _coco calls and the two evaluator classes against
the float64 oracle of tests/coco_ref.py (which is written per image and accumulates, where the kernel walks each class once),
and the drivers' --ap-protocol coco.  Every comparison is np.array_equal on float64."""
import ctypes as C
import functools
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ap_ref
import coco_ref as R
import test_coco_ref as H
import test_gpu_ap_device as D
from ssd_tensorflow_amd import average_precision as apm, coco_eval as ce, ssdutils as su
from ssd_tensorflow_amd._lib import lib, check, np_ptr
from ssd_tensorflow_amd.utils import Box, FlaggedBox, Size, abs2prop, prop2abs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = Size(1000, 1000)
THRESHOLDS = {1: (0.5,), 3: (0.5, 0.75, 0.95), 10: tuple(float(v) for v in np.linspace(0.5, 0.95, 10))}


def gpu_eval(det_box, det_conf, det_cls, det_sample, gt_box, gt_cls, gt_sample, gt_flags, gt_area, sample_scale, ncls, thresholds):
    db = np.ascontiguousarray(det_box, np.float32).reshape(-1, 4); dc = np.ascontiguousarray(det_conf, np.float32)
    dk = np.ascontiguousarray(det_cls, np.int32); ds = np.ascontiguousarray(det_sample, np.int32)
    gb = np.ascontiguousarray(gt_box, np.float64).reshape(-1, 4); gk = np.ascontiguousarray(gt_cls, np.int32)
    gs = np.ascontiguousarray(gt_sample, np.int32); gf = np.ascontiguousarray(gt_flags, np.uint8)
    ga = np.ascontiguousarray(gt_area, np.float64); sc = np.ascontiguousarray(sample_scale, np.float64)
    thr = np.ascontiguousarray(thresholds, np.float64)
    ap = np.full((4, len(thr), ncls), 7.0); ar = np.full((6, len(thr), ncls), 7.0); present = np.full((4, ncls), 7, np.int32)
    check(lib.ssd_coco_eval(0, len(dc), np_ptr(db), np_ptr(dc), np_ptr(dk), np_ptr(ds), len(gk), np_ptr(gb), np_ptr(gk), np_ptr(gs), np_ptr(gf),
                            np_ptr(ga), len(sc), np_ptr(sc), ncls, len(thr), np_ptr(thr), np_ptr(ap), np_ptr(ar), np_ptr(present)))
    return ap, ar, present


def gpu_eval_set(s, thresholds):
    return gpu_eval(s['det_box'], s['det_conf'], s['det_cls'], s['det_sample'], s['gt_box'], s['gt_cls'], s['gt_sample'], s['gt_flags'],
                    s['gt_area'], s['sample_scale'], s['ncls'], thresholds)


def assert_same(got, want):
    for name, g, w in zip(('ap', 'ar', 'present'), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


# ------------------------------------------------------------------------------------- 1. the hand-worked cases
def test_hand_worked_cases_through_the_kernel(monkeypatch):
    """every case of tests/test_coco_ref.py again, its oracle call doubled by ssd_coco_eval on the same arrays"""
    oracle = R.evaluate
    calls = []

    def both(*args, mutate=None, details=None):
        want = oracle(*args, details=details)
        assert_same(gpu_eval(*args), want)
        calls.append(len(args[1]))
        return want
    monkeypatch.setattr(R, 'evaluate', both)
    for case, want in H.CASES.items():
        assert case() == want
    H.test_class_with_only_crowd_boxes_is_not_present()
    H.test_empty_evaluation_gives_minus_one()
    H.test_summary_numbers_on_two_classes()
    assert len(calls) == len(H.CASES) + 3 and max(calls) == 101 and min(calls) == 0


# ------------------------------------------------------------------------------------- 2. a crafted set
@functools.lru_cache(maxsize=None)
def crafted():
    """3 classes, 6 images (sizes mixed).  Class 0: 130 detections in image 0 (past the cap of 100 and the 64 lanes) with duplicate
    boxes, exactly 100 in image 1, a crowd box under 5 detections in image 2, annotated areas of exactly 1024 and 9216, a
    zero-width detection, detections in image 3, which has no ground truth; confidences from 16 values, so they repeat within and
    across images.  Class 1: ground truth, no detection.  Class 2: only crowd boxes, with detections."""
    rng = np.random.default_rng(11)
    sizes = [(640, 480), (500, 375), (1000, 1000), (640, 480), (333, 500), (640, 427)]
    gt = []            # (box, cls, sample, flags, area)
    det = []           # (box, cls, sample)
    dup = (100, 300, 100, 300)
    gt += [(dup, 0, 0, 0, 1024.0), (dup, 0, 0, 0, 9216.0), ((400, 700, 400, 800), 0, 0, 0, 30000.0), ((10, 60, 10, 50), 0, 0, 0, 400.0)]
    for i in range(130):
        base = (dup, (400, 700, 400, 800), (10, 60, 10, 50), (600, 900, 20, 200))[i % 4]
        j = rng.integers(-12, 13, 4) if i % 3 else np.zeros(4, np.int64)
        det.append((tuple(int(v) for v in np.array(base) + j), 0, 0))
    gt += [((200, 500, 200, 600), 0, 1, 0, 9216.0), ((200, 500, 200, 600), 0, 1, 1, 5000.0), ((600, 800, 600, 800), 1, 1, 0, 2000.0)]
    for i in range(100):
        j = rng.integers(-40, 41, 4)
        det.append((tuple(int(v) for v in np.array((200, 500, 200, 600)) + j), 0, 1))
    gt += [((0, 400, 0, 400), 0, 2, 3, 50000.0), ((500, 700, 500, 700), 0, 2, 0, 1024.0), ((0, 300, 500, 900), 2, 2, 3, 8000.0)]
    for i in range(5):
        det.append(((20 + 60 * i, 80 + 60 * i, 30, 120), 0, 2))
    det += [((500, 700, 500, 700), 0, 2), ((510, 700, 500, 690), 0, 2), ((300, 300, 100, 200), 0, 2), ((10, 200, 520, 800), 2, 2)]
    det += [((100, 300, 100, 300), 0, 3), ((0, 50, 0, 50), 2, 3)]                              # image 3: no ground truth
    gt += [((100, 200, 100, 200), 1, 4, 0, 1500.0), ((50, 950, 50, 950), 0, 4, 0, 120000.0)]
    det += [((60, 940, 60, 960), 0, 4), ((50, 950, 50, 950), 0, 4)]
    gt += [((700, 900, 100, 300), 2, 5, 3, 900.0)]
    det += [((700, 900, 100, 300), 2, 5), ((0, 1000, 0, 1000), 0, 5)]
    conf = (rng.integers(1, 17, len(det)) / 16.0).astype(np.float32)
    gt.sort(key=lambda g: g[2])
    return dict(det_box=np.array([d[0] for d in det], np.float32), det_conf=conf, det_cls=np.array([d[1] for d in det], np.int32),
                det_sample=np.array([d[2] for d in det], np.int32), gt_box=np.array([g[0] for g in gt], np.float64),
                gt_cls=np.array([g[1] for g in gt], np.int32), gt_sample=np.array([g[2] for g in gt], np.int32),
                gt_flags=np.array([g[3] for g in gt], np.uint8), gt_area=np.array([g[4] for g in gt], np.float64),
                sample_scale=np.array([w * h / 1e6 for w, h in sizes]), ncls=3)


@pytest.mark.parametrize('n_thr', [1, 10])
def test_crafted_set(n_thr):
    s = crafted()
    per = {(int(k), int(i)): int(np.count_nonzero((s['det_cls'] == k) & (s['det_sample'] == i))) for k in range(3) for i in range(6)}
    assert per[(0, 0)] == 130 and per[(0, 1)] == 100 and not (s['det_cls'] == 1).any() and len(np.unique(s['det_conf'])) <= 16
    assert ((s['det_box'][:, 0] == s['det_box'][:, 1])).any() and not (s['gt_sample'] == 3).any()
    want = R.evaluate_set(s, THRESHOLDS[n_thr])
    ap, ar, present = want
    assert present[:, 2].tolist() == [0, 0, 0, 0] and present[:, 1].tolist() == [1, 0, 1, 0] and present[:, 0].tolist() == [1, 1, 1, 1]
    assert 0.05 < ap[0, 0, 0] < 0.95 and (ar[0, :, 1] == 0.0).all() and ar[4, 0, 0] < ar[5, 0, 0] <= ar[0, 0, 0]
    assert_same(gpu_eval_set(s, THRESHOLDS[n_thr]), want)


def test_no_detections():
    s = dict(crafted())
    for k in ('det_box', 'det_conf', 'det_cls', 'det_sample'):
        s[k] = s[k][:0]
    want = R.evaluate_set(s, THRESHOLDS[3])
    assert (want[0][0][:, :2] == 0.0).all() and (want[0][0][:, 2] == -1.0).all()
    assert_same(gpu_eval_set(s, THRESHOLDS[3]), want)


@functools.lru_cache(maxsize=None)
def crafted_many_rows():
    """Images with more than 64 ground-truth rows: the walk stages an image's rows 64 at a time, and past 64 it restages every
    chunk in both of its passes.  3 classes, 3 images.  Image 0 has 70 rows (chunks of 64 + 6), image 1 has 130 (64 + 64 + 2),
    image 2 has 64 exactly (the last size of the single-chunk path); classes mixed, class 0 in every chunk.  In image 0, for class 0:
      row 3 (chunk 0) is a FLAGGED copy of the first detection (IoU 1), row 66 (chunk 1) an ordinary box with IoU 0.6: the match;
      rows 6 (chunk 0) and 69 (chunk 1) are the two halves of the second detection, IoU 0.5 each: the later one is matched, and
      the third detection, that half itself, finds it taken;
      row 67 (chunk 1) is a crowd region with three detections inside.
    In image 1 the rows 63 | 64 and 127 | 128 are the same box of the same class on both sides of a chunk boundary, 5 % of the
    rows are crowd, and the annotated areas spread over all ranges, so which rows a lane ignores differs from lane to lane."""
    rng = np.random.default_rng(64)
    sizes = [(1000, 1000), (640, 480), (500, 375)]
    gt, det, conf = [], [], []                       # (box, cls, sample, flags, area); (box, cls, sample); confidence
    rows = [((10 * i, 10 * i + 8, 5 * (i % 7), 5 * (i % 7) + 9), i % 3, 0, 0, 72.0) for i in range(70)]      # fillers above y = 50
    first, second = (100, 200, 100, 160), (400, 500, 400, 500)
    rows[3] = (first, 0, 0, 1, 20000.0)
    rows[66] = ((100, 200, 100, 200), 0, 0, 0, 20000.0)
    rows[6] = ((400, 500, 400, 450), 0, 0, 0, 20000.0)
    rows[69] = ((400, 500, 450, 500), 0, 0, 0, 20000.0)
    rows[67] = ((600, 900, 600, 900), 0, 0, 3, 50000.0)
    gt += rows
    det += [(first, 0, 0), (second, 0, 0), ((400, 500, 450, 500), 0, 0), ((620, 700, 620, 700), 0, 0), ((710, 800, 620, 700), 0, 0),
            ((620, 700, 710, 800), 0, 0)]
    conf += [0.99, 0.98, 0.97, 0.96, 0.95, 0.94]
    for i in (0, 9, 30, 63, 64, 65, 68, 1, 2, 61, 62):                                       # fillers of every class, in both chunks
        det.append((rows[i][0], rows[i][1], 0)); conf.append(0.5 + 0.005 * (i % 16))
    for n_rows, s in ((130, 1), (64, 2)):
        img = []
        for i in range(n_rows):
            area = float(10.0 ** rng.uniform(1, 5))
            side = max(3, int(np.sqrt(area / (sizes[s][0] * sizes[s][1] / 1e6))))
            x0, y0 = (int(v) for v in rng.integers(0, 1000 - side, 2))
            img.append(((x0, x0 + side, y0, y0 + side), int(rng.integers(0, 3)), s, 3 if rng.random() < 0.05 else 0, area))
        if n_rows == 130:
            for i in (63, 127):
                img[i] = (img[i][0], 0, s, 0, img[i][4])                                     # class 0, not crowd
                img[i + 1] = img[i]
        gt += img
        for _ in range(150 if n_rows == 130 else 40):
            g = img[int(rng.integers(0, n_rows))]
            w = g[0][1] - g[0][0]
            j = rng.integers(-1, 2, 4) * rng.integers(0, max(2, w // 6), 4) if rng.random() < 0.7 else np.zeros(4, np.int64)
            det.append((tuple(int(v) for v in np.array(g[0]) + j), g[1] if rng.random() < 0.9 else int(rng.integers(0, 3)), s))
            conf.append(float(rng.integers(1, 60)) / 64.0)
        if n_rows == 130:
            for i in (63, 64, 127, 128, 129):                                                # both copies of a pair get a detection
                det.append((img[i][0], img[i][1], s)); conf.append(0.93)
    return dict(det_box=np.array([d[0] for d in det], np.float32), det_conf=np.array(conf, np.float32), det_cls=np.array([d[1] for d in det], np.int32),
                det_sample=np.array([d[2] for d in det], np.int32), gt_box=np.array([g[0] for g in gt], np.float64),
                gt_cls=np.array([g[1] for g in gt], np.int32), gt_sample=np.array([g[2] for g in gt], np.int32),
                gt_flags=np.array([g[3] for g in gt], np.uint8), gt_area=np.array([g[4] for g in gt], np.float64),
                sample_scale=np.array([w * h / 1e6 for w, h in sizes]), ncls=3)


@pytest.mark.parametrize('n_thr', [1, 10])
def test_images_with_more_than_64_rows(n_thr):
    s = crafted_many_rows()
    assert np.bincount(s['gt_sample']).tolist() == [70, 130, 64] and (np.diff(s['gt_sample']) >= 0).all()
    for img, cuts in ((0, (0, 64, 70)), (1, (0, 64, 128, 130))):                             # every class in every chunk
        k = s['gt_cls'][s['gt_sample'] == img]
        assert all((k[a:b] == 0).any() for a, b in zip(cuts, cuts[1:])) and all(len(set(k[a:b].tolist())) == 3 for a, b in zip(cuts, cuts[1:]) if b - a > 2)
    in1 = np.nonzero(s['gt_sample'] == 1)[0]
    assert (s['gt_box'][in1[63]] == s['gt_box'][in1[64]]).all() and (s['gt_box'][in1[127]] == s['gt_box'][in1[128]]).all()
    assert (s['gt_flags'][in1[64:]] == 3).any()                                              # crowd rows behind the first chunk
    details = {}
    want = R.evaluate_set(s, THRESHOLDS[n_thr], details=details)
    # class 0, range all, IoU 0.5: the non-ignored match of chunk 1 is kept; the later half wins the tie; its own detection finds
    # it taken; three detections in the crowd region
    assert ''.join(details[(0, 0, 0)][:6]) == 'TTFIII'
    assert want[2].all() and 0.05 < want[0][0, 0].min() and want[0][0, 0].max() < 0.95
    assert_same(gpu_eval_set(s, THRESHOLDS[n_thr]), want)


# ------------------------------------------------------------------------------------- 3. random sets
@functools.lru_cache(maxsize=None)
def random_set(ncls, nimg, n_det):
    s = R.random_set(np.random.default_rng(ncls * 1000 + nimg), ncls, nimg, n_det, crowd_rate=0.05)
    assert len(s['det_conf']) == n_det
    return s


@functools.lru_cache(maxsize=None)
def random_oracle(ncls, nimg, n_det, n_thr):
    return R.evaluate_set(random_set(ncls, nimg, n_det), THRESHOLDS[n_thr])


@pytest.mark.parametrize('n_thr', [1, 3, 10])
@pytest.mark.parametrize('shape', [(1, 3, 50), (20, 16, 2000), (127, 40, 6000)])
def test_random_sets(shape, n_thr):
    s = random_set(*shape)
    want = random_oracle(*shape, n_thr)
    assert_same(gpu_eval_set(s, THRESHOLDS[n_thr]), want)
    if shape[0] == 20:
        assert (s['gt_flags'] == 3).any() and want[2][1:].sum() > 10 and want[0][0][want[0][0] >= 0].max() > 0.3


# ------------------------------------------------------------------------------------- 4. the accumulator and the classes
SIZES = [Size(640, 480), Size(500, 375), Size(1000, 1000), Size(333, 500)]


def coco_passes(seed, b, out_cap, n_pass, ncls, bad_cls=()):
    """test_gpu_ap_device's passes, their ground truth turned into COCO's: areas on most boxes, some crowd, image sizes mixed"""
    rng = np.random.default_rng(seed + 1)
    out = []
    for slots, gts in D.make_passes(seed, b, out_cap, n_pass, ncls, flag_rate=0.1, bad_cls=bad_cls):
        sizes = [SIZES[int(rng.integers(0, len(SIZES)))] for _ in range(b)]
        new = []
        for gt, size in zip(gts, sizes):
            row = []
            for g in gt:
                u = rng.random()
                px = g.size.w * size.w * g.size.h * size.h
                if u < 0.15:
                    g = FlaggedBox(*g, crowd=True, area=px * 0.7)
                elif u < 0.8:
                    g = FlaggedBox(*g, getattr(g, 'difficult', False), area=float(10.0 ** rng.uniform(1, 5)))
                row.append(g)
            new.append(row)
        out.append((slots, new, sizes))
    return out


def feed_device(calc, passes, b, out_cap):
    keep = []
    for slots, gts, sizes in passes:
        t = {k: torch.from_numpy(v).cuda() for k, v in slots.items()}
        keep.append(t)
        calc.add_pass((t['count'].data_ptr(), t['conf'].data_ptr(), t['cls'].data_ptr(), t['box'].data_ptr(), b, out_cap), gts, sizes)
    return keep


def feed_host(calc, passes, out_cap):
    for slots, gts, sizes in passes:
        for i, gt in enumerate(gts):
            n = min(int(slots['count'][i]), out_cap)
            det = dict(conf=slots['conf'][i, :n], cls=slots['cls'][i, :n], box=slots['box'][i, :n])
            calc.add_detections(gt, su.boxes_from_detection(det, D.NAMES), sizes[i])


def arrays_of_passes(passes, out_cap, ncls):
    """the arrays the oracle takes, and the number of out-of-range class ids"""
    db, dc, dk, ds, gb, gk, gs, gf, ga, sc = [], [], [], [], [], [], [], [], [], []
    bad = 0
    for slots, gts, sizes in passes:
        for i, gt in enumerate(gts):
            sample = len(sc)
            sc.append(sizes[i].w * sizes[i].h / 1e6)
            for g in gt:
                gb.append(prop2abs(g.center, g.size, IMG)); gk.append(g.labelid); gs.append(sample)
                gf.append(3 if getattr(g, 'crowd', False) else int(getattr(g, 'difficult', False)))
                area = getattr(g, 'area', None)
                ga.append((g.size.w * sizes[i].w) * (g.size.h * sizes[i].h) if area is None else area)
            for j in range(min(int(slots['count'][i]), out_cap)):
                if 0 <= slots['cls'][i, j] < ncls:
                    db.append(D.roundtrip(slots['box'][i, j])); dc.append(slots['conf'][i, j]); dk.append(slots['cls'][i, j]); ds.append(sample)
                else:
                    bad += 1
    return dict(det_box=np.array(db, np.float32).reshape(-1, 4), det_conf=np.array(dc, np.float32), det_cls=np.array(dk, np.int32),
                det_sample=np.array(ds, np.int32), gt_box=np.array(gb, np.float64).reshape(-1, 4), gt_cls=np.array(gk, np.int32),
                gt_sample=np.array(gs, np.int32), gt_flags=np.array(gf, np.uint8), gt_area=np.array(ga, np.float64),
                sample_scale=np.array(sc, np.float64), ncls=ncls), bad


def same_result(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ('ap', 'ar', 'present', 'thresholds')) and a['labels'] == b['labels']


def test_accumulator_and_both_evaluators_against_the_oracle():
    b, out_cap, ncls = 5, 40, 20
    passes = coco_passes(21, b, out_cap, 4, ncls, bad_cls=(20, -1))
    s, bad = arrays_of_passes(passes, out_cap, ncls)
    assert bad > 0 and (s['gt_flags'] == 3).any() and (s['gt_flags'] == 1).any() and len(s['det_conf']) > 300
    want = R.evaluate_set(s)
    host = ce.COCOEvaluator(num_classes=ncls)
    feed_host(host, passes, out_cap)
    calc = ce.DeviceCOCOEvaluator(0, ncls)
    keep = feed_device(calc, passes[:3], b, out_cap)                     # three passes through ssd_ap_add_dev_coco ...
    other = ce.DeviceCOCOEvaluator(0, ncls)
    keep += feed_device(other, passes[3:], b, out_cap)
    calc.merge(pickle.loads(pickle.dumps(other.state())))                # ... and one through ssd_ap_add_host_coco
    got, got_host = calc.compute(), host.compute()
    assert_same((got['ap'], got['ar'], got['present']), want)
    assert same_result(got, got_host)
    assert calc.num_detections() == len(s['det_conf'])
    assert calc.num_dropped() + other.num_dropped() == bad == host.dropped
    assert calc.summary() == host.summary() == R.summarize(*want) and list(calc.summary()) == list(ce.SUMMARY_NAMES)
    assert list(calc.compute_aps().items()) == list(host.compute_aps().items()) and len(calc.compute_aps()) > 3
    assert calc.compute_aps() == {label: float(np.mean(want[0][0][:, k])) for label, k in got['labels'].items() if want[2][0, k]}
    assert ce.format_summary(calc.summary()).count('\n') == 11
    # the VOC protocols on the same accumulator: a crowd box is a flagged box
    thr = np.ascontiguousarray(THRESHOLDS[10]); ap = np.zeros((10, ncls)); present = np.zeros(ncls, np.int32)
    n = C.c_longlong(); dropped = C.c_longlong()
    check(lib.ssd_ap_compute(calc._acc, 2, 10, np_ptr(thr), np_ptr(ap), np_ptr(present), C.byref(n), C.byref(dropped)))
    want_ap, want_present = ap_ref.compute(s['det_box'], s['det_conf'], s['det_cls'], s['det_sample'], s['gt_box'], s['gt_cls'], s['gt_sample'],
                                           s['gt_flags'], ncls=ncls, protocol=ap_ref.VOC12, minoverlaps=THRESHOLDS[10])
    assert np.array_equal(ap, want_ap) and np.array_equal(present, want_present) and n.value == len(s['det_conf'])
    # a host evaluator merged from states gives the same
    merged = ce.COCOEvaluator(num_classes=ncls)
    merged.merge(pickle.loads(pickle.dumps(host.state())))
    assert same_result(merged.compute(), got_host)
    # clear, then reuse with other passes and other thresholds
    calc.clear(); host.clear()
    assert calc.num_detections() == 0 and all(v == -1.0 for v in calc.summary().values())
    again = coco_passes(5, b, out_cap, 2, ncls)
    calc.thresholds = host.thresholds = np.ascontiguousarray(THRESHOLDS[3])
    keep += feed_device(calc, again, b, out_cap)
    feed_host(host, again, out_cap)
    s2, _ = arrays_of_passes(again, out_cap, ncls)
    got2 = calc.compute()
    assert_same((got2['ap'], got2['ar'], got2['present']), R.evaluate_set(s2, THRESHOLDS[3]))
    assert same_result(got2, host.compute()) and calc.summary()['AP75'] != -1.0
    calc.close(); other.close()


def test_plain_pass_bars_the_coco_computation():
    b, out_cap, ncls = 3, 10, 20
    passes = D.make_passes(2, b, out_cap, 1, ncls)
    plain = apm.DeviceAPCalculator(0, ncls, 'voc12')
    keep = D.feed_device(plain, passes, b, out_cap)
    thr = np.ascontiguousarray(THRESHOLDS[1]); ap = np.zeros((4, 1, ncls)); ar = np.zeros((6, 1, ncls)); present = np.zeros((4, ncls), np.int32)
    with pytest.raises(RuntimeError, match='without areas'):
        check(lib.ssd_ap_compute_coco(plain._acc, 1, np_ptr(thr), np_ptr(ap), np_ptr(ar), np_ptr(present), None, None))
    assert len(plain.compute_aps()) > 0                                  # it still serves its own protocol
    plain.close()
    del keep


def test_stage_times_switch_leaves_the_results_alone():
    s = random_set(20, 16, 2000)
    want = random_oracle(20, 16, 2000, 3)
    ms = np.full(3, -1.0)
    check(lib.ssd_ap_kernel_times(1, None))
    try:
        assert_same(gpu_eval_set(s, THRESHOLDS[3]), want)
    finally:
        check(lib.ssd_ap_kernel_times(0, np_ptr(ms)))
    assert (ms > 0).all() and (ms < 1000).all()                            # count, sort, walk of that call, in milliseconds
    assert_same(gpu_eval_set(s, THRESHOLDS[3]), want)                       # off again: no events, same arrays
    again = np.full(3, -1.0)
    check(lib.ssd_ap_kernel_times(0, np_ptr(again)))
    assert np.array_equal(again, ms)                                        # the untimed call left the last times as they were


# ------------------------------------------------------------------------------------- 5. argument checks
def test_refusals():
    s = dict(random_set(1, 3, 50))
    for thr in ((), (0.5,) * 11):
        with pytest.raises(RuntimeError, match='thresholds'):
            gpu_eval_set(s, thr)
    bad = dict(s); bad['gt_sample'] = s['gt_sample'][::-1].copy()
    assert (np.diff(bad['gt_sample']) < 0).any()
    with pytest.raises(RuntimeError, match='ascending'):
        gpu_eval_set(bad, (0.5,))
    for v in (0.0, -1.0):
        bad = dict(s); bad['sample_scale'] = s['sample_scale'].copy(); bad['sample_scale'][1] = v
        with pytest.raises(RuntimeError, match='sample_scale'):
            gpu_eval_set(bad, (0.5,))
    bad = dict(s); bad['gt_cls'] = s['gt_cls'].copy(); bad['gt_cls'][0] = 1
    with pytest.raises(RuntimeError, match='class id'):
        gpu_eval_set(bad, (0.5,))
    bad = dict(s); bad['gt_area'] = s['gt_area'].copy(); bad['gt_area'][0] = -1.0
    with pytest.raises(RuntimeError, match='gt_area'):
        gpu_eval_set(bad, (0.5,))
    thr = np.ascontiguousarray((0.5,)); ap = np.zeros((4, 1, 1)); ar = np.zeros((6, 1, 1)); present = np.zeros((4, 1), np.int32)
    outs = [np_ptr(ap), np_ptr(ar), np_ptr(present)]
    for i in range(3):
        o = list(outs); o[i] = None
        with pytest.raises(RuntimeError, match='null output'):
            check(lib.ssd_coco_eval(0, len(s['det_conf']), np_ptr(s['det_box']), np_ptr(s['det_conf']), np_ptr(s['det_cls']), np_ptr(s['det_sample']),
                                    len(s['gt_cls']), np_ptr(s['gt_box']), np_ptr(s['gt_cls']), np_ptr(s['gt_sample']), np_ptr(s['gt_flags']),
                                    np_ptr(s['gt_area']), len(s['sample_scale']), np_ptr(s['sample_scale']), 1, 1, np_ptr(thr), *o))
    assert (ap == 0).all() and (ar == 0).all()                            # nothing ran
    with pytest.raises(ValueError):
        ce.COCOEvaluator(thresholds=())
    with pytest.raises(ValueError):
        ce.DeviceCOCOEvaluator(0, 20, thresholds=(0.5,) * 11)


# ------------------------------------------------------------------------------------- 6. the driver
COCO_LINE = re.compile(r'Average (Precision|Recall) +\((AP|AR)\) @\[ IoU=')


def _infer_child(tmp_path, ap_on, extra=()):
    cmd = [sys.executable, '-m', 'ssd_tensorflow_amd.infer', '--name', str(tmp_path / 'none'), '--preset', 'vgg300', '--synthetic', '8',
           '--synthetic-boxes', '3', '--batch-size', '4', '--threshold', '0.01', '--output-dir', str(tmp_path / ('out_' + ap_on)),
           '--ap-protocol', 'coco', '--ap-on', ap_on, *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_infer_driver_prints_the_same_twelve_lines_on_host_and_gpu(tmp_path):
    lines = {}
    for ap_on in ('host', 'gpu'):
        r = _infer_child(tmp_path, ap_on)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines[ap_on] = [l for l in r.stdout.splitlines() if COCO_LINE.search(l) or l.startswith('[i] AP [') or l.startswith('[i] mAP')]
        assert '[i] AP protocol:        coco' in r.stdout
    assert lines['gpu'] == lines['host'], lines
    assert sum(1 for l in lines['host'] if COCO_LINE.search(l)) == 12 and any(l.startswith('[i] mAP') for l in lines['host'])


def test_train_driver_prints_the_same_lines_on_host_and_gpu(tmp_path, capsys):
    from ssd_tensorflow_amd import train
    common = ['--batch-size', '8', '--synthetic-train', '16', '--synthetic-valid', '8', '--synthetic-classes', '1', '--epochs', '2',
              '--checkpoint-interval', '10', '--lr-values', '0.0001', '--lr-boundaries', '', '--tensorboard-dir', str(tmp_path / 'tb'),
              '--ap-protocol', 'coco']
    lines = {}
    for ap_on in ('host', 'gpu'):
        assert train.main(['--name', str(tmp_path / ap_on), '--ap-on', ap_on] + common) == 0
        lines[ap_on] = [l for l in capsys.readouterr().out.splitlines() if l.startswith('[i] mAP') or COCO_LINE.search(l)]
    assert lines['gpu'] == lines['host'] and len(lines['host']) == 13, lines


def test_infer_driver_refuses_coco_results_without_a_coco_source(tmp_path):
    r = _infer_child(tmp_path, 'host', ('--coco-results', str(tmp_path / 'results.json')))
    assert r.returncode != 0 and 'image_ids' in r.stdout + r.stderr
    assert not os.path.exists(tmp_path / 'results.json')
