"""Oracle of the three average-precision protocols (include/ssdvgg_hip.h, "average precision") in float64, written as
explicit sequential loops over Python floats -- IEEE double, round to nearest, one operation at a time: the operations of the
kernels in the kernels' order, so every comparison against them is ==.

  0 'reference'  the reference's average_precision.py: flags ignored, every box in the denominator, 11-point AP
  1 'voc07'      the devkit's VOCevaldet with difficult objects, 11-point AP
  2 'voc12'      the same matching, the all-point area (VOC2010 on)

Shared: IoU in the +1 form; a class's detections by descending confidence, equal confidences in order of arrival; the
candidate of a detection is the first ground-truth box of its image and class with the largest IoU."""
import numpy as np

REFERENCE, VOC07, VOC12 = 0, 1, 2
RECALL_STEPS = [float(v) for v in np.arange(0, 1.1, 0.1)]      # the reference's thresholds, as it computes them


def iou_plus1(b, a):
    areaa = (a[1] - a[0] + 1.0) * (a[3] - a[2] + 1.0)
    areab = (b[1] - b[0] + 1.0) * (b[3] - b[2] + 1.0)
    w = max(0.0, min(b[1], a[1]) - max(b[0], a[0]) + 1.0)
    h = max(0.0, min(b[3], a[3]) - max(b[2], a[2]) + 1.0)
    inter = w * h
    return inter / (areab + areaa - inter)


def eleven_point(recall, prec):
    ap = 0.0
    for r in RECALL_STEPS:
        best = None
        for rc, pr in zip(recall, prec):
            if rc >= r and (best is None or pr > best):
                best = pr
        if best is not None:
            ap = ap + best
    return ap / 11.0


def eleven_point_fast(recall, prec):
    """eleven_point in one pass (recall never decreases: the points with recall >= r are a suffix)"""
    n = len(prec)
    suffix = [0.0] * (n + 1)
    have = n > 0
    for i in range(n - 1, -1, -1):
        suffix[i] = prec[i] if i == n - 1 or prec[i] > suffix[i + 1] else suffix[i + 1]
    ap = 0.0
    i = 0
    for r in RECALL_STEPS:
        while i < n and not recall[i] >= r:
            i += 1
        if i < n and have:
            ap = ap + suffix[i]
    return ap / 11.0


def all_point(recall, prec):
    """VOCevaldet.m / voc_eval(use_07_metric=False), the sum taken in ascending order"""
    mrec = [0.0] + list(recall) + [1.0]
    mpre = [0.0] + list(prec) + [0.0]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(len(mrec) - 1):
        if mrec[i + 1] != mrec[i]:
            ap = ap + (mrec[i + 1] - mrec[i]) * mpre[i + 1]
    return ap


def compute(det_box, det_conf, det_cls, det_sample, gt_box, gt_cls, gt_sample, gt_flags=None, ncls=None, protocol=REFERENCE,
            minoverlaps=(0.5,), slow_eleven=False):
    """(ap float64 [n_thr, ncls], present int [ncls])"""
    det_box = np.asarray(det_box, np.float32).reshape(-1, 4).astype(np.float64)      # float32 boxes, promoted exactly
    det_conf = np.asarray(det_conf, np.float32); det_cls = np.asarray(det_cls, np.int64); det_sample = np.asarray(det_sample, np.int64)
    gt_box = np.asarray(gt_box, np.float64).reshape(-1, 4); gt_cls = np.asarray(gt_cls, np.int64); gt_sample = np.asarray(gt_sample, np.int64)
    flags = np.zeros(len(gt_cls), bool) if gt_flags is None or protocol == REFERENCE else np.asarray(gt_flags).astype(bool)
    if ncls is None:
        ncls = int(max(gt_cls.max(initial=-1), det_cls.max(initial=-1))) + 1
    dbox = det_box.tolist(); gbox = gt_box.tolist()
    rows = {}                                          # (sample, class) -> ground-truth rows in order
    for g in range(len(gt_cls)):
        rows.setdefault((int(gt_sample[g]), int(gt_cls[g])), []).append(g)
    ap = np.zeros((len(minoverlaps), ncls), np.float64)
    present = np.zeros(ncls, np.int64)
    for k in range(ncls):
        mine = gt_cls == k
        npos = int(np.count_nonzero(mine & ~flags))
        present[k] = npos > 0
        if npos == 0:
            continue
        dsel = np.nonzero(det_cls == k)[0]
        order = dsel[np.lexsort((dsel, -det_conf[dsel].astype(np.float64)))]      # confidence descending, arrival ascending
        for t, minoverlap in enumerate(minoverlaps):
            minoverlap = float(minoverlap)
            matched = set()
            tp = 0.0; fp = 0.0
            recall, prec = [], []
            for d in order:
                arg = -1; iou_max = 0.0
                for g in rows.get((int(det_sample[d]), k), ()):
                    iou = iou_plus1(dbox[d], gbox[g])
                    if arg < 0 or iou > iou_max:
                        iou_max = iou; arg = g
                if arg < 0 or iou_max < minoverlap:
                    fp = fp + 1.0
                elif flags[arg]:
                    continue                           # a difficult object: neither way, no curve point
                elif arg in matched:
                    fp = fp + 1.0
                else:
                    tp = tp + 1.0
                    matched.add(arg)
                recall.append(tp / float(npos))
                prec.append(tp / (tp + fp))
            if protocol == VOC12:
                ap[t, k] = all_point(recall, prec)
            else:
                ap[t, k] = eleven_point(recall, prec) if slow_eleven else eleven_point_fast(recall, prec)
    return ap, present


def random_set(rng, nimg, ncls, n_det=None, flag_rate=0.0, ties=False, dup_gt=False, empty_classes=(), flagged_only=()):
    """A seeded evaluation set with the awkward cases: images without ground truth, classes without ground truth
    (`empty_classes`) or without detections, classes whose boxes are all flagged (`flagged_only`), duplicate ground-truth boxes
    (IoU ties), equal confidences.  Returns dict(det_box f32, det_conf f32, det_cls, det_sample, gt_box f64, gt_cls, gt_sample,
    gt_flags u8); ground truth ascending by sample; exactly n_det detections when given."""
    gb, gk, gs, gf, db, dk, ds = [], [], [], [], [], [], []
    allowed = [k for k in range(ncls) if k not in empty_classes] or [0]
    for img in range(nimg):
        for _ in range(int(rng.integers(0, 5))):                   # 0: an image without ground truth
            x0, y0 = (int(v) for v in rng.integers(0, 700, 2)); w, h = (int(v) for v in rng.integers(30, 300, 2))
            k = int(allowed[int(rng.integers(0, len(allowed)))])
            for _rep in range(2 if dup_gt and rng.random() < 0.3 else 1):      # the same box twice: an IoU tie
                gb.append([x0, x0 + w, y0, y0 + h]); gk.append(k); gs.append(img)
                gf.append(1 if k in flagged_only else int(rng.random() < flag_rate))
            for _rep in range(int(rng.integers(0, 4))):
                j = rng.integers(-40, 40, 4)
                db.append([x0 + j[0], x0 + w + j[1], y0 + j[2], y0 + h + j[3]])
                dk.append(k if rng.random() < 0.8 else int(rng.integers(0, ncls))); ds.append(img)
    if n_det is not None:
        while len(db) < n_det:                                     # strays: anywhere, any class, any image
            x0, y0 = (int(v) for v in rng.integers(0, 700, 2)); w, h = (int(v) for v in rng.integers(30, 300, 2))
            db.append([x0, x0 + w, y0, y0 + h]); dk.append(int(rng.integers(0, ncls))); ds.append(int(rng.integers(0, max(nimg, 1))))
        db, dk, ds = db[:n_det], dk[:n_det], ds[:n_det]
    n = len(db)
    if ties:
        dc = (rng.integers(1, 8, n) / 8.0).astype(np.float32)      # seven values: many equal confidences
    else:
        dc = ((rng.permutation(n) + 1) / (n + 1.0)).astype(np.float32)
    return dict(det_box=np.array(db, np.float32).reshape(-1, 4), det_conf=dc, det_cls=np.array(dk, np.int32), det_sample=np.array(ds, np.int32),
                gt_box=np.array(gb, np.float64).reshape(-1, 4), gt_cls=np.array(gk, np.int32), gt_sample=np.array(gs, np.int32),
                gt_flags=np.array(gf, np.uint8))
