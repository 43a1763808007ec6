"""COCO's bounding-box evaluation over the HIP kernels behind ssd_coco_eval / ssd_ap_compute_coco (the rule is in
include/ssdvgg_hip.h, "COCO box evaluation"): COCOEvaluator collects host lists as APCalculator does, DeviceCOCOEvaluator keeps
the detections on the GPU as DeviceAPCalculator does.  Both give the same arrays for the same passes, and from them the twelve
numbers COCO's tools print.  A ground-truth box's `crowd` and `area` attributes (utils.FlaggedBox) are read; without an area a
box has its own w*h in pixels.  The class index is the boxes' `labelid`."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check, np_ptr
from .average_precision import IMG_SIZE
from .utils import prop2abs

DEFAULT_THRESHOLDS = np.linspace(0.5, 0.95, 10)
SUMMARY_NAMES = ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl')
# (title, IoU text of a single threshold or None, area, maxDets) of the twelve lines, in COCO's order
_LINES = (('Average Precision', None, 'all', 100), ('Average Precision', '0.50', 'all', 100), ('Average Precision', '0.75', 'all', 100),
          ('Average Precision', None, 'small', 100), ('Average Precision', None, 'medium', 100), ('Average Precision', None, 'large', 100),
          ('Average Recall', None, 'all', 1), ('Average Recall', None, 'all', 10), ('Average Recall', None, 'all', 100),
          ('Average Recall', None, 'small', 100), ('Average Recall', None, 'medium', 100), ('Average Recall', None, 'large', 100))


def _thresholds(thresholds):
    thr = np.ascontiguousarray(DEFAULT_THRESHOLDS if thresholds is None else list(thresholds), np.float64)
    if not 1 <= len(thr) <= 10:
        raise ValueError('1..10 IoU thresholds (got %d)' % len(thr))
    return thr


def coco_gt_arrays(gt_boxes, imgsizes):
    """(box f64 [n, 4] on the 1000 grid, class id, image index, flags (1 = ignored, 2 = crowd), area in pixels^2, W*H/1e6 per
    image) of one list of Box and one Size per image"""
    if len(gt_boxes) != len(imgsizes):
        raise ValueError('%d lists of ground truth for %d image sizes' % (len(gt_boxes), len(imgsizes)))
    gb, gk, gi, gf, ga = [], [], [], [], []
    for i, (boxes, size) in enumerate(zip(gt_boxes, imgsizes)):
        for box in boxes:
            gb.append(prop2abs(box.center, box.size, IMG_SIZE)); gk.append(box.labelid); gi.append(i)
            crowd = getattr(box, 'crowd', False)
            gf.append(3 if crowd else (1 if getattr(box, 'difficult', False) else 0))
            area = getattr(box, 'area', None)
            ga.append((box.size.w * size[0]) * (box.size.h * size[1]) if area is None else area)
    scale = [float(s[0]) * float(s[1]) / 1e6 for s in imgsizes]
    return (np.ascontiguousarray(gb, np.float64).reshape(-1, 4), np.ascontiguousarray(gk, np.int32), np.ascontiguousarray(gi, np.int32),
            np.ascontiguousarray(gf, np.uint8), np.ascontiguousarray(ga, np.float64), np.ascontiguousarray(scale, np.float64))


def _mean(x, mask):
    x = x[:, mask]
    return float(np.mean(x)) if x.size else -1.0


def summarize(result):
    """{name: value} of the twelve numbers in COCO's order, from compute()'s arrays; -1.0 where nothing is present"""
    ap, ar, p, thr = result['ap'], result['ar'], result['present'].astype(bool), result['thresholds']

    def at(value):
        idx = np.nonzero(thr == value)[0]
        return _mean(ap[0][idx[:1]], p[0]) if len(idx) else -1.0
    return {'AP': _mean(ap[0], p[0]), 'AP50': at(0.5), 'AP75': at(0.75), 'APs': _mean(ap[1], p[1]), 'APm': _mean(ap[2], p[2]),
            'APl': _mean(ap[3], p[3]), 'AR1': _mean(ar[4], p[0]), 'AR10': _mean(ar[5], p[0]), 'AR100': _mean(ar[0], p[0]),
            'ARs': _mean(ar[1], p[1]), 'ARm': _mean(ar[2], p[2]), 'ARl': _mean(ar[3], p[3])}


def aps_of(result):
    """{label: AP averaged over the thresholds, area all} of compute()'s arrays, for the classes present there, in first-appearance
    order: what APs2mAP and the drivers' per-class tables take"""
    return {label: float(np.mean(result['ap'][0][:, k])) for label, k in result['labels'].items() if result['present'][0, k]}


def format_summary(summary, thresholds=None):
    """The twelve lines in the layout COCO's tools print them."""
    thr = _thresholds(thresholds)
    span = '{:0.2f}:{:0.2f}'.format(thr[0], thr[-1])
    lines = []
    for name, (title, iou, area, max_dets) in zip(SUMMARY_NAMES, _LINES):
        lines.append(' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
            title, '(AP)' if title.endswith('Precision') else '(AR)', iou or span, area, max_dets, summary[name]))
    return '\n'.join(lines)


class _Results:
    """The result methods both evaluators share; compute() is theirs."""

    def summary(self):
        return summarize(self.compute())

    def compute_aps(self):
        """{label: AP averaged over the thresholds, area all} for the classes present there, in first-appearance order: what
        APs2mAP and the drivers' per-class table take."""
        return aps_of(self.compute())

    def _labels(self):
        label_id = {}
        for boxes in self.gt_boxes:
            for box in boxes:
                if label_id.setdefault(box.label, box.labelid) != box.labelid:
                    raise ValueError('label %r has the class ids %d and %d' % (box.label, label_id[box.label], box.labelid))
        return label_id

    def _empty(self, ncls):
        return (np.full((4, len(self.thresholds), ncls), -1.0), np.full((6, len(self.thresholds), ncls), -1.0), np.zeros((4, ncls), np.int32))


class COCOEvaluator(_Results):
    """COCO box AP / AR from host lists.  num_classes None: the largest class id of the ground truth + 1."""

    def __init__(self, thresholds=None, num_classes=None):
        self.thresholds = _thresholds(thresholds)
        self.num_classes = num_classes
        self.clear()

    def add_detections(self, gt_boxes, boxes, imgsize):
        """gt_boxes: list of Box; boxes: list of (confidence, Box) with a correctly set labelid; imgsize: Size of the image."""
        sample_id = len(self.gt_boxes)
        self.gt_boxes.append(gt_boxes)
        self.imgsizes.append((int(imgsize[0]), int(imgsize[1])))
        for conf, box in boxes:
            self.det_params.append(prop2abs(box.center, box.size, IMG_SIZE))
            self.det_confidence.append(conf)
            self.det_classes.append(box.labelid)
            self.det_sample_ids.append(sample_id)

    def compute(self):
        """dict(ap [4, T, ncls], ar [6, T, ncls], present [4, ncls], thresholds [T], labels {label: class id})"""
        labels = self._labels()
        gb, gk, gs, gf, ga, scale = coco_gt_arrays(self.gt_boxes, self.imgsizes)
        ncls = self.num_classes if self.num_classes is not None else int(gk.max(initial=0)) + 1
        ap, ar, present = self._empty(ncls)
        keep = [i for i, k in enumerate(self.det_classes) if 0 <= k < ncls]
        self.dropped = len(self.det_classes) - len(keep)
        db = np.ascontiguousarray([self.det_params[i] for i in keep], np.float32).reshape(-1, 4)
        dc = np.ascontiguousarray([self.det_confidence[i] for i in keep], np.float32)
        dk = np.ascontiguousarray([self.det_classes[i] for i in keep], np.int32)
        ds = np.ascontiguousarray([self.det_sample_ids[i] for i in keep], np.int32)
        thr = self.thresholds
        check(lib.ssd_coco_eval(_lib.device(), len(dc), np_ptr(db), np_ptr(dc), np_ptr(dk), np_ptr(ds), len(gk), np_ptr(gb), np_ptr(gk),
                                np_ptr(gs), np_ptr(gf), np_ptr(ga), len(scale), np_ptr(scale), ncls, len(thr), np_ptr(thr), np_ptr(ap),
                                np_ptr(ar), np_ptr(present)))
        return dict(ap=ap, ar=ar, present=present, thresholds=thr, labels=labels)

    def state(self):
        """Everything add_detections has collected, as plain lists (picklable: one rank's share of a data-parallel run)."""
        return dict(det_params=self.det_params, det_confidence=self.det_confidence, det_classes=self.det_classes,
                    det_sample_ids=self.det_sample_ids, gt_boxes=self.gt_boxes, imgsizes=self.imgsizes)

    def merge(self, state):
        """Append another evaluator's state(); its sample ids are shifted behind the samples already held."""
        base = len(self.gt_boxes)
        self.gt_boxes.extend(state['gt_boxes'])
        self.imgsizes.extend(state['imgsizes'])
        self.det_params.extend(state['det_params'])
        self.det_confidence.extend(state['det_confidence'])
        self.det_classes.extend(state['det_classes'])
        self.det_sample_ids.extend(i + base for i in state['det_sample_ids'])

    def clear(self):
        self.det_params = []
        self.det_confidence = []
        self.det_classes = []
        self.det_sample_ids = []
        self.gt_boxes = []
        self.imgsizes = []


class DeviceCOCOEvaluator(_Results):
    """COCOEvaluator whose detections never visit the host: add_pass enqueues the accumulator's append kernel behind a
    detection pass (ssd_ap_add_dev_coco); compute runs the evaluation kernels on the stored arrays (ssd_ap_compute_coco)."""

    def __init__(self, device, num_classes, thresholds=None):
        self.device, self.num_classes = int(device), int(num_classes)
        self.thresholds = _thresholds(thresholds)
        self.gt_boxes, self.imgsizes = [], []
        self.dropped = 0
        acc = C.c_void_p()
        check(lib.ssd_ap_create(self.device, self.num_classes, C.byref(acc)))
        self._acc = acc

    def close(self):
        acc, self._acc = self._acc, None
        if acc is not None:
            check(lib.ssd_ap_destroy(acc))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_pass(self, slots, gt_boxes, imgsizes, stream=None):
        """slots: as DeviceAPCalculator.add_pass takes them; gt_boxes: one list of Box per image of the pass; imgsizes: one
        Size per image.  Returns at once."""
        if hasattr(slots, 'dev_slots'):
            count, conf, cls, box, b, out_cap, stream = slots.dev_slots()
        else:
            count, conf, cls, box, b, out_cap = slots
        if len(gt_boxes) != b or len(imgsizes) != b:
            raise ValueError('%d lists of ground truth and %d image sizes for a pass of %d images' % (len(gt_boxes), len(imgsizes), b))
        imgsizes = [(int(s[0]), int(s[1])) for s in imgsizes]
        gb, gk, gi, gf, ga, scale = coco_gt_arrays(gt_boxes, imgsizes)
        check(lib.ssd_ap_add_dev_coco(self._acc, int(b), int(out_cap), count, conf, cls, box, len(gk), np_ptr(gb), np_ptr(gk), np_ptr(gi),
                                      np_ptr(gf), np_ptr(ga), np_ptr(scale), stream or None))
        self.gt_boxes.extend(gt_boxes)
        self.imgsizes.extend(imgsizes)

    def compute(self):
        """The dict COCOEvaluator.compute returns for the same passes (waits for them)."""
        ap, ar, present = self._empty(self.num_classes)
        thr = self.thresholds
        n = C.c_longlong(); dropped = C.c_longlong()
        check(lib.ssd_ap_compute_coco(self._acc, len(thr), np_ptr(thr), np_ptr(ap), np_ptr(ar), np_ptr(present), C.byref(n), C.byref(dropped)))
        self.dropped = dropped.value
        return dict(ap=ap, ar=ar, present=present, thresholds=thr, labels=self._labels())

    def num_detections(self):
        """Detections held (waits for the passes in flight)."""
        n = C.c_longlong(); dropped = C.c_longlong()
        check(lib.ssd_ap_count(self._acc, C.byref(n), C.byref(dropped)))
        self.dropped = dropped.value
        return n.value

    def num_dropped(self):
        """Detections that were not stored: their class id was outside 0..num_classes-1."""
        self.num_detections()
        return self.dropped

    def state(self):
        """Everything the passes have collected, as host arrays (picklable: one rank's share of a data-parallel run)."""
        n = self.num_detections()
        box = np.zeros((n, 4), np.float32); conf = np.zeros(n, np.float32); cls = np.zeros(n, np.int32); smp = np.zeros(n, np.int32)
        got = C.c_longlong()
        check(lib.ssd_ap_fetch(self._acc, n, np_ptr(box), np_ptr(conf), np_ptr(cls), np_ptr(smp), C.byref(got)))
        assert got.value == n
        return dict(det_box=box, det_confidence=conf, det_classes=cls, det_sample_ids=smp, gt_boxes=self.gt_boxes, imgsizes=self.imgsizes)

    def merge(self, state):
        """Append another DeviceCOCOEvaluator's state(); its sample ids are shifted behind the samples already held."""
        gb, gk, gs, gf, ga, scale = coco_gt_arrays(state['gt_boxes'], state['imgsizes'])
        box = np.ascontiguousarray(state['det_box'], np.float32); conf = np.ascontiguousarray(state['det_confidence'], np.float32)
        cls = np.ascontiguousarray(state['det_classes'], np.int32); smp = np.ascontiguousarray(state['det_sample_ids'], np.int32)
        check(lib.ssd_ap_add_host_coco(self._acc, len(conf), np_ptr(box), np_ptr(conf), np_ptr(cls), np_ptr(smp), len(state['gt_boxes']),
                                       len(gk), np_ptr(gb), np_ptr(gk), np_ptr(gs), np_ptr(gf), np_ptr(ga), np_ptr(scale)))
        self.gt_boxes.extend(state['gt_boxes'])
        self.imgsizes.extend(state['imgsizes'])

    def clear(self):
        check(lib.ssd_ap_clear(self._acc))
        self.gt_boxes, self.imgsizes = [], []
