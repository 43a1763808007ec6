"""Mirror of the reference's average_precision.py (APs2mAP :30-42, APCalculator :45-192) over the HIP kernels behind
ssd_average_precision_ex.  Same class, same methods, same dict-of-label results; beside the reference's protocol the
devkit's VOC07 (difficult objects count neither way) and VOC12 (all-point area) forms, and DeviceAPCalculator, which keeps
the detections of a run on the GPU (include/ssdvgg_hip.h, "average precision")."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check, np_ptr
from .utils import Size, prop2abs

IMG_SIZE = Size(1000, 1000)
PROTOCOLS = {'reference': 0, 'voc07': 1, 'voc12': 2}


def APs2mAP(aps):
    """Mean of the APs over all classes (summed in the dict's order)."""
    num_classes = 0.
    sum_ap = 0.
    for _, v in aps.items():
        sum_ap += v
        num_classes += 1
    if num_classes == 0:
        return 0
    return sum_ap / num_classes


def add_ap_arguments(parser):
    """--ap-protocol / --ap-on of the drivers that compute AP (infer.py, train.py)"""
    parser.add_argument('--ap-protocol', default='reference', choices=list(PROTOCOLS) + ['coco'],
                        help="reference: the reference's 11-point AP, every ground-truth box counts; voc07: the devkit's 11-point AP, "
                             'difficult objects count neither way; voc12: the same matching, all-point AP (VOC2010 on); coco: '
                             "COCO's box AP / AR over IoU 0.50:0.95, area ranges and detection caps (coco_eval.py), twelve numbers")
    parser.add_argument('--ap-on', default='host', choices=['host', 'gpu'],
                        help='host: the detections are collected in Python lists; gpu: a kernel behind each detection pass appends them '
                             'to buffers on the GPU, they come to the host only where files or pictures need them (same AP)')


def _protocol_id(protocol):
    if protocol not in PROTOCOLS:
        raise ValueError('protocol must be one of %s (got %r)' % (', '.join(PROTOCOLS), protocol))
    return PROTOCOLS[protocol]


def _thresholds(minoverlap):
    """(float64 array, is a sequence)"""
    many = not np.isscalar(minoverlap)
    thr = np.ascontiguousarray(list(minoverlap) if many else [minoverlap], np.float64)
    if not 1 <= len(thr) <= 10:
        raise ValueError('1..10 IoU thresholds (got %d)' % len(thr))
    return thr, many


def _result(label_id, ap, present, many):
    """{label: AP, or the list of APs of a threshold list} for the classes that are part of the mAP, in label_id's order"""
    return {label: ([float(v) for v in ap[:, k]] if many else float(ap[0, k])) for label, k in label_id.items() if present[k]}


class APCalculator:
    """Average precision from host lists.  protocol 'reference': the reference's VOC07 11-point form (see its docstring for
    its peculiarities); 'voc07' / 'voc12': the devkit's, where a ground-truth box with a true `.difficult` (utils.FlaggedBox)
    counts neither way.  minoverlap: one IoU threshold, or a sequence of up to 10 -- then every value of the dict is a list."""

    def __init__(self, minoverlap=0.5, protocol='reference'):
        self.minoverlap = minoverlap
        self.protocol = protocol
        _protocol_id(protocol); _thresholds(minoverlap)
        self.clear()

    def add_detections(self, gt_boxes, boxes):
        """gt_boxes: list of Box; boxes: list of (confidence, Box) with a correctly set label."""
        sample_id = len(self.gt_boxes)
        self.gt_boxes.append(gt_boxes)
        for conf, box in boxes:
            self.det_params.append(prop2abs(box.center, box.size, IMG_SIZE))
            self.det_confidence.append(conf)
            self.det_labels.append(box.label)
            self.det_sample_ids.append(sample_id)

    def compute_aps(self):
        """{label: AP} for every label that is part of the mAP, in first-appearance order."""
        label_id = {}
        gb, gk, gs, gf = [], [], [], []
        for sample_id, boxes in enumerate(self.gt_boxes):
            for box in boxes:
                k = label_id.setdefault(box.label, len(label_id))
                gb.append(prop2abs(box.center, box.size, IMG_SIZE)); gk.append(k); gs.append(sample_id)
                gf.append(1 if getattr(box, 'difficult', False) else 0)
        if not label_id:
            return {}
        ncls = len(label_id)
        keep = [i for i, l in enumerate(self.det_labels) if l in label_id]      # detections of classes without ground truth are ignored
        db = np.ascontiguousarray([self.det_params[i] for i in keep], np.float32).reshape(-1, 4)
        dc = np.ascontiguousarray([self.det_confidence[i] for i in keep], np.float32)
        dk = np.ascontiguousarray([label_id[self.det_labels[i]] for i in keep], np.int32)
        ds = np.ascontiguousarray([self.det_sample_ids[i] for i in keep], np.int32)
        gb = np.ascontiguousarray(gb, np.float64).reshape(-1, 4)
        gk = np.ascontiguousarray(gk, np.int32); gs = np.ascontiguousarray(gs, np.int32); gf = np.ascontiguousarray(gf, np.uint8)
        thr, many = _thresholds(self.minoverlap)
        ap = np.zeros((len(thr), ncls), np.float64); present = np.zeros(ncls, np.int32)
        check(lib.ssd_average_precision_ex(_lib.device(), len(dc), np_ptr(db), np_ptr(dc), np_ptr(dk), np_ptr(ds), len(gk), np_ptr(gb),
                                           np_ptr(gk), np_ptr(gs), np_ptr(gf), ncls, _protocol_id(self.protocol), len(thr), np_ptr(thr),
                                           np_ptr(ap), np_ptr(present)))
        return _result(label_id, ap, present, many)

    def state(self):
        """Everything add_detections has collected, as plain lists (picklable: one rank's share of a data-parallel run)."""
        return dict(det_params=self.det_params, det_confidence=self.det_confidence, det_labels=self.det_labels,
                    det_sample_ids=self.det_sample_ids, gt_boxes=self.gt_boxes)

    def merge(self, state):
        """Append another calculator's state(); its sample ids are shifted behind the samples already held."""
        base = len(self.gt_boxes)
        self.gt_boxes.extend(state['gt_boxes'])
        self.det_params.extend(state['det_params'])
        self.det_confidence.extend(state['det_confidence'])
        self.det_labels.extend(state['det_labels'])
        self.det_sample_ids.extend(i + base for i in state['det_sample_ids'])

    def clear(self):
        self.det_params = []
        self.det_confidence = []
        self.det_labels = []
        self.det_sample_ids = []
        self.gt_boxes = []


def gt_arrays(gt_boxes):
    """(box f64 [n, 4] on the 1000 grid, class id, image index, difficult flag) of one list of Box per image"""
    gb, gk, gi, gf = [], [], [], []
    for i, boxes in enumerate(gt_boxes):
        for box in boxes:
            gb.append(prop2abs(box.center, box.size, IMG_SIZE)); gk.append(box.labelid); gi.append(i)
            gf.append(1 if getattr(box, 'difficult', False) else 0)
    return (np.ascontiguousarray(gb, np.float64).reshape(-1, 4), np.ascontiguousarray(gk, np.int32), np.ascontiguousarray(gi, np.int32),
            np.ascontiguousarray(gf, np.uint8))


class DeviceAPCalculator:
    """APCalculator whose detections never visit the host: add_pass enqueues one kernel behind a detection pass, which appends
    the pass's detections to buffers on the GPU (ssd_ap_add_dev); compute_aps runs the AP kernels on them.  Only the ground
    truth -- a few boxes per image -- passes through Python.  The class index is the boxes' `labelid` (0..num_classes-1), the
    keys of the result are the ground truth's labels in first-appearance order, as APCalculator's."""

    def __init__(self, device, num_classes, protocol='reference', minoverlap=0.5):
        self.device, self.num_classes = int(device), int(num_classes)
        self.minoverlap, self.protocol = minoverlap, protocol
        _protocol_id(protocol); _thresholds(minoverlap)
        self.gt_boxes = []
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

    def add_pass(self, slots, gt_boxes, stream=None):
        """slots: the ticket of SSDVGG.detect_last_launch or TiledDetector.launch that has just been launched, or a tuple
        (count, conf, cls, box, b, out_cap) of device pointers in that layout (then `stream`: the stream pointer the arrays are
        written on; None: the legacy default stream).  gt_boxes: one list of Box per image of the pass.  Returns at once."""
        if hasattr(slots, 'dev_slots'):
            count, conf, cls, box, b, out_cap, stream = slots.dev_slots()
        else:
            count, conf, cls, box, b, out_cap = slots
        if len(gt_boxes) != b:
            raise ValueError('%d lists of ground truth for a pass of %d images' % (len(gt_boxes), b))
        gb, gk, gi, gf = gt_arrays(gt_boxes)
        check(lib.ssd_ap_add_dev(self._acc, int(b), int(out_cap), count, conf, cls, box, len(gk), np_ptr(gb), np_ptr(gk), np_ptr(gi),
                                 np_ptr(gf), stream or None))
        self.gt_boxes.extend(gt_boxes)

    def _labels(self):
        label_id = {}
        for boxes in self.gt_boxes:
            for box in boxes:
                if label_id.setdefault(box.label, box.labelid) != box.labelid:
                    raise ValueError('label %r has the class ids %d and %d' % (box.label, label_id[box.label], box.labelid))
        return label_id

    def compute_aps(self):
        """The dict APCalculator.compute_aps returns for the same passes (waits for them)."""
        label_id = self._labels()
        if not label_id:
            return {}
        thr, many = _thresholds(self.minoverlap)
        ap = np.zeros((len(thr), self.num_classes), np.float64); present = np.zeros(self.num_classes, np.int32)
        n = C.c_longlong(); dropped = C.c_longlong()
        check(lib.ssd_ap_compute(self._acc, _protocol_id(self.protocol), len(thr), np_ptr(thr), np_ptr(ap), np_ptr(present),
                                 C.byref(n), C.byref(dropped)))
        self.dropped = dropped.value
        return _result(label_id, ap, present, many)

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
        return dict(det_box=box, det_confidence=conf, det_classes=cls, det_sample_ids=smp, gt_boxes=self.gt_boxes)

    def merge(self, state):
        """Append another DeviceAPCalculator's state(); its sample ids are shifted behind the samples already held."""
        gb, gk, gs, gf = gt_arrays(state['gt_boxes'])
        box = np.ascontiguousarray(state['det_box'], np.float32); conf = np.ascontiguousarray(state['det_confidence'], np.float32)
        cls = np.ascontiguousarray(state['det_classes'], np.int32); smp = np.ascontiguousarray(state['det_sample_ids'], np.int32)
        check(lib.ssd_ap_add_host(self._acc, len(conf), np_ptr(box), np_ptr(conf), np_ptr(cls), np_ptr(smp), len(state['gt_boxes']),
                                  len(gk), np_ptr(gb), np_ptr(gk), np_ptr(gs), np_ptr(gf)))
        self.gt_boxes.extend(state['gt_boxes'])

    def clear(self):
        check(lib.ssd_ap_clear(self._acc))
        self.gt_boxes = []
