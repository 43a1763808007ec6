"""Geometry helpers and record types of the reference's utils.py (:64-135), host side.

These are the scalar conversions a caller uses to turn the GPU's integer boxes back into the
reference's Box(center, size) records; the batched arithmetic itself runs in the HIP library.
"""
import argparse
import math
from collections import namedtuple

Label = namedtuple('Label', ['name', 'color'])
Size = namedtuple('Size', ['w', 'h'])
Point = namedtuple('Point', ['x', 'y'])
Sample = namedtuple('Sample', ['filename', 'boxes', 'imgsize'])
Box = namedtuple('Box', ['label', 'labelid', 'center', 'size'])
Score = namedtuple('Score', ['idx', 'score'])


class FlaggedBox(Box):
    """A Box that carries VOC's <difficult> flag, and COCO's `iscrowd` and annotation `area` (pixels^2; None: the box's own
    w*h).  It IS the reference's 4-field tuple -- it compares, hashes, unpacks and indexes like Box, so every consumer of Box
    takes it -- with attributes more, which pickling keeps.  A crowd box is difficult as well: the VOC protocols ignore it."""

    def __new__(cls, label, labelid, center, size, difficult=False, *, crowd=False, area=None):
        self = super().__new__(cls, label, labelid, center, size)
        self.crowd = bool(crowd)
        self.difficult = bool(difficult) or self.crowd
        self.area = None if area is None else float(area)
        return self

    def __reduce__(self):
        if not self.crowd and self.area is None:
            return FlaggedBox, (self.label, self.labelid, self.center, self.size, self.difficult)
        return _flagged_box, (self.label, self.labelid, self.center, self.size, self.difficult, self.crowd, self.area)

    def _replace(self, **kwargs):
        difficult = kwargs.pop('difficult', self.difficult)
        crowd = kwargs.pop('crowd', self.crowd)
        area = kwargs.pop('area', self.area)
        return FlaggedBox(*Box._replace(Box(*self), **kwargs), difficult=difficult, crowd=crowd, area=area)

    def __repr__(self):
        more = (', crowd=%r' % self.crowd if self.crowd else '') + (', area=%r' % self.area if self.area is not None else '')
        return Box.__repr__(self)[:-1] + ', difficult=%r%s)' % (self.difficult, more)


def _flagged_box(label, labelid, center, size, difficult, crowd, area):
    """(pickle's constructor of a FlaggedBox with keyword attributes)"""
    return FlaggedBox(label, labelid, center, size, difficult, crowd=crowd, area=area)


def box_like(box, center, size):
    """`box` with another centre and size: a transform's result keeps the label, the flags and the annotation's area."""
    crowd, area = getattr(box, 'crowd', False), getattr(box, 'area', None)
    if crowd or area is not None:
        return FlaggedBox(box.label, box.labelid, center, size, box.difficult, crowd=crowd, area=area)
    if getattr(box, 'difficult', False):
        return FlaggedBox(box.label, box.labelid, center, size, True)
    return Box(box.label, box.labelid, center, size)
Overlap = namedtuple('Overlap', ['best', 'good'])


def str2bool(v):
    """utils.py:73-82"""
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Boolean value expected.')


def abs2prop(xmin, xmax, ymin, ymax, imgsize):
    """Absolute min/max bounds -> proportional centre/size (utils.py:85-97)."""
    width = float(xmax - xmin)
    height = float(ymax - ymin)
    cx = float(xmin) + width / 2
    cy = float(ymin) + height / 2
    return Point(cx / imgsize.w, cy / imgsize.h), Size(width / imgsize.w, height / imgsize.h)


def prop2abs(center, size, imgsize):
    """Proportional centre/size -> absolute bounds; int() truncates toward zero (utils.py:100-108)."""
    width2 = size.w * imgsize.w / 2
    height2 = size.h * imgsize.h / 2
    cx = center.x * imgsize.w
    cy = center.y * imgsize.h
    return int(cx - width2), int(cx + width2), int(cy - height2), int(cy + height2)


def box_is_valid(box):
    """utils.py:111-115"""
    return not any(math.isnan(v) or math.isinf(v) for v in (box.center.x, box.center.y, box.size.w, box.size.h))


def normalize_box(box):
    """Clip to the 1000x1000 integer grid (utils.py:118-135)."""
    if not box_is_valid(box):
        return box
    img = Size(1000, 1000)
    xmin, xmax, ymin, ymax = prop2abs(box.center, box.size, img)
    xmin = max(xmin, 0); xmax = min(xmax, img.w - 1)
    ymin = max(ymin, 0); ymax = min(ymax, img.h - 1)
    xmin = min(xmin, xmax); ymin = min(ymin, ymax)
    center, size = abs2prop(xmin, xmax, ymin, ymax, img)
    return box_like(box, center, size)


def load_data_source(data_source):
    """utils.py:44-55: the module `source_<name>` must provide get_source()"""
    import importlib
    try:
        module = importlib.import_module('ssd_tensorflow_amd.source_' + data_source)
    except ImportError:
        module = importlib.import_module('source_' + data_source)
    return module.get_source()


def default_colors(names):
    """{name: (b, g, r)} for a list of class names no data source colours: the VOC colours for the VOC names
    (source_pascal_voc), else evenly spaced hues at full saturation, deterministic in the list's order."""
    import colorsys
    from .source_pascal_voc import VOC_NAMES, label_defs
    names = [str(n) for n in names]
    if names == list(VOC_NAMES):
        return {l.name: tuple(l.color) for l in label_defs}
    out = {}
    for i, n in enumerate(names):
        r, g, b = colorsys.hsv_to_rgb(i / max(len(names), 1), 1.0, 1.0)
        out[n] = (int(round(b * 255)), int(round(g * 255)), int(round(r * 255)))
    return out


def draw_box(img, box, color, device=None):
    """utils.py:138-148: draw one Box on `img` IN PLACE -- a numpy uint8 or float32 [H, W, 3] BGR array -- through the HIP
    library (annotate.py; the rule is in include/ssdvgg_hip.h).  A float image stays float and is not clamped, like the
    reference's.  `color`: (b, g, r)."""
    import numpy as np
    import torch
    from . import _lib
    from . import annotate as A
    if not isinstance(img, np.ndarray) or img.ndim != 3 or img.shape[2] != 3 or img.dtype not in (np.uint8, np.float32):
        raise ValueError('draw_box needs a uint8 or float32 [H, W, 3] numpy array')
    h, w = img.shape[:2]
    rect = prop2abs(box.center, box.size, Size(w, h))
    dev = torch.device('cuda', _lib.device() if device is None else int(device))
    style = A.Style([tuple(int(c) for c in color)], ['' if box.label is None else str(box.label)], dev.index)
    try:
        is_f = img.dtype == np.float32
        src = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
        count = torch.ones(1, dtype=torch.int32, device=dev)
        cls = torch.zeros(1, dtype=torch.int32, device=dev)
        rect_t = torch.tensor([rect], dtype=torch.int32, device=dev)
        dst, offs, shapes = A.annotate_batch(src, [0], [(h, w)], count, cls, rect_t, 1, style, boxes_on_1000_grid=False, dst_float=is_f)
        img[...] = A.unpack(dst.cpu().numpy(), offs, shapes)[0]
    finally:
        style.close()
