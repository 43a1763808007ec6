"""numpy restatement of the drawing rule of include/ssdvgg_hip.h ("drawing detections"), the yardstick of
tests/test_annotate.py and tests/test_gpu_annotate.py.  Integer coverage and separately rounded float32 arithmetic only, so
everything compared with it is compared for exact equality.  The glyph rows come from ssd_annotate_glyph: the art is not
duplicated here."""
import numpy as np

from ssd_tensorflow_amd import annotate as A
from ssd_tensorflow_amd.utils import Size, abs2prop, prop2abs

F32 = np.float32
_GLYPHS = {}


def glyph(ch):
    if ch not in _GLYPHS:
        _GLYPHS[ch] = A.glyph(ch)
    return _GLYPHS[ch]


def rect1000(box, w, h):
    """pixel rectangle of an integer box (xmin, xmax, ymin, ymax) on the 1000 grid: the reference's own functions"""
    return prop2abs(*abs2prop(int(box[0]), int(box[1]), int(box[2]), int(box[3]), Size(1000, 1000)), Size(w, h))


def label_bytes(label):
    return str(label).encode('ascii', 'replace')[:31]


def _fill(mask, x0, x1, y0, y1, val=True):
    h, w = mask.shape
    xa, xb, ya, yb = max(x0, 0), min(x1, w - 1), max(y0, 0), min(y1, h - 1)
    if xa <= xb and ya <= yb:
        mask[ya:yb + 1, xa:xb + 1] = val


def coverage(shape, rect, label):
    """(covered, text) boolean [h, w] masks of one box"""
    xmin, xmax, ymin, ymax = (int(v) for v in rect)
    cov = np.zeros(shape, bool); txt = np.zeros(shape, bool)
    _fill(cov, xmin - 1, xmax + 1, ymin - 1, ymax + 1)
    _fill(cov, xmin + 2, xmax - 2, ymin + 2, ymax - 2, False)
    _fill(cov, xmin - 1, xmax + 1, ymin - 20, ymin)
    for i, ch in enumerate(label_bytes(label)):
        rows = glyph(ch)
        for r in range(7):
            for c in range(5):
                if rows[r] >> (4 - c) & 1:
                    x, y = xmin + 5 + 12 * i + 2 * c, ymin - 18 + 2 * r
                    _fill(txt, x, x + 1, y, y + 1)
    return cov | txt, txt


def draw(img, boxes):
    """boxes: list of (pixel rect, (b, g, r), label), applied in order on a copy of img (uint8 or float32 [h, w, 3]); a uint8
    image is rounded half to even and saturated after every box, a float32 one stays float"""
    out = img.copy()
    for rect, color, label in boxes:
        cov, txt = coverage(out.shape[:2], rect, label)
        if not cov.any():
            continue
        d = np.where(txt[cov][:, None], F32(255), np.asarray(color, F32)[None, :]).astype(F32)
        s = F32(0.8) * d + F32(0.2) * out[cov].astype(F32)
        assert s.dtype == F32
        out[cov] = np.clip(np.rint(s), 0, 255).astype(np.uint8) if img.dtype == np.uint8 else s
    return out


def to_u8(imgf):
    """ImageSummary.push: img[img > 255] = 255; img[img < 0] = 0; astype(uint8)"""
    return np.clip(imgf, 0, 255).astype(np.uint8)


def _taps(src, dst):
    d = np.arange(dst)
    fx = ((d + 0.5) * (src / dst) - 0.5).astype(F32)
    sx = np.floor(fx).astype(np.int64)
    f = (fx - sx.astype(F32)).astype(F32)
    f = np.where(sx < 0, F32(0), f); sx = np.where(sx < 0, 0, sx)
    f = np.where(sx >= src - 1, F32(0), f); sx = np.where(sx >= src - 1, src - 1, sx)
    return sx, np.minimum(sx + 1, src - 1), f.astype(F32)


def resize_linear(img, w, h):
    """cv2.resize(img, (w, h)) for a float32 image, restated as OpenCV's float INTER_LINEAR path: the horizontal pass, then the
    vertical one, every product and sum rounded to float32"""
    img = np.asarray(img, F32)
    if img.shape[:2] == (h, w):
        return img.copy()
    x0, x1, fx = _taps(img.shape[1], w)
    y0, y1, fy = _taps(img.shape[0], h)
    fx = fx[None, :, None]; fy = fy[:, None, None]
    rows = img[:, x0, :] * (F32(1) - fx) + img[:, x1, :] * fx
    out = rows[y0] * (F32(1) - fy) + rows[y1] * fy
    assert out.dtype == F32
    return out


def style_boxes(rects, classes, colors, names):
    """(rect, colour, label) per box; a class id outside 0..len(names)-1 is white with the label '?'"""
    out = []
    for r, c in zip(rects, classes):
        c = int(c)
        ok = 0 <= c < len(names)
        out.append((tuple(int(v) for v in r), tuple(colors[c]) if ok else (255, 255, 255), names[c] if ok else '?'))
    return out
