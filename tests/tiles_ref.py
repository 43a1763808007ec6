"""Numpy restatement of tiled detection: the windows of a picture and the merge of the windows' boxes, built from
oracle.boxes.decode / suppress.  The yardstick of tests/test_tiles_ref.py (CPU) and tests/test_gpu_tiles.py; pure numpy.

  plan_tiles_ref   the windows (x0, y0, w, h, interior) of a picture
  merge_ref        one picture: per-tile decode() records -> edge drop, the picture's 1000 grid, order, suppress, [:max_out]
  merge_ref_all    a list of (image, tile, (W, H)) with one decode() record set per entry -> one result per picture
  planted_scene    the test scene: objects planted on a picture, every tile's prediction tensor
"""
import math

import numpy as np

from oracle import boxes as ob

F32 = np.float32


def _windows_ref(n, tile, overlap):
    if n <= tile:
        return [(0, n)]
    stride = max(1, int(tile * (1 - overlap)))
    k = int(math.ceil((n - tile) / stride)) + 1
    return [(min(i * stride, n - tile), tile) for i in range(k)]


def plan_tiles_ref(w, h, tile, overlap=0.25, whole=True):
    if tile < 32 or not 0 <= overlap <= 0.9:
        raise ValueError('tile >= 32 and 0 <= overlap <= 0.9')
    out = []
    for y0, th in _windows_ref(h, tile, overlap):          # row-major, y outer
        for x0, tw in _windows_ref(w, tile, overlap):
            interior = (1 if x0 > 0 else 0) | (2 if x0 + tw < w else 0) | (4 if y0 > 0 else 0) | (8 if y0 + th < h else 0)
            out.append((x0, y0, tw, th, interior))
    if whole and len(out) > 1:
        out.append((0, 0, w, h, 0))
    return out


def candidates_ref(dets, tiles, size, edge_margin=2, tile_cap=None):
    """Steps 1-3 for one picture of size (W, H): dets[t] = decode() of tile t (idx, cls, conf, box; confidence order), tiles[t] =
    (x0, y0, w, h, interior).  Returns the ordered union as a dict of arrays: conf, cls, idx, tile, box (int64 on the picture's
    1000 grid)."""
    W, H = int(size[0]), int(size[1])
    conf, cls, idx, tl, box = [], [], [], [], []
    for t, (d, (x0, y0, w, h, interior)) in enumerate(zip(dets, tiles)):
        n = len(d['idx']) if tile_cap is None else min(len(d['idx']), tile_cap)
        for j in range(n):
            xmin, xmax, ymin, ymax = (int(v) for v in d['box'][j])
            m = edge_margin
            if m >= 0 and ((interior & 1 and xmin <= m) or (interior & 2 and xmax >= 999 - m) or (interior & 4 and ymin <= m)
                           or (interior & 8 and ymax >= 999 - m)):
                continue
            conf.append(F32(d['conf'][j])); cls.append(int(d['cls'][j])); idx.append(int(d['idx'][j])); tl.append(t)
            box.append((min((1000 * x0 + xmin * w) // W, 999), min((1000 * x0 + xmax * w) // W, 999),
                        min((1000 * y0 + ymin * h) // H, 999), min((1000 * y0 + ymax * h) // H, 999)))
    conf = np.array(conf, F32); cls = np.array(cls, np.int64); idx = np.array(idx, np.int64); tl = np.array(tl, np.int64)
    box = np.array(box, np.int64).reshape(-1, 4)
    order = np.lexsort((idx, tl, -conf.astype(np.float64)))      # confidence descending by value, then tile, then anchor
    return dict(conf=conf[order], cls=cls[order], idx=idx[order], tile=tl[order], box=box[order])


def merge_ref(dets, tiles, size, edge_margin=2, max_out=None, tile_cap=None):
    """The merged detections of one picture: dict conf, cls, idx, tile, box."""
    cand = candidates_ref(dets, tiles, size, edge_margin, tile_cap)
    keep = ob.suppress(cand, max_out)                            # step 4: oracle.boxes.suppress, then [:max_out]
    return {k: v[keep] for k, v in cand.items()}


def merge_ref_all(dets, tiles, edge_margin=2, max_out=None, tile_cap=None):
    """tiles = [(image, (x0, y0, w, h, interior), (W, H))], the images ascending from 0; dets one decode() record set per entry"""
    out = []
    for i in range(max(t[0] for t in tiles) + 1):
        sel = [k for k, t in enumerate(tiles) if t[0] == i]
        out.append(merge_ref([dets[k] for k in sel], [tuple(tiles[k][1]) for k in sel], tiles[sel[0]][2], edge_margin, max_out, tile_cap))
    return out


def decode_tiles(pred, anch, thr, tile_cap):
    return [ob.decode(pred[t], anch, thr, tile_cap) for t in range(pred.shape[0])]


# ------------------------------------------------------------------------------------------------ the planted scene
def plant(pred, anch, anch_abs, part, cls, confs):
    """Make the len(confs) anchors that overlap `part` (xmin, xmax, ymin, ymax on the tile's 1000 grid) best predict it: class
    `cls` at those confidences, offsets that decode to the part."""
    iou = ob.iou_plus1(np.array(part, np.float64), anch_abs)
    best = np.argsort(-iou, kind='stable')[:len(confs)]
    cx, cy, w, h = ob.abs2prop(part[0], part[1], part[2], part[3])
    for a, c in zip(best, confs):
        if pred[a, :-5].max() > 0:
            continue                                             # the anchor already speaks for another object
        pred[a, cls] = c
        pred[a, -4:] = ob.encode_location((float(cx), float(cy), max(float(w), 1e-3), max(float(h), 1e-3)), anch[a]).astype(F32)


def planted_scene(pname='vgg300', size=(1000, 700), tile=400, overlap=0.25, n_objects=25, num_classes=20, seed=5, whole=True):
    """Objects planted on a picture of `size` = (W, H): every tile's prediction holds three hot anchors per visible part of an
    object (at least a quarter of it in both directions), the confidences rounded to 1/64 so that ties occur within and
    across tiles.  Returns (pred [n_tiles, A, C+5] f32, tiles [(x0, y0, w, h, interior)], anchors [A, 4])."""
    preset = ob.get_preset(pname)
    anch = ob.anchors(preset)
    anch_abs = ob.anchors_abs(anch)
    W, H = size
    rng = np.random.default_rng(seed)
    tiles = plan_tiles_ref(W, H, tile, overlap, whole)
    objs = []
    for _ in range(n_objects):
        w, h = int(rng.integers(60, 200)), int(rng.integers(60, 200))
        x0, y0 = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
        objs.append((x0, y0, w, h, int(rng.integers(0, num_classes)), float(rng.integers(36, 62)) / 64))
    pred = np.zeros((len(tiles), anch.shape[0], num_classes + 5), F32)
    pred[:, :, num_classes] = 1
    for t, (tx, ty, tw, th, _) in enumerate(tiles):
        for (x0, y0, w, h, cls, base) in objs:
            ix0, ix1 = max(x0, tx), min(x0 + w, tx + tw)
            iy0, iy1 = max(y0, ty), min(y0 + h, ty + th)
            if ix1 - ix0 < w / 4 or iy1 - iy0 < h / 4:
                continue
            part = ((ix0 - tx) * 1000 // tw, min((ix1 - tx) * 1000 // tw, 999), (iy0 - ty) * 1000 // th, min((iy1 - ty) * 1000 // th, 999))
            plant(pred[t], anch, anch_abs, part, cls, [F32(base), F32(base - 1 / 64), F32(base - 4 / 64)])
    return pred, tiles, anch
