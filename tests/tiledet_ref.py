"""Numpy oracle of tiled detection with the DetectionOutput decode, built on oracle/boxes.py like tests/detout_ref.py
and tests/tiles_ref.py.

One picture of W x H source pixels, tiles t = 0 .. T-1 = (x0, y0, w, h, interior), pred_t [A, C+5] f32:
  1. per tile and foreground class c the anchors with !(pred_t[a, c] < conf_thr), by confidence descending (by float value), ties
     by lower anchor; the first nms_top_k; their boxes as decode_box decodes them, on the tile's 1000 grid.  No suppression
     inside a tile.
  2. edge drop, after step 1's cut: tiles_ref's rule on the tile-grid box with the tile's interior bits (m < 0 drops nothing).
  3. the picture's grid: X = min((1000 x0 + x w) // W, 999), Y alike.
  4. per class across tiles: the union by (confidence descending, tile ascending, anchor ascending); the first nms_top_k of the
     picture; oracle.boxes.nms_class on them.
  5. across classes: the survivors by (confidence descending, tile, anchor, class ascending); the first keep_top_k.
Every tie rule is one descending order of the unique key conf bits << 32 | (255 - tile) << 24 | (32767 - anchor) << 8 |
(127 - class) (`key`): candidates are non-negative floats, whose bit patterns order as their values.

`mutant` switches one rule to a plausible wrong one; tests/test_tiledet_ref.py shows that the cases of tests/test_gpu_tiledet.py
tell every mutant from the oracle."""
import numpy as np

from oracle import boxes as ob

F32 = np.float32
MUTANTS = ('edge_drop_before_cut', 'nms_inside_tile', 'no_picture_cut', 'nms_on_tile_grid', 'cut_ties_by_anchor_before_tile',
           'final_ties_by_class_before_anchor', 'keep_top_k_per_tile', 'class_agnostic_nms')


def key(conf, tile, anchor, cls):
    """the 64-bit key of a record"""
    return (int(np.array(conf, F32).view(np.uint32)) << 32) | ((255 - int(tile)) << 24) | ((32767 - int(anchor)) << 8) | (127 - int(cls))


def _empty():
    z = np.zeros(0, np.int64)
    return dict(idx=z, cls=z.copy(), tile=z.copy(), conf=np.zeros(0, F32), box=np.zeros((0, 4), np.int64))


def _cut(box, interior, m):
    xmin, xmax, ymin, ymax = box
    return m >= 0 and bool((interior & 1 and xmin <= m) or (interior & 2 and xmax >= 999 - m) or (interior & 4 and ymin <= m)
                           or (interior & 8 and ymax >= 999 - m))


def detout_tiles(preds, tiles, size, anch, thr, nms_top_k=400, keep_top_k=200, edge_margin=2, mutant=None):
    """-> dict(idx, cls, tile, conf f32, box int64 [n, 4] on the picture's grid) of one picture, in step 5's order.
    preds [T, A, C+5]; tiles [(x0, y0, w, h, interior)]; size (W, H)."""
    assert mutant is None or mutant in MUTANTS, mutant
    preds = np.asarray(preds, F32)
    T, A, nv = preds.shape
    assert T == len(tiles)
    C = nv - 5
    W, H = int(size[0]), int(size[1])
    thr = F32(thr)
    k, m = nms_top_k, edge_margin
    tbox, pbox = {}, {}

    def tile_box(t, a):                       # on the tile's grid
        if (t, a) not in tbox:
            loc = preds[t, a, C + 1:].copy()
            loc[loc > 100] = 100
            tbox[t, a] = ob.normalize_abs_np2(*ob.decode_location_np2(loc, anch[a]))
        return tbox[t, a]

    def pic_box(t, a):                        # on the picture's grid
        if (t, a) not in pbox:
            x0, y0, w, h, _ = tiles[t]
            xmin, xmax, ymin, ymax = tile_box(t, a)
            pbox[t, a] = (min((1000 * x0 + xmin * w) // W, 999), min((1000 * x0 + xmax * w) // W, 999),
                          min((1000 * y0 + ymin * h) // H, 999), min((1000 * y0 + ymax * h) // H, 999))
        return pbox[t, a]

    def nms(recs, grid=pic_box):
        if not recs:
            return []
        return [recs[i] for i in ob.nms_class(np.array([grid(r[1], r[2]) for r in recs], np.int64).reshape(-1, 4))]

    def final_order(recs):                    # records are (conf, tile, anchor, class)
        if mutant == 'final_ties_by_class_before_anchor':
            return sorted(recs, key=lambda r: (-float(r[0]), r[1], r[3], r[2]))
        return sorted(recs, key=lambda r: (-float(r[0]), r[1], r[2], r[3]))

    # steps 1, 2 per tile
    per_tile = []
    for t in range(T):
        interior = tiles[t][4]
        recs = []
        for c in range(C):
            col = preds[t, :, c]
            cand = np.nonzero(~(col < thr))[0]
            cand = cand[np.lexsort((cand, -col[cand].astype(np.float64)))]
            if mutant == 'edge_drop_before_cut':
                cand = np.array([a for a in cand if not _cut(tile_box(t, int(a)), interior, m)], np.int64)
            sel = [(col[a], t, int(a), c) for a in cand[:k]]
            if mutant == 'nms_inside_tile':
                sel = nms(sel, tile_box)
            recs += [r for r in sel if not _cut(tile_box(t, r[2]), interior, m)]
        if mutant == 'keep_top_k_per_tile':
            recs = final_order(recs)[:keep_top_k]
        per_tile.append(recs)
    # step 4 per class
    sel = []
    for c in range(C):
        union = [r for recs in per_tile for r in recs if r[3] == c]
        if mutant == 'cut_ties_by_anchor_before_tile':
            union.sort(key=lambda r: (-float(r[0]), r[2], r[1]))
        else:
            union.sort(key=lambda r: (-float(r[0]), r[1], r[2]))
        sel.append(union if mutant == 'no_picture_cut' else union[:k])
    if mutant == 'class_agnostic_nms':
        out = nms(final_order([r for s in sel for r in s]))
    elif mutant == 'nms_on_tile_grid':
        out = [r for s in sel for r in nms(s, tile_box)]
    else:
        out = [r for s in sel for r in nms(s)]
    # step 5
    out = final_order(out)[:keep_top_k]
    if not out:
        return _empty()
    return dict(idx=np.array([r[2] for r in out], np.int64), cls=np.array([r[3] for r in out], np.int64),
                tile=np.array([r[1] for r in out], np.int64), conf=np.array([r[0] for r in out], F32),
                box=np.array([pic_box(r[1], r[2]) for r in out], np.int64).reshape(-1, 4))


def detout_tiles_all(preds, tiles, anch, thr, nms_top_k=400, keep_top_k=200, edge_margin=2, mutant=None):
    """tiles = [(image, (x0, y0, w, h, interior), (W, H))], the images ascending from 0; preds [n_tiles, A, C+5] -> one result per
    picture"""
    out = []
    for i in range(max(t[0] for t in tiles) + 1):
        sel = [j for j, t in enumerate(tiles) if t[0] == i]
        out.append(detout_tiles(preds[sel], [tuple(tiles[j][1]) for j in sel], tiles[sel[0]][2], anch, thr, nms_top_k, keep_top_k,
                                edge_margin, mutant))
    return out


def same(a, b):
    """two results agree in count, confidence bits, class, anchor, tile and box"""
    return (len(a['idx']) == len(b['idx']) and np.array_equal(a['conf'].view(np.uint32), b['conf'].view(np.uint32))
            and np.array_equal(a['cls'], b['cls']) and np.array_equal(a['idx'], b['idx']) and np.array_equal(a['tile'], b['tile'])
            and np.array_equal(a['box'], b['box']))
