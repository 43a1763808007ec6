"""Numpy oracle of the mosaic augmentation: the layout of a centre, the box mapping in float64 and the
composition of per-cell arrays into samples.  Written from the contract, not from the product's code: tests compare the two."""
import numpy as np


def layout(mx, my, W, H):
    """The four cells (x0, y0, w, h) of centre (mx, my): top-left, top-right, bottom-left, bottom-right."""
    assert 1 <= mx <= W - 1 and 1 <= my <= H - 1
    return [(0, 0, mx, my), (mx, 0, W - mx, my), (0, my, mx, H - my), (mx, my, W - mx, H - my)]


def coverage(cells, W, H):
    """How often every pixel of a W x H sample is covered by the cells (a tiling: all ones)."""
    n = np.zeros((H, W), np.int64)
    for x0, y0, w, h in cells:
        assert w >= 1 and h >= 1 and 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= H
        n[y0:y0 + h, x0:x0 + w] += 1
    return n


def map_box(box, cell, W, H):
    """(cx, cy, w, h) proportional to the cell -> proportional to the sample, float64"""
    cx, cy, w, h = (np.float64(v) for v in box)
    x0, y0, cw, ch = cell
    return ((x0 + cx * cw) / W, (y0 + cy * ch) / H, w * cw / W, h * ch / H)


def compose(cell_arrays, cells, W, H, b=None):
    """cell_arrays[i] ([h][w][3]) pasted at (x0, y0) of sample cells[i][0]; cells: rows (sample, x0, y0, w, h).  Every pixel
    must be written exactly once.  -> float32 [b][H][W][3]"""
    cells = np.asarray(cells).reshape(-1, 5)
    b = int(cells[:, 0].max()) + 1 if b is None else b
    out = np.full((b, H, W, 3), np.nan, np.float32)
    seen = np.zeros((b, H, W), np.int64)
    for a, (s, x0, y0, w, h) in zip(cell_arrays, cells):
        a = np.asarray(a)
        assert a.shape == (h, w, 3), (a.shape, (h, w))
        out[s, y0:y0 + h, x0:x0 + w] = a
        seen[s, y0:y0 + h, x0:x0 + w] += 1
    assert (seen == 1).all()
    return out
